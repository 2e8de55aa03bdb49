"""CPU side of draft verification (include/million_hip.h, "Draft verification"): the closed form of million_window_commit equals
single decode steps over every window state, the block-merge formula equals an fp64 softmax over the concatenated keys, the
rows-as-heads view puts every draft row under its kv head, the two new entries validate their arguments before any HIP call, and
PagedPQCache.commit - on a CPU cache with the launches stubbed - moves the host mirror as single steps do, takes its pages before
the launch and refuses before anything moves."""
import ctypes

import numpy as np
import pytest

from tests import lse_ref as R
from tests import verify_model as VM

ERR_ARG, ERR_SHAPE, ERR_ALIGN = -3, -1, -2


# ---------------------------------------------------------------- commit: closed form = single steps -----------------------
@pytest.mark.parametrize("ps", [32, 64])
@pytest.mark.parametrize("cap_pages", [1, 2])
def test_commit_model_equals_single_steps(ps, cap_pages):
    cap = cap_pages * ps
    T0 = 37      # not a page multiple: a flush may straddle two pages
    n = 0
    for r in range(cap + 1):
        for a in range(17):
            for start in (0, 1, cap - 1):
                got = VM.commit_closed(T0, r, start, a, ps, cap)
                want = VM.commit_sequential(T0, r, start, a, ps, cap)
                assert got[:3] == want[:3], (r, a, start, got[:3], want[:3])                      # T, r, start
                assert got[3] == want[3], (r, a, start)                                           # which row is coded at which token
                assert VM.live_ring(got[4], *got[1:3], cap) == VM.live_ring(want[4], *want[1:3], cap), (r, a, start)
                assert got[1] <= cap and (got[0] - T0) in (0, ps)
                n += 1
    assert n == (cap + 1) * 17 * 3


def test_commit_model_flushes_new_rows_when_the_window_is_short():
    """cap = ps = 32, r = 20, a = 16: the flush takes the 20 window rows and the first 12 new rows; 4 new rows stay."""
    T, r, start, coded, ring = VM.commit_closed(64, 20, 5, 16, 32, 32)
    assert (T, r, start) == (96, 4, 5)
    assert [coded[64 + j] for j in range(32)] == [("w", j) for j in range(20)] + [("n", i) for i in range(12)]
    assert VM.live_ring(ring, r, start, 32) == {5 + j: ("n", 12 + j) for j in range(4)}


# ---------------------------------------------------------------- block merge = softmax over [past; block] ------------------
@pytest.mark.parametrize("bs,nh,nhk,n,d,n_past", [(2, 8, 2, 5, 128, 77), (1, 4, 4, 16, 64, 300), (3, 8, 8, 1, 128, 0)])
def test_block_merge_model_is_the_softmax_over_all_keys(bs, nh, nhk, n, d, n_past):
    rs = np.random.RandomState(n + d)
    q = rs.standard_normal((bs, nh, n, d))
    k, v = rs.standard_normal((bs, nhk, n, d)), rs.standard_normal((bs, nhk, n, d))
    Kp, Vp = rs.standard_normal((bs, nhk, n_past, d)), rs.standard_normal((bs, nhk, n_past, d))
    out_a, lse_a = R.attend(q, Kp, Vp)
    got_o, got_l = VM.block_merge(q, k, v, out_a, lse_a)
    for i in range(n):
        K = np.concatenate([Kp, k[:, :, :i + 1]], axis=2)
        V = np.concatenate([Vp, v[:, :, :i + 1]], axis=2)
        wo, wl = R.attend(q[:, :, i:i + 1], K, V)
        rel = np.linalg.norm(got_o[:, :, i] - wo[:, :, 0], axis=-1) / np.linalg.norm(wo[:, :, 0], axis=-1)
        assert rel.max() < 1e-3 and rel.max() < 1e-12
        assert np.abs(got_l[:, :, i] - wl[:, :, 0]).max() <= R.LSE_TOL
        # and it is lse_ref.merge of the two parts
        bo, bl = R.attend(q[:, :, i:i + 1], k[:, :, :i + 1], v[:, :, :i + 1])
        mo, ml = R.merge([out_a[:, :, i:i + 1], bo], [lse_a[:, :, i:i + 1], bl])
        assert np.abs(mo[:, :, 0] - got_o[:, :, i]).max() <= 1e-12 and np.abs(ml[:, :, 0] - got_l[:, :, i]).max() <= 1e-12


def test_block_merge_model_edges():
    rs = np.random.RandomState(3)
    bs, nh, nhk, n, d = 3, 4, 2, 4, 64
    q, k, v = rs.standard_normal((bs, nh, n, d)), rs.standard_normal((bs, nhk, n, d)), rs.standard_normal((bs, nhk, n, d))
    out_a, lse_a = rs.standard_normal((bs, nh, n, d)), rs.standard_normal((bs, nh, n))
    lse_a[0, 1, 2] = np.nan
    lse_a[1] = -np.inf
    out_a[1] = 1e30      # a -inf part's out is never used
    k[2, :, 1:], v[2, :, 1:], q[2, :, 1:] = np.nan, np.nan, np.nan
    out, lse = VM.block_merge(q, k, v, out_a, lse_a, n_valid=[4, 4, 1])
    assert np.isnan(out[0, 1, 2]).all() and np.isnan(lse[0, 1, 2])
    assert np.isfinite(np.delete(out[0].reshape(-1, d), 1 * n + 2, 0)).all()
    own, own_l = VM.block_merge(q[1:2], k[1:2], v[1:2], np.zeros_like(out_a[1:2]), np.full_like(lse_a[1:2], -np.inf))
    assert np.array_equal(out[1], own[0]) and np.array_equal(lse[1], own_l[0])      # the block's own attention
    assert np.isfinite(out[2, :, 0]).all() and np.all(out[2, :, 1:] == 0) and np.all(np.isneginf(lse[2, :, 1:]))


# ---------------------------------------------------------------- the rows-as-heads view ------------------------------------
@pytest.mark.parametrize("G", [1, 3, 4, 8])
def test_rows_as_heads_view_keeps_the_kv_head(G):
    """q (bs, nh, n, d) contiguous viewed as (bs, nh * n, 1, d): virtual head v = h n + i, served as one of G n query heads of
    kv head v // (G n), which is h // G."""
    nhk = 2
    nh = G * nhk
    for n in range(1, 17):
        q = np.arange(nh * n * 2).reshape(1, nh, n, 2)
        flat = q.reshape(1, nh * n, 1, 2)
        for h in range(nh):
            for i in range(n):
                vh = h * n + i
                assert np.array_equal(flat[0, vh, 0], q[0, h, i])
                assert vh // (G * n) == h // G


# ---------------------------------------------------------------- the entries refuse before any HIP call -------------------
@pytest.fixture(scope="module")
def lib():
    from million_amd import build, _lib
    build.build()
    return _lib.load()


A = 0x100000      # made-up aligned device addresses: a refused call dereferences nothing


def _bm_desc(L, bs=2, nh=8, nhk=2, n=4, d=128):
    desc = L.BlockMergeDesc()
    desc.struct_size = ctypes.sizeof(L.BlockMergeDesc)
    desc.bs, desc.nh, desc.nh_k, desc.n, desc.d = bs, nh, nhk, n, d
    for arr, heads in ((desc.q_stride, nh), (desc.a_stride, nh), (desc.o_stride, nh), (desc.k_stride, nhk), (desc.v_stride, nhk)):
        arr[0], arr[1], arr[2] = heads * n * d, n * d, d
    desc.stage_stride_b, desc.stage_stride_h = nhk * 16 * d, 16 * d
    return desc


def _bm_call(lib, desc, q=A, k=A + 0x10000, v=A + 0x20000, out_a=A + 0x30000, lse_a=A + 0x40000, dev_n=None, out=A + 0x30000,
             lse_out=None, k_stage=None, v_stage=None):
    return lib.million_attn_block_merge(ctypes.byref(desc), q, k, v, out_a, lse_a, dev_n, out, lse_out, k_stage, v_stage, None)


def test_block_merge_refuses_without_a_gpu(lib):
    from million_amd import _lib as L
    assert L.SYMBOLS["million_attn_block_merge"] == (ctypes.c_int32, [ctypes.POINTER(L.BlockMergeDesc)] + [ctypes.c_void_p] * 11)
    assert ctypes.sizeof(L.BlockMergeDesc) == 24 + 8 * 17
    d = _bm_desc(L)
    d.struct_size -= 8
    assert _bm_call(lib, d) == ERR_ARG and b"struct_size" in lib.million_last_error()
    for n in (0, 17):
        assert _bm_call(lib, _bm_desc(L, n=n)) == ERR_SHAPE and b"n=" in lib.million_last_error()
    assert _bm_call(lib, _bm_desc(L, d=96)) == ERR_SHAPE and b"d=96" in lib.million_last_error()
    assert _bm_call(lib, _bm_desc(L, nh=7)) == ERR_SHAPE
    assert _bm_call(lib, _bm_desc(L), q=A + 8) == ERR_ALIGN and b"aligned" in lib.million_last_error()
    assert _bm_call(lib, _bm_desc(L), lse_a=A + 2) == ERR_ALIGN
    for part in ("q", "k", "v", "out_a", "lse_a", "out"):
        assert _bm_call(lib, _bm_desc(L), **{part: None}) == ERR_ARG and b"null" in lib.million_last_error(), part
    assert _bm_call(lib, _bm_desc(L), k_stage=A + 0x50000) == ERR_ARG and b"together" in lib.million_last_error()
    d = _bm_desc(L)
    d.q_stride[2] = 132
    assert _bm_call(lib, d) == ERR_ALIGN and b"stride" in lib.million_last_error()


def _wc_desc(L, n_layers=2, bs=2, nhk=2, d=128, M=64, C=256, n_bound=4, ps=32, cap=64, n_pages_cap=8):
    desc = L.WindowCommitDesc()
    desc.struct_size = ctypes.sizeof(L.WindowCommitDesc)
    desc.n_layers, desc.bs, desc.nh_k, desc.d, desc.M, desc.C, desc.n_bound = n_layers, bs, nhk, d, M, C, n_bound
    desc.page_size, desc.n_pages_cap, desc.resid_cap = ps, n_pages_cap, cap
    desc.n_pool = n_layers * bs * nhk * n_pages_cap
    desc.new_stride_l, desc.new_stride_b, desc.new_stride_h, desc.new_stride_n = bs * nhk * 16 * d, nhk * 16 * d, 16 * d, d
    desc.ids_layer_stride, desc.rows_layer_stride, desc.lengths_layer_stride = bs * nhk * n_pages_cap, bs * nhk * cap * d, bs * 4
    return desc


_WC_ARGS = ("k_new", "v_new", "k_resid", "v_resid", "k_prep", "v_prep", "k_pool", "v_pool", "page_ids", "dev_lengths", "dev_n")


def _wc_call(lib, desc, **over):
    args = {name: A + 0x10000 * i for i, name in enumerate(_WC_ARGS)}
    args.update(over)
    return lib.million_window_commit(ctypes.byref(desc), *[args[name] for name in _WC_ARGS], None)


def test_window_commit_refuses_without_a_gpu(lib):
    from million_amd import _lib as L
    assert L.SYMBOLS["million_window_commit"] == (ctypes.c_int32, [ctypes.POINTER(L.WindowCommitDesc)] + [ctypes.c_void_p] * 12)
    assert ctypes.sizeof(L.WindowCommitDesc) == 48 + 8 * 7
    d = _wc_desc(L)
    d.struct_size += 8
    assert _wc_call(lib, d) == ERR_ARG and b"struct_size" in lib.million_last_error()
    for n in (0, 17):
        assert _wc_call(lib, _wc_desc(L, n_bound=n, ps=64)) == ERR_SHAPE and b"n_bound" in lib.million_last_error()
    assert _wc_call(lib, _wc_desc(L, n_bound=33, ps=32)) == ERR_SHAPE and b"page_size=32" in lib.million_last_error()      # n_bound > page_size
    assert _wc_call(lib, _wc_desc(L, d=96)) == ERR_SHAPE and b"d=96" in lib.million_last_error()
    assert _wc_call(lib, _wc_desc(L, ps=48)) == ERR_SHAPE
    assert _wc_call(lib, _wc_desc(L, ps=64, cap=32)) == ERR_SHAPE and b"resid_cap" in lib.million_last_error()
    assert _wc_call(lib, _wc_desc(L), k_new=A + 8) == ERR_ALIGN and b"aligned" in lib.million_last_error()
    assert _wc_call(lib, _wc_desc(L), dev_n=A + 2) == ERR_ALIGN
    for part in _WC_ARGS:
        assert _wc_call(lib, _wc_desc(L), **{part: None}) == ERR_ARG and b"null" in lib.million_last_error(), part
    d = _wc_desc(L)
    d.new_stride_n = 132
    assert _wc_call(lib, d) == ERR_ALIGN and b"stride" in lib.million_last_error()
    d = _wc_desc(L)
    d.lengths_layer_stride = 4
    assert _wc_call(lib, d) == ERR_ARG and b"layer strides" in lib.million_last_error()


# ---------------------------------------------------------------- commit's host side: mirror, pages, refusals ---------------
def _host_cache(monkeypatch, preallocate, log):
    """A PagedPQCache on the CPU with the launches of verify / commit stubbed: what is left is the host logic."""
    import torch
    from million_amd import ops
    from million_amd.pq_cache import PagedPQCache
    monkeypatch.setattr(ops, "decode_workspace_bytes", lambda *a, **k: 16)
    monkeypatch.setattr(ops, "pq_decode_attn", lambda q, *a, **k: (torch.zeros_like(q), torch.zeros(q.shape[0], q.shape[1], 1)))
    monkeypatch.setattr(ops, "attn_block_merge", lambda q, k, v, out_a, lse_a, dev_n, **kw: out_a)
    monkeypatch.setattr(ops, "window_commit", lambda *a, **k: log.append((a[10].tolist(), k["n_bound"])))
    cache = PagedPQCache(bs=3, nh=8, num_key_value_heads=2, M=64, layer_num=2, d=128, page_size=32, extended_residual_size=64,
                         max_tokens=256, preallocate=preallocate, device="cpu")
    cache._kprep = cache._vprep = None
    return cache


def _host_verify(cache, n=4, n_draft=None, layers=None):
    import torch
    q, kv = torch.zeros(cache.bs, cache.nh, n, cache.d, dtype=torch.float16), torch.zeros(cache.bs, 2, n, cache.d, dtype=torch.float16)
    for l in range(cache.layer_num) if layers is None else layers:
        cache.verify(q, kv, kv, l, n_draft=n_draft)


@pytest.mark.parametrize("preallocate", [True, False])
def test_commit_moves_the_mirror_as_single_steps(monkeypatch, preallocate):
    log = []
    cache = _host_cache(monkeypatch, preallocate, log)
    ps, cap = cache.page_size, cache.extended_residual_size
    state = [(40, 62, 5, 102), (0, 0, 0, 0), (64, 64, 63, 128)]      # (T, r, start, seen) per slot: nearly full, empty, full
    for b, (T, r, st, seen) in enumerate(state):
        cache._T_a[:, b], cache._r_a[:, b], cache._rs_a[:, b], cache._seen_a[:, b] = T, r, st, seen
        if not preallocate:
            for l in range(cache.layer_num):
                cache._assign_pages(l, -(-T // ps), b)
    cache._pre_a[:, 2] = 1      # slot 2's oldest page was encoded ahead: the commit's flush clears the flag
    rs = np.random.RandomState(0)
    for rnd in range(40):
        n_accept = [0, 0, 0] if rnd == 3 else [int(x) for x in rs.randint(0, 5, 3)]
        if max(int(cache._T_a[0, b]) for b in range(3)) + ps > cache.max_tokens:
            break
        before = [tuple(int(a[0, b]) for a in (cache._T_a, cache._r_a, cache._rs_a, cache._seen_a)) for b in range(3)]
        _host_verify(cache)
        n_calls = len(log)
        cache.commit(n_accept)
        assert len(log) == n_calls + (1 if any(n_accept) else 0) and (not any(n_accept) or log[-1] == (n_accept, 4))
        for b in range(3):
            T, r, st, seen = before[b]
            want = VM.commit_sequential(T, r, st, n_accept[b], ps, cap)[:3]
            for l in range(cache.layer_num):
                got = tuple(int(a[l, b]) for a in (cache._T_a, cache._r_a, cache._rs_a, cache._seen_a))
                assert got == want + (seen + n_accept[b],), (rnd, b, l, got, want)
                assert int(cache._pages_a[l, b]) * ps >= want[0]      # the flush's pages were there before the launch
            if want[0] != T:
                assert not cache._pre_a[:, b].any()
    assert rnd >= 10 and int(cache._T_a[0, 1]) >= 32      # the empty slot crossed a flush


def test_commit_refuses_on_the_host(monkeypatch):
    log = []
    cache = _host_cache(monkeypatch, False, log)
    cache._r_a[:] = 62
    snap = lambda: [a.copy() for a in (cache._T_a, cache._r_a, cache._rs_a, cache._seen_a, cache._pages_a)] + [set(cache.page_manager.free_pages)]
    same = lambda x, y: all(np.array_equal(a, b) if isinstance(a, np.ndarray) else a == b for a, b in zip(x, y))
    before = snap()

    def refused(match, n_accept):
        with pytest.raises(RuntimeError, match=match):
            cache.commit(n_accept)
        assert same(before, snap()) and not log

    refused("verify", [1, 1, 1])
    _host_verify(cache, layers=[0])
    refused("every layer", [1, 1, 1])
    _host_verify(cache, n_draft=[4, 0, 2])
    refused("n_accept", [4, 1, 2])
    refused("n_accept", [4, 0])
    refused("n_accept", [-1, 0, 0])
    cache._r_a[1, 0] += 1      # layer 1 of slot 0 is a row ahead: mid-step
    before = snap()
    refused("mid-step", [1, 0, 0])
    cache._r_a[1, 0] -= 1
    taken = [cache.page_manager.allocate_page() for _ in range(len(cache.page_manager.free_pages) - 3)]      # 3 pages left, a flush of one slot needs 4
    before = snap()
    refused("free pages", [4, 0, 0])
    for pid in taken:
        cache.page_manager.free_page(pid)
    cache.commit([4, 0, 2])
    assert log == [([4, 0, 2], 4)] and cache._T_a[:, 0].tolist() == [32, 32] and cache._r_a[:, 0].tolist() == [34, 34] and cache._r_a[:, 2].tolist() == [64, 64]
    with pytest.raises(RuntimeError, match="verify"):
        cache.commit([0, 0, 0])
    with pytest.raises(RuntimeError, match="draft rows"):
        _host_verify(cache, n=17)
    with pytest.raises(RuntimeError, match="n_draft"):
        _host_verify(cache, n_draft=[5, 0, 0])
