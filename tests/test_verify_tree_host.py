"""CPU side of draft verification over a tree (include/million_hip.h, "Draft verification"): the masked block-merge model
equals the chain's model on every node's gathered ancestor chain, the mask sanitisation rule, the commit of chosen rows, the two
new entries validate their arguments before any HIP call, PagedPQCache.verify(tree=) / commit(path=) - on a CPU cache with the
launches stubbed - refuse before anything moves and move the host mirror as commit(len) does, and spec_tree.greedy_path."""
import ctypes

import numpy as np
import pytest

from tests import verify_model as VM
from tests import verify_tree_model as TM

ERR_ARG, ERR_SHAPE, ERR_ALIGN = -3, -1, -2


# ---------------------------------------------------------------- the trees of the tests ------------------------------------
def test_tree_set_covers_the_shapes():
    trees = TM.tree_set()
    for _, n, ps in trees:
        assert len(ps) == n and all(-1 <= p < i for i, p in enumerate(ps)), ps
    assert {n for _, n, _ in trees} == {1, 2, 5, 16}
    for n in (2, 5, 16):
        mine = [ps for _, m, ps in trees if m == n]
        assert [i - 1 for i in range(n)] in mine, "a chain"
        assert [-1] * n in mine, "a star"
        assert any(ps[-1] == 0 and not TM.children(ps, n - 1) for ps in mine), "the last node a leaf under node 0"
    big = [ps for _, m, ps in trees if m == 16]
    assert any(max(len(TM.children(ps, i)) for i in range(16)) >= 3 for ps in big), "a node with 3 children"
    assert any(max(TM.depth(ps, i) for i in range(16)) >= 4 and ps != [i - 1 for i in range(16)] for ps in big), "depth 4 off a chain"
    assert max(TM.depth(TM.binary_tree(8), i) for i in range(8)) == 4


def test_ancestor_masks():
    from million_amd import spec_tree
    assert spec_tree.ancestor_masks([-1, 0, 0, 1, -1]).tolist() == [0b1, 0b11, 0b101, 0b1011, 0b10000]
    for _, n, ps in TM.tree_set():
        got = spec_tree.ancestor_masks(ps)
        assert got.dtype == np.int32 and got.shape == (n,) and np.array_equal(got, TM.ancestor_masks(ps))
        for i in range(n):
            assert [j for j in range(n) if (got[i] >> j) & 1] == TM.chain_of(ps, i) == spec_tree.chain_of(ps, i)
            assert TM.sanitise(got[i], i) == got[i]      # a clean mask passes the device rule unchanged
    assert spec_tree.ancestor_masks(range(-1, 15)).tolist() == [(2 << i) - 1 for i in range(16)]
    for bad in ([0], [-1, 1], [-2], [-1, -1, 2], [-1] * 17):
        with pytest.raises(ValueError):
            spec_tree.ancestor_masks(bad)


def test_mask_sanitisation_rule():
    """m = (mask & ((2u << i) - 1)) | (1u << i): the row itself always, no later row, no bit at or above 16 - for any word."""
    rs = np.random.RandomState(0)
    words = [0, -1, 0x7FFFFFFF, -0x80000000] + [int(x) for x in rs.randint(-2 ** 31, 2 ** 31, 200)]
    for i in range(16):
        for w in words:
            m = TM.sanitise(w, i)
            assert (m >> i) == 1, (w, i)                                              # bit i set, nothing above it
            assert m & ((1 << i) - 1) == (w & 0xFFFFFFFF) & ((1 << i) - 1), (w, i)    # the bits below i as given
    assert TM.sanitise(0, 15) == 0x8000 and TM.sanitise(-1, 15) == 0xFFFF and TM.sanitise(-1, 0) == 1


# ---------------------------------------------------------------- the masked block merge -------------------------------------
def _block(rs, bs, nh, nhk, n, d):
    q = rs.standard_normal((bs, nh, n, d))
    k, v = rs.standard_normal((bs, nhk, n, d)), rs.standard_normal((bs, nhk, n, d))
    out_a, lse_a = rs.standard_normal((bs, nh, n, d)), rs.standard_normal((bs, nh, n)) * 2 + 3
    return q, k, v, out_a, lse_a


def test_tree_model_is_the_chain_model_on_every_gathered_chain():
    rs = np.random.RandomState(1)
    nh, nhk, d = 4, 2, 16
    for seed, n, ps in TM.tree_set():
        q, k, v, out_a, lse_a = _block(rs, 1, nh, nhk, n, d)
        got_o, got_l = TM.tree_block_merge(q, k, v, out_a, lse_a, [TM.ancestor_masks(ps)])
        for i in range(n):
            c = TM.chain_of(ps, i)
            wo, wl = VM.block_merge(q[:, :, c], k[:, :, c], v[:, :, c], out_a[:, :, c], lse_a[:, :, c])
            assert np.array_equal(got_o[:, :, i], wo[:, :, -1]) and np.array_equal(got_l[:, :, i], wl[:, :, -1]), (seed, n, i)
        if ps == [i - 1 for i in range(n)]:
            wo, wl = VM.block_merge(q, k, v, out_a, lse_a)
            assert np.array_equal(got_o, wo) and np.array_equal(got_l, wl)


def test_tree_model_edges():
    rs = np.random.RandomState(2)
    q, k, v, out_a, lse_a = _block(rs, 2, 4, 2, 5, 16)
    ps = [-1, 0, 0, 1, -1]
    masks = np.stack([TM.ancestor_masks(ps)] * 2)
    lse_a[0, 1, 2] = np.nan
    lse_a[0, 0] = -np.inf
    q[1, :, 2:], k[1, :, 2:], v[1, :, 2:] = np.nan, np.nan, np.nan
    dirty = masks.copy()
    dirty[1, 2:] = -1
    dirty[:, :] |= np.int32(-65536)                     # bits 16 .. 31
    for i in range(5):
        dirty[0, i] |= np.int32(-1 << (i + 1))          # every bit above i
    out, lse = TM.tree_block_merge(q, k, v, out_a, lse_a, dirty, n_valid=[5, 2])
    clean = TM.tree_block_merge(q, k, v, out_a, lse_a, masks, n_valid=[5, 2])
    assert np.array_equal(out, clean[0], equal_nan=True) and np.array_equal(lse, clean[1], equal_nan=True)
    assert np.isnan(out[0, 1, 2]).all() and np.isnan(lse[0, 1, 2]) and np.isfinite(out[0, 0]).all()
    assert np.isfinite(out[1, :, :2]).all() and not out[1, :, 2:].any() and np.all(np.isneginf(lse[1, :, 2:]))


# ---------------------------------------------------------------- the commit of chosen rows -----------------------------------
def test_commit_rows_model():
    ps, cap = 32, 32
    # r = 20 window rows, the path 0 -> 2 -> 5 -> ... of 16 rows: the flush takes the window and the first 12 path rows
    rows = [0, 2, 5, 6, 7, 8, 9, 10, 11, 12, 13, 14, 15, 3, 1, 4]
    T, r, start, coded, ring = TM.commit_rows(64, 20, 5, 16, ps, cap, rows, 16)
    assert (T, r, start) == (96, 4, 5)
    assert [coded[64 + j] for j in range(32)] == [("w", j) for j in range(20)] + [("n", x) for x in rows[:12]]
    assert VM.live_ring(ring, r, start, cap) == {5 + j: ("n", rows[12 + j]) for j in range(4)}
    # the identity gives million_window_commit; a clamped index; entries at or past a never matter
    for r0 in range(cap + 1):
        for a in range(7):
            want = VM.commit_closed(40, r0, 3, a, ps, cap)
            got = TM.commit_rows(40, r0, 3, a, ps, cap, list(range(a)) + [-1, 0x7FFFFFFF], 6)
            assert got[:4] == want[:4] and VM.live_ring(got[4], *got[1:3], cap) == VM.live_ring(want[4], *want[1:3], cap)
    got = TM.commit_rows(0, 0, 0, 3, ps, cap, [-7, 99, 2], 6)
    assert VM.live_ring(got[4], 3, 0, cap) == {0: ("n", 0), 1: ("n", 5), 2: ("n", 2)}


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


def _tm_call(lib, desc, q=A, k=A + 0x10000, v=A + 0x20000, out_a=A + 0x30000, lse_a=A + 0x40000, dev_n=None, dev_mask=A + 0x60000,
             out=A + 0x30000, lse_out=None, k_stage=None, v_stage=None):
    return lib.million_attn_tree_merge(ctypes.byref(desc), q, k, v, out_a, lse_a, dev_n, dev_mask, out, lse_out, k_stage, v_stage, None)


def test_tree_merge_refuses_without_a_gpu(lib):
    from million_amd import _lib as L
    assert L.SYMBOLS["million_attn_tree_merge"] == (ctypes.c_int32, [ctypes.POINTER(L.BlockMergeDesc)] + [ctypes.c_void_p] * 12)
    assert ctypes.sizeof(L.BlockMergeDesc) == 24 + 8 * 17      # the chain's desc, unchanged
    d = _bm_desc(L)
    d.struct_size -= 8
    assert _tm_call(lib, d) == ERR_ARG and b"struct_size" in lib.million_last_error()
    for n in (0, 17):
        assert _tm_call(lib, _bm_desc(L, n=n)) == ERR_SHAPE and b"n=" in lib.million_last_error()
    assert _tm_call(lib, _bm_desc(L, d=96)) == ERR_SHAPE and b"d=96" in lib.million_last_error()
    assert _tm_call(lib, _bm_desc(L, nh=7)) == ERR_SHAPE
    assert _tm_call(lib, _bm_desc(L), dev_mask=None) == ERR_ARG and b"null dev_mask" in lib.million_last_error()
    assert _tm_call(lib, _bm_desc(L), dev_mask=A + 2) == ERR_ALIGN and b"dev_mask" in lib.million_last_error()
    assert _tm_call(lib, _bm_desc(L), q=A + 8) == ERR_ALIGN and b"aligned" in lib.million_last_error()
    assert _tm_call(lib, _bm_desc(L), lse_a=A + 2) == ERR_ALIGN
    for part in ("q", "k", "v", "out_a", "lse_a", "out"):
        assert _tm_call(lib, _bm_desc(L), **{part: None}) == ERR_ARG and b"null" in lib.million_last_error(), part
    assert _tm_call(lib, _bm_desc(L), k_stage=A + 0x50000) == ERR_ARG and b"together" in lib.million_last_error()
    assert b"attn_tree_merge" in lib.million_last_error()
    d = _bm_desc(L)
    d.q_stride[2] = 132
    assert _tm_call(lib, d) == ERR_ALIGN and b"stride" in lib.million_last_error()


def _wc_desc(L, n_layers=2, bs=2, nhk=2, d=128, M=64, C=256, n_bound=4, ps=32, cap=64, n_pages_cap=8):
    desc = L.WindowCommitDesc()
    desc.struct_size = ctypes.sizeof(L.WindowCommitDesc)
    desc.n_layers, desc.bs, desc.nh_k, desc.d, desc.M, desc.C, desc.n_bound = n_layers, bs, nhk, d, M, C, n_bound
    desc.page_size, desc.n_pages_cap, desc.resid_cap = ps, n_pages_cap, cap
    desc.n_pool = n_layers * bs * nhk * n_pages_cap
    desc.new_stride_l, desc.new_stride_b, desc.new_stride_h, desc.new_stride_n = bs * nhk * 16 * d, nhk * 16 * d, 16 * d, d
    desc.ids_layer_stride, desc.rows_layer_stride, desc.lengths_layer_stride = bs * nhk * n_pages_cap, bs * nhk * cap * d, bs * 4
    return desc


_WC_ARGS = ("k_new", "v_new", "k_resid", "v_resid", "k_prep", "v_prep", "k_pool", "v_pool", "page_ids", "dev_lengths", "dev_n", "dev_rows")


def _wc_call(lib, desc, **over):
    args = {name: A + 0x10000 * i for i, name in enumerate(_WC_ARGS)}
    args.update(over)
    return lib.million_window_commit_rows(ctypes.byref(desc), *[args[name] for name in _WC_ARGS], None)


def test_window_commit_rows_refuses_without_a_gpu(lib):
    from million_amd import _lib as L
    assert L.SYMBOLS["million_window_commit_rows"] == (ctypes.c_int32, [ctypes.POINTER(L.WindowCommitDesc)] + [ctypes.c_void_p] * 13)
    assert ctypes.sizeof(L.WindowCommitDesc) == 48 + 8 * 7      # the desc of million_window_commit, unchanged
    d = _wc_desc(L)
    d.struct_size += 8
    assert _wc_call(lib, d) == ERR_ARG and b"struct_size" in lib.million_last_error()
    for n in (0, 17):
        assert _wc_call(lib, _wc_desc(L, n_bound=n, ps=64)) == ERR_SHAPE and b"n_bound" in lib.million_last_error()
    assert _wc_call(lib, _wc_desc(L, n_bound=33, ps=32)) == ERR_SHAPE and b"page_size=32" in lib.million_last_error()
    assert _wc_call(lib, _wc_desc(L, d=96)) == ERR_SHAPE and b"d=96" in lib.million_last_error()
    assert _wc_call(lib, _wc_desc(L), k_new=A + 8) == ERR_ALIGN and b"aligned" in lib.million_last_error()
    assert _wc_call(lib, _wc_desc(L), dev_n=A + 2) == ERR_ALIGN
    assert _wc_call(lib, _wc_desc(L), dev_rows=A + 2) == ERR_ALIGN and b"dev_rows" in lib.million_last_error()
    for part in _WC_ARGS:
        assert _wc_call(lib, _wc_desc(L), **{part: None}) == ERR_ARG and b"null" in lib.million_last_error(), part
    assert b"window_commit_rows: null dev_rows" in lib.million_last_error()
    d = _wc_desc(L)
    d.new_stride_n = 132
    assert _wc_call(lib, d) == ERR_ALIGN and b"stride" in lib.million_last_error()


def test_new_kernels_have_no_scratch_and_no_spills(lib):
    """tools/kernel_meta.py on the masked block merge (its LDS is the chain's: the K and V block) and on the commit of rows."""
    import pathlib
    import subprocess
    import sys
    root = pathlib.Path(__file__).resolve().parents[1]
    meta = lambda part: subprocess.run([sys.executable, str(root / "tools" / "kernel_meta.py"), str(root / "million_amd" / "libmillion_hip.so"), part],
                                       capture_output=True, text=True, check=True).stdout.splitlines()
    rows = [l for l in meta("attn_block_merge_kernel") if "attn_block_merge_kernel" in l]
    assert len(rows) == 4, rows                                   # d = 128 / 64, chain / tree
    for l in rows:
        assert l.rstrip().endswith("vgpr_spill 0 sgpr_spill 0 scratch 0 B"), l
        assert (" lds 8192 B " if "ILi128E" in l else " lds 4096 B ") in l, l
    rows = [l for l in meta("CommitRowsParams") if "CommitRowsParams" in l]
    assert len(rows) == 4 + 1, rows                               # the encode launch's d_m instances, the append kernel
    for l in rows:
        assert l.rstrip().endswith("vgpr_spill 0 sgpr_spill 0 scratch 0 B") and " lds 0 B " in l, l


# ---------------------------------------------------------------- the cache's host side ----------------------------------------
def _host_cache(monkeypatch, preallocate, log):
    """A PagedPQCache on the CPU with the launches of verify / commit stubbed: what is left is the host logic."""
    import torch
    from million_amd import ops
    from million_amd.pq_cache import PagedPQCache
    monkeypatch.setattr(ops, "decode_workspace_bytes", lambda *a, **k: 16)
    monkeypatch.setattr(ops, "pq_decode_attn", lambda q, *a, **k: (torch.zeros_like(q), torch.zeros(q.shape[0], q.shape[1], 1)))
    monkeypatch.setattr(ops, "pq_chunk_attn", lambda q, kc, vc, *a, **k: (log.append(("chunk", kc, vc)), (torch.zeros_like(q), torch.zeros(q.shape[:3])))[1])
    monkeypatch.setattr(ops, "attn_block_merge", lambda q, k, v, out_a, lse_a, dev_n, **kw: (log.append(("merge", kw.get("dev_mask"))), out_a)[1])
    monkeypatch.setattr(ops, "window_commit", lambda *a, **k: log.append(("commit", a[10].tolist(), k["n_bound"], k["dev_rows"].tolist() if "dev_rows" in k else None)))
    cache = PagedPQCache(bs=3, nh=8, num_key_value_heads=2, M=64, layer_num=2, d=128, page_size=32, extended_residual_size=64,
                         max_tokens=256, preallocate=preallocate, device="cpu")
    cache._kprep = cache._vprep = None
    return cache


def _host_verify(cache, n=5, n_draft=None, layers=None, **kw):
    import torch
    q, kv = torch.zeros(cache.bs, cache.nh, n, cache.d, dtype=torch.float16), torch.zeros(cache.bs, 2, n, cache.d, dtype=torch.float16)
    for l in range(cache.layer_num) if layers is None else layers:
        cache.verify(q, kv, kv, l, n_draft=n_draft, **kw)


def _snap(cache):
    return [a.copy() for a in (cache._T_a, cache._r_a, cache._rs_a, cache._seen_a, cache._pages_a)] + [set(cache.page_manager.free_pages)]


def _same(x, y):
    return all(np.array_equal(a, b) if isinstance(a, np.ndarray) else a == b for a, b in zip(x, y))


TREE = [-1, 0, 0, 1, -1]      # 0 -> {1 -> 3, 2}; 4 a second root


def test_verify_tree_refusals_and_record(monkeypatch):
    log = []
    cache = _host_cache(monkeypatch, True, log)
    before = _snap(cache)
    for bad, n in (([-1, 1, 0, 1, 2], 5),            # parent >= index
                   ([-1, 0, 2, 1, 2], 5),            # parent == index
                   ([-2, 0, 0, 1, 2], 5),            # parent < -1
                   ([-1, 0, 0, 1], 5),               # wrong length
                   ([-1, 0, 0, 1, -1, 2], 5),
                   ([TREE, TREE], 5),                # per-slot list of the wrong size
                   ([TREE] * 4, 5),
                   ([TREE, TREE, [-1, 0, 0, 3, 1]], 5)):
        with pytest.raises(RuntimeError, match="tree"):
            _host_verify(cache, n=n, layers=[0], tree=bad)
        assert cache._verify_rec is None and not log and _same(before, _snap(cache)), bad
    _host_verify(cache, tree=TREE)
    rec = cache._verify_rec
    assert rec["tree"] == (tuple(TREE),) * 3 and rec["layers"] == {0, 1}
    assert str(rec["dev_mask"].dtype) == "torch.int32" and rec["dev_mask"].tolist() == [TM.ancestor_masks(TREE).tolist()] * 3
    assert [e[0] for e in log] == ["merge", "merge"] and all(e[1] is rec["dev_mask"] for e in log)      # route "heads", masks made once
    _host_verify(cache, tree=[TREE] * 3)                  # the same tree per slot: the same record
    assert cache._verify_rec is rec
    _host_verify(cache, layers=[0], tree=[TREE, TREE, [-1] * 5])      # another tree: a new record, of one layer
    assert cache._verify_rec is not rec and cache._verify_rec["layers"] == {0}
    assert cache._verify_rec["dev_mask"][2].tolist() == [1, 2, 4, 8, 16]
    _host_verify(cache, layers=[0])                       # no tree: a new record again, and the unmasked call
    assert "tree" not in cache._verify_rec and log[-1] == ("merge", None)
    del log[:]
    _host_verify(cache, layers=[1], tree=TREE, route="chunk")      # chunk attention over the past only, then the masked merge
    assert log[0] == ("chunk", None, None) and log[1][0] == "merge" and log[1][1] is cache._verify_rec["dev_mask"]
    assert _same(before, _snap(cache))


def test_commit_path_refusals(monkeypatch):
    log = []
    cache = _host_cache(monkeypatch, False, log)
    cache._r_a[:] = 62
    before = _snap(cache)

    def refused(match, *a, **k):
        rec = cache._verify_rec
        layers = None if rec is None else set(rec["layers"])
        with pytest.raises(RuntimeError, match=match):
            cache.commit(*a, **k)
        assert _same(before, _snap(cache)) and not [e for e in log if e[0] == "commit"]
        assert cache._verify_rec is rec and (rec is None or rec["layers"] == layers)

    refused("verify", path=[[0], [], []])                             # no verification at all
    _host_verify(cache, layers=[0], tree=TREE)
    refused("every layer", path=[[0], [], []])
    _host_verify(cache, n_draft=[5, 0, 3], tree=TREE)
    refused("path", [1, 0, 0])                                        # a tree record needs path
    refused("path", path=[[1], [], []])                               # not starting at a root
    refused("path", path=[[0, 3], [], []])                            # a skipped ancestor
    refused("path", path=[[0, 1, 3, 4], [], []])                      # a second root below the chain
    refused("path", path=[[0, 1], [], [0, 1, 3]])                     # node 3 >= n_draft[2] = 3
    refused("n_accept", path=[[0], [0], []])                          # n_draft[1] = 0
    refused("path", path=[[0, 0], [], []])
    refused("path", path=[[-1], [], []])
    refused("n_accept", path=[[0], []])                               # one path per slot
    refused("path", [2, 0, 0], path=[[0, 1, 3], [], []])              # n_accept and path disagree
    refused("n_accept or path")
    cache._r_a[1, 0] += 1
    before = _snap(cache)
    refused("mid-step", path=[[0], [], []])
    cache._r_a[1, 0] -= 1
    before = _snap(cache)
    cache.commit([3, 0, 2], path=[[0, 1, 3], [], [0, 2]])             # both given and agreeing; the second flushes nothing
    assert log[-1] == ("commit", [3, 0, 2], 5, [[0, 1, 3, 0, 0], [0] * 5, [0, 2, 0, 0, 0]])
    assert cache._T_a[:, 0].tolist() == [32, 32] and cache._r_a[:, 0].tolist() == [33, 33] and cache._r_a[:, 2].tolist() == [64, 64]
    # a record without a tree: path only as range(a), and then today's call
    del log[:]
    before = _snap(cache)
    _host_verify(cache, n=4)
    refused("chain", path=[[0, 2], [], []])
    refused("chain", path=[[1], [], []])
    cache.commit(path=[[0, 1], [], [0]])
    assert log[-1] == ("commit", [2, 0, 1], 4, None)


@pytest.mark.parametrize("preallocate", [True, False])
def test_commit_path_moves_the_mirror_as_commit_len(monkeypatch, preallocate):
    log = []
    A_, B_ = _host_cache(monkeypatch, preallocate, log), _host_cache(monkeypatch, preallocate, log)
    ps = A_.page_size
    state = [(40, 62, 5, 102), (0, 0, 0, 0), (64, 64, 63, 128)]
    for cache in (A_, B_):
        for b, (T, r, st, seen) in enumerate(state):
            cache._T_a[:, b], cache._r_a[:, b], cache._rs_a[:, b], cache._seen_a[:, b] = T, r, st, seen
            if not preallocate:
                for l in range(cache.layer_num):
                    cache._assign_pages(l, -(-T // ps), b)
    rs = np.random.RandomState(5)
    for rnd in range(30):
        if max(int(A_._T_a[0, b]) for b in range(3)) + ps > A_.max_tokens:
            break
        trees = [TM.random_tree(int(rs.randint(100)), 6) for _ in range(3)]
        n_draft = [6, int(rs.randint(0, 7)), 6]
        path = [TM.random_path(rs, trees[b], n_draft[b]) for b in range(3)]
        _host_verify(A_, n=6, n_draft=n_draft, tree=trees)
        _host_verify(B_, n=6, n_draft=n_draft)
        A_.commit(path=path)
        if any(path):
            assert log[-1][1] == [len(p) for p in path] and [row[:len(p)] for row, p in zip(log[-1][3], path)] == path
        B_.commit([len(p) for p in path])
        assert _same(_snap(A_), _snap(B_)), (rnd, path)
        assert not any(path) or log[-1][3] is None
    assert rnd >= 10 and int(A_._T_a[0, 0]) >= 72      # slot 0 crossed a flush


# ---------------------------------------------------------------- greedy acceptance ---------------------------------------------
def test_greedy_path():
    from million_amd.spec_tree import greedy_path
    #        0        4
    #      1   2
    #      3   5
    ps = [-1, 0, 0, 1, -1, 2]
    draft = [7, 8, 9, 1, 6, 2]
    assert greedy_path(ps, draft, [8, 1, 2, 0, 0, 0], 6, 7) == [0, 1, 3]           # 0 (prev 7), 1 (target at 0: 8), 3 (target at 1: 1)
    assert greedy_path(ps, draft, [9, 1, 2, 0, 0, 0], 6, 7) == [0, 2, 5]           # the target at 0 says 9: the other child
    assert greedy_path(ps, draft, [9, 1, 2, 0, 0, 0], 5, 7) == [0, 2]              # node 5 is not live
    assert greedy_path(ps, draft, [5, 1, 2, 0, 0, 0], 6, 7) == [0]                 # no child matches
    assert greedy_path(ps, draft, [8, 1, 2, 0, 0, 0], 6, 6) == [4]                 # the previous token picks the other root
    assert greedy_path(ps, draft, [8, 1, 2, 0, 0, 0], 6, 3) == []                  # no root matches
    assert greedy_path(ps, draft, [8, 1, 2, 0, 0, 0], 0, 7) == []
    # ties: two roots with the same token, two children with the same token - the lowest index wins
    assert greedy_path([-1, -1], [4, 4], [0, 0], 2, 4) == [0]
    assert greedy_path([-1, 0, 0], [4, 5, 5], [5, 0, 0], 3, 4) == [0, 1]
    assert greedy_path([-1, 0, 0, 2], [4, 5, 5, 6], [5, 0, 6, 0], 4, 4) == [0, 2, 3]      # but a longer chain beats a lower index
    assert greedy_path([-1, -1, 0, 1], [4, 4, 5, 5], [5, 5, 0, 0], 4, 4) == [0, 2]        # equal lengths: the chain ending lowest
    # a chain: the accepted prefix
    assert greedy_path([-1, 0, 1, 2], [1, 2, 3, 4], [2, 3, 9, 9], 4, 1) == [0, 1, 2]
    # a rejected parent hides an accepted-looking child
    assert greedy_path([-1, 0, 1], [1, 2, 3], [9, 3, 0], 3, 1) == [0]
