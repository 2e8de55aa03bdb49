"""CPU side of the sink rows (include/million_hip.h, "Sink rows"): the entry exists with its argument types and the struct has the
header's layout, every refusal happens before any HIP call with its status, the fp64 model of the formula is lse_ref.merge of two
explicit parts, the constructors refuse what they must, and the host logic of a PagedPQCache with sink_tokens - on a CPU cache with
the launches stubbed - takes, forks and drops the sink rows and their counts."""
import ctypes
import subprocess
import tempfile
from pathlib import Path

import numpy as np
import pytest

from tests import lse_ref as R
from tests import sink_model as SM

ROOT = Path(__file__).resolve().parents[1]
ERR_ARG, ERR_SHAPE, ERR_ALIGN = -3, -1, -2
A = 0x100000      # made-up aligned device addresses: a refused call dereferences nothing


@pytest.fixture(scope="module")
def lib():
    from million_amd import build, _lib
    build.build()
    return _lib.load()


def _desc(L, bs=2, nh=8, nhk=2, n=4, d=128, s_cap=4, n_sink=4):
    desc = L.SinkMergeDesc()
    desc.struct_size = ctypes.sizeof(L.SinkMergeDesc)
    desc.bs, desc.nh, desc.nh_k, desc.n, desc.d, desc.s_cap, desc.n_sink = bs, nh, nhk, n, d, s_cap, n_sink
    for arr in (desc.q_stride, desc.a_stride, desc.o_stride):
        arr[0], arr[1], arr[2] = nh * n * d, n * d, d
    desc.sink_stride_b, desc.sink_stride_h = nhk * s_cap * d, s_cap * d
    return desc


def _call(lib, desc, q=A, k=A + 0x10000, v=A + 0x20000, out_a=A + 0x30000, lse_a=A + 0x40000, dev_s=None, dev_n=None,
          out=A + 0x30000, lse_out=None):
    return lib.million_attn_sink_merge(ctypes.byref(desc), q, k, v, out_a, lse_a, dev_s, dev_n, out, lse_out, None)


def test_symbol_and_struct(lib):
    from million_amd import _lib as L
    assert L.SYMBOLS["million_attn_sink_merge"] == (ctypes.c_int32, [ctypes.POINTER(L.SinkMergeDesc)] + [ctypes.c_void_p] * 10)
    assert lib.million_attn_sink_merge.restype is ctypes.c_int32
    assert ctypes.sizeof(L.SinkMergeDesc) == 32 + 8 * 11
    src = ('#include "million_hip.h"\n#include <stdio.h>\n#include <stddef.h>\nint main(){printf("%zu %zu %zu %zu\\n", '
           'sizeof(million_sink_merge_desc), offsetof(million_sink_merge_desc, n_sink), offsetof(million_sink_merge_desc, q_stride), '
           'offsetof(million_sink_merge_desc, sink_stride_h));return 0;}\n')
    with tempfile.TemporaryDirectory() as td:
        (Path(td) / "a.c").write_text(src)
        subprocess.check_call(["gcc", "-std=c11", "-I", str(ROOT / "include"), "-o", f"{td}/a", f"{td}/a.c"])
        size, o_ns, o_q, o_sh = map(int, subprocess.check_output([f"{td}/a"]).split())
    D = L.SinkMergeDesc
    assert (size, o_ns, o_q, o_sh) == (ctypes.sizeof(D), D.n_sink.offset, D.q_stride.offset, D.sink_stride_h.offset)


def test_sink_merge_refuses_without_a_gpu(lib):
    from million_amd import _lib as L
    err = lib.million_last_error
    d = _desc(L)
    d.struct_size -= 8
    assert _call(lib, d) == ERR_ARG and b"struct_size" in err()
    assert lib.million_attn_sink_merge(None, A, A, A, A, A, None, None, A, None, None) == ERR_ARG
    for n in (0, -3):
        assert _call(lib, _desc(L, n=n)) == ERR_SHAPE and b"n=" in err()
    for d_ in (96, 0, 256):
        assert _call(lib, _desc(L, d=d_)) == ERR_SHAPE and b"d=" in err()
    for s_cap in (0, 65, -1):
        assert _call(lib, _desc(L, s_cap=s_cap, n_sink=0)) == ERR_SHAPE and b"s_cap=" in err()
    for n_sink in (-1, 5):
        assert _call(lib, _desc(L, n_sink=n_sink)) == ERR_SHAPE and b"n_sink=" in err()
    assert _call(lib, _desc(L, n_sink=5), dev_s=A + 0x50000) == ERR_SHAPE      # validated whether or not it is used
    assert _call(lib, _desc(L, nh=7)) == ERR_SHAPE and b"nh_k" in err()
    assert _call(lib, _desc(L, bs=0)) == ERR_SHAPE
    for part in ("q", "k", "v", "out_a", "lse_a", "out"):
        assert _call(lib, _desc(L), **{part: None}) == ERR_ARG and b"null" in err(), part
    for part in ("q", "k", "v", "out_a", "out"):
        assert _call(lib, _desc(L), **{part: A + 0x60008}) == ERR_ALIGN and b"16-byte" in err(), part
    for part in ("lse_a", "lse_out", "dev_s", "dev_n"):
        assert _call(lib, _desc(L), **{part: A + 0x60002}) == ERR_ALIGN and b"4-byte" in err(), part
    for name in ("q_stride", "a_stride", "o_stride"):
        for k in range(3):
            d = _desc(L)
            getattr(d, name)[k] += 4
            assert _call(lib, d) == ERR_ALIGN and b"stride" in err(), (name, k)
    for name in ("sink_stride_b", "sink_stride_h"):
        d = _desc(L)
        setattr(d, name, getattr(d, name) + 2)
        assert _call(lib, d) == ERR_ALIGN and b"stride" in err(), name
    # the grid: bs * nh * ceil(n / 16) single-wave workgroups must fit an int
    assert _call(lib, _desc(L, bs=1 << 20, nh=1 << 10, nhk=1 << 10, n=17 * 16)) == ERR_SHAPE and b"workgroups" in err()
    assert _call(lib, _desc(L, bs=1 << 20, nh=1 << 10, nhk=1 << 10, n=2 * 16)) == ERR_SHAPE
    # a shape error is reported before a null pointer, a null pointer before an alignment
    assert _call(lib, _desc(L, d=96), q=None) == ERR_SHAPE
    assert _call(lib, _desc(L), q=None, k=A + 8) == ERR_ARG


# ---------------------------------------------------------------- the model ------------------------------------------------
@pytest.mark.parametrize("bs,nh,nhk,n,d,s_cap,n_past", [(2, 8, 2, 5, 128, 4, 77), (1, 4, 4, 17, 64, 64, 300), (3, 7, 1, 1, 128, 9, 0)])
def test_model_is_the_merge_of_two_parts_and_the_softmax_over_all_keys(bs, nh, nhk, n, d, s_cap, n_past):
    rs = np.random.RandomState(n + d + s_cap)
    q = rs.standard_normal((bs, nh, n, d))
    ks, vs = rs.standard_normal((bs, nhk, s_cap, d)), rs.standard_normal((bs, nhk, s_cap, d))
    Kp, Vp = rs.standard_normal((bs, nhk, n_past, d)), rs.standard_normal((bs, nhk, n_past, d))
    out_a, lse_a = R.attend(q, Kp, Vp)
    s_valid = [s_cap, 1, 0][:bs]
    got_o, got_l = SM.sink_merge(q, ks, vs, out_a, lse_a, s_valid=s_valid)
    for b in range(bs):
        sb = s_valid[b]
        so, sl = R.attend(q[b:b + 1], ks[b:b + 1, :, :sb], vs[b:b + 1, :, :sb])
        mo, ml = R.merge([out_a[b:b + 1], so], [lse_a[b:b + 1], sl])
        assert np.abs(mo[0] - got_o[b]).max() <= 1e-12
        assert np.array_equal(np.isneginf(ml[0]), np.isneginf(got_l[b]))
        fin = np.isfinite(ml[0])
        assert np.abs(ml[0][fin] - got_l[b][fin]).max() <= 1e-12 if fin.any() else True
        wo, wl = R.attend(q[b:b + 1], np.concatenate([ks[b:b + 1, :, :sb], Kp[b:b + 1]], axis=2),
                          np.concatenate([vs[b:b + 1, :, :sb], Vp[b:b + 1]], axis=2))
        assert np.abs(wo[0] - got_o[b]).max() <= 1e-12
        if fin.any():
            assert np.abs(wl[0][fin] - got_l[b][fin]).max() <= 1e-12


def test_model_edges():
    rs = np.random.RandomState(5)
    bs, nh, nhk, n, d, s_cap = 4, 4, 2, 3, 64, 4
    q, ks, vs = rs.standard_normal((bs, nh, n, d)), rs.standard_normal((bs, nhk, s_cap, d)), rs.standard_normal((bs, nhk, s_cap, d))
    out_a, lse_a = rs.standard_normal((bs, nh, n, d)), rs.standard_normal((bs, nh, n))
    lse_a[0, 1, 2] = np.nan
    lse_a[1] = -np.inf
    out_a[1] = 1e30                            # a -inf part's out is never used
    ks[2, :, 1:], vs[2, :, 1:] = np.nan, np.nan      # sink rows past s_b reach nothing
    q[3, :, 1:], out_a[3, :, 1:] = np.nan, np.nan    # query rows past n_b reach nothing
    out, lse = SM.sink_merge(q, ks, vs, out_a, lse_a, s_valid=[4, 4, 1, -5], n_valid=[3, 3, 3, 1])
    assert np.isnan(out[0, 1, 2]).all() and np.isnan(lse[0, 1, 2])
    assert np.isfinite(np.delete(out[0].reshape(-1, d), 1 * n + 2, 0)).all()
    own, own_l = R.attend(q[1:2], ks[1:2], vs[1:2])                       # pure sink attention
    assert np.abs(out[1] - own[0]).max() <= 1e-12 and np.abs(lse[1] - own_l[0]).max() <= 1e-12
    assert np.isfinite(out[2]).all() and np.isfinite(lse[2]).all()
    assert np.array_equal(out[3, :, 0], out_a[3, :, 0]) and np.array_equal(lse[3, :, 0], lse_a[3, :, 0])      # s_b = 0: the identity
    assert np.all(out[3, :, 1:] == 0) and np.all(np.isneginf(lse[3, :, 1:]))
    # no past and no sink: zeros, -inf
    out, lse = SM.sink_merge(q[:1], ks[:1], vs[:1], out_a[:1], np.full_like(lse_a[:1], -np.inf), s_valid=[0])
    assert np.all(out == 0) and np.all(np.isneginf(lse))
    # garbage counts are clamped
    a = SM.sink_merge(q[:1], ks[:1], vs[:1], out_a[:1], lse_a[:1] * 0, s_valid=[1000], n_valid=[99])
    b = SM.sink_merge(q[:1], ks[:1], vs[:1], out_a[:1], lse_a[:1] * 0, s_valid=[s_cap], n_valid=[n])
    assert np.array_equal(a[0], b[0], equal_nan=True) and np.array_equal(a[1], b[1], equal_nan=True)


def test_request_model_orders_its_keys():
    r = SM.Request(4, 2, 8)
    rows = np.arange(2 * 10 * 8, dtype=np.float16).reshape(2, 10, 8)
    r.store(rows[:, :7], rows[:, :7])
    r.append(rows[:, 7:], rows[:, 7:])
    assert (r.s, r.seen) == (4, 10)
    deq = -np.ones((2, 3, 8))      # rows 4 .. 6 are codes
    K, _ = r.keys(deq, deq)
    assert K.shape == (2, 10, 8) and np.array_equal(K[:, :4], rows[:, :4]) and np.all(K[:, 4:7] == -1) and np.array_equal(K[:, 7:], rows[:, 7:])
    late = SM.Request(4, 2, 8)
    late.append(rows[:, :1], rows[:, :1])      # first token by a decode step: no sinks, ever
    late.store(rows[:, 1:5], rows[:, 1:5])
    assert late.s == 0
    short = SM.Request(4, 2, 8)
    short.store(rows[:, :3], rows[:, :3])
    assert short.s == 3
    m = SM.causal_tail_mask(3, 8)
    assert m[:, :5].all() and np.array_equal(m[:, 5:], np.tril(np.ones((3, 3), bool)))
    t = SM.tree_tail_mask([-1, 0, 0, 1], 6)
    assert np.array_equal(t[:, 2:].astype(int), [[1, 0, 0, 0], [1, 1, 0, 0], [1, 0, 1, 0], [1, 1, 0, 1]])


# ---------------------------------------------------------------- constructors ---------------------------------------------
KW = dict(bs=2, nh=4, num_key_value_heads=2, M=64, layer_num=2, d=128, page_size=64, extended_residual_size=64, max_tokens=512,
          device="cpu")


@pytest.mark.parametrize("bad", [-1, 65, 1000, 2.5, True])
def test_constructor_refuses_sink_tokens_outside_0_64(bad):
    from million_amd.pq_cache import PagedPQCache
    with pytest.raises(ValueError, match="sink_tokens"):
        PagedPQCache(**KW, sink_tokens=bad)


def test_constructor_default_allocates_nothing():
    from million_amd.pq_cache import PagedPQCache
    c = PagedPQCache(**KW)
    assert c.sink_tokens == 0 and c._ksink_all is None and c._vsink_all is None and c._sink_all is None
    st = c.get_cache_stats()
    assert st["memory_breakdown"]["sink_memory_mb"] == 0 and st["sink_tokens"] == 0
    for S in (1, 64):
        c = PagedPQCache(**KW, sink_tokens=S)
        assert tuple(c._ksink_all.shape) == tuple(c._vsink_all.shape) == (2, 2, 2, S, 128) and c._ksink_all.dtype.is_floating_point
        assert tuple(c._sink_all.shape) == (2, 2) and str(c._sink_all.dtype) == "torch.int32" and c._sink_a.shape == (2, 2)
        st = c.get_cache_stats()
        assert st["memory_breakdown"]["sink_memory_mb"] == 2 * 2 * 2 * 2 * S * 128 * 2 / 2 ** 20
        assert st["total_memory_usage_mb"] == st["memory_breakdown"]["total_memory_mb"] >= st["memory_breakdown"]["sink_memory_mb"]


def test_dynamic_cache_refuses_sink_tokens():
    from million_amd.pq_cache import DynamicPQCache
    with pytest.raises(NotImplementedError, match="sink_tokens"):
        DynamicPQCache(bs=1, nh=4, num_key_value_heads=2, M=64, layer_num=1, device="cpu", sink_tokens=4)


# ---------------------------------------------------------------- host logic of the cache, launches stubbed ----------------
def _host_cache(monkeypatch, S=4, preallocate=True, log=None):
    import torch
    from million_amd import ops
    from million_amd.pq_cache import PagedPQCache
    log = [] if log is None else log
    monkeypatch.setattr(ops, "pq_encode_into", lambda X, *a, **k: log.append(("encode", k["n"], tuple(X.shape), k["token_start"])))
    monkeypatch.setattr(ops, "prefill_attn", lambda q, k, v, **kw: torch.zeros_like(q))
    monkeypatch.setattr(ops, "cache_fork", lambda *a, **k: log.append(("fork",)))
    cache = PagedPQCache(**dict(KW, preallocate=preallocate), sink_tokens=S)
    cache.key_cent = cache.value_cent = cache._kprep = cache._vprep = None
    return cache, log


def _rows(seed, n, nk=2, d=128):
    import torch
    g = torch.Generator().manual_seed(seed)
    return torch.randn(1, nk, n, d, generator=g).half(), torch.randn(1, nk, n, d, generator=g).half()


@pytest.mark.parametrize("preallocate", [True, False])
def test_store_takes_the_sinks_once(monkeypatch, preallocate):
    import torch
    cache, log = _host_cache(monkeypatch, preallocate=preallocate)
    q = torch.zeros(1, 4, 70, 128, dtype=torch.float16)
    k0, v0 = _rows(1, 70)
    k1, v1 = _rows(2, 3)
    for l in range(2):
        cache.prefill_request(0, q, k0, v0, l)
        cache.prefill_request(1, q[:, :, :3], k1, v1, l)
    assert cache._sink_a.tolist() == [[4, 3], [4, 3]] and cache._sink_all.tolist() == [[4, 3], [4, 3]]
    assert cache._T_a.tolist() == [[66, 0], [66, 0]] and cache._seen_a.tolist() == [[70, 3], [70, 3]] and not cache._r_a.any()
    assert cache.lengths[0].tolist() == [[66, 0, 0, 0], [0, 0, 0, 0]]
    # only the rows behind the sinks are encoded, behind token 0; a prompt of no more rows than sinks encodes nothing
    assert [e for e in log if e[0] == "encode"] == [("encode", 66, (1, 2, 66, 128), 0)] * 4
    for l in range(2):
        assert torch.equal(cache._ksink_all[l][0], k0[0, :, :4]) and torch.equal(cache._vsink_all[l][0], v0[0, :, :4])
        assert torch.equal(cache._ksink_all[l][1, :, :3], k1[0]) and not cache._ksink_all[l][1, :, 3].any()
    # a slot that holds nothing but sinks is not empty
    with pytest.raises(RuntimeError, match="empty slot"):
        cache.prefill_request(1, q[:, :, :3], k1, v1, 0)
    st = cache.get_cache_stats()
    assert st["sink_rows_live"] == 14
    # release: the count returns to zero, host and device, in every layer; the next prompt takes its own sinks
    cache.release(1)
    assert cache._sink_a.tolist() == [[4, 0], [4, 0]] and cache._sink_all.tolist() == [[4, 0], [4, 0]] and not cache._seen_a[:, 1].any()
    k2, v2 = _rows(3, 2)
    for l in range(2):
        cache.prefill_request(1, q[:, :, :2], k2, v2, l)
    assert cache._sink_a[:, 1].tolist() == [2, 2] and cache._sink_all[:, 1].tolist() == [2, 2] and cache._seen_a[:, 1].tolist() == [2, 2]
    cache.cleanup()
    assert not cache._sink_a.any() and not cache._sink_all.any() and not cache._seen_a.any() and not cache._ksink_all.any()


@pytest.mark.parametrize("n_tokens", [None, 0, 40])
def test_fork_copies_the_sinks(monkeypatch, n_tokens):
    import torch
    cache, log = _host_cache(monkeypatch)
    q = torch.zeros(1, 4, 70, 128, dtype=torch.float16)
    k0, v0 = _rows(1, 70)
    for l in range(2):
        cache.prefill_request(0, q, k0, v0, l)
    cache.fork(0, 1, n_tokens=n_tokens)
    assert ("fork",) in log
    T = 66 if n_tokens is None else n_tokens
    assert cache._sink_a.tolist() == [[4, 4], [4, 4]] and cache._sink_all.tolist() == [[4, 4], [4, 4]]
    assert cache._T_a[:, 1].tolist() == [T, T] and cache._seen_a[:, 1].tolist() == [T + 4, T + 4]      # n_tokens: coded tokens; every sink kept
    assert cache._seen_a[:, 0].tolist() == [70, 70]
    assert torch.equal(cache._ksink_all[:, 1], cache._ksink_all[:, 0]) and torch.equal(cache._vsink_all[:, 1], cache._vsink_all[:, 0])
    assert torch.equal(cache._ksink_all[1][1], k0[0, :, :4])


def test_out_of_scope_calls_name_sink_tokens(monkeypatch):
    import torch
    from million_amd.shared_prefix import SharedPrefix
    cache, _ = _host_cache(monkeypatch)
    plain, _ = _host_cache(monkeypatch, S=0)
    for call in (lambda: cache.swap_out(0), lambda: cache.snapshot_request(0), lambda: cache.swap_in(0, None),
                 lambda: SharedPrefix(cache, 0, plain), lambda: SharedPrefix(plain, 0, cache)):
        with pytest.raises(NotImplementedError, match="sink_tokens"):
            call()
    q, k = torch.zeros(2, 4, 5, 128, dtype=torch.float16), torch.zeros(2, 2, 5, 128, dtype=torch.float16)
    for form in (cache.prefill_ragged, cache.extend_ragged):
        with pytest.raises(NotImplementedError, match="sink_tokens"):
            form(q, k, k, 0, [5, 2], device_store=True)
    assert not cache._seen_a.any() and not cache._sink_a.any()
