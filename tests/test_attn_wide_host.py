"""CPU side of the decode step over uint16 codes (include/million_hip.h, million_pq_decode_attn_wide): the fp64 model
of the GPU tests agrees with the oracle's own forms, the new entries refuse what they must before any HIP call and the uint8
entries answer what they always did, ops refuses before the library is entered, and the host logic of a PagedPQCache with nbits
9 .. 12 - on a CPU cache with the launches stubbed - refuses the follow-ups by name, leaves an nbits = 8 cache as it was and follows
oracle.PagedPolicy across two flushes."""
import ctypes

import numpy as np
import pytest

from tests import wide_model as W

ERR_ARG, ERR_SHAPE, ERR_ALIGN, ERR_WORKSPACE = -3, -1, -2, -4
A = 0x100000      # made-up aligned device addresses: a refused call dereferences nothing


@pytest.fixture(scope="module")
def lib():
    from million_amd import build, _lib
    build.build()
    return _lib.load()


# ---------------------------------------------------------------- the model ------------------------------------------------
def _inputs(C, dtype, seed, bs=2, nh=8, nhk=2, d=128, M=64, T=45, cap=32):
    rs = np.random.RandomState(seed)
    return dict(q=rs.standard_normal((bs, nh, 1, d)).astype(np.float16), k_codes=rs.randint(0, C, (bs, nhk, T, M)).astype(dtype),
                v_codes=rs.randint(0, C, (bs, nhk, T, M)).astype(dtype), k_cents=rs.standard_normal((M, C, d // M)).astype(np.float16),
                v_cents=rs.standard_normal((M, C, d // M)).astype(np.float16), k_res=rs.standard_normal((bs, nhk, cap, d)).astype(np.float16),
                v_res=rs.standard_normal((bs, nhk, cap, d)).astype(np.float16))


@pytest.mark.parametrize("C,d,M", [(1024, 128, 64), (4096, 128, 32), (2048, 64, 16)])
def test_model_agrees_with_the_dense_numpy_oracle_at_uint16(oracle, C, d, M):
    x = _inputs(C, np.uint16, C, d=d, M=M)
    assert x["k_codes"].max() >= 256
    for r in (0, 7, 32):
        ref = oracle.decode_attn_dense_numpy(x["q"], x["k_codes"], x["v_codes"], x["k_cents"], x["v_cents"], x["k_res"], x["v_res"], r)
        out, lse = W.decode_attn(x["q"], x["k_codes"], x["v_codes"], x["k_cents"], x["v_cents"], x["k_res"], x["v_res"], r)
        assert out.shape == ref.shape and np.abs(out - ref).max() < 1e-12 and np.isfinite(lse).all()


def test_model_agrees_with_the_c_oracle_at_256_centroids(oracle):
    x = _inputs(256, np.uint8, 3)
    for r in (1, 32):
        ref, ref_l = oracle.decode_attn(x["q"], x["k_codes"], x["v_codes"], x["k_cents"], x["v_cents"], x["k_res"], x["v_res"], r, return_lse=True)
        out, lse = W.decode_attn(x["q"], x["k_codes"].astype(np.uint16), x["v_codes"].astype(np.uint16), x["k_cents"], x["v_cents"],
                                 x["k_res"], x["v_res"], r)
        assert np.abs(out - ref).max() < 5e-6 and np.abs(lse - ref_l).max() < 5e-6


def test_model_ring_append_and_empty():
    x = _inputs(512, np.uint16, 4, T=9, cap=8)
    new_k, new_v = x["k_res"][:, :, 2:3], x["v_res"][:, :, 2:3]
    a, la = W.decode_attn(x["q"], x["k_codes"], x["v_codes"], x["k_cents"], x["v_cents"], x["k_res"], x["v_res"], 5, T=[9, 4], start=[6, 5])
    for b, (T, st) in enumerate(((9, 6), (4, 5))):
        rows = [(st + i) % 8 for i in range(5)]
        o, l = W.decode_attn(x["q"][b:b + 1], x["k_codes"][b:b + 1, :, :T], x["v_codes"][b:b + 1, :, :T], x["k_cents"], x["v_cents"],
                             x["k_res"][b:b + 1][:, :, rows], x["v_res"][b:b + 1][:, :, rows], 5)
        assert np.array_equal(o[0], a[b]) and np.array_equal(l[0], la[b])
    # the appended row is one more window row behind the ring
    o1, l1 = W.decode_attn(x["q"], x["k_codes"], x["v_codes"], x["k_cents"], x["v_cents"], x["k_res"], x["v_res"], 2, start=0, k_new=new_k, v_new=new_v)
    o2, l2 = W.decode_attn(x["q"], x["k_codes"], x["v_codes"], x["k_cents"], x["v_cents"], x["k_res"], x["v_res"], 3, start=0)
    assert np.array_equal(o1, o2) and np.array_equal(l1, l2)
    o, l = W.decode_attn(x["q"], x["k_codes"], x["v_codes"], x["k_cents"], x["v_cents"], x["k_res"], x["v_res"], 0, T=0)
    assert not o.any() and np.isneginf(l).all()


# ---------------------------------------------------------------- the C ABI ------------------------------------------------
def _desc(L, C=1024, nh=8, nhk=2, d=128, M=64, k_layout=1, v_layout=1, T=4133, r=3):
    x = L.AttnDesc()
    x.struct_size = ctypes.sizeof(L.AttnDesc)
    x.bs, x.nh, x.nh_k, x.d, x.M, x.C = 2, nh, nhk, d, M, C
    x.n_tokens, x.r, x.resid_start, x.resid_cap = T, r, 0, 128
    x.resid_stride_b, x.resid_stride_h = nhk * 128 * d, 128 * d
    x.k_layout, x.v_layout, x.page_size, x.n_pages_cap = k_layout, v_layout, 64, 70
    return x


def _call(lib, desc, **kw):
    a = dict(q=A, k_new=None, v_new=None, k_codes=A + 0x10000, v_codes=A + 0x20000, k_ids=A + 0x30000, v_ids=A + 0x30000,
             k_cents=A + 0x40000, v_cents=A + 0x50000, k_res=A + 0x60000, v_res=A + 0x70000, out=A + 0x80000, lse=None, ws=A + 0x90000,
             ws_bytes=1 << 30)
    a.update(kw)
    return lib.million_pq_decode_attn_wide(ctypes.byref(desc), a["q"], a["k_new"], a["v_new"], a["k_codes"], a["v_codes"], a["k_ids"],
                                           a["v_ids"], a["k_cents"], a["v_cents"], a["k_res"], a["v_res"], a["out"], a["lse"], a["ws"],
                                           a["ws_bytes"], None)


REFUSED_SHAPES = [dict(C=256), dict(C=300), dict(k_layout=0), dict(v_layout=0), dict(nh=34)]      # the last: nh / nh_k = 17


def test_symbols(lib):
    from million_amd import _lib as L
    vp = ctypes.c_void_p
    assert L.SYMBOLS["million_pq_decode_attn_wide"] == (ctypes.c_int32, [ctypes.POINTER(L.AttnDesc)] + [vp] * 14 + [ctypes.c_size_t, vp])
    assert L.SYMBOLS["million_attn_wide_splits"] == (ctypes.c_int32, [ctypes.POINTER(L.AttnDesc)])
    assert L.SYMBOLS["million_attn_wide_workspace_bytes"] == (ctypes.c_size_t, [ctypes.POINTER(L.AttnDesc)])
    header = (L.HERE.parent / "include" / "million_hip.h").read_text()
    for name in ("million_pq_decode_attn_wide", "million_attn_wide_splits", "million_attn_wide_workspace_bytes"):
        assert name + "(" in header and hasattr(lib, name)


def test_wide_entry_refuses_without_a_gpu(lib):
    from million_amd import _lib as L
    err = lib.million_last_error
    d = _desc(L)
    d.struct_size -= 8
    assert _call(lib, d) == ERR_ARG and b"struct_size" in err()
    assert lib.million_attn_wide_splits(ctypes.byref(d)) == -1 and lib.million_attn_wide_workspace_bytes(ctypes.byref(d)) == 0
    assert lib.million_pq_decode_attn_wide(None, *([None] * 14), 0, None) == ERR_ARG
    for kw in REFUSED_SHAPES:
        d = _desc(L, **kw)
        assert lib.million_pq_decode_attn_wide(ctypes.byref(d), *([None] * 14), 0, None) == ERR_SHAPE, kw      # before any null pointer
        assert _call(lib, d) == ERR_SHAPE and b"attn_wide" in err(), kw
        assert lib.million_attn_wide_splits(ctypes.byref(d)) == -1, kw
        assert lib.million_attn_wide_workspace_bytes(ctypes.byref(d)) == 0, kw
    for kw in (dict(d=128, M=16), dict(d=128, M=128), dict(d=96, M=48), dict(C=8192), dict(C=65536)):
        assert _call(lib, _desc(L, **kw)) == ERR_SHAPE, kw
    for kw in (dict(), dict(C=512), dict(C=4096, M=32), dict(d=64, M=32, C=2048), dict(d=64, M=16), dict(nh=32), dict(nh=2)):
        d = _desc(L, **kw)
        assert lib.million_pq_decode_attn_wide(ctypes.byref(d), *([None] * 14), 0, None) == ERR_ARG and b"null" in err(), kw
        assert lib.million_attn_wide_splits(ctypes.byref(d)) >= 2 and lib.million_attn_wide_workspace_bytes(ctypes.byref(d)) > 0, kw
    assert lib.million_attn_wide_splits(ctypes.byref(_desc(L, T=0))) == 1
    d = _desc(L)
    for part in ("q", "k_cents", "v_cents", "k_res", "v_res", "out", "ws", "k_codes", "v_codes", "k_ids", "v_ids"):
        assert _call(lib, d, **{part: None}) == ERR_ARG, part
    assert _call(lib, _desc(L, T=0), k_codes=None, v_codes=None, k_ids=None, v_ids=None, ws_bytes=0) == ERR_WORKSPACE      # T = 0 needs no codes
    assert _call(lib, d, k_new=A + 0xa0000) == ERR_ARG and b"k_new" in err()
    assert _call(lib, _desc(L, r=128), k_new=A + 0xa0000, v_new=A + 0xb0000) == ERR_ARG and b"full window" in err()
    assert _call(lib, d, ws_bytes=lib.million_attn_wide_workspace_bytes(ctypes.byref(d)) - 1) == ERR_WORKSPACE
    for part in ("q", "k_codes", "v_codes", "k_res", "v_res", "out", "ws"):
        assert _call(lib, d, **{part: A + 0xc0008}) == ERR_ALIGN and b"16-byte" in err(), part
    # a codebook is aligned to one entry: 4 bytes at d_m = 2, 8 bytes at d_m = 4
    assert _call(lib, d, k_cents=A + 0x40002) == ERR_ALIGN and b"entry" in err()
    assert _call(lib, _desc(L, M=32), v_cents=A + 0x40004) == ERR_ALIGN
    assert _call(lib, d, lse=A + 0xd0002) == ERR_ALIGN and b"lse" in err()
    bad = _desc(L)
    bad.n_pages_cap = 10
    assert _call(lib, bad) == ERR_ARG and b"n_pages_cap" in err()
    bad = _desc(L)
    bad.page_size = 48
    assert _call(lib, bad) == ERR_SHAPE


def test_uint8_entries_answer_what_they_did(lib):
    from million_amd import _lib as L
    d = _desc(L, C=512)
    assert lib.million_attn_kernel_kind(ctypes.byref(d)) == -1
    assert lib.million_pq_decode_attn(ctypes.byref(d), *([A] * 10), A, 1 << 30, None) == ERR_SHAPE and b"uint8 codes" in lib.million_last_error()
    assert lib.million_attn_kernel_kind(ctypes.byref(_desc(L, C=256))) == 1
    assert lib.million_attn_kernel_kind(ctypes.byref(_desc(L, C=256, d=64, M=16, T=0))) == 3
    assert lib.million_prepare_cents(A, 64, 512, 2, A, None) == ERR_SHAPE


def test_ops_refuse_before_the_library(monkeypatch):
    import torch
    from million_amd import ops
    monkeypatch.setattr(ops.L, "load", lambda: pytest.fail("the library was entered"))
    q, res = torch.zeros(1, 4, 1, 128, dtype=torch.float16), torch.zeros(1, 2, 64, 128, dtype=torch.float16)
    pool = torch.zeros(4, 64, 64, dtype=torch.uint16)
    cents = torch.zeros(64, 1024, 2, dtype=torch.float16)
    ids = torch.zeros(1, 2, 2, dtype=torch.int32)
    with pytest.raises(RuntimeError, match="device tensors"):
        ops.pq_decode_attn_wide(q, pool, pool.transpose(1, 2).contiguous(), cents, cents, res, res, 0, n_tokens=0, page_ids=ids, page_size=64)
    with pytest.raises(RuntimeError, match="codes must be uint8"):      # the uint8 op keeps its message for uint16 codes
        monkeypatch.setattr(ops, "_need_cuda", lambda *a: None)
        ops.pq_decode_attn(q, pool, pool, cents, cents, res, res, 0, M=64, C=1024, k_page_ids=ids, v_page_ids=ids, page_size=64, n_tokens=0)
    vpool = pool.transpose(1, 2).contiguous()
    wide = lambda **kw: ops.pq_decode_attn_wide(*[kw.get(n, v) for n, v in (("q", q), ("k_pool", pool), ("v_pool", vpool), ("k_cents", cents),
                                                                          ("v_cents", cents), ("k_res", res), ("v_res", res))], 0,
                                                n_tokens=0, page_ids=kw.get("ids", ids), page_size=64)
    for kw, msg in ((dict(k_pool=pool.view(torch.int16).to(torch.uint8)), "uint16"), (dict(q=q.float()), "fp16"),
                    (dict(k_cents=cents.float()), "codebooks"), (dict(k_pool=torch.zeros(4, 64, 128, dtype=torch.uint16)[:, :, ::2]), "contiguous"),
                    (dict(v_pool=torch.zeros(4, 32, 64, dtype=torch.uint16)), "pools must be"), (dict(ids=ids.float()), "page_ids"), (dict(q=q[:, :, :, ::2]), "q must be")):
        with pytest.raises(RuntimeError, match=msg):
            wide(**kw)


# ---------------------------------------------------------------- the cache, launches stubbed ------------------------------
KW = dict(bs=2, nh=4, num_key_value_heads=2, M=64, layer_num=2, d=128, page_size=32, extended_residual_size=64, max_tokens=512,
          device="cpu")


def test_constructor_code_types():
    import torch
    from million_amd.pq_cache import PagedPQCache
    for nbits, dt in ((9, torch.uint16), (10, torch.uint16), (12, torch.uint16), (8, torch.uint8)):
        c = PagedPQCache(**KW, nbits=nbits, dtype=dt)
        assert c.key_page_pool.dtype == c.value_page_pool.dtype == dt and c.C == 2 ** nbits
        assert tuple(c.key_page_pool.shape[1:]) == (32, 64) and tuple(c.value_page_pool.shape[1:]) == (64, 32)
    assert PagedPQCache(**KW).key_page_pool.dtype == torch.uint8
    for nbits, dt in ((7, torch.uint8), (13, torch.uint16), (16, torch.uint16), (10, torch.uint8), (8, torch.uint16), (10, torch.int16)):
        with pytest.raises(NotImplementedError, match="nbits 9 .. 12"):
            PagedPQCache(**KW, nbits=nbits, dtype=dt)
    with pytest.raises(NotImplementedError, match="nbits"):
        PagedPQCache(**KW, nbits=10, dtype=torch.uint16, sink_tokens=4)
    with pytest.raises(ValueError, match="centroids"):
        PagedPQCache(**KW, nbits=10, dtype=torch.uint16).set_cent(torch.zeros(64, 512, 2), torch.zeros(64, 512, 2))
    c = PagedPQCache(**KW, nbits=10, dtype=torch.uint16)
    c.set_cent(torch.zeros(64, 1024, 2), torch.zeros(64, 1024, 2))
    assert c._kprep is None and c._vprep is None and c.key_cent.dtype == torch.float16


def _host_cache(monkeypatch, nbits, log):
    import torch
    from million_amd import ops
    from million_amd.pq_cache import PagedPQCache
    rec = lambda name, ret=None: (lambda *a, **k: (log.append((name, k)), ret(*a, **k) if ret else None)[1])
    zeros_q = lambda q, *a, **k: torch.zeros_like(q)
    chunk = lambda q, *a, **k: (torch.zeros_like(q), torch.zeros(q.shape[:3])) if k.get("return_lse") else torch.zeros_like(q)
    monkeypatch.setattr(ops, "pq_encode_into", rec("encode"))
    monkeypatch.setattr(ops, "prefill_attn", rec("prefill_attn", lambda q, k, v, **kw: torch.zeros_like(q)))
    monkeypatch.setattr(ops, "pq_chunk_attn", rec("chunk", chunk))
    monkeypatch.setattr(ops, "pq_decode_attn", rec("decode", zeros_q))
    monkeypatch.setattr(ops, "pq_decode_attn_wide", rec("decode_wide", zeros_q))
    monkeypatch.setattr(ops, "pq_decode", rec("pq_decode", lambda codes, cents: torch.zeros(*codes.shape[:-1], 128, dtype=torch.float16)))
    monkeypatch.setattr(ops, "pq_flush", rec("flush"))
    monkeypatch.setattr(ops, "lengths_advance", rec("advance"))
    for name in ("cache_fork", "cache_swap", "pq_store_ragged", "window_commit"):
        monkeypatch.setattr(ops, name, rec(name))
    cache = PagedPQCache(**KW, nbits=nbits, dtype=torch.uint8 if nbits == 8 else torch.uint16)
    cache.key_cent = cache.value_cent = torch.zeros(64, 2 ** nbits, 2, dtype=torch.float16)
    cache._kprep = cache._vprep = None
    return cache


def _follow_ups(cache, other, snap):
    """Every call DESIGN.md 4.14 lists as refused on a cache with uint16 codes, as (name, thunk)."""
    import torch
    from million_amd.shared_prefix import SharedPrefix
    q5, k5 = torch.zeros(2, 4, 5, 128, dtype=torch.float16), torch.zeros(2, 2, 5, 128, dtype=torch.float16)
    return [("extend", lambda: cache.extend(q5, k5, k5, 0)),
            ("extend_request", lambda: cache.extend_request(1, q5[:1], k5[:1], k5[:1], 0)),
            ("extend_ragged", lambda: cache.extend_ragged(q5, k5, k5, 0, [5, 2])),
            ("prefill_ragged", lambda: cache.prefill_ragged(q5, k5, k5, 0, [0, 0])),
            ("fork", lambda: cache.fork(0, 1)),
            ("snapshot_request", lambda: cache.snapshot_request(0)),
            ("swap_out", lambda: cache.swap_out(0, release=False)),
            ("swap_in", lambda: cache.swap_in(1, snap)),
            ("verify", lambda: cache.verify(q5, k5, k5, 0, route="chunk")),
            ("commit", lambda: cache.commit([0, 0])),
            ("update", lambda: cache.update(k5, k5, 0)),
            ("SharedPrefix(prefix)", lambda: SharedPrefix(cache, 0, other)),
            ("SharedPrefix(continuations)", lambda: SharedPrefix(other, 0, cache))]


def _mirror(cache):
    return [a.copy() for a in cache.host_state()] + [cache._pages_a.copy()] + [l.clone() for l in cache.lengths]


def _same(a, b):
    import torch
    return all(torch.equal(x, y) if isinstance(x, torch.Tensor) else np.array_equal(x, y) for x, y in zip(a, b))


def test_wide_cache_refuses_the_follow_ups_by_name(monkeypatch):
    import torch
    log = []
    cache = _host_cache(monkeypatch, 10, log)
    plain = _host_cache(monkeypatch, 8, log)
    q = torch.zeros(1, 4, 40, 128, dtype=torch.float16)
    k = torch.zeros(1, 2, 40, 128, dtype=torch.float16)
    for l in range(2):
        cache.prefill_request(0, q, k, k, l)
        plain.prefill_request(0, q, k, k, l)
    snap = plain.snapshot_request(0)
    before, n_log = _mirror(cache), len(log)
    for name, call in _follow_ups(cache, plain, snap):
        with pytest.raises(NotImplementedError, match="nbits"):
            call()
        assert _same(before, _mirror(cache)) and len(log) == n_log, name
    assert cache._verify_rec is None and not cache._r_a.any() and cache._T_a.tolist() == [[40, 0], [40, 0]]


def test_the_same_calls_on_a_uint8_cache_still_run(monkeypatch):
    import torch
    from million_amd.shared_prefix import SharedPrefix
    log = []
    cache = _host_cache(monkeypatch, 8, log)
    other = _host_cache(monkeypatch, 8, log)
    q = torch.zeros(1, 4, 40, 128, dtype=torch.float16)
    k = torch.zeros(1, 2, 40, 128, dtype=torch.float16)
    for l in range(2):
        cache.prefill_request(0, q, k, k, l)
    snap = cache.snapshot_request(0)
    q5, k5 = torch.zeros(2, 4, 5, 128, dtype=torch.float16), torch.zeros(2, 2, 5, 128, dtype=torch.float16)
    cache.fork(0, 1)
    assert cache._T_a.tolist() == [[40, 40], [40, 40]]
    for l in range(2):
        cache.verify(q5, k5, k5, l, route="chunk", use_dev_lengths=False)
    cache.commit([2, 2])
    assert cache._r_a.tolist() == [[2, 2], [2, 2]]
    for l in range(2):
        cache.extend(q5, k5, k5, l)
    assert cache._T_a.tolist() == [[47, 47], [47, 47]] and not cache._r_a.any()
    for l in range(2):
        cache.extend_request(1, q5[:1], k5[:1], k5[:1], l)
        cache.extend_ragged(q5, k5, k5, l, [5, 2])
        cache.prefill_ragged(q5, k5, k5, l, [0, 0])
    assert cache._T_a.tolist() == [[52, 54], [52, 54]]
    cache.release(1)
    cache.swap_in(1, snap)
    assert cache._T_a[:, 1].tolist() == [40, 40]
    cache.release(1)
    cache.release(0)
    kk, vv = cache.update(k5, k5, 0)
    assert kk.shape == k5.shape and cache._T_a[0].tolist() == [5, 5]
    SharedPrefix(other, 0, cache)
    names = {e[0] for e in log}
    assert {"cache_fork", "cache_swap", "chunk", "window_commit", "encode", "prefill_attn"} <= names and "decode_wide" not in names


@pytest.mark.parametrize("use_dev", [False, True])
def test_wide_host_mirror_follows_the_paged_policy(monkeypatch, oracle, use_dev):
    import torch
    from million_amd import _lib as L
    log = []
    cache = _host_cache(monkeypatch, 10, log)
    ps, cap = KW["page_size"], KW["extended_residual_size"]
    q = torch.zeros(2, 4, 70, 128, dtype=torch.float16)
    k = torch.zeros(2, 2, 70, 128, dtype=torch.float16)
    for l in range(2):
        cache.prefill(q, k, k, l)
    assert [e[0] for e in log] == ["encode", "encode", "prefill_attn"] * 2 and log[0][1]["n"] == 70 and log[0][1]["prepared"] is None
    pol = oracle.PagedPolicy(page_size=ps, residual=cap, prefill=70)
    q1, k1 = q[:, :, :1].contiguous(), k[:, :, :1].contiguous()
    flushes = 0
    for step in range(2 * cap + 3):
        del log[:]
        kind = cache.begin_step(use_dev_lengths=use_dev)
        assert kind == cache.next_step_kind() == ("flush" if cache._r_a[0, 0] >= cap else "plain") and not log      # reported, nothing launched
        cache.flush_ahead(use_dev_lengths=use_dev)
        assert not log and cache._ahead is None
        T0, rs0 = int(cache._T_a[0, 0]), int(cache._rs_a[0, 0])
        for l in range(2):
            cache.decoding_with_pages(q1, k1, k1, l, use_dev_lengths=use_dev)
        T, r = pol.step()
        assert cache._T_a.tolist() == [[T, T]] * 2 and cache._r_a.tolist() == [[r, r]] * 2 and cache._seen_a[0, 0] == 70 + step + 1
        per_layer = [e[0] for e in log][:len(log) // 2]
        if kind == "flush":      # two encode launches out of the ring, the advance with device lengths, then the fused step
            flushes += 1
            assert per_layer == ["encode", "encode"] + (["advance"] if use_dev else []) + ["decode_wide"]
            for e, layout in zip(log[:2], (L.MILLION_CODES_KPAGES, L.MILLION_CODES_VPAGES)):
                kw = e[1]
                assert (kw["layout"], kw["n"], kw["token_start"], kw["x_row_start"], kw["x_row_mod"], kw["page_size"]) == (layout, ps, T0, rs0, cap, ps)
            assert int(cache._rs_a[0, 0]) == (rs0 + ps) % cap
        else:
            assert per_layer == ["decode_wide"]
        kw = log[-1][1]
        assert kw["resid_start"] == int(cache._rs_a[1, 0]) and kw["n_tokens"] == (cache.max_tokens if use_dev else T)
        assert (kw["dev_lengths"] is not None) == use_dev and kw["k_new"] is k1
    assert flushes == pol.flushes == 3      # at steps 65, 97 and 129: the window holds two pages
    # a ragged batch: its windows fill at different steps, which the two-launch flush does not serve
    cache.release(0)
    for l in range(2):
        cache.prefill_request(0, q[:1], k[:1], k[:1], l)
    cache._r_a[:, 1] = cap
    with pytest.raises(RuntimeError, match="lockstep"):
        cache.decoding_with_pages(q1, k1, k1, 0, use_dev_lengths=True)
    st = cache.get_cache_stats()
    assert st["memory_breakdown"]["cache_memory_mb"] == 2 * 2 * 64 * 2 * float(cache._T_a.sum()) / 2 ** 20
    saved = cache.host_state()
    cache.cleanup()
    assert not cache._T_a.any() and not cache._r_a.any() and not any(l.any() for l in cache.lengths)
    cache.set_host_state(saved)
    assert np.array_equal(cache._T_a, saved[2])
