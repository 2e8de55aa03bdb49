"""CPU side of packed code pages (include/million_hip.h, "Packed code pages"): the numpy model round-trips, the
page sizes are ops.packed_page_bytes', the new entries exist and refuse what they must before any HIP call, ops refuses before
the library is entered, and a PagedPQCache(packed=True) - on the CPU, launches stubbed as in tests/test_attn_wide_host.py -
allocates packed pools, refuses what a wide cache refuses and asks for exactly the launches of the wide cache's life."""
import ctypes
import itertools

import numpy as np
import pytest

from tests import packed_model as P
from tests.test_attn_wide_host import A, ERR_ALIGN, ERR_ARG, ERR_SHAPE, KW, _desc, _follow_ups, _mirror, _same

GEOMS = list(itertools.product((32, 64, 128), (16, 32, 64), (512, 1024, 2048, 4096)))


@pytest.fixture(scope="module")
def lib():
    from million_amd import build, _lib
    build.build()
    return _lib.load()


# ---------------------------------------------------------------- the model ------------------------------------------------
@pytest.mark.parametrize("ps,M,C", GEOMS)
def test_model_round_trips(ps, M, C):
    rs = np.random.RandomState(ps + M + C)
    for side, shape in (("k", (3, ps, M)), ("v", (3, M, ps))):
        x = rs.randint(0, C, shape).astype(np.uint16)
        x.reshape(-1)[:2] = (C - 1, 0)
        packed = P.pack(x, side, C)
        assert packed.dtype == np.uint8 and packed.shape == (3, P.page_bytes(ps, M, C))
        assert np.array_equal(P.unpack(packed, side, ps, M, C), x)
        assert packed.shape[1] % 16 == 0 and (ps * M) % 16 == 0      # both planes are multiples of 16 bytes
    # the low plane of a K page is the uint8 K page, of a V page the transposed uint8 page
    k = rs.randint(0, C, (1, ps, M)).astype(np.uint16)
    assert np.array_equal(P.pack(k, "k", C)[0, :ps * M], (k & 0xFF).astype(np.uint8).reshape(-1))
    assert np.array_equal(P.pack(k.transpose(0, 2, 1), "v", C)[0, :ps * M], (k & 0xFF).astype(np.uint8)[0].T.reshape(-1))


def test_model_bit_positions_and_single_token_stores():
    ps, M = 32, 16
    for C, h in ((1024, 2), (4096, 4)):
        per = 8 // h
        for m in range(M):
            x = np.zeros((1, ps, M), np.uint16)
            x[0, 5, m] = ((1 << h) - 1) << 8      # only the high field of (token 5, subspace m)
            pk, pv = P.pack(x, "k", C)[0], P.pack(x.transpose(0, 2, 1), "v", C)[0]
            want = ((1 << h) - 1) << (h * (m % per))
            assert pk[ps * M + 5 * (M * h // 8) + m // per] == want and np.count_nonzero(pk) == 1
            assert pv[M * ps + (m // per) * ps + 5] == want and np.count_nonzero(pv) == 1
        # a store of some tokens changes no byte of another token, and equals packing the page as a whole
        rs = np.random.RandomState(C)
        codes = rs.randint(0, C, (ps, M)).astype(np.uint16)
        for side in ("k", "v"):
            page = np.full(P.page_bytes(ps, M, C), 0xA5, np.uint8)
            P.put_tokens(page, side, np.arange(3, 9), codes[3:9], ps, M, C)
            blank = P.unpack(np.full((1, P.page_bytes(ps, M, C)), 0xA5, np.uint8), side, ps, M, C)[0]      # what 0xA5 bytes read as
            whole = blank if side == "k" else blank.T.copy()
            assert set(np.unique(whole)) <= {0x1A5, 0x2A5, 0x5A5, 0xAA5}
            whole[3:9] = codes[3:9]
            assert np.array_equal(P.unpack(page[None], side, ps, M, C)[0], whole if side == "k" else whole.T)
            other = np.full(P.page_bytes(ps, M, C), 0xA5, np.uint8)      # the bytes of the other tokens: untouched
            P.put_tokens(other, side, np.arange(3, 9), np.full((6, M), 0x1A5 if h == 2 else 0x5A5), ps, M, C)
            assert np.count_nonzero(other != page) <= 6 * M * (8 + h) // 8


@pytest.mark.parametrize("ps,M,C", GEOMS)
def test_page_sizes_match_ops(ps, M, C):
    from million_amd import ops
    assert ops.packed_page_bytes(ps, M, C) == P.page_bytes(ps, M, C) == ps * M * (8 + ops.packed_hi_bits(C)) // 8
    assert ops.packed_hi_bits(C) == P.hi_bits(C) == (2 if C <= 1024 else 4)


def test_hi_bits_refuses_other_codebooks():
    from million_amd import ops
    for C in (256, 128, 300, 8192):
        with pytest.raises(RuntimeError, match="packed"):
            ops.packed_hi_bits(C)


# ---------------------------------------------------------------- the C ABI ------------------------------------------------
def test_symbols(lib):
    from million_amd import _lib as L
    vp = ctypes.c_void_p
    assert L.SYMBOLS["million_pq_decode_attn_packed"] == L.SYMBOLS["million_pq_decode_attn_wide"]
    assert L.SYMBOLS["million_pq_encode_packed"] == L.SYMBOLS["million_pq_encode"]
    assert L.SYMBOLS["million_pq_repack_pages"] == (ctypes.c_int32, [ctypes.c_int32, vp, vp, ctypes.c_int64] + [ctypes.c_int32] * 4 + [vp])
    header = (L.HERE.parent / "include" / "million_hip.h").read_text()
    for name in ("million_pq_encode_packed", "million_pq_decode_attn_packed", "million_pq_repack_pages"):
        assert name + "(" in header and hasattr(lib, name)
    assert "MILLION_REPACK_PACK = 0" in header and "MILLION_REPACK_UNPACK = 1" in header
    assert (L.MILLION_REPACK_PACK, L.MILLION_REPACK_UNPACK) == (0, 1)
    dbg = L.HERE / "libmillion_hip_dbgids.so"      # the diagnostic library carries the three entries too
    if dbg.exists():
        d = ctypes.CDLL(str(dbg))
        assert all(hasattr(d, n) for n in ("million_pq_encode_packed", "million_pq_decode_attn_packed", "million_pq_repack_pages"))


def _packed_call(lib, desc, **kw):
    a = dict(q=A, k_new=None, v_new=None, k_codes=A + 0x10000, v_codes=A + 0x20000, k_ids=A + 0x30000, v_ids=A + 0x30000,
             k_cents=A + 0x40000, v_cents=A + 0x50000, k_res=A + 0x60000, v_res=A + 0x70000, out=A + 0x80000, lse=None, ws=A + 0x90000,
             ws_bytes=1 << 30)
    a.update(kw)
    return lib.million_pq_decode_attn_packed(ctypes.byref(desc), a["q"], a["k_new"], a["v_new"], a["k_codes"], a["v_codes"], a["k_ids"],
                                             a["v_ids"], a["k_cents"], a["v_cents"], a["k_res"], a["v_res"], a["out"], a["lse"], a["ws"],
                                             a["ws_bytes"], None)


def test_packed_decode_entry_refuses_as_the_wide_entry(lib):
    from million_amd import _lib as L
    err = lib.million_last_error
    for kw in (dict(C=256), dict(C=300), dict(k_layout=0), dict(v_layout=0), dict(nh=34), dict(d=128, M=16), dict(C=8192)):
        assert _packed_call(lib, _desc(L, **kw)) == ERR_SHAPE, kw
    d = _desc(L)
    for part in ("q", "k_cents", "v_cents", "k_res", "v_res", "out", "ws", "k_codes", "v_codes", "k_ids", "v_ids"):
        assert _packed_call(lib, d, **{part: None}) == ERR_ARG, part
    for part in ("q", "k_codes", "v_codes", "k_res", "v_res", "out", "ws"):
        assert _packed_call(lib, d, **{part: A + 0xc0008}) == ERR_ALIGN and b"16-byte" in err(), part
    assert _packed_call(lib, d, k_new=A + 0xa0000) == ERR_ARG and b"k_new" in err()
    assert _packed_call(lib, d, ws_bytes=lib.million_attn_wide_workspace_bytes(ctypes.byref(d)) - 1) == -4


def _enc_desc(L, C=1024, M=64, d=128, layout=1, ps=64, n=5):
    x = L.EncodeDesc()
    x.struct_size = ctypes.sizeof(L.EncodeDesc)
    x.bs, x.nh_k, x.n, x.d, x.M, x.C = 2, 2, n, d, M, C
    x.x_stride_b, x.x_stride_h, x.x_stride_n = 2 * n * d, n * d, d
    x.dst_layout, x.dst_token_start, x.page_size, x.n_pages_cap = layout, 0, ps, 4
    return x


def test_packed_encode_and_repack_refuse_without_a_gpu(lib):
    from million_amd import _lib as L
    err = lib.million_last_error
    enc = lambda desc, dst=A + 0x20000: lib.million_pq_encode_packed(ctypes.byref(desc), A, A + 0x10000, dst, A + 0x30000, None)
    assert enc(_enc_desc(L, layout=L.MILLION_CODES_ROWMAJOR)) == ERR_SHAPE and b"row-major" in err()
    for kw in (dict(C=256), dict(C=128), dict(C=768), dict(C=8192), dict(M=2, d=4), dict(ps=48)):
        assert enc(_enc_desc(L, **kw)) == ERR_SHAPE, kw
    assert enc(_enc_desc(L), dst=A + 0x20008) == ERR_ALIGN
    bad = _enc_desc(L)
    bad.struct_size -= 4
    assert enc(bad) == ERR_ARG
    assert lib.million_pq_encode_packed(ctypes.byref(_enc_desc(L)), A, A, None, A, None) == ERR_ARG
    assert enc(_enc_desc(L, n=0)) == 0      # nothing to store: no launch
    rp = lambda direction=0, src=A, dst=A + 0x100000, n=3, ps=64, M=64, C=1024, side=0: lib.million_pq_repack_pages(direction, src, dst, n, ps, M, C, side, None)
    assert rp(direction=2) == ERR_ARG and rp(side=2) == ERR_ARG and rp(n=-1) == ERR_ARG
    for kw in (dict(C=256), dict(C=8192), dict(M=6), dict(ps=48)):
        assert rp(**kw) == ERR_SHAPE, kw
    assert rp(src=None) == ERR_ARG and rp(dst=None) == ERR_ARG and rp(src=A + 8) == ERR_ALIGN
    assert rp(n=0, src=None, dst=None) == 0


# ---------------------------------------------------------------- ops, before the library ----------------------------------
def test_ops_refuse_before_the_library(monkeypatch):
    import torch
    from million_amd import ops
    L = ops.L
    monkeypatch.setattr(ops.L, "load", lambda: pytest.fail("the library was entered"))
    q, res = torch.zeros(1, 4, 1, 128, dtype=torch.float16), torch.zeros(1, 2, 64, 128, dtype=torch.float16)
    pb = ops.packed_page_bytes(64, 64, 1024)
    pool = torch.zeros(4, pb, dtype=torch.uint8)
    cents = torch.zeros(64, 1024, 2, dtype=torch.float16)
    ids = torch.zeros(1, 2, 2, dtype=torch.int32)
    X = torch.zeros(1, 2, 5, 128, dtype=torch.float16)
    with pytest.raises(RuntimeError, match="device tensors"):
        ops.pq_decode_attn_packed(q, pool, pool, cents, cents, res, res, 0, n_tokens=0, page_ids=ids, page_size=64)
    monkeypatch.setattr(ops, "_need_cuda", lambda *a: None)
    dec = lambda **kw: ops.pq_decode_attn_packed(*[kw.get(n, v) for n, v in (("q", q), ("k_pool", pool), ("v_pool", pool), ("k_cents", cents),
                                                                              ("v_cents", cents), ("k_res", res), ("v_res", res))], 0,
                                                 n_tokens=0, page_ids=kw.get("ids", ids), page_size=64)
    u16 = torch.zeros(4, 64, 64, dtype=torch.uint16)
    for kw, msg in ((dict(k_pool=u16), "packed pools must be uint8"), (dict(v_pool=pool.view(torch.int8)), "uint8"),
                    (dict(k_pool=torch.zeros(4, pb + 16, dtype=torch.uint8)), "packed pool must be"),
                    (dict(v_pool=torch.zeros(4, 64, 80, dtype=torch.uint8)), "packed pool must be"),
                    (dict(k_pool=torch.zeros(4, 2 * pb, dtype=torch.uint8)[:, ::2]), "contiguous"),
                    (dict(k_cents=torch.zeros(64, 256, 2, dtype=torch.float16), v_cents=torch.zeros(64, 256, 2, dtype=torch.float16)), "C=256"),
                    (dict(q=q.float()), "fp16"), (dict(ids=ids.float()), "page_ids")):
        with pytest.raises(RuntimeError, match=msg):
            dec(**kw)
    enc = lambda **kw: ops.pq_encode_into_packed(kw.get("X", X), kw.get("cents", cents), kw.get("dst", pool), layout=kw.get("layout", L.MILLION_CODES_KPAGES),
                                                 page_ids=kw.get("ids", ids), page_size=64)
    for kw, msg in ((dict(layout=L.MILLION_CODES_ROWMAJOR), "row-major"), (dict(dst=u16), "packed pool must be"),
                    (dict(dst=torch.zeros(4, pb - 16, dtype=torch.uint8)), "packed pool must be"),
                    (dict(cents=torch.zeros(64, 256, 2, dtype=torch.float16)), "C=256"), (dict(X=X.float()), "fp16"),
                    (dict(ids=ids.long()), "page_ids")):
        with pytest.raises(RuntimeError, match=msg):
            enc(**kw)
    with pytest.raises(RuntimeError, match="uint16"):
        ops.pq_pack_pages(torch.zeros(4, 64, 64, dtype=torch.uint8), side="k", C=1024)
    with pytest.raises(RuntimeError, match="C=256"):
        ops.pq_pack_pages(u16, side="k", C=256)
    with pytest.raises(RuntimeError, match="packed pool must be"):
        ops.pq_unpack_pages(torch.zeros(4, pb + 1, dtype=torch.uint8), side="v", page_size=64, M=64, C=1024)
    with pytest.raises(RuntimeError, match="side"):
        ops.pq_pack_pages(u16, side="x", C=1024)


# ---------------------------------------------------------------- the cache, launches stubbed ------------------------------
def _packed_cache(monkeypatch, nbits, log, packed=True):
    """tests/test_attn_wide_host.py's _host_cache with the packed launches stubbed too."""
    import torch
    from million_amd import ops
    from tests.test_attn_wide_host import _host_cache
    rec = lambda name, ret=None: (lambda *a, **k: (log.append((name, k)), ret(*a, **k) if ret else None)[1])
    monkeypatch.setattr(ops, "pq_encode_into_packed", rec("encode_packed"))
    monkeypatch.setattr(ops, "pq_decode_attn_packed", rec("decode_packed", lambda q, *a, **k: torch.zeros_like(q)))
    if not packed:
        return _host_cache(monkeypatch, nbits, log)
    from million_amd.pq_cache import PagedPQCache
    _host_cache(monkeypatch, 8, log)      # (installs the other stubs)
    cache = PagedPQCache(**KW, nbits=nbits, dtype=torch.uint16, packed=True)
    cache.key_cent = cache.value_cent = torch.zeros(64, 2 ** nbits, 2, dtype=torch.float16)
    cache._kprep = cache._vprep = None
    return cache


def test_constructor():
    import torch
    from million_amd import ops
    from million_amd.pq_cache import PagedPQCache
    for nbits in (9, 10, 11, 12):
        c = PagedPQCache(**KW, nbits=nbits, dtype=torch.uint16, packed=True)
        twin = PagedPQCache(**KW, nbits=nbits, dtype=torch.uint16)
        pb = ops.packed_page_bytes(32, 64, 2 ** nbits)
        assert c.packed and not twin.packed and c.C == 2 ** nbits
        for pool, tp in ((c.key_page_pool, twin.key_page_pool), (c.value_page_pool, twin.value_page_pool)):
            assert pool.dtype == torch.uint8 and tuple(pool.shape) == (tp.shape[0], pb) and pool.is_contiguous()
            h = 2 if nbits <= 10 else 4
            assert pool.numel() * 16 == tp.numel() * tp.element_size() * (8 + h)      # exactly (8 + h) / 16 of the bytes
    with pytest.raises(ValueError, match="packed"):
        PagedPQCache(**KW, nbits=8, dtype=torch.uint8, packed=True)
    assert PagedPQCache(**KW).packed is False and PagedPQCache(**KW).key_page_pool.dtype == torch.uint8
    for nbits, dt in ((7, torch.uint8), (13, torch.uint16), (10, torch.uint8), (8, torch.uint16)):      # the wide cache's refusals come first
        with pytest.raises(NotImplementedError, match="nbits 9 .. 12"):
            PagedPQCache(**KW, nbits=nbits, dtype=dt, packed=True)
    with pytest.raises(NotImplementedError, match="nbits"):
        PagedPQCache(**KW, nbits=10, dtype=torch.uint16, sink_tokens=4, packed=True)
    with pytest.raises(ValueError, match="centroids"):
        PagedPQCache(**KW, nbits=10, dtype=torch.uint16, packed=True).set_cent(torch.zeros(64, 512, 2), torch.zeros(64, 512, 2))


def test_packed_cache_refuses_the_follow_ups_as_a_wide_cache(monkeypatch):
    import torch
    log = []
    cache = _packed_cache(monkeypatch, 10, log)
    plain = _packed_cache(monkeypatch, 8, log, packed=False)
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
    assert cache._T_a.tolist() == [[40, 0], [40, 0]]


@pytest.mark.parametrize("use_dev", [False, True])
def test_packed_cache_asks_for_the_wide_cache_launches(monkeypatch, oracle, use_dev):
    import torch
    from million_amd import _lib as L
    log = []
    cache = _packed_cache(monkeypatch, 11, log)
    ps, cap = KW["page_size"], KW["extended_residual_size"]
    q = torch.zeros(2, 4, 70, 128, dtype=torch.float16)
    k = torch.zeros(2, 2, 70, 128, dtype=torch.float16)
    for l in range(2):
        cache.prefill(q, k, k, l)
    assert [e[0] for e in log] == ["encode_packed", "encode_packed", "prefill_attn"] * 2 and log[0][1]["n"] == 70
    assert (log[0][1]["layout"], log[1][1]["layout"]) == (L.MILLION_CODES_KPAGES, L.MILLION_CODES_VPAGES) and "prepared" not in log[0][1]
    pol = oracle.PagedPolicy(page_size=ps, residual=cap, prefill=70)
    q1, k1 = q[:, :, :1].contiguous(), k[:, :, :1].contiguous()
    flushes = 0
    for step in range(2 * cap + 3):
        del log[:]
        kind = cache.begin_step(use_dev_lengths=use_dev)
        assert kind == ("flush" if cache._r_a[0, 0] >= cap else "plain") and not log
        T0, rs0 = int(cache._T_a[0, 0]), int(cache._rs_a[0, 0])
        for l in range(2):
            cache.decoding_with_pages(q1, k1, k1, l, use_dev_lengths=use_dev, return_lse=bool(step % 2))
        T, r = pol.step()
        assert cache._T_a.tolist() == [[T, T]] * 2 and cache._r_a.tolist() == [[r, r]] * 2
        per_layer = [e[0] for e in log][:len(log) // 2]
        if kind == "flush":      # exactly: two packed encodes out of the ring, the advance with device lengths, the fused step
            flushes += 1
            assert per_layer == ["encode_packed", "encode_packed"] + (["advance"] if use_dev else []) + ["decode_packed"]
            for e, layout in zip(log[:2], (L.MILLION_CODES_KPAGES, L.MILLION_CODES_VPAGES)):
                kw = e[1]
                assert (kw["layout"], kw["n"], kw["token_start"], kw["x_row_start"], kw["x_row_mod"], kw["page_size"]) == (layout, ps, T0, rs0, cap, ps)
        else:
            assert per_layer == ["decode_packed"]
        kw = log[-1][1]
        assert kw["n_tokens"] == (cache.max_tokens if use_dev else T) and (kw["dev_lengths"] is not None) == use_dev and kw["k_new"] is k1
        assert kw.get("return_lse", False) == bool(step % 2)
    assert flushes == pol.flushes == 3      # at steps 65, 97 and 129
    # the real bytes: 12 bits per code at nbits = 11
    assert cache.pq_cache_size() == 2 * 2 * 64 * 1.5 * float(cache._T_a.sum())
    assert cache.get_cache_stats()["memory_breakdown"]["cache_memory_mb"] == cache.pq_cache_size() / 2 ** 20
    cache._r_a[:, 1] = cap      # a ragged batch: refused as the wide cache refuses it
    cache._T_a[:, 1] += 1
    with pytest.raises(RuntimeError, match="lockstep"):
        cache.decoding_with_pages(q1, k1, k1, 0, use_dev_lengths=True)
    cache._T_a[:, 1] -= 1
    saved = cache.host_state()
    cache.release(1)
    assert not cache._T_a[:, 1].any() and cache._T_a[:, 0].all()
    cache.cleanup()
    assert not cache._T_a.any() and not cache._r_a.any() and not any(l.any() for l in cache.lengths)
    cache.set_host_state(saved)
    assert np.array_equal(cache._T_a, saved[2])
