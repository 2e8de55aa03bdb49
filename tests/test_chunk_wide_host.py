"""CPU side of chunk attention over uint16 codes (include/million_hip.h, million_pq_chunk_attn_wide): the two new
entries are exported, size their workspace as the uint8 entry does and refuse what they must before any HIP call; the uint8
entries answer what they always did; ops.pq_chunk_attn_wide refuses before the library is entered; DynamicPQCache.extend - on a CPU
cache with the launches stubbed - takes the wide call at nbits 9 .. 12, prefill() on an empty cache, and still raises past 12."""
import ctypes

import numpy as np
import pytest

from tests import chunk_wide_model as CM

ERR_ARG, ERR_SHAPE, ERR_ALIGN, ERR_WORKSPACE = -3, -1, -2, -4
A = 0x100000      # made-up aligned device addresses: a refused call dereferences nothing


@pytest.fixture(scope="module")
def lib():
    from million_amd import build, _lib
    build.build()
    return _lib.load()


def _desc(L, C=1024, bs=2, nh=8, nhk=2, d=128, M=64, n_q=5, T=4133, r=3, k_layout=1, v_layout=1, n_c=None):
    x = L.ChunkAttnDesc()
    x.struct_size = ctypes.sizeof(L.ChunkAttnDesc)
    x.bs, x.nh, x.nh_k, x.d, x.M, x.C = bs, nh, nhk, d, M, C
    x.n_q, x.n_c, x.n_tokens, x.r, x.resid_start, x.resid_cap = n_q, n_q if n_c is None else n_c, T, r, 0, 128
    x.resid_stride_b, x.resid_stride_h = nhk * 128 * d, 128 * d
    x.k_layout, x.v_layout, x.page_size, x.n_pages_cap = k_layout, v_layout, 64, -(-max(T, 1) // 64)
    x.k_stride_b, x.k_stride_h = nhk * (T + 64) * M * 2, (T + 64) * M * 2
    x.v_stride_b, x.v_stride_h = x.k_stride_b, x.k_stride_h
    for nm, rows, heads in (("q", n_q, nh), ("kc", n_q, nhk), ("vc", n_q, nhk), ("o", n_q, nh)):
        setattr(x, nm + "_stride_b", heads * rows * d), setattr(x, nm + "_stride_h", rows * d), setattr(x, nm + "_stride_n", d)
    return x


def _call(lib, desc, **kw):
    a = dict(q=A, k_chunk=A + 0x1000, v_chunk=A + 0x2000, k_codes=A + 0x10000, v_codes=A + 0x20000, k_ids=A + 0x30000, v_ids=A + 0x30000,
             k_cents=A + 0x40000, v_cents=A + 0x50000, k_res=A + 0x60000, v_res=A + 0x70000, out=A + 0x80000, lse=None, ws=A + 0x90000,
             ws_bytes=1 << 40)
    a.update(kw)
    return lib.million_pq_chunk_attn_wide(ctypes.byref(desc), a["q"], a["k_chunk"], a["v_chunk"], a["k_codes"], a["v_codes"], a["k_ids"],
                                          a["v_ids"], a["k_cents"], a["v_cents"], a["k_res"], a["v_res"], a["out"], a["lse"], a["ws"],
                                          a["ws_bytes"], None)


def test_symbols(lib):
    from million_amd import _lib as L
    vp = ctypes.c_void_p
    assert L.SYMBOLS["million_pq_chunk_attn_wide"] == (ctypes.c_int32, [ctypes.POINTER(L.ChunkAttnDesc)] + [vp] * 14 + [ctypes.c_size_t, vp])
    assert L.SYMBOLS["million_chunk_attn_wide_workspace_bytes"] == (ctypes.c_size_t, [ctypes.POINTER(L.ChunkAttnDesc)])
    header = (L.HERE.parent / "include" / "million_hip.h").read_text()
    for name in ("million_pq_chunk_attn_wide", "million_chunk_attn_wide_workspace_bytes"):
        assert name + "(" in header and hasattr(lib, name)


@pytest.mark.parametrize("bs,nhk,n_q,G,T,S", [(1, 8, 16, 4, 32768, 32), (1, 2, 5, 4, 40, 1), (1, 2, 5, 4, 4097, 64), (4, 2, 5, 4, 4097, 32),
                                             (1, 8, 2048, 4, 32768, 1), (2, 2, 257, 8, 1000, 8), (1, 1, 1, 1, 0, 1), (3, 2, 65, 1, 65, 2)])
def test_workspace_is_the_uint8_entrys(lib, bs, nhk, n_q, G, T, S):
    """One formula: the bytes are million_chunk_attn_workspace_bytes of the same descriptor with C = 256, which are the header's
    bs * nh_k * S * n_q * G * (d + 2) * 4 (0 at S = 1)."""
    from million_amd import _lib as L
    for d, M, C in ((128, 64, 1024), (64, 16, 4096)):
        wide = _desc(L, C=C, bs=bs, nh=nhk * G, nhk=nhk, d=d, M=M, n_q=n_q, T=T)
        u8 = _desc(L, C=256, bs=bs, nh=nhk * G, nhk=nhk, d=d, M=M, n_q=n_q, T=T)
        want = bs * nhk * S * n_q * G * (d + 2) * 4 if S > 1 else 0
        assert lib.million_chunk_attn_wide_workspace_bytes(ctypes.byref(wide)) == lib.million_chunk_attn_workspace_bytes(ctypes.byref(u8)) == want
        if want:
            assert _call(lib, wide, ws_bytes=want - 1) == ERR_WORKSPACE and _call(lib, wide, ws=None) == ERR_WORKSPACE


REFUSED_SHAPES = [dict(C=256), dict(C=128), dict(C=300), dict(C=768), dict(C=8192), dict(C=65536), dict(d=128, M=128), dict(d=128, M=16),
                  dict(d=64, M=64), dict(d=64, M=8), dict(d=96, M=48), dict(d=256, M=64), dict(nh=9), dict(n_c=3)]
ACCEPTED_SHAPES = [dict(), dict(C=512), dict(C=4096, M=32), dict(d=64, M=32, C=2048), dict(d=64, M=16), dict(nh=64), dict(nh=2),
                   dict(k_layout=0), dict(v_layout=0), dict(k_layout=0, v_layout=0), dict(n_c=0)]


def test_wide_entry_refuses_without_a_gpu(lib):
    from million_amd import _lib as L
    err = lib.million_last_error
    ws_bytes = lambda d: lib.million_chunk_attn_wide_workspace_bytes(ctypes.byref(d))
    d = _desc(L)
    d.struct_size -= 8
    assert _call(lib, d) == ERR_ARG and b"struct_size" in err() and ws_bytes(d) == 0
    assert lib.million_pq_chunk_attn_wide(None, *([None] * 14), 0, None) == ERR_ARG and lib.million_chunk_attn_wide_workspace_bytes(None) == 0
    for kw in REFUSED_SHAPES:
        d = _desc(L, **kw)
        assert lib.million_pq_chunk_attn_wide(ctypes.byref(d), *([None] * 14), 0, None) == ERR_SHAPE, kw      # before any null pointer
        assert _call(lib, d) == ERR_SHAPE and b"chunk_attn" in err(), kw
        if "n_c" not in kw and "nh" not in kw:
            assert b"uint16 codes" in err() and ws_bytes(d) == 0, kw
    for kw in ACCEPTED_SHAPES:
        d = _desc(L, **kw)
        assert lib.million_pq_chunk_attn_wide(ctypes.byref(d), *([None] * 14), 0, None) == ERR_ARG and b"null" in err(), kw
        assert ws_bytes(d) > 0, kw
    d = _desc(L)
    for part in ("q", "out", "k_chunk", "v_chunk", "k_res", "v_res", "k_codes", "v_codes", "k_cents", "v_cents", "k_ids", "v_ids", "ws"):
        assert _call(lib, d, **{part: None}) in (ERR_ARG, ERR_WORKSPACE), part
    for part in ("q", "k_chunk", "v_chunk", "k_codes", "v_codes", "k_res", "v_res", "out", "ws", "k_cents", "v_cents"):
        assert _call(lib, d, **{part: A + 0xc0008}) == ERR_ALIGN and b"16-byte" in err(), part
    assert _call(lib, d, lse=A + 0xd0002) == ERR_ALIGN and b"lse" in err()
    bad = _desc(L, k_layout=0)
    bad.k_stride_h += 8
    assert _call(lib, bad) == ERR_ALIGN and b"code strides" in err()
    bad = _desc(L)
    bad.q_stride_n += 4
    assert _call(lib, bad) == ERR_ALIGN
    bad = _desc(L)
    bad.n_pages_cap = 10
    assert _call(lib, bad) == ERR_SHAPE and b"pages" in err()
    bad = _desc(L)
    bad.page_size = 48
    assert _call(lib, bad) == ERR_SHAPE
    bad = _desc(L, r=200)
    assert _call(lib, bad) == ERR_ARG and b"r=200" in err()
    assert _call(lib, _desc(L, n_q=0)) == 0      # nothing to do: MILLION_OK before any pointer is looked at


def test_uint8_entries_answer_what_they_did(lib):
    from million_amd import _lib as L
    args = [A + 0x1000 * i for i in range(12)]
    for C in (512, 1024, 4096):
        d = _desc(L, C=C)
        assert lib.million_pq_chunk_attn(ctypes.byref(d), *args, A, 1 << 40, None) == ERR_SHAPE and b"uint8 codes" in lib.million_last_error()
        assert lib.million_pq_chunk_attn_lse(ctypes.byref(d), *args, A, A, 1 << 40, None) == ERR_SHAPE
        assert lib.million_chunk_attn_workspace_bytes(ctypes.byref(d)) == lib.million_chunk_attn_workspace_bytes(ctypes.byref(_desc(L, C=256)))
    d = _desc(L, C=256)
    assert lib.million_pq_chunk_attn(ctypes.byref(d), *([None] * 13), 0, None) == ERR_ARG and b"null" in lib.million_last_error()
    assert lib.million_pq_chunk_attn_lse(ctypes.byref(d), *args, None, A, 1 << 40, None) == ERR_ARG and b"lse" in lib.million_last_error()


# ---------------------------------------------------------------- ops ------------------------------------------------------
def test_ops_refuse_before_the_library(monkeypatch):
    import torch
    from million_amd import ops
    monkeypatch.setattr(ops.L, "load", lambda: pytest.fail("the library was entered"))
    h = torch.float16
    q, res, ch = torch.zeros(1, 4, 3, 128, dtype=h), torch.zeros(1, 2, 64, 128, dtype=h), torch.zeros(1, 2, 3, 128, dtype=h)
    rows = torch.zeros(1, 2, 100, 64, dtype=torch.uint16)
    kpool, vpool = torch.zeros(4, 64, 64, dtype=torch.uint16), torch.zeros(4, 64, 64, dtype=torch.uint16)
    cents = torch.zeros(64, 1024, 2, dtype=h)
    ids = torch.zeros(1, 2, 2, dtype=torch.int32)
    base = dict(q=q, k_chunk=ch, v_chunk=ch, k_codes=rows, v_codes=rows, k_cents=cents, v_cents=cents, k_res=res, v_res=res)

    def wide(C=1024, M=64, n_tokens=90, **kw):
        a = dict(base)
        a.update({k: v for k, v in kw.items() if k in base})
        more = {k: v for k, v in kw.items() if k not in base}
        return ops.pq_chunk_attn_wide(*[a[n] for n in base], 0, M=M, C=C, n_tokens=n_tokens, **more)

    with pytest.raises(RuntimeError, match="device tensors"):
        wide()
    monkeypatch.setattr(ops, "_need_cuda", lambda *a: None)
    u8 = torch.zeros(1, 2, 100, 64, dtype=torch.uint8)
    with pytest.raises(RuntimeError, match="codes must be uint8"):      # the uint8 op keeps its message for uint16 codes
        ops.pq_chunk_attn(q, ch, ch, rows, rows, cents, cents, res, res, 0, M=64, C=256, n_tokens=90)
    paged = dict(k_codes=kpool, v_codes=vpool, k_page_ids=ids, v_page_ids=ids, page_size=64)
    for kw, msg in ((dict(k_codes=u8), "uint16"), (dict(v_codes=u8), "uint16"), (dict(q=q.float()), "fp16"),
                    (dict(C=512), "codebooks"), (dict(C=2048), "codebooks"), (dict(M=32), "codebooks"),       # C / M against the codebooks' shape
                    (dict(v_cents=torch.zeros(64, 512, 2, dtype=h)), "codebooks"), (dict(k_cents=cents.float()), "codebooks"),
                    (dict(k_cents=torch.zeros(64, 1024, 4, dtype=h)[:, :, ::2]), "codebooks"),
                    (dict(C=256, k_cents=cents[:, :256].contiguous(), v_cents=cents[:, :256].contiguous()), "C=256"),
                    (dict(paged, v_page_ids=ids.long()), "page ids must agree"), (dict(paged, v_page_ids=torch.zeros(1, 2, 3, dtype=torch.int32)), "page ids must agree"),
                    (dict(paged, page_size=None), "page_size"), (dict(paged, k_page_ids=ids.float()), "page ids"),
                    (dict(n_tokens=101), "n_tokens exceeds"), (dict(v_chunk=None), "go together"),
                    (dict(dev_n_q=torch.zeros(2, dtype=torch.int32)), "dev_n_q"), (dict(out=torch.zeros(1, 4, 3, 128)), "out must be")):
        with pytest.raises(RuntimeError, match=msg):
            wide(**kw)


def test_row_major_strides_are_bytes():
    import torch
    from million_amd import ops
    q, res = torch.zeros(1, 4, 3, 128, dtype=torch.float16), torch.zeros(1, 2, 64, 128, dtype=torch.float16)
    for dt, size in ((torch.uint8, 1), (torch.uint16, 2)):
        rows = torch.zeros(1, 2, 100, 64, dtype=dt)
        desc = ops.chunk_attn_desc(q, res, nh_k=2, M=64, C=256 * size * size, n_tokens=90, r=0, n_c=0, k_codes=rows, v_codes=rows)
        assert (desc.k_stride_b, desc.k_stride_h, desc.v_stride_b, desc.v_stride_h) == (2 * 6400 * size, 6400 * size) * 2


# ---------------------------------------------------------------- DynamicPQCache, launches stubbed -------------------------
def _host_cache(monkeypatch, nbits, log, M=64):
    import torch
    from million_amd import ops
    from million_amd.pq_cache import DynamicPQCache
    rec = lambda name, ret=None: (lambda *a, **k: (log.append((name, a, k)), ret(*a, **k) if ret else None)[1])
    zeros_q = lambda q, *a, **k: torch.zeros_like(q)
    monkeypatch.setattr(ops, "pq_encode_into", rec("encode"))
    monkeypatch.setattr(ops, "prefill_attn", rec("prefill_attn", lambda q, k, v, **kw: torch.zeros_like(q)))
    monkeypatch.setattr(ops, "pq_chunk_attn", rec("chunk", zeros_q))
    monkeypatch.setattr(ops, "pq_chunk_attn_wide", rec("chunk_wide", zeros_q))
    monkeypatch.setattr(ops, "pq_decode", rec("pq_decode", lambda codes, cents: torch.zeros(*codes.shape[:-1], 128, dtype=torch.float16)))
    cache = DynamicPQCache(bs=2, nh=8, num_key_value_heads=2, M=M, layer_num=2, d=128, nbits=nbits, max_tokens=256, device="cpu")
    cache.key_cent = cache.value_cent = torch.zeros(M, 2 ** nbits, 128 // M, dtype=torch.float16)
    cache._kprep = cache._vprep = None if nbits > 8 else torch.zeros(4 * 128 * 2 ** nbits, dtype=torch.float16)
    return cache


def _rows(n):
    import torch
    return torch.zeros(2, 8, n, 128, dtype=torch.float16), torch.zeros(2, 2, n, 128, dtype=torch.float16)


@pytest.mark.parametrize("nbits,M", [(9, 64), (10, 64), (12, 32)])
def test_extend_takes_the_wide_call(monkeypatch, nbits, M):
    import torch
    log = []
    cache = _host_cache(monkeypatch, nbits, log, M)
    assert cache.dtype == torch.uint16
    q, k = _rows(50)
    out = cache.extend(q, k, k, 0)                   # an empty cache: prefill()
    assert [e[0] for e in log] == ["encode", "encode", "prefill_attn"] and out.shape == q.shape and cache._T[0] == 50
    assert all(e[2]["prepared"] is None for e in log[:2])
    T = 50
    for n in (5, 70, 1):
        del log[:]
        q, k = _rows(n)
        out = cache.extend(q, k, k, 0)
        assert [e[0] for e in log] == ["chunk_wide", "encode", "encode"] and out.shape == q.shape
        name, a, kw = log[0]
        assert kw["n_tokens"] == T and (kw["M"], kw["C"]) == (M, 2 ** nbits) and a[9] == 0      # r = 0: extend leaves no window
        assert a[3] is cache._k_store[0] and a[4] is cache._v_store[0] and a[3].dtype == torch.uint16
        assert a[5] is cache.key_cent and a[6] is cache.value_cent and a[1] is k and a[2] is k
        assert [e[2]["token_start"] for e in log[1:]] == [T, T] and [e[2]["n"] for e in log[1:]] == [n, n]
        T += n
        assert cache._T[0] == T and cache.seen_tokens[0] == T and cache.residualed_tokens[0] == 0 and cache._T[1] == 0
    with pytest.raises(RuntimeError, match="max_tokens"):
        cache.extend(*[_rows(200)[i] for i in (0, 1, 1)], 0)


@pytest.mark.parametrize("nbits", [13, 14, 16])
def test_extend_past_12_bits_still_raises(monkeypatch, nbits):
    log = []
    cache = _host_cache(monkeypatch, nbits, log)
    q, k = _rows(5)
    with pytest.raises(NotImplementedError, match="9 .. 12"):
        cache.extend(q, k, k, 0)
    assert not log and cache._T[0] == 0


def test_a_uint8_cache_still_takes_the_uint8_call(monkeypatch):
    log = []
    cache = _host_cache(monkeypatch, 8, log)
    q, k = _rows(50)
    cache.extend(q, k, k, 0)
    q, k = _rows(5)
    del log[:]
    cache.extend(q, k, k, 0)
    assert [e[0] for e in log] == ["chunk", "encode", "encode"] and log[0][2]["n_tokens"] == 50 and log[0][1][5] is cache._kprep
    assert cache._T[0] == 55


# ---------------------------------------------------------------- the model ------------------------------------------------
def test_model_agrees_with_the_uint8_chunk_model_and_the_decode_model(oracle):
    """At 256 centroids the model is tests/test_chunk_attn_gpu.py's (the oracle's dequantisation); one query row without a chunk is
    wide_model.decode_attn; rows past n_q are zeros with lse -inf."""
    from tests import test_chunk_attn_gpu as U
    from tests import wide_model as W
    rs = np.random.RandomState(1)
    f = lambda *s: rs.standard_normal(s).astype(np.float16)
    bs, nh, nhk, d, M, T, cap, n_q = 2, 8, 2, 128, 64, 70, 32, 6
    q, kch, vch, kres, vres = f(bs, nh, n_q, d), f(bs, nhk, n_q, d), f(bs, nhk, n_q, d), f(bs, nhk, cap, d), f(bs, nhk, cap, d)
    for C, dt in ((256, np.uint8), (1024, np.uint16)):
        kc, vc = rs.randint(0, C, (bs, nhk, T, M)).astype(dt), rs.randint(0, C, (bs, nhk, T, M)).astype(dt)
        ck, cv = f(M, C, d // M), f(M, C, d // M)
        ring = (29 + np.arange(7)) % cap
        out, lse = CM.chunk_attn(q, kc, vc, ck, cv, kres, vres, 7, start=29, k_chunk=kch, v_chunk=vch)
        if C == 256:
            ref = U.model(oracle, q, kc, vc, ck, cv, kres[:, :, ring], vres[:, :, ring], kch, vch)
            assert np.abs(out - ref).max() < 1e-12 and np.isfinite(lse).all()
        o1, l1 = CM.chunk_attn(q[:, :, :1], kc, vc, ck, cv, kres, vres, 7, start=29)
        o2, l2 = W.decode_attn(q[:, :, :1], kc, vc, ck, cv, kres, vres, 7, start=29)
        assert np.abs(o1 - o2).max() < 1e-12 and np.abs(l1[:, :, 0] - l2).max() < 1e-12
        o3, l3 = CM.chunk_attn(q, kc, vc, ck, cv, kres, vres, [7, 0], T=[T, 0], start=[29, 0], k_chunk=kch, v_chunk=vch, n_q=[4, 0])
        assert np.array_equal(o3[0, :, :4], CM.chunk_attn(q[:1, :, :4], kc[:1], vc[:1], ck, cv, kres[:1], vres[:1], 7, start=29,
                                                          k_chunk=kch[:1, :, :4], v_chunk=vch[:1, :, :4])[0][0])
        assert not o3[0, :, 4:].any() and not o3[1].any() and np.isneginf(l3[0, :, 4:]).all() and np.isneginf(l3[1]).all()
