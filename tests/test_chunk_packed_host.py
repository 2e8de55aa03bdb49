"""CPU side of chunk attention and the row gather over packed code pages (include/million_hip.h, "Packed code pages"; DESIGN.md
4.18): the two new entries are exported and prototyped and refuse what they must before any HIP call; ops refuses before the library
is entered; the calls without packed= reach the library with the arguments they always did; million_amd.paged_turns - on CPU caches
with the launches stubbed, as tests/test_packed_host.py does - picks the op per (packed, route), checks capacity before any
launch, hands an 8-bit cache to its own methods and calls a bad route a ValueError."""
import ctypes

import pytest

from tests.test_attn_wide_host import KW, _mirror, _same
from tests.test_chunk_blocks_host import _gdesc
from tests.test_chunk_wide_host import A, ERR_ALIGN, ERR_ARG, ERR_SHAPE, ERR_WORKSPACE, _desc
from tests.test_packed_host import _packed_cache


@pytest.fixture(scope="module")
def lib():
    from million_amd import build, _lib
    build.build()
    return _lib.load()


def _chunk_call(lib, desc, **kw):
    a = dict(q=A, k_chunk=A + 0x1000, v_chunk=A + 0x2000, k_codes=A + 0x10000, v_codes=A + 0x20000, k_ids=A + 0x30000, v_ids=A + 0x30000,
             k_cents=A + 0x40000, v_cents=A + 0x50000, k_res=A + 0x60000, v_res=A + 0x70000, out=A + 0x80000, lse=None, ws=A + 0x90000,
             ws_bytes=1 << 40)
    a.update(kw)
    return lib.million_pq_chunk_attn_packed(ctypes.byref(desc), a["q"], a["k_chunk"], a["v_chunk"], a["k_codes"], a["v_codes"], a["k_ids"],
                                            a["v_ids"], a["k_cents"], a["v_cents"], a["k_res"], a["v_res"], a["out"], a["lse"], a["ws"],
                                            a["ws_bytes"], None)


def test_symbols(lib):
    from million_amd import _lib as L
    vp = ctypes.c_void_p
    assert L.SYMBOLS["million_pq_chunk_attn_packed"] == L.SYMBOLS["million_pq_chunk_attn_wide"]
    assert L.SYMBOLS["million_pq_chunk_attn_packed"] == (ctypes.c_int32, [ctypes.POINTER(L.ChunkAttnDesc)] + [vp] * 14 + [ctypes.c_size_t, vp])
    assert L.SYMBOLS["million_pq_gather_rows_packed"] == L.SYMBOLS["million_pq_gather_rows"] == (ctypes.c_int32, [ctypes.POINTER(L.GatherRowsDesc)] + [vp] * 11)
    header = (L.HERE.parent / "include" / "million_hip.h").read_text()
    for name in ("million_pq_chunk_attn_packed", "million_pq_gather_rows_packed"):
        assert name + "(" in header and hasattr(lib, name)
    assert "million_pq_gather_rows / million_pq_decode over packed pages do not exist" not in header


def test_chunk_entry_refuses_without_a_gpu(lib):
    from million_amd import _lib as L
    err = lib.million_last_error
    null = lambda d: lib.million_pq_chunk_attn_packed(ctypes.byref(d), *([None] * 14), 0, None)
    d = _desc(L)
    d.struct_size -= 8
    assert _chunk_call(lib, d) == ERR_ARG and b"struct_size" in err()
    assert lib.million_pq_chunk_attn_packed(None, *([None] * 14), 0, None) == ERR_ARG
    # a row-major side: there is no packed row-major format - MILLION_ERR_SHAPE before any pointer is looked at
    for kw in (dict(k_layout=0), dict(v_layout=0), dict(k_layout=0, v_layout=0)):
        d = _desc(L, **kw)
        assert null(d) == ERR_SHAPE and b"MILLION_KV_PAGED" in err(), kw
        assert _chunk_call(lib, d) == ERR_SHAPE, kw
    for kw in (dict(C=256), dict(C=128), dict(C=768), dict(C=8192), dict(d=128, M=128), dict(d=128, M=16), dict(d=64, M=64), dict(d=96, M=48)):
        d = _desc(L, **kw)
        assert null(d) == ERR_SHAPE and b"chunk_attn_packed" in err(), kw
    for ps in (16, 48, 256, 0):
        d = _desc(L)
        d.page_size = ps
        assert null(d) == ERR_SHAPE and b"page_size" in err(), ps
        d = _desc(L, T=0)      # no token yet: the page size is part of the format all the same
        d.page_size = ps
        assert null(d) == ERR_SHAPE and b"page_size" in err(), ps
    for kw in (dict(), dict(C=512), dict(C=4096, M=32), dict(d=64, M=32, C=2048), dict(d=64, M=16), dict(nh=64), dict(n_c=0)):
        for ps in (32, 64, 128):
            d = _desc(L, **kw)
            d.page_size, d.n_pages_cap = ps, -(-4133 // ps)
            assert null(d) == ERR_ARG and b"null" in err(), (kw, ps)
            # the same split count and workspace as the uint16 entry: one function answers for both
            need = lib.million_chunk_attn_wide_workspace_bytes(ctypes.byref(d))
            assert need > 0 and _chunk_call(lib, d, ws_bytes=need - 1) == ERR_WORKSPACE and _chunk_call(lib, d, ws=None) == ERR_WORKSPACE
    d = _desc(L)
    for part in ("q", "out", "k_chunk", "v_chunk", "k_res", "v_res", "k_codes", "v_codes", "k_cents", "v_cents", "k_ids", "v_ids"):
        assert _chunk_call(lib, d, **{part: None}) == ERR_ARG, part
    for part in ("q", "k_codes", "v_codes", "out", "k_cents"):
        assert _chunk_call(lib, d, **{part: A + 0xc0008}) == ERR_ALIGN and b"16-byte" in err(), part
    assert _chunk_call(lib, d, lse=A + 0xd0002) == ERR_ALIGN and b"lse" in err()
    bad = _desc(L)
    bad.n_pages_cap = 10
    assert _chunk_call(lib, bad) == ERR_SHAPE and b"pages" in err()
    assert _chunk_call(lib, _desc(L, n_q=0)) == 0      # nothing to do


def test_gather_entry_refuses_without_a_gpu(lib):
    ptrs = [0x1000, 0x2000, 0x3000, 0x3000, 0x4000, 0x5000, 0x6000, 0x7000, 0x8000, 0x9000]
    err = lib.million_last_error
    call = lambda d, p=ptrs: lib.million_pq_gather_rows_packed(ctypes.byref(d), *p, None)
    good = dict(C=1024, code_bytes=2)
    assert call(_gdesc(struct_size=8, **good)) == ERR_ARG and b"struct_size" in err()
    assert call(_gdesc(C=1024, code_bytes=1)) == ERR_SHAPE                                       # uint8 codes with C = 1024
    assert call(_gdesc(C=256, code_bytes=1)) == ERR_SHAPE and b"code_bytes=1" in err()           # a packed code is never one byte
    assert call(_gdesc(C=256, code_bytes=2)) == ERR_SHAPE and b"C=256" in err()
    assert call(_gdesc(M=16, **good)) == ERR_SHAPE and b"gather_rows_packed" in err()            # d / M = 8
    assert call(_gdesc(d=64, M=64, **good)) == ERR_SHAPE and b"gather_rows_packed" in err()      # d / M = 1
    for kw in (dict(k_layout=0), dict(v_layout=0), dict(k_layout=0, v_layout=0)):
        assert call(_gdesc(**good, **kw), [None] * 10) == ERR_SHAPE and b"MILLION_KV_PAGED" in err(), kw
    for ps in (16, 48, 256):
        assert call(_gdesc(page_size=ps, **good)) == ERR_SHAPE and b"page_size" in err(), ps
    assert call(_gdesc(t0=200, **good)) == ERR_ARG and b"t0=200 t1=171" in err()
    assert call(_gdesc(n_pages_cap=2, **good)) == ERR_ARG and b"n_pages_cap" in err()
    assert call(_gdesc(**good), [None] * 10) == ERR_ARG and b"null" in err()
    for i in (0, 1):      # the pools: 16-byte aligned
        p = list(ptrs)
        p[i] += 8
        assert call(_gdesc(**good), p) == ERR_ALIGN and b"16-byte" in err(), i
    for kw in (dict(C=512), dict(C=4096, M=32), dict(d=64, M=32, C=2048), dict(d=64, M=16, C=1024)):
        d = _gdesc(**dict(good, **kw))
        d.o_stride_b, d.o_stride_h, d.resid_stride_b, d.resid_stride_h = 2 * 400 * d.d, 400 * d.d, 2 * 64 * d.d, 64 * d.d
        assert call(d, [None] * 10) == ERR_ARG and b"null" in err(), kw
    assert call(_gdesc(t0=5, t1=5, r=0, **good), [None] * 10) == 0      # nothing to do


# ---------------------------------------------------------------- ops ------------------------------------------------------
class _FakeLib:
    """Records every entry point that is called; each answers MILLION_OK (workspace functions: 0 bytes)."""

    def __init__(self):
        self.calls = []

    def __getattr__(self, name):
        return lambda *a: (self.calls.append((name, a)), 0)[1]


def _chunk_inputs(torch, ops, M=64, C=1024, ps=64):
    h = torch.float16
    pb = ops.packed_page_bytes(ps, M, C)
    return dict(q=torch.zeros(1, 4, 3, 128, dtype=h), k_chunk=torch.zeros(1, 2, 3, 128, dtype=h), v_chunk=torch.zeros(1, 2, 3, 128, dtype=h),
                k_codes=torch.zeros(4, pb, dtype=torch.uint8), v_codes=torch.zeros(4, pb, dtype=torch.uint8),
                k_cents=torch.zeros(M, C, 128 // M, dtype=h), v_cents=torch.zeros(M, C, 128 // M, dtype=h),
                k_res=torch.zeros(1, 2, 64, 128, dtype=h), v_res=torch.zeros(1, 2, 64, 128, dtype=h))


def test_ops_chunk_refuses_before_the_library(monkeypatch):
    import torch
    from million_amd import ops
    monkeypatch.setattr(ops.L, "load", lambda: pytest.fail("the library was entered"))
    base = _chunk_inputs(torch, ops)
    ids = torch.zeros(1, 2, 2, dtype=torch.int32)
    pb = ops.packed_page_bytes(64, 64, 1024)

    def packed(C=1024, M=64, n_tokens=90, page_size=64, k_page_ids=ids, v_page_ids=ids, **kw):
        a = dict(base)
        a.update({k: v for k, v in kw.items() if k in base})
        more = {k: v for k, v in kw.items() if k not in base}
        return ops.pq_chunk_attn_packed(*[a[n] for n in base], 0, M=M, C=C, n_tokens=n_tokens, page_size=page_size, k_page_ids=k_page_ids,
                                        v_page_ids=v_page_ids, **more)

    with pytest.raises(RuntimeError, match="device tensors"):
        packed()
    monkeypatch.setattr(ops, "_need_cuda", lambda *a: None)
    u16 = torch.zeros(4, 64, 64, dtype=torch.uint16)
    small = torch.zeros(64, 256, 2, dtype=torch.float16)
    for kw, msg in ((dict(k_page_ids=None), "pages only"), (dict(v_page_ids=None), "pages only"), (dict(k_page_ids=None, v_page_ids=None), "pages only"),
                    (dict(k_codes=u16), "packed pool must be"), (dict(v_codes=u16), "packed pool must be"),
                    (dict(k_codes=torch.zeros(4, pb + 16, dtype=torch.uint8)), "packed pool must be"),      # a wrong page_bytes
                    (dict(v_codes=torch.zeros(4, 64, 80, dtype=torch.uint8)), "packed pool must be"),
                    (dict(k_codes=torch.zeros(4, 2 * pb, dtype=torch.uint8)[:, ::2]), "contiguous"),
                    (dict(page_size=32), "packed pool must be"),                                           # the pools are those of pages of 64
                    (dict(page_size=16), "page_size=16"), (dict(page_size=None), "page_size"),
                    (dict(C=256, k_cents=small, v_cents=small), "C=256"), (dict(C=2048), "packed pool must be"),
                    (dict(M=32), "packed pool must be"), (dict(k_cents=base["k_cents"].float()), "codebooks"),
                    (dict(v_page_ids=ids.long()), "page ids must agree"), (dict(q=base["q"].float()), "fp16"),
                    (dict(v_chunk=None), "go together"), (dict(dev_n_q=torch.zeros(2, dtype=torch.int32)), "dev_n_q")):
        with pytest.raises(RuntimeError, match=msg):
            packed(**kw)


def test_ops_chunk_reaches_the_packed_entry(monkeypatch):
    import torch
    from million_amd import ops
    fake = _FakeLib()
    monkeypatch.setattr(ops.L, "load", lambda: fake)
    monkeypatch.setattr(ops, "_need_cuda", lambda *a: None)
    monkeypatch.setattr(ops, "_stream", lambda: 0)
    for M, C, ps in ((64, 1024, 64), (32, 4096, 128), (64, 512, 32)):
        a = _chunk_inputs(torch, ops, M, C, ps)
        ids = torch.zeros(1, 2, 2, dtype=torch.int64)
        for lse in (False, True):
            del fake.calls[:]
            ops.pq_chunk_attn_packed(*a.values(), 0, M=M, C=C, n_tokens=40, k_page_ids=ids, v_page_ids=ids, page_size=ps, return_lse=lse)
            assert [c[0] for c in fake.calls] == ["million_chunk_attn_wide_workspace_bytes", "million_pq_chunk_attn_packed"]
            args = fake.calls[1][1]
            desc = args[0]._obj
            assert (desc.k_layout, desc.v_layout, desc.page_size, desc.page_ids_i64, desc.M, desc.C) == (1, 1, ps, 1, M, C)
            assert args[4] == a["k_codes"].data_ptr() and args[5] == a["v_codes"].data_ptr() and args[8] == a["k_cents"].data_ptr()
            assert (args[13] is not None) == lse
    # the uint16 op still goes where it went
    del fake.calls[:]
    a = _chunk_inputs(torch, ops)
    a["k_codes"] = a["v_codes"] = torch.zeros(4, 64, 64, dtype=torch.uint16)
    ids = torch.zeros(1, 2, 2, dtype=torch.int32)
    ops.pq_chunk_attn_wide(*a.values(), 0, M=64, C=1024, n_tokens=40, k_page_ids=ids, v_page_ids=ids, page_size=64)
    assert [c[0] for c in fake.calls] == ["million_chunk_attn_wide_workspace_bytes", "million_pq_chunk_attn_wide"]


def _gather_inputs(torch, ops, packed, M=64, C=1024, ps=64, d=128):
    h = torch.float16
    pools = ((torch.zeros(4, ops.packed_page_bytes(ps, M, C), dtype=torch.uint8),) * 2 if packed else
             (torch.zeros(4, ps, M, dtype=torch.uint16), torch.zeros(4, M, ps, dtype=torch.uint16)))
    return dict(k_codes=pools[0], v_codes=pools[1], k_cents=torch.zeros(M, C, d // M, dtype=h), v_cents=torch.zeros(M, C, d // M, dtype=h),
                k_out=torch.zeros(1, 2, 200, d, dtype=h), v_out=torch.zeros(1, 2, 200, d, dtype=h))


def test_ops_gather_packed_flag(monkeypatch):
    import torch
    from million_amd import ops
    monkeypatch.setattr(ops, "_need_cuda", lambda *a: None)
    monkeypatch.setattr(ops, "_stream", lambda: 0)
    monkeypatch.setattr(ops.L, "load", lambda: pytest.fail("the library was entered"))
    ids = torch.zeros(1, 2, 2, dtype=torch.int32)
    a = _gather_inputs(torch, ops, True)
    call = lambda **kw: ops.pq_gather_rows(*[kw.get(n, v) for n, v in a.items()], t0=3, t1=90, packed=True,
                                           **{"k_page_ids": ids, "v_page_ids": ids, "page_size": 64, **{k: v for k, v in kw.items() if k not in a}})
    u16 = _gather_inputs(torch, ops, False)
    small = torch.zeros(64, 256, 2, dtype=torch.float16)
    for kw, msg in ((dict(k_codes=u16["k_codes"]), "packed pool must be"), (dict(v_codes=u16["v_codes"]), "packed pool must be"),
                    (dict(k_codes=torch.zeros(4, 5136, dtype=torch.uint8)), "packed pool must be"), (dict(page_size=32), "packed pool must be"),
                    (dict(page_size=16), "page_size=16"), (dict(k_page_ids=None), "pages only"), (dict(v_page_ids=None), "pages only"),
                    (dict(k_cents=small, v_cents=small), "C=256"),
                    (dict(k_cents=torch.zeros(16, 1024, 8, dtype=torch.float16), v_cents=torch.zeros(16, 1024, 8, dtype=torch.float16),
                          k_codes=torch.zeros(4, 64 * 16 * 10 // 8, dtype=torch.uint8), v_codes=torch.zeros(4, 64 * 16 * 10 // 8, dtype=torch.uint8)), "d / M")):
        with pytest.raises(RuntimeError, match=msg):
            call(**kw)
    with pytest.raises(RuntimeError, match="C=1024 does not go with torch.uint8"):      # without the flag a uint8 pool means 8-bit codes
        ops.pq_gather_rows(*a.values(), t0=3, t1=90, k_page_ids=ids, v_page_ids=ids, page_size=64)
    with pytest.raises(TypeError):      # keyword-only
        ops.pq_gather_rows(*a.values(), 3, 90)
    fake = _FakeLib()
    monkeypatch.setattr(ops.L, "load", lambda: fake)
    assert call() == 87
    (name, args), = fake.calls
    desc = args[0]._obj
    assert name == "million_pq_gather_rows_packed" and (desc.code_bytes, desc.k_layout, desc.v_layout, desc.page_size, desc.C, desc.t0, desc.t1) == (2, 1, 1, 64, 1024, 3, 90)
    assert args[1] == a["k_codes"].data_ptr() and args[3] == ids.data_ptr() and args[5] == a["k_cents"].data_ptr()
    # without the flag: the entry, the descriptor and the pointers the call always had - uint16 pools, and uint8 codes with C <= 256
    for inp, cb in ((u16, 2), (dict(_gather_inputs(torch, ops, False, C=256), k_codes=torch.zeros(4, 64, 64, dtype=torch.uint8),
                                    v_codes=torch.zeros(4, 64, 64, dtype=torch.uint8)), 1)):
        del fake.calls[:]
        assert ops.pq_gather_rows(*inp.values(), t0=3, t1=90, k_page_ids=ids, v_page_ids=ids, page_size=64) == 87
        (name, args), = fake.calls
        desc = args[0]._obj
        assert name == "million_pq_gather_rows" and len(args) == 12 and (desc.code_bytes, desc.k_layout, desc.v_layout, desc.t0, desc.t1) == (cb, 1, 1, 3, 90)
        assert args[1:7] == (inp["k_codes"].data_ptr(), inp["v_codes"].data_ptr(), ids.data_ptr(), ids.data_ptr(), inp["k_cents"].data_ptr(),
                             inp["v_cents"].data_ptr())


def test_ops_blocks_passes_the_flag_to_the_gather_only(monkeypatch):
    import torch
    from million_amd import ops
    monkeypatch.setattr(ops, "_need_cuda", lambda *a: None)
    log = []
    monkeypatch.setattr(ops, "pq_gather_rows", lambda *a, **k: (log.append(("gather", a, k)), k["t1"] - k["t0"] + k["r"])[1])
    monkeypatch.setattr(ops, "prefill_attn", lambda *a, **k: log.append(("prefill", a, k)))
    monkeypatch.setattr(ops, "attn_merge", lambda *a, **k: log.append(("merge", a, k)))
    ids = torch.zeros(1, 2, 4, dtype=torch.int32)
    kw = dict(M=64, C=1024, n_tokens=200, k_page_ids=ids, v_page_ids=ids, page_size=64, block_tokens=64)
    shapes = []
    for packed in (False, True):
        a = _chunk_inputs(torch, ops)
        if not packed:
            a["k_codes"], a["v_codes"] = torch.zeros(4, 64, 64, dtype=torch.uint16), torch.zeros(4, 64, 64, dtype=torch.uint16)
        del log[:]
        ops.pq_chunk_attn_blocks(*a.values(), 5, **kw, **({"packed": True} if packed else {}))
        gathers = [e for e in log if e[0] == "gather"]
        assert [e[0] for e in log] == ["gather", "prefill"] * 4 + ["prefill", "merge"]
        for e in gathers:
            assert ("packed" in e[2]) == packed and e[2].get("packed", False) == packed      # without the flag: the keywords the gather always got
            assert e[1][0] is a["k_codes"] and e[1][1] is a["v_codes"] and e[1][2] is a["k_cents"] and e[1][3] is a["v_cents"]
        shapes.append([(e[0], {k: v for k, v in e[2].items() if k in ("t0", "t1", "r", "resid_start", "causal", "page_size")}) for e in log])
    assert shapes[0] == shapes[1]      # nothing else in the route changes
    # a uint8 pool without the flag still means uint8 codes behind PREPARED codebooks
    a = _chunk_inputs(torch, ops)
    with pytest.raises(RuntimeError, match="prepared"):
        ops.pq_chunk_attn_blocks(*a.values(), 5, **kw)


# ---------------------------------------------------------------- paged_turns, launches stubbed ----------------------------
def _turn_caches(monkeypatch, nbits, log, packed):
    import torch
    from million_amd import ops
    cache = _packed_cache(monkeypatch, nbits, log, packed=packed)
    if not packed and nbits > 8:      # _packed_cache(packed=False) builds tests/test_attn_wide_host.py's cache of this nbits
        assert cache.key_page_pool.dtype == torch.uint16
    rec = lambda name: (lambda q, *a, **k: (log.append((name, dict(k, args=(q,) + a))),
                                            (torch.zeros_like(q), torch.zeros(q.shape[:3])) if k.get("return_lse") else torch.zeros_like(q))[1])
    for name in ("pq_chunk_attn_wide", "pq_chunk_attn_packed", "pq_chunk_attn_blocks"):
        monkeypatch.setattr(ops, name, rec(name))
    return cache


def _rows(bs, n):
    import torch
    return torch.zeros(bs, 4, n, 128, dtype=torch.float16), torch.zeros(bs, 2, n, 128, dtype=torch.float16)


@pytest.mark.parametrize("packed", [True, False], ids=["packed", "uint16"])
@pytest.mark.parametrize("route", [None, "chunk", "blocks"])
def test_turns_pick_the_op(monkeypatch, packed, route):
    from million_amd import paged_turns
    log = []
    cache = _turn_caches(monkeypatch, 10, log, packed)
    enc = "encode_packed" if packed else "encode"
    want = "pq_chunk_attn_blocks" if route == "blocks" else ("pq_chunk_attn_packed" if packed else "pq_chunk_attn_wide")
    q, k = _rows(2, 50)
    out = paged_turns.extend(cache, q, k, k, 0, route=route)      # an empty cache: prefill()
    assert [e[0] for e in log] == [enc, enc, "prefill_attn"] and out.shape == q.shape and cache._T_a[0].tolist() == [50, 50]
    T = 50
    for n in (5, 1):
        del log[:]
        q, k = _rows(2, n)
        out = paged_turns.extend(cache, q, k, k, 0, route=route)
        assert [e[0] for e in log] == [want, enc, enc] and out.shape == q.shape
        kw = log[0][1]
        assert (kw["n_tokens"], kw["M"], kw["C"], kw["page_size"], kw["resid_start"]) == (T, 64, 1024, 32, 0) and kw["args"][9] == 0
        assert kw["args"][3] is cache.key_page_pool and kw["args"][4] is cache.value_page_pool
        assert kw["args"][5] is cache.key_cent and kw["args"][6] is cache.value_cent and kw["args"][1] is k
        assert kw["k_page_ids"].shape[0] == 2 and kw["k_page_ids"] is kw["v_page_ids"]
        assert kw.get("packed", False) == (packed and route == "blocks") and ("packed" in kw) == (packed and route == "blocks")
        assert [e[1]["token_start"] for e in log[1:]] == [T, T] and [e[1]["n"] for e in log[1:]] == [n, n]
        T += n
        assert cache._T_a[0].tolist() == [T, T] and not cache._r_a.any() and cache._T_a[1].tolist() == [0, 0]
    # one slot: batch-1 tensors, its own row of the table, the other slot untouched
    del log[:]
    q, k = _rows(1, 7)
    out, lse = paged_turns.extend_request(cache, 1, q, k, k, 0, return_lse=True, route=route)
    assert [e[0] for e in log] == [want, enc, enc] and out.shape == q.shape and lse.shape == q.shape[:3]
    assert log[0][1]["return_lse"] is True and log[0][1]["k_page_ids"].shape[0] == 1 and log[0][1]["n_tokens"] == T
    assert cache._T_a[0].tolist() == [T, T + 7]
    with pytest.raises(RuntimeError, match="different lengths"):
        paged_turns.extend(cache, *[_rows(2, 1)[i] for i in (0, 1, 1)], 0, route=route)
    # an empty slot: prefill_request - with lse, chunk attention over the chunk alone whatever the route
    del log[:]
    q, k = _rows(1, 9)
    paged_turns.extend_request(cache, 0, q, k, k, 1, route=route)
    assert [e[0] for e in log] == [enc, enc, "prefill_attn"] and cache._T_a[1].tolist() == [9, 0]
    del log[:]
    paged_turns.extend_request(cache, 1, q, k, k, 1, return_lse=True, route=route)
    assert [e[0] for e in log] == ["pq_chunk_attn_packed" if packed else "pq_chunk_attn_wide", enc, enc] and log[0][1]["n_tokens"] == 0
    assert cache._T_a[1].tolist() == [9, 9]
    with pytest.raises(RuntimeError, match="batch 1"):
        paged_turns.extend_request(cache, 0, *[_rows(2, 1)[i] for i in (0, 1, 1)], 0)


@pytest.mark.parametrize("packed", [True, False], ids=["packed", "uint16"])
def test_turns_check_route_and_capacity_before_any_launch(monkeypatch, packed):
    from million_amd import paged_turns
    log = []
    cache = _turn_caches(monkeypatch, 12, log, packed)
    q, k = _rows(2, 40)
    paged_turns.extend(cache, q, k, k, 0)
    before, n_log = _mirror(cache), len(log)
    for call in (lambda r: paged_turns.extend(cache, q, k, k, 0, route=r), lambda r: paged_turns.extend_request(cache, 0, q[:1], k[:1], k[:1], 0, route=r)):
        for r in ("block", "", "wide", 3):
            with pytest.raises(ValueError, match="route"):
                call(r)
    big = _rows(2, KW["max_tokens"] - 40 + 1)
    with pytest.raises(RuntimeError, match="max_tokens"):
        paged_turns.extend(cache, big[0], big[1], big[1], 0)
    with pytest.raises(RuntimeError, match="max_tokens"):
        paged_turns.extend_request(cache, 1, big[0][:1], big[1][:1], big[1][:1], 0, route="blocks")
    with pytest.raises(RuntimeError, match="max_tokens"):      # an empty layer: before prefill's encode too
        paged_turns.extend(cache, *[_rows(2, KW["max_tokens"] + 1)[i] for i in (0, 1, 1)], 1)
    assert _same(before, _mirror(cache)) and len(log) == n_log
    # the cache's own methods keep refusing
    with pytest.raises(NotImplementedError, match="nbits"):
        cache.extend(q, k, k, 0)
    with pytest.raises(NotImplementedError, match="nbits"):
        cache.extend_request(0, q[:1], k[:1], k[:1], 0)
    assert _same(before, _mirror(cache)) and len(log) == n_log


def test_turns_delegate_an_8_bit_cache(monkeypatch):
    from million_amd import paged_turns
    log = []
    cache = _turn_caches(monkeypatch, 8, log, False)
    calls = []
    monkeypatch.setattr(cache, "extend", lambda *a, **k: calls.append(("extend", a, k)) or "E")
    monkeypatch.setattr(cache, "extend_request", lambda *a, **k: calls.append(("extend_request", a, k)) or "R")
    q, k = _rows(2, 5)
    assert paged_turns.extend(cache, q, k, k, 1, route="blocks") == "E"
    assert paged_turns.extend_request(cache, 1, q[:1], k[:1], k[:1], 0, return_lse=True) == "R"
    assert calls[0][1] == (q, k, k, 1) and calls[0][2] == dict(route="blocks")
    assert calls[1][1][0] == 1 and calls[1][1][4] == 0 and calls[1][2] == dict(return_lse=True, route=None)
    assert not log
