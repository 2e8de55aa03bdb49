"""CPU side of the one-launch flush and ragged store of wide code pages (include/million_hip.h: million_pq_flush_wide,
million_pq_store_ragged_wide): the symbols are prototyped, both entries refuse bad shapes, alignments and nulls
before any HIP call with messages that name the entry, ops refuses before the library is entered, and the two jobs of
ops.CodeFormat hand each op its keywords - the 8-bit jobs are the pq_flush / pq_store_ragged calls they always were.  The numpy
rule the GPU tests compare with is checked against hand-written expectations."""
import ctypes

import numpy as np
import pytest

from tests import ragged_wide_common as R

ERR_ARG, ERR_SHAPE, ERR_ALIGN = -3, -1, -2
A = 0x100000      # made-up aligned device addresses: a refused call dereferences nothing


@pytest.fixture(scope="module")
def lib():
    from million_amd import build, _lib
    build.build()
    return _lib.load()


def test_symbols(lib):
    from million_amd import _lib as L
    vp, i32 = ctypes.c_void_p, ctypes.c_int32
    assert L.SYMBOLS["million_pq_flush_wide"] == (i32, [ctypes.POINTER(L.EncodeDesc)] + [vp] * 8 + [i32, i32, i32, vp])
    assert L.SYMBOLS["million_pq_store_ragged_wide"] == (i32, [ctypes.POINTER(L.StoreRaggedDesc)] + [vp] * 11 + [i32, vp])
    header = (L.HERE.parent / "include" / "million_hip.h").read_text()
    for name in ("million_pq_flush_wide", "million_pq_store_ragged_wide"):
        assert name + "(" in header and hasattr(lib, name)


# ---------------------------------------------------------------- million_pq_flush_wide ------------------------------------
def _fdesc(L, d=128, M=64, C=1024, n=32, ps=32, cap=64, bs=3, nhk=2, npc=16, dev=None, **kw):
    x = L.EncodeDesc()
    x.struct_size = ctypes.sizeof(L.EncodeDesc)
    x.bs, x.nh_k, x.n, x.d, x.M, x.C = bs, nhk, n, d, M, C
    x.x_stride_b, x.x_stride_h, x.x_stride_n = nhk * cap * d, cap * d, d
    x.x_row_start, x.x_row_mod = 0, cap
    x.dst_layout, x.dst_token_start = L.MILLION_CODES_KPAGES, 0
    x.page_size, x.n_pages_cap = ps, npc
    x.dev_lengths = dev
    for k, v in kw.items():
        setattr(x, k, v)
    return x


def _flush(lib, desc, cap=64, min_r=0, packed=0, **kw):
    a = dict(k_rows=A, v_rows=A + 0x10000, k_cents=A + 0x20000, v_cents=A + 0x30000, k_pool=A + 0x40000, v_pool=A + 0x50000,
             ids=A + 0x60000, dev=desc.dev_lengths)
    a.update(kw)
    return lib.million_pq_flush_wide(ctypes.byref(desc), a["k_rows"], a["v_rows"], a["k_cents"], a["v_cents"], a["k_pool"], a["v_pool"],
                                     a["ids"], a["dev"], cap, min_r, packed, None)


def test_flush_wide_refuses_without_a_gpu(lib):
    from million_amd import _lib as L
    err = lib.million_last_error
    d = _fdesc(L)
    d.struct_size -= 8
    assert _flush(lib, d) == ERR_ARG and b"flush_wide" in err() and b"struct_size" in err()
    assert lib.million_pq_flush_wide(None, *([None] * 8), 64, 0, 0, None) == ERR_ARG
    shapes = [dict(C=256), dict(C=300), dict(C=8192), dict(d=128, M=16), dict(d=96, M=48), dict(d=128, M=128), dict(ps=48), dict(ps=256),
              dict(n=33), dict(ps=64, n=65), dict(n=-1), dict(bs=0), dict(nhk=0), dict(bs=20000), dict(npc=0), dict(npc=2 ** 27)]
    for kw in shapes:
        d = _fdesc(L, **kw)
        assert lib.million_pq_flush_wide(ctypes.byref(d), *([None] * 8), 64, 0, 0, None) == ERR_SHAPE, kw      # before any null pointer
        assert _flush(lib, d) == ERR_SHAPE and b"flush_wide" in err(), kw
        assert _flush(lib, d, packed=1) == ERR_SHAPE and b"flush_wide" in err(), kw
    for kw in (dict(), dict(C=512), dict(C=4096, M=32), dict(d=64, M=32, C=2048), dict(d=64, M=16, C=512), dict(ps=64, cap=128, n=64), dict(ps=128, cap=128, n=100)):
        for packed in (0, 1):
            d = _fdesc(L, **kw)
            cap = kw.get("cap", 64)
            assert lib.million_pq_flush_wide(ctypes.byref(d), *([None] * 8), cap, 0, packed, None) == ERR_ARG and b"flush_wide: null" in err(), kw
    assert lib.million_pq_flush_wide(ctypes.byref(_fdesc(L, n=0)), *([None] * 8), 64, 0, 0, None) == 0      # nothing to flush, whatever the pointers
    d = _fdesc(L)
    for part in ("k_rows", "v_rows", "k_cents", "v_cents", "k_pool", "v_pool", "ids"):
        assert _flush(lib, d, **{part: None}) == ERR_ARG and b"null" in err(), part
    for part in ("k_rows", "v_rows", "k_cents", "v_cents", "k_pool", "v_pool"):
        assert _flush(lib, d, **{part: A + 0xc0008}) == ERR_ALIGN and b"flush_wide" in err() and b"16-byte" in err(), part
    assert _flush(lib, d, ids=A + 0x60002) == ERR_ALIGN and b"4-byte" in err()
    assert _flush(lib, _fdesc(L, x_stride_n=132)) == ERR_ALIGN and b"strides" in err()
    # the arguments around the descriptor
    assert _flush(lib, _fdesc(L, dst_layout=L.MILLION_CODES_ROWMAJOR)) == ERR_ARG and b"KPAGES" in err()
    assert _flush(lib, d, cap=0) == ERR_ARG and _flush(lib, d, cap=128) == ERR_ARG and b"x_row_mod" in err()
    assert _flush(lib, _fdesc(L, ps=64, cap=32, n=64), cap=32) == ERR_ARG and b"resid_cap" in err()      # a ring shorter than the flush
    assert _flush(lib, d, dev=A + 0x70000) == ERR_ARG and b"dev_lengths must equal" in err()
    dv = _fdesc(L, dev=A + 0x70000)
    assert _flush(lib, dv, min_r=65) == ERR_ARG and _flush(lib, dv, min_r=-1) == ERR_ARG and b"min_r" in err()
    assert _flush(lib, _fdesc(L, dev=A + 0x70002), min_r=64) == ERR_ALIGN
    # the host-length form checks what the device form clamps
    assert _flush(lib, _fdesc(L, dst_token_start=-1)) == ERR_ARG and b"dst_token_start" in err()
    assert _flush(lib, _fdesc(L, dst_token_start=512 - 31)) == ERR_ARG and b"too short" in err()
    assert _flush(lib, _fdesc(L, x_row_start=64)) == ERR_ARG and _flush(lib, _fdesc(L, x_row_start=-1)) == ERR_ARG and b"x_row_start" in err()
    assert _flush(lib, _fdesc(L, dev=A + 0x70000, dst_token_start=-1, x_row_start=99), k_rows=None) == ERR_ARG and b"null" in err()      # not read with device lengths


# ---------------------------------------------------------------- million_pq_store_ragged_wide -----------------------------
def _sdesc(L, d=128, M=64, C=1024, ps=32, cap=64, bs=3, nhk=2, npc=16, nb=40, **kw):
    x = L.StoreRaggedDesc()
    x.struct_size = ctypes.sizeof(L.StoreRaggedDesc)
    x.bs, x.nh_k, x.d, x.M, x.C, x.n_bound = bs, nhk, d, M, C, nb
    x.kn_stride_b, x.kn_stride_h, x.kn_stride_n = nhk * nb * d, nb * d, d
    x.vn_stride_b, x.vn_stride_h, x.vn_stride_n = nhk * nb * d, nb * d, d
    x.resid_cap, x.page_size, x.n_pages_cap = cap, ps, npc
    x.resid_stride_b, x.resid_stride_h = nhk * cap * d, cap * d
    for k, v in kw.items():
        setattr(x, k, v)
    return x


STORE_PARTS = ("k_new", "v_new", "k_res", "v_res", "k_cents", "v_cents", "k_pool", "v_pool", "ids", "lengths", "dev_n")


def _store(lib, desc, packed=0, **kw):
    a = {name: A + 0x10000 * i for i, name in enumerate(STORE_PARTS)}
    a.update(kw)
    return lib.million_pq_store_ragged_wide(ctypes.byref(desc), *[a[n] for n in STORE_PARTS], packed, None)


def test_store_ragged_wide_refuses_without_a_gpu(lib):
    from million_amd import _lib as L
    err = lib.million_last_error
    d = _sdesc(L)
    d.struct_size -= 8
    assert _store(lib, d) == ERR_ARG and b"store_ragged_wide" in err()
    assert lib.million_pq_store_ragged_wide(None, *([None] * 11), 0, None) == ERR_ARG
    for kw in (dict(C=256), dict(C=300), dict(C=8192), dict(d=128, M=16), dict(d=96, M=48), dict(ps=48), dict(bs=0), dict(nhk=0), dict(nb=-1),
               dict(bs=20000), dict(npc=0), dict(npc=2 ** 27)):
        d = _sdesc(L, **kw)
        assert lib.million_pq_store_ragged_wide(ctypes.byref(d), *([None] * 11), 0, None) == ERR_SHAPE, kw      # before any null pointer
        assert _store(lib, d) == ERR_SHAPE and b"store_ragged_wide" in err(), kw
        assert _store(lib, d, packed=1) == ERR_SHAPE, kw
    assert lib.million_pq_store_ragged_wide(ctypes.byref(_sdesc(L, nb=0)), *([None] * 11), 0, None) == 0      # no request can have a row
    assert _store(lib, _sdesc(L, resid_cap=-1)) == ERR_ARG
    for kw in (dict(), dict(C=512), dict(C=4096, M=32), dict(d=64, M=32, C=2048), dict(ps=128)):
        for packed in (0, 1):
            d = _sdesc(L, **kw)
            for part in STORE_PARTS:
                assert _store(lib, d, packed, **{part: None}) == ERR_ARG and b"store_ragged_wide: null" in err(), (kw, part)
    d = _sdesc(L)
    for part in STORE_PARTS[:8]:
        assert _store(lib, d, **{part: A + 0xc0008}) == ERR_ALIGN and b"store_ragged_wide" in err() and b"16-byte" in err(), part
    for part in STORE_PARTS[8:]:
        assert _store(lib, d, **{part: A + 0xc0002}) == ERR_ALIGN and b"4-byte" in err(), part
    assert _store(lib, _sdesc(L, kn_stride_n=132)) == ERR_ALIGN and b"strides" in err()
    # the uint8 entry answers a wide codebook as it did
    assert lib.million_pq_store_ragged(ctypes.byref(_sdesc(L)), *([A] * 11), None) == ERR_SHAPE and b"uint8 codes" in err()


# ---------------------------------------------------------------- ops ------------------------------------------------------
def _ops_args(torch, packed=False, M=64, C=1024, d=128):
    from million_amd import ops
    win, new = torch.zeros(3, 2, 64, d, dtype=torch.float16), torch.zeros(3, 2, 40, d, dtype=torch.float16)
    cents = torch.zeros(M, C, d // M, dtype=torch.float16)
    if packed:
        kp = vp = torch.zeros(8, ops.packed_page_bytes(32, M, C), dtype=torch.uint8)
    else:
        kp, vp = torch.zeros(8, 32, M, dtype=torch.uint16), torch.zeros(8, M, 32, dtype=torch.uint16)
    return dict(win=win, new=new, cents=cents, kp=kp, vp=vp, ids=torch.zeros(3, 2, 16, dtype=torch.int32),
                lengths=torch.zeros(3, 4, dtype=torch.int32), dev_n=torch.zeros(3, dtype=torch.int32))


def test_ops_refuse_before_the_library(monkeypatch):
    import torch
    from million_amd import ops
    monkeypatch.setattr(ops.L, "load", lambda: pytest.fail("the library was entered"))
    a = _ops_args(torch)
    with pytest.raises(RuntimeError, match="device tensors"):
        ops.pq_flush_wide(a["win"], a["win"], a["cents"], a["cents"], a["kp"], a["vp"], a["ids"], n=32, page_size=32)
    with pytest.raises(RuntimeError, match="device tensors"):
        ops.pq_store_ragged_wide(a["new"], a["new"], a["win"], a["win"], a["cents"], a["cents"], a["kp"], a["vp"], a["ids"], a["lengths"], a["dev_n"],
                                 M=64, C=1024, page_size=32)
    monkeypatch.setattr(ops, "_need_cuda", lambda *a: None)
    for packed in (False, True):
        a = _ops_args(torch, packed)

        def flush(n=32, page_size=32, packed=packed, **kw):
            g = lambda name: kw.get(name, a[name])
            return ops.pq_flush_wide(g("win"), kw.get("v_win", a["win"]), g("cents"), g("cents"), g("kp"), g("vp"), g("ids"), n=n,
                                     page_size=page_size, dev_lengths=kw.get("lengths"), min_r=0, packed=packed)

        def store(packed=packed, M=64, C=1024, **kw):
            g = lambda name: kw.get(name, a[name])
            return ops.pq_store_ragged_wide(g("new"), kw.get("v_new", a["new"]), g("win"), kw.get("v_win", a["win"]), g("cents"), g("cents"), g("kp"),
                                            g("vp"), g("ids"), g("lengths"), g("dev_n"), M=M, C=C, page_size=32, packed=packed)

        u8 = torch.zeros(8, 32, 64, dtype=torch.uint8)
        both = [(dict(cents=a["cents"].float()), "codebooks"), (dict(cents=torch.zeros(64, 256, 2, dtype=torch.float16)), "C=256"),
                (dict(cents=torch.zeros(64, 300, 2, dtype=torch.float16)), "C=300"), (dict(cents=torch.zeros(32, 1024, 2, dtype=torch.float16)), "d=128"),
                (dict(ids=a["ids"].long()), "page_ids"), (dict(ids=a["ids"][:2]), "page_ids"), (dict(win=a["win"].float()), "fp16"),
                (dict(kp=a["kp"][:, :-1]), "k_pool" if not packed else "packed pool"), (dict(lengths=torch.zeros(3, 4)), "dev_lengths")]
        if not packed:
            both += [(dict(kp=u8, vp=u8), "8-bit codes"), (dict(vp=torch.zeros(8, 32, 64, dtype=torch.uint16).transpose(1, 2)), "contiguous"),
                     (dict(vp=torch.zeros(8, 32, 64, dtype=torch.uint16)), r"v_pool must be \(n_pool, 64, 32\)"),
                     (dict(vp=torch.zeros(8, 64, 32, dtype=torch.uint8)), "both sides alike")]
        else:
            u16 = torch.zeros(8, 32, 64, dtype=torch.uint16)
            both += [(dict(kp=u16, vp=u16), "packed pool")]
        for kw, msg in both:
            with pytest.raises(RuntimeError, match="pq_flush_wide.*" + msg):
                flush(**kw)
            if "win" in kw:
                msg = "windows must be"
            with pytest.raises(RuntimeError, match="pq_store_ragged_wide.*" + msg):
                store(**kw)
        for kw, msg in ((dict(n=33), "n=33"), (dict(n=-1), "n=-1"), (dict(v_win=a["win"][:, :, :32]), "same shape")):
            with pytest.raises(RuntimeError, match="pq_flush_wide.*" + msg):
                flush(**kw)
        for kw, msg in ((dict(M=32), "M=32"), (dict(C=512), "C=512"), (dict(dev_n=torch.zeros(3)), "dev_n"), (dict(v_new=a["new"][:, :, :8]), "one shape"),
                        (dict(new=a["new"].float()), "fp16"), (dict(win=a["win"][:, :1]), "windows must be")):
            with pytest.raises(RuntimeError, match="pq_store_ragged_wide.*" + msg):
                store(**kw)
        if packed:
            with pytest.raises(RuntimeError, match="page_size=48"):
                flush(page_size=48, n=32)


def test_the_jobs_hand_each_op_its_keywords(monkeypatch):
    from million_amd import ops
    log = []
    for name in ("pq_flush", "pq_flush_wide", "pq_store_ragged", "pq_store_ragged_wide"):
        monkeypatch.setattr(ops, name, lambda *a, _n=name, **k: log.append((_n, a, k)))
    cents, prep = ("kc", "vc"), ("kp", "vp")
    fkw = dict(n=32, page_size=32, token_start=45, x_row_start=40, dev_lengths="len", min_r=64)
    skw = dict(M=64, C=1024, page_size=32)
    for fmt, flush, store, first, extra in ((ops.FMT_U8, "pq_flush", "pq_store_ragged", prep, {}),
                                           (ops.FMT_U16, "pq_flush_wide", "pq_store_ragged_wide", cents, dict(packed=False)),
                                           (ops.FMT_PACKED, "pq_flush_wide", "pq_store_ragged_wide", cents, dict(packed=True))):
        del log[:]
        fmt.flush_pages("kw", "vw", cents, "kpool", "vpool", "ids", **fkw)
        fmt.store_ragged_pages("kn", "vn", "kr", "vr", cents, prep, "kpool", "vpool", "ids", "len", "dev_n", **skw)
        assert log == [(flush, ("kw", "vw", "kc", "vc", "kpool", "vpool", "ids"), dict(fkw, **extra)),
                       (store, ("kn", "vn", "kr", "vr", *first, "kpool", "vpool", "ids", "len", "dev_n"), dict(skw, **extra))], fmt.name
    assert [(f.flush, f.store_ragged) for f in ops.CODE_FORMATS] == [("million_pq_flush_layers", "million_pq_store_ragged")] + \
        [("million_pq_flush_wide", "million_pq_store_ragged_wide")] * 2


# ---------------------------------------------------------------- the rule of the GPU tests --------------------------------
def test_flush_rule_by_hand():
    p = R.FlushPlan((45, 64, 40), 32, 64)
    assert p.live and p.ring.tolist() == list(range(40, 64)) + list(range(8)) and p.tokens.tolist() == list(range(45, 77)) and p.kept.all()
    assert p.after == (77, 32, 8)
    p = R.FlushPlan((33, 17, 5), 32, 64)
    assert not p.live and p.after == (33, 17, 5)
    p = R.FlushPlan((R.INT_MAX, 1000, -1), 32, 64)
    assert p.live and (p.T, p.r, p.start) == (512, 64, 0) and not p.kept.any() and p.after == (512, 32, 32)
    p = R.FlushPlan((502, 64, 70), 32, 64)
    assert p.kept.sum() == 10 and p.ring[0] == 0 and p.after == (512, 32, 32)
    # the numpy pools take codes the way both formats store them: what goes in comes out, nothing else changes
    rs = np.random.RandomState(0)
    ids = rs.permutation(40)[:32].reshape(2, 16)
    for M, C in ((64, 1024), (32, 4096)):
        kc, vc = rs.randint(0, C, (2, 32, M)).astype(np.uint16), rs.randint(0, C, (2, 32, M)).astype(np.uint16)
        for packed in (False, True):
            pools = R.fill_pools(40, M, C, packed)
            R.put(pools, ids, 45 + np.arange(32), np.arange(32) != 7, kc, vc, M, C, packed)
            k, v = R.codes_of(pools, ids, 45, 77, M, C, packed)
            keep = np.arange(32) != 7
            assert np.array_equal(k[:, keep], kc[:, keep]) and np.array_equal(v[:, keep], vc[:, keep])
            fresh = R.fill_pools(40, M, C, packed)
            untouched = np.setdiff1d(np.arange(40), ids[:, 1:3].ravel())
            assert all(np.array_equal(p[untouched], f[untouched]) for p, f in zip(pools, fresh))
