"""CPU side of the log-sum-exp surface (include/million_hip.h, "Log-sum-exp"; million_attn_merge): the merge formula of
tests/lse_ref.py is exact on exact partials, the three new entries exist and validate their arguments without touching a
GPU, and the kernels' arithmetic for the lse - restated in fp32 with fp16-rounded probabilities feeding the denominator -
leaves the GPU test half of its bar on the same inputs."""
import ctypes

import numpy as np
import pytest

from tests import decode_poison as P
from tests import lse_ref as R


# ---------------------------------------------------------------- the merge formula ----------------------------------------
def _context(seed, n=301, d=16, rows=5):
    rs = np.random.RandomState(seed)
    q, K, V = rs.standard_normal((rows, d)), rs.standard_normal((n, d)), rs.standard_normal((n, d))
    return q @ K.T / np.sqrt(d), V


@pytest.mark.parametrize("cuts", [(120,), (7, 200)])
def test_merge_of_exact_partials_is_the_whole(cuts):
    s, V = _context(1)
    whole = R.softmax_state(s, V)
    edges = (0,) + cuts + (s.shape[1],)
    parts = [R.softmax_state(s[:, a:b], V[a:b]) for a, b in zip(edges[:-1], edges[1:])]
    out, lse = R.merge([p[0] for p in parts], [p[1] for p in parts])
    assert np.abs(out - whole[0]).max() <= 1e-12 and np.abs(lse - whole[1]).max() <= 1e-12


def test_merge_is_associative_through_lse_out():
    s, V = _context(2)
    a, b, c = (R.softmax_state(s[:, x:y], V[x:y]) for x, y in ((0, 50), (50, 210), (210, 301)))
    flat = R.merge([a[0], b[0], c[0]], [a[1], b[1], c[1]])
    ab = R.merge([a[0], b[0]], [a[1], b[1]])
    left = R.merge([ab[0], c[0]], [ab[1], c[1]])
    bc = R.merge([b[0], c[0]], [b[1], c[1]])
    right = R.merge([a[0], bc[0]], [a[1], bc[1]])
    for got in (left, right):
        assert np.abs(got[0] - flat[0]).max() <= 1e-12 and np.abs(got[1] - flat[1]).max() <= 1e-12


def test_merge_with_empty_parts():
    s, V = _context(3)
    a, b = R.softmax_state(s[:, :100], V[:100]), R.softmax_state(s[:, 100:], V[100:])
    e = R.softmax_state(s[:, :0], V[:0])
    assert np.all(e[0] == 0) and np.all(np.isneginf(e[1]))
    whole = R.softmax_state(s, V)
    out, lse = R.merge([e[0], a[0], e[0], b[0]], [e[1], a[1], e[1], b[1]])      # some parts -inf
    assert np.abs(out - whole[0]).max() <= 1e-12 and np.abs(lse - whole[1]).max() <= 1e-12
    junk = np.full_like(e[0], 1e30)                                              # a -inf part's out is never used
    out, lse = R.merge([junk, a[0]], [e[1], a[1]])
    assert np.array_equal(out, a[0]) and np.array_equal(lse, a[1])
    out, lse = R.merge([e[0], junk], [e[1], e[1]])                               # all of them
    assert np.all(out == 0) and np.all(np.isneginf(lse))
    bad = a[1].copy()
    bad[2] = np.nan                                                              # a NaN lse: that row is NaN, the others are not
    out, lse = R.merge([a[0], b[0]], [bad, b[1]])
    assert np.isnan(out[2]).all() and np.isnan(lse[2]) and np.isfinite(np.delete(out, 2, 0)).all() and np.isfinite(np.delete(lse, 2)).all()


def test_reference_lse_is_the_oracles(oracle):
    """decode_ref's lse is the lse the C oracle has returned all along, on a case with a wrapped ring and an append."""
    c = P.BY_NAME["lean-d64-M32-C128"]
    built = P.build(c)
    out, lse = R.decode_ref(c, built, oracle)
    cl = built["clean"]
    kw = np.concatenate([np.roll(cl["k_res"], -c.rs, axis=2)[:, :, :c.r], cl["k_new"]], axis=2)
    vw = np.concatenate([np.roll(cl["v_res"], -c.rs, axis=2)[:, :, :c.r], cl["v_new"]], axis=2)
    g, gl = oracle.decode_attn(cl["q"], built["k_codes"], built["v_codes"], cl["k_cents"], cl["v_cents"], kw, vw, c.r + 1,
                               return_lse=True)
    assert np.abs(out - g).max() <= 1e-9 * np.abs(g).max()
    assert np.abs(lse - gl).max() <= 1e-9


# ---------------------------------------------------------------- the entries -----------------------------------------------
@pytest.fixture(scope="module")
def lib():
    from million_amd import build, _lib
    build.build()
    return _lib.load()


def test_symbols_and_argument_types(lib):
    from million_amd import _lib as L
    vp, sz = ctypes.c_void_p, ctypes.c_size_t
    res, args = L.SYMBOLS["million_pq_decode_attn_lse"]
    assert res is ctypes.c_int32 and args == [ctypes.POINTER(L.AttnDesc)] + [vp] * 14 + [sz, vp]
    assert len(args) == len(L.SYMBOLS["million_pq_decode_attn_append"][1]) + 1
    res, args = L.SYMBOLS["million_pq_chunk_attn_lse"]
    assert res is ctypes.c_int32 and args == [ctypes.POINTER(L.ChunkAttnDesc)] + [vp] * 14 + [sz, vp]
    assert len(args) == len(L.SYMBOLS["million_pq_chunk_attn"][1]) + 1
    res, args = L.SYMBOLS["million_attn_merge"]
    assert res is ctypes.c_int32 and args == [ctypes.POINTER(L.AttnMergeDesc), ctypes.POINTER(vp), ctypes.POINTER(vp), vp, vp, vp]
    for name in ("million_pq_decode_attn_lse", "million_pq_chunk_attn_lse", "million_attn_merge"):
        assert getattr(lib, name) is not None
    # the descriptor as include/million_hip.h lays it out: 6 words, then 8 x 3 + 8 x 3 + 3 + 3 strides of 8 bytes
    assert ctypes.sizeof(L.AttnMergeDesc) == 24 + 8 * (2 * 3 * L.MILLION_MERGE_MAX_PARTS + 6) and L.MILLION_MERGE_MAX_PARTS == 8
    assert lib.million_version() == 1      # additive: the version and the other structs stay
    assert ctypes.sizeof(L.AttnDesc) == 136


def _merge_desc(L, n_parts=2, d=128, bs=1, nh=4, n_q=1):
    desc = L.AttnMergeDesc()
    desc.struct_size = ctypes.sizeof(L.AttnMergeDesc)
    desc.n_parts, desc.bs, desc.nh, desc.n_q, desc.d = n_parts, bs, nh, n_q, d
    for i in range(L.MILLION_MERGE_MAX_PARTS):
        desc.out_stride[i][0], desc.out_stride[i][1], desc.out_stride[i][2] = nh * n_q * d, n_q * d, d
        desc.lse_stride[i][0], desc.lse_stride[i][1], desc.lse_stride[i][2] = nh * n_q, n_q, 1
    desc.res_out_stride[0], desc.res_out_stride[1], desc.res_out_stride[2] = nh * n_q * d, n_q * d, d
    desc.res_lse_stride[0], desc.res_lse_stride[1], desc.res_lse_stride[2] = nh * n_q, n_q, 1
    return desc


def _merge_call(lib, L, desc, outs=None, lses=None, out=0x10000):
    """Host-side validation only: the pointers are made-up device addresses, never dereferenced by a call that is refused."""
    n = max(desc.n_parts, 1)
    outs = [0x20000 + 0x1000 * i for i in range(n)] if outs is None else outs
    lses = [0x80000 + 0x1000 * i for i in range(n)] if lses is None else lses
    po, pl = (ctypes.c_void_p * len(outs))(*outs), (ctypes.c_void_p * len(lses))(*lses)
    return lib.million_attn_merge(ctypes.byref(desc), po, pl, out, None, None)


ERR_ARG, ERR_SHAPE, ERR_ALIGN = -3, -1, -2


def test_error_codes_are_the_headers():
    import re
    from pathlib import Path
    text = (Path(__file__).resolve().parents[1] / "include" / "million_hip.h").read_text()
    for name, val in (("MILLION_ERR_ARG", ERR_ARG), ("MILLION_ERR_SHAPE", ERR_SHAPE), ("MILLION_ERR_ALIGN", ERR_ALIGN)):
        m = re.search(rf"{name}\s*=?\s*(-?\d+)", text)
        assert m and int(m.group(1)) == val, name


def test_attn_merge_refuses_without_a_gpu(lib):
    from million_amd import _lib as L
    d = _merge_desc(L)
    d.struct_size -= 8
    assert _merge_call(lib, L, d) == ERR_ARG and b"struct_size" in lib.million_last_error()
    for n in (0, 9):
        d = _merge_desc(L, n_parts=n)
        assert _merge_call(lib, L, d) == ERR_ARG and b"n_parts" in lib.million_last_error()
    assert _merge_call(lib, L, _merge_desc(L, d=96)) == ERR_SHAPE and b"d=96" in lib.million_last_error()
    assert _merge_call(lib, L, _merge_desc(L), outs=[0x20000, None]) == ERR_ARG and b"part 1" in lib.million_last_error()
    assert _merge_call(lib, L, _merge_desc(L), lses=[None, 0x80000]) == ERR_ARG and b"part 0" in lib.million_last_error()
    d = _merge_desc(L)
    d.out_stride[1][2] = 132      # an odd stride: not a multiple of 8 elements
    assert _merge_call(lib, L, d) == ERR_ALIGN and b"stride" in lib.million_last_error()
    d = _merge_desc(L)
    d.res_out_stride[1] = 4
    assert _merge_call(lib, L, d) == ERR_ALIGN
    assert _merge_call(lib, L, _merge_desc(L), outs=[0x20000, 0x21008]) == ERR_ALIGN and b"aligned" in lib.million_last_error()
    assert _merge_call(lib, L, _merge_desc(L), out=None) == ERR_ARG


def test_decode_attn_lse_refuses_a_null_lse(lib):
    from million_amd import _lib as L
    c = P.BY_NAME["lean-d128-M64-ps64-C256"]
    desc = P.make_desc(c, L)
    a = 0x100000      # made-up aligned device addresses: the call is refused before anything is read
    rc = lib.million_pq_decode_attn_lse(ctypes.byref(desc), a, None, None, a, a, a, a, a, a, a, a, a, None, a, 1 << 30, None)
    assert rc == ERR_ARG and b"lse" in lib.million_last_error()
    cd = L.ChunkAttnDesc()
    cd.struct_size = ctypes.sizeof(L.ChunkAttnDesc)
    rc = lib.million_pq_chunk_attn_lse(ctypes.byref(cd), a, None, None, a, a, a, a, a, a, a, a, a, None, None, 0, None)
    assert rc == ERR_ARG and b"lse" in lib.million_last_error()


# ---------------------------------------------------------------- numerics ---------------------------------------------------
# Measured (profiles/attn_lse.txt): the emulation's worst error over the heads sampled here.
@pytest.mark.parametrize("cname", [c.name for c in P.CASES])
def test_lse_arithmetic_leaves_half_the_bar(cname, oracle):
    """The inputs of test_attn_lse_gpu.py section a.: on the first head of the first request and the last head of the last one,
    an fp32 evaluation with fp16-rounded probabilities in the denominator is within half the LSE bar of the fp64 reference,
    so a kernel that misses the bar is wrong by more than its number formats explain."""
    c = P.BY_NAME[cname]
    built = P.build(c)
    K, _ = R.keys_of_decode(c, built, oracle)
    _, lse = R.decode_ref(c, built, oracle)
    q = built["clean"]["q"]
    G = c.nh // c.nhk
    worst = 0.0
    for b, h in ((0, 0), (c.bs - 1, c.nh - 1)):
        got = R.lse_model_f32(q[b, h, 0], K[b, h // G])
        worst = max(worst, abs(got - lse[b, h]))
    print(f"{cname}: emulated lse error {worst:.3e}")
    assert worst <= 0.5 * R.LSE_TOL, f"{cname}: emulated lse off by {worst:.3e}"
