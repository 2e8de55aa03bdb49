"""Far addresses on the GPU, second file (tests/big_address.py): the kernels and kernel instances that do their own address
arithmetic and came after tests/test_big_address_gpu.py - decode and chunk attention over 16-bit codes, pq_gather_rows at both
code widths, pq_encode_into to uint16 pages, prompt attention with lse, the merges over far views, the block route, a wide
PagedPQCache past 4 GiB.  The contract is that file's: every call runs on a compact twin (twice) and through page ids and
strides that put its bytes past 2^31 and 2^32 bytes from the base of a 4 GiB buffer; what it writes is bitwise the twin's, the
twin is held against the suite's fp64 model of the op at that op's bar, every far table passes _assert_far, and a sentinel
scan of both buffers follows.  The fixtures and helpers are that file's, imported: its module-scoped buffers are dropped with
it, so the two files never hold them together.

A pool of 2-byte codes is the same 4 GiB seen as uint16: its page ids reach byte 2^31 and byte 2^32 at half the values of a
uint8 pool, and an offset kept as a 32-bit index of code words wraps exactly at byte 2^32 (tests/test_big_address_host.py)."""
import gc
import zlib

import numpy as np
import pytest

from tests import big_address as BA
from tests import chunk_blocks_model as B
from tests import chunk_wide_model as CM
from tests import lse_ref, sink_model, synth
from tests import verify_model as VM
from tests import verify_tree_model as VT
from tests import wide_model as W
from tests.test_big_address_gpu import NEED_FREE, S16, _assert_far, _bits, _cu, _far_pools, _far_table, _same, env, far, flat_store  # noqa: F401
from tests.test_chunk_attn_gpu import _state as chunk_state

pytestmark = pytest.mark.gpu
TOL = 1e-3      # the suite's attention bar: rel-L2 and mean-abs of every (request, head) against fp64


def _heads(got, ref, what):
    g = got.float().cpu().numpy()
    rel, mabs = W.head_errors(g, np.asarray(ref))
    print(f"BIGADDR {what}: worst (request, head) rel-L2 {rel.max():.3e}, mean-abs {mabs.max():.3e}")
    assert np.isfinite(g).all() and rel.max() < TOL and mabs.max() < TOL, \
        f"{what}: worst rel-L2 {rel.max():.3e} mean-abs {mabs.max():.3e} at {np.unravel_index(rel.argmax(), rel.shape)}"


def _lse_close(got, ref, what):
    err = CM.lse_error(got.cpu().numpy().reshape(np.asarray(ref).shape), ref)      # -inf exactly where the model's is
    print(f"BIGADDR {what}: worst |lse - model| {err:.3e}")
    assert err < lse_ref.LSE_TOL, f"{what}: lse off by {err:.3e}"


def _pools(k_codes, v_codes, ps, fill=0):
    """Row-major codes (bs, nh_k, T, M) of any width -> (K pool (n, ps, M), V pool (n, M, ps), ids arange (bs, nh_k, n_pages))."""
    bs, nhk, T, M = k_codes.shape
    npg = max(1, -(-T // ps))
    pad = np.full((bs, nhk, npg * ps - T, M), fill, k_codes.dtype)
    kp = np.concatenate([k_codes, pad], axis=2).reshape(bs * nhk * npg, ps, M)
    vp = np.concatenate([v_codes, pad], axis=2).reshape(bs * nhk * npg, ps, M).transpose(0, 2, 1)
    return np.ascontiguousarray(kp), np.ascontiguousarray(vp), np.arange(bs * nhk * npg).reshape(bs, nhk, npg)


def _from_pools(kpool, vpool, ids, T):
    return B.from_pools(kpool, vpool, ids, T)


def _sentinel_pool(torch, dt, n, *tail):
    """A compact pool of the sentinel: the twin of a writer starts as the far buffers do."""
    if dt == torch.uint8:
        return torch.full((n, *tail), BA.SENTINEL, dtype=torch.uint8, device="cuda")
    return torch.full((n, *tail), S16, dtype=torch.int16, device="cuda").view(torch.uint16)


def _host(t):
    return t.cpu().numpy()


def _reset(*views):
    """Views of the far buffers back to the sentinel, whatever their element type."""
    import torch
    for v in views:
        if v.element_size() == 2:
            v.view(torch.int16).fill_(S16)
        elif v.element_size() == 1:
            v.fill_(BA.SENTINEL)
        else:
            v.view(torch.int32).fill_(int.from_bytes(bytes([BA.SENTINEL]) * 4, "little", signed=True))


def _fill(view, src):
    view.copy_(src)
    return view


# ------------------------------------------------------------------------------------- 1. wide decode attention, far pages ---
# name, d, M, C, ps, G
WIDE_FORMS = [("d128-M64-C1024", 128, 64, 1024, 64, 4), ("d128-M32-C4096", 128, 32, 4096, 128, 16),
              ("d64-M32-C512", 64, 32, 512, 64, 7), ("d64-M16-C2048", 64, 16, 2048, 32, 16)]
WIDE_BY = {f[0]: f for f in WIDE_FORMS}
_wide_cases = {}


def _wide_case(form, T, r, cap=128):
    """Inputs of one wide decode call and its fp64 model, with and without the appended row: drawn and computed once."""
    key = (form[0], T, r)
    if key not in _wide_cases:
        name, d, M, C, ps, G = form
        bs, nhk, _ = BA.TABLE
        rs_ = np.random.RandomState(zlib.crc32(name.encode()) % 10000 + T)
        f = lambda *s: rs_.standard_normal(s).astype(np.float16)
        c = dict(q=f(bs, nhk * G, 1, d), k_cents=f(M, C, d // M), v_cents=f(M, C, d // M),
                 k_codes=rs_.randint(0, C, (bs, nhk, T, M)).astype(np.uint16), v_codes=rs_.randint(0, C, (bs, nhk, T, M)).astype(np.uint16),
                 k_res=f(bs, nhk, cap, d), v_res=f(bs, nhk, cap, d), k_new=f(bs, nhk, 1, d), v_new=f(bs, nhk, 1, d))
        assert T == 0 or (c["k_codes"].max() >= 256 and c["v_codes"].max() >= 256)
        model = lambda app: W.decode_attn(c["q"], c["k_codes"], c["v_codes"], c["k_cents"], c["v_cents"], c["k_res"], c["v_res"], r, T=T,
                                          k_new=c["k_new"] if app else None, v_new=c["v_new"] if app else None)
        _wide_cases[key] = (c, {False: model(False), True: model(True)})
    return _wide_cases[key]


def _wide_decode_pair(torch, ops, far, form, *, i64=False, lse=False, append=False):
    name, d, M, C, ps, G = form
    bs, nhk, npg = BA.TABLE
    assert (ps, M) in BA.WIDE_GEOMS
    T, r, cap, Bp = npg * ps - 7, 17, 128, ps * M * 2
    c, models = _wide_case(form, T, r, cap)
    kpool_c, vpool_c, ids_c = _pools(c["k_codes"], c["v_codes"], ps)
    assert ids_c.shape == BA.TABLE
    fid, tab_far = _far_table(torch, ids_c, Bp, 11, i64)
    assert BA.sensitive_rows(fid[ids_c], Bp, 31, 2).all()      # a 31-bit offset in code words: byte 2^32
    kpc, vpc = _cu(torch, kpool_c), _cu(torch, vpool_c)
    kbig, vbig = _far_pools(torch, far, ps, M, kpc, vpc, fid, code_bytes=2)
    tab_c = _cu(torch, ids_c.astype(np.int64 if i64 else np.int32))
    t = {k: _cu(torch, v) for k, v in c.items()}

    def call(kpool, vpool, tab):
        kr, vr = t["k_res"].clone(), t["v_res"].clone()
        dl = torch.tensor([[T, r, 0, 0]] * bs, dtype=torch.int32, device="cuda") if append else None
        res = ops.pq_decode_attn_wide(t["q"], kpool, vpool, t["k_cents"], t["v_cents"], kr, vr, r, n_tokens=T, page_ids=tab, page_size=ps,
                                      out=torch.full_like(t["q"], float("nan")), dev_lengths=dl, k_new=t["k_new"] if append else None,
                                      v_new=t["v_new"] if append else None, return_lse=lse)
        torch.cuda.synchronize()
        out, l = res if lse else (res, None)
        return dict(out=out, lse=l, k_res=kr, v_res=vr, lengths=dl)

    twin, twin2, got = call(kpc, vpc, tab_c), call(kpc, vpc, tab_c), call(kbig, vbig, tab_far)
    assert ops.tail_faults() == 0
    gold, gold_lse = models[append]
    vs_out = lambda o, what: _heads(o, gold, what)
    vs_out(twin["out"], f"wide decode {name} twin")
    _same(got["out"], twin["out"], twin2["out"], f"wide decode {name} i64={i64} out", vs_out)
    if lse:
        vs_lse = lambda l, what: _lse_close(l, gold_lse, what)
        vs_lse(twin["lse"], f"wide decode {name} twin lse")
        _same(got["lse"], twin["lse"], twin2["lse"], f"wide decode {name} i64={i64} lse", vs_lse)
    if append:      # the window row and the lengths row the call writes
        kres, vres = c["k_res"].copy(), c["v_res"].copy()
        kres[:, :, r], vres[:, :, r] = c["k_new"][:, :, 0], c["v_new"][:, :, 0]
        np.testing.assert_array_equal(_host(twin["k_res"]), kres)
        np.testing.assert_array_equal(_host(twin["v_res"]), vres)
        assert twin["lengths"].cpu().tolist() == [[T, r + 1, 0, 0]] * bs
        for nm in ("k_res", "v_res", "lengths"):
            assert _bits(got[nm]) == _bits(twin[nm]), f"{name}: {nm} after the far call differs from the twin's"
    # the call reads the pools and writes none of them
    BA.assert_only_these_pages(kbig, fid, kpc, far[0], f"wide decode {name} K pool")
    BA.assert_only_these_pages(vbig, fid, vpc, far[1], f"wide decode {name} V pool")


@pytest.mark.parametrize("i64", [False, True], ids=["i32", "i64"])
@pytest.mark.parametrize("form", WIDE_FORMS, ids=[f[0] for f in WIDE_FORMS])
def test_wide_decode_far_pages(form, i64, env, far):
    """pq_decode_attn_wide reads uint16 K pages and transposed V pages on both sides of byte 2^31 and byte 2^32 of its pools,
    through int32 ids and through the low dwords of int64 ids."""
    torch, ops = env
    _wide_decode_pair(torch, ops, far, form, i64=i64)


def test_wide_decode_far_pages_lse(env, far):
    torch, ops = env
    _wide_decode_pair(torch, ops, far, WIDE_BY["d128-M64-C1024"], lse=True)


def test_wide_decode_far_pages_append_device_lengths(env, far):
    torch, ops = env
    _wide_decode_pair(torch, ops, far, WIDE_BY["d128-M32-C4096"], append=True)


# ------------------------------------------------------------------------------------ 2. wide decode attention, far window ---
@pytest.mark.parametrize("T", [633, 0], ids=["T633", "T0-window-only"])
def test_wide_decode_far_window(T, env, far):
    """k_res / v_res whose batch stride puts request 1 past element 2^31 (byte 2^32), with the fused append writing into that
    window (tile_wave.h); T = 0: the window alone.  The pools are compact."""
    torch, ops = env
    name, d, M, C, ps, G = WIDE_FORMS[0]
    bs, nhk, _ = BA.TABLE
    r, cap = 17, 128
    c, models = _wide_case(WIDE_FORMS[0], T, r, cap)
    t = {k: _cu(torch, v) for k, v in c.items()}
    kpool_c, vpool_c, ids_c = _pools(c["k_codes"], c["v_codes"], ps)
    kpc, vpc, tab = _cu(torch, kpool_c), _cu(torch, vpool_c), _cu(torch, ids_c.astype(np.int32))
    sb = BA.far_stride(nhk * cap * d)
    shape, strides = (bs, nhk, cap, d), (sb, cap * d, d, 1)
    kres_far, vres_far = BA.far_view(far[0], shape, strides, torch.float16), BA.far_view(far[1], shape, strides, torch.float16)
    assert kres_far.stride(0) * 2 > 2 ** 32

    def call(kr, vr):
        out = ops.pq_decode_attn_wide(t["q"], kpc, vpc, t["k_cents"], t["v_cents"], kr, vr, r, n_tokens=T, page_ids=tab, page_size=ps,
                                      out=torch.full_like(t["q"], float("nan")), k_new=t["k_new"], v_new=t["v_new"])
        torch.cuda.synchronize()
        return out

    def twin_call():
        kr, vr = t["k_res"].clone(), t["v_res"].clone()
        return call(kr, vr), kr, vr

    (o1, kr1, vr1), (o2, _, _) = twin_call(), twin_call()
    _fill(kres_far, t["k_res"]); _fill(vres_far, t["v_res"])
    og = call(kres_far, vres_far)
    assert ops.tail_faults() == 0
    kres, vres = c["k_res"].copy(), c["v_res"].copy()
    kres[:, :, r], vres[:, :, r] = c["k_new"][:, :, 0], c["v_new"][:, :, 0]
    vs = lambda o, what: _heads(o, models[True][0], what)
    vs(o1, f"wide decode far window T={T} twin")
    np.testing.assert_array_equal(_host(kr1), kres)
    np.testing.assert_array_equal(_host(vr1), vres)
    _same(og, o1, o2, f"wide decode far window T={T}", vs)
    assert _bits(kres_far) == _bits(kr1) and _bits(vres_far) == _bits(vr1), "the far window after the append differs from the twin's"
    _reset(kres_far, vres_far)
    assert BA.only_sentinel(far[0]) and BA.only_sentinel(far[1])


# ------------------------------------------------------------------------------------------------ 3. wide chunk attention ---
def _chunk16(seed, bs, nh, nhk, d, M, C, n_q, T, cap):
    rs_ = np.random.RandomState(seed)
    f = lambda *s: rs_.standard_normal(s).astype(np.float16)
    st = dict(q=f(bs, nh, n_q, d), k_cents=f(M, C, d // M), v_cents=f(M, C, d // M),
              k_codes=rs_.randint(0, C, (bs, nhk, T, M)).astype(np.uint16), v_codes=rs_.randint(0, C, (bs, nhk, T, M)).astype(np.uint16),
              k_res=f(bs, nhk, cap, d), v_res=f(bs, nhk, cap, d), k_ch=f(bs, nhk, n_q, d), v_ch=f(bs, nhk, n_q, d))
    assert st["k_codes"].max() >= 256 and st["v_codes"].max() >= 256
    return st


def _chunk16_model(st, r, rstart, T=None, n_q=None):
    return CM.chunk_attn(st["q"], st["k_codes"], st["v_codes"], st["k_cents"], st["v_cents"], st["k_res"], st["v_res"], r, T=T, start=rstart,
                         k_chunk=st["k_ch"], v_chunk=st["v_ch"], n_q=n_q)


@pytest.mark.parametrize("n_q", [1, 16])
@pytest.mark.parametrize("i64", [False, True], ids=["i32", "i64"])
@pytest.mark.parametrize("d,M,C,ps", [(128, 64, 1024, 64), (64, 16, 2048, 32)], ids=["d128-M64-C1024", "d64-M16-C2048"])
def test_wide_chunk_attn_far_pages_and_strides(d, M, C, ps, i64, n_q, env, far):
    """pq_chunk_attn_wide over far uint16 pages; q, k_chunk, v_chunk and out with request 1 past element 2^31: request 0 in the
    first pages of the pools' buffers (the far ids keep clear of them), request 1 in the bytes past the pools' last page."""
    torch, ops = env
    bs, nhk, npg = BA.TABLE
    assert (ps, M) in BA.WIDE_GEOMS
    G, r, cap, rstart, Bp = 4, 40, 64, 50, ps * M * 2
    nh, T = G * nhk, npg * ps - 7
    st = _chunk16(300 + n_q + d, bs, nh, nhk, d, M, C, n_q, T, cap)
    kpool_c, vpool_c, ids_c = _pools(st["k_codes"], st["v_codes"], ps)
    dt = np.int64 if i64 else np.int32
    qn, cn = nh * n_q * d, nhk * n_q * d
    low = -(-(qn + cn) * 2 // Bp) + 1
    fid = BA.far_ids(bs * nhk * npg + low + 8, Bp, 21)
    fid = fid[fid >= low][:bs * nhk * npg]
    tabn = fid[ids_c]
    _assert_far(tabn, Bp)
    assert BA.sensitive_rows(tabn, Bp, 31, 2).all()
    kpc, vpc = _cu(torch, kpool_c), _cu(torch, vpool_c)
    kbig, vbig = _far_pools(torch, far, ps, M, kpc, vpc, fid, code_bytes=2)
    t = {k: _cu(torch, v) for k, v in st.items()}
    sb = BA.n_pool(Bp) * Bp // 2      # fp16 elements from page 0 to the first byte past the pool
    assert sb > 2 ** 31 and sb % 8 == 0 and (qn + cn) * 2 <= low * Bp and fid.min() >= low and (qn + cn) * 2 <= BA.FLAT_BYTES - 2 * sb
    mk = lambda flat, off, heads: BA.far_view(flat[2 * off:], (bs, heads, n_q, d), (sb, n_q * d, d, 1), torch.float16)
    q_far, kch_far, out_far, vch_far = mk(far[0], 0, nh), mk(far[0], qn, nhk), mk(far[1], 0, nh), mk(far[1], qn, nhk)
    _fill(q_far, t["q"]); _fill(kch_far, t["k_ch"]); _fill(vch_far, t["v_ch"])

    def call(q, kch, vch, kpool, vpool, tab, out):
        res = ops.pq_chunk_attn_wide(q, kch, vch, kpool, vpool, t["k_cents"], t["v_cents"], t["k_res"], t["v_res"], r, M=M, C=C, n_tokens=T,
                                     resid_start=rstart, k_page_ids=tab, v_page_ids=tab, page_size=ps, out=out)
        torch.cuda.synchronize()
        return res

    tab_c, tab_far = _cu(torch, ids_c.astype(dt)), _cu(torch, tabn.astype(dt))
    new_out = lambda: torch.full((bs, nh, n_q, d), float("nan"), dtype=torch.float16, device="cuda")
    twin = call(t["q"], t["k_ch"], t["v_ch"], kpc, vpc, tab_c, new_out())
    twin2 = call(t["q"], t["k_ch"], t["v_ch"], kpc, vpc, tab_c, new_out())
    got = call(q_far, kch_far, vch_far, kbig, vbig, tab_far, out_far)
    assert got.data_ptr() == out_far.data_ptr() and out_far.stride(0) > 2 ** 31
    gold, _ = _chunk16_model(st, r, rstart)
    vs = lambda o, what: _heads(o, gold, what)
    vs(twin, "wide chunk twin")
    _same(got, twin, twin2, f"wide chunk far pages d={d} i64={i64} n_q={n_q}", vs)
    _reset(q_far, kch_far, out_far, vch_far)
    BA.assert_only_these_pages(kbig, fid, kpc, far[0], "wide chunk K pool")
    BA.assert_only_these_pages(vbig, fid, vpc, far[1], "wide chunk V pool")


@pytest.mark.parametrize("n_q", [1, 16])
def test_wide_chunk_attn_far_window_and_rowmajor_strides(n_q, env, far):
    """pq_chunk_attn_wide with row-major uint16 K and V codes whose batch stride in bytes passes 2^32, and k_res / v_res whose
    batch stride puts request 1 past element 2^31."""
    torch, ops = env
    bs, nh, nhk, d, M, C, T, r, cap, rstart = 2, 8, 2, 128, 64, 1024, 633, 40, 64, 50
    st = _chunk16(400 + n_q, bs, nh, nhk, d, M, C, n_q, T, cap)
    t = {k: _cu(torch, v) for k, v in st.items()}
    sb, ksb, woff = BA.far_stride(nhk * cap * d), BA.HI + 64, 1 << 18
    assert nhk * T * M * 2 <= 2 * woff
    mk_res = lambda flat: BA.far_view(flat[2 * woff:], (bs, nhk, cap, d), (sb, cap * d, d, 1), torch.float16)
    mk_codes = lambda flat: BA.far_view(flat, (bs, nhk, T, M), (ksb // 2, T * M, M, 1), torch.uint16)
    kres_far, vres_far, kc_far, vc_far = mk_res(far[0]), mk_res(far[1]), mk_codes(far[0]), mk_codes(far[1])
    assert kres_far.stride(0) * 2 > 2 ** 32 and kc_far.stride(0) * 2 > 2 ** 32 and 2 ** 31 < kc_far.stride(0) < 2 ** 32
    _fill(kres_far, t["k_res"]); _fill(vres_far, t["v_res"]); _fill(kc_far, t["k_codes"]); _fill(vc_far, t["v_codes"])

    def call(kc, vc, kr, vr):
        out = ops.pq_chunk_attn_wide(t["q"], t["k_ch"], t["v_ch"], kc, vc, t["k_cents"], t["v_cents"], kr, vr, r, M=M, C=C, n_tokens=T,
                                     resid_start=rstart, out=torch.full((bs, nh, n_q, d), float("nan"), dtype=torch.float16, device="cuda"))
        torch.cuda.synchronize()
        return out

    twin, twin2 = (call(t["k_codes"], t["v_codes"], t["k_res"], t["v_res"]) for _ in range(2))
    got = call(kc_far, vc_far, kres_far, vres_far)
    gold, _ = _chunk16_model(st, r, rstart)
    vs = lambda o, what: _heads(o, gold, what)
    vs(twin, "wide chunk far strides twin")
    _same(got, twin, twin2, f"wide chunk far window and row-major strides n_q={n_q}", vs)
    assert _bits(kres_far) == _bits(t["k_res"]) and _bits(vres_far) == _bits(t["v_res"])
    assert _bits(kc_far) == _bits(t["k_codes"]) and _bits(vc_far) == _bits(t["v_codes"])
    _reset(kres_far, vres_far, kc_far, vc_far)
    assert BA.only_sentinel(far[0]) and BA.only_sentinel(far[1])


def test_wide_chunk_attn_far_pages_ragged_lse(env, far):
    """One ragged call with its lse: per-request lengths and query counts read on the device, far uint16 pages."""
    torch, ops = env
    bs, nhk, npg = BA.TABLE
    d, M, C, G, ps, cap, n_q = 128, 64, 1024, 4, 64, 64, 16
    nh, T, Bp = G * nhk, npg * ps - 7, ps * M * 2
    lens, nq = [[T, 40, 50, 0], [T - 300, 9, 3, 0]], [16, 5]
    st = _chunk16(31, bs, nh, nhk, d, M, C, n_q, T, cap)
    kpool_c, vpool_c, ids_c = _pools(st["k_codes"], st["v_codes"], ps)
    fid, tab_far = _far_table(torch, ids_c, Bp, 23)
    assert BA.sensitive_rows(fid[ids_c], Bp, 31, 2).all()
    kpc, vpc = _cu(torch, kpool_c), _cu(torch, vpool_c)
    kbig, vbig = _far_pools(torch, far, ps, M, kpc, vpc, fid, code_bytes=2)
    t = {k: _cu(torch, v) for k, v in st.items()}
    dl, dn = torch.tensor(lens, dtype=torch.int32, device="cuda"), torch.tensor(nq, dtype=torch.int32, device="cuda")

    def call(kpool, vpool, tab):
        res = ops.pq_chunk_attn_wide(t["q"], t["k_ch"], t["v_ch"], kpool, vpool, t["k_cents"], t["v_cents"], t["k_res"], t["v_res"], 0, M=M, C=C,
                                     n_tokens=T, k_page_ids=tab, v_page_ids=tab, page_size=ps, dev_lengths=dl, dev_n_q=dn, return_lse=True,
                                     out=torch.full((bs, nh, n_q, d), float("nan"), dtype=torch.float16, device="cuda"))
        torch.cuda.synchronize()
        return res

    tab_c = _cu(torch, ids_c.astype(np.int32))
    twin, twin2, got = call(kpc, vpc, tab_c), call(kpc, vpc, tab_c), call(kbig, vbig, tab_far)
    gold, gold_l = _chunk16_model(st, [l[1] for l in lens], [l[2] for l in lens], T=[l[0] for l in lens], n_q=nq)

    def vs(o, what):
        _heads(o, gold, what)
        for b in range(bs):
            assert not o[b, :, nq[b]:].any(), f"{what}: rows past n_q of request {b}"

    vs(twin[0], "wide ragged chunk twin")
    _same(got[0], twin[0], twin2[0], "wide chunk far pages, ragged, out", vs)
    vs_l = lambda l, what: _lse_close(l, gold_l, what)      # rows past a request's n_q: -inf, as the model's
    vs_l(twin[1], "wide ragged chunk twin lse")
    _same(got[1], twin[1], twin2[1], "wide chunk far pages, ragged, lse", vs_l)
    BA.assert_only_these_pages(kbig, fid, kpc, far[0], "wide ragged chunk K pool")
    BA.assert_only_these_pages(vbig, fid, vpc, far[1], "wide ragged chunk V pool")


# ------------------------------------------------------------------------------------------ 4. pq_gather_rows, both widths ---
GATHER_WIDTHS = [("u8", np.uint8, 64, 256, 128), ("u16", np.uint16, 64, 1024, 128)]      # name, code type, M, C, d
GATHER_RINGS = [(50, 37), (0, 0)]      # (resid_start, r) in a ring of 64: one that wraps, and no window
G_CAP = 64


def _gather_inputs(dt, M, C, d, T, seed):
    bs, nhk, _ = BA.TABLE
    rs_ = np.random.RandomState(seed)
    f = lambda *s: rs_.standard_normal(s).astype(np.float16)
    return dict(k_codes=rs_.randint(0, C, (bs, nhk, T, M)).astype(dt), v_codes=rs_.randint(0, C, (bs, nhk, T, M)).astype(dt),
                k_cents=f(M, C, d // M), v_cents=f(M, C, d // M), k_res=f(bs, nhk, G_CAP, d), v_res=f(bs, nhk, G_CAP, d))


@pytest.mark.parametrize("ps", [64, 128])
@pytest.mark.parametrize("wname,dt,M,C,d", GATHER_WIDTHS, ids=[w[0] for w in GATHER_WIDTHS])
def test_gather_rows_far_pages(wname, dt, M, C, d, ps, env, oracle, far):
    """pq_gather_rows dequantises token ranges out of K pages and transposed V pages named by far ids.  uint16 codes at page size
    128 and M = 64 make pages of 32 KiB: the pool then has 32 pages past byte 2^32 (BA.n_pool), every smaller page its 64."""
    torch, ops = env
    bs, nhk, npg = BA.TABLE
    cb = np.dtype(dt).itemsize
    T, Bp = npg * ps - 7, ps * M * cb
    inp = _gather_inputs(dt, M, C, d, T, 500 + ps + cb)
    kpool_c, vpool_c, ids_c = _pools(inp["k_codes"], inp["v_codes"], ps)
    fid, tab_far = _far_table(torch, ids_c, Bp, 71)
    if cb == 2:
        assert BA.sensitive_rows(fid[ids_c], Bp, 31, 2).all()
    kpc, vpc = _cu(torch, kpool_c), _cu(torch, vpool_c)
    kbig, vbig = _far_pools(torch, far, ps, M, kpc, vpc, fid, code_bytes=cb)
    tab_c = _cu(torch, ids_c.astype(np.int32))
    t = {k: _cu(torch, v) for k, v in inp.items()}
    rows_cap = T + 37 + 5

    def call(kpool, vpool, tab, t0, t1, rs, r):
        k_out = torch.full((bs, nhk, rows_cap, d), S16, dtype=torch.int16, device="cuda").view(torch.float16)
        v_out = k_out.clone()
        n = ops.pq_gather_rows(kpool, vpool, t["k_cents"], t["v_cents"], k_out, v_out, t0=t0, t1=t1, k_res=t["k_res"], v_res=t["v_res"], r=r,
                               resid_start=rs, k_page_ids=tab, v_page_ids=tab, page_size=ps)
        torch.cuda.synchronize()
        return n, k_out.view(torch.int16), v_out.view(torch.int16)

    for t0, t1 in ((37, 171), (0, T)):
        for rs, r in GATHER_RINGS:
            what = f"gather {wname} ps{ps} [{t0}, {t1}) ring ({rs}, {r})"
            n, tk, tv = call(kpc, vpc, tab_c, t0, t1, rs, r)
            n2, tk2, tv2 = call(kpc, vpc, tab_c, t0, t1, rs, r)
            ng, gk, gv = call(kbig, vbig, tab_far, t0, t1, rs, r)
            assert n == n2 == ng == (t1 - t0) + r
            for side, tw, tw2, g, codes, cents, res in (("K", tk, tk2, gk, "k_codes", "k_cents", "k_res"), ("V", tv, tv2, gv, "v_codes", "v_cents", "v_res")):
                want = B.gather_ref(oracle, inp[codes], inp[cents], inp[res], t0, t1, r, rs)
                twn = _host(tw)
                assert np.array_equal(twn[:, :, :n], want.view(np.int16)), f"{what} {side}: the twin is not pq_decode of the codes, then the ring rows"
                assert (twn[:, :, n:] == S16).all(), f"{what} {side}: rows past {n} were written"
                assert torch.equal(tw, tw2) and torch.equal(g, tw), f"{what} {side}: the far call differs from its compact twin"
    BA.assert_only_these_pages(kbig, fid, kpc, far[0], f"gather {wname} K pool")
    BA.assert_only_these_pages(vbig, fid, vpc, far[1], f"gather {wname} V pool")


@pytest.mark.parametrize("wname,dt,M,C,d", GATHER_WIDTHS, ids=[w[0] for w in GATHER_WIDTHS])
def test_gather_rows_far_rowmajor_out_and_window(wname, dt, M, C, d, env, oracle, far):
    """pq_gather_rows, the writer's strides: row-major codes whose batch stride in bytes passes 2^32, k_out / v_out whose request 1
    starts past byte 2^32, a window whose request 1 does.  K side in the first buffer, V side in the second: codes at the base,
    the destination 256 KiB behind them, the window behind that."""
    torch, ops = env
    bs, nhk, _ = BA.TABLE
    cb = np.dtype(dt).itemsize
    tdt = torch.uint8 if cb == 1 else torch.uint16
    T = 633
    rows_cap = T + 37 + 5
    inp = _gather_inputs(dt, M, C, d, T, 600 + cb)
    t = {k: _cu(torch, v) for k, v in inp.items()}
    off_out, off_win = 256 << 10, (256 << 10) + (-(-nhk * rows_cap * d * 2 // 4096) * 4096)
    assert nhk * T * M * cb <= off_out and off_win + nhk * G_CAP * d * 2 + 2 * 64 * 8 <= BA.FLAT_BYTES - BA.HI
    sb_o, sb_w = BA.far_stride(nhk * rows_cap * d), BA.far_stride(nhk * G_CAP * d)
    mk_codes = lambda flat: BA.far_view(flat, (bs, nhk, T, M), ((BA.HI + 64) // cb, T * M, M, 1), tdt)
    mk_out = lambda flat: BA.far_view(flat[off_out:], (bs, nhk, rows_cap, d), (sb_o, rows_cap * d, d, 1), torch.float16)
    mk_win = lambda flat: BA.far_view(flat[off_win:], (bs, nhk, G_CAP, d), (sb_w, G_CAP * d, d, 1), torch.float16)
    kc_far, vc_far, ko_far, vo_far, kw_far, vw_far = mk_codes(far[0]), mk_codes(far[1]), mk_out(far[0]), mk_out(far[1]), mk_win(far[0]), mk_win(far[1])
    assert kc_far.stride(0) * cb > 2 ** 32 and ko_far.stride(0) * 2 > 2 ** 32 and kw_far.stride(0) * 2 > 2 ** 32
    _fill(kc_far, t["k_codes"]); _fill(vc_far, t["v_codes"]); _fill(kw_far, t["k_res"]); _fill(vw_far, t["v_res"])

    def twin_call(t0, t1, rs, r):
        k_out = torch.full((bs, nhk, rows_cap, d), S16, dtype=torch.int16, device="cuda").view(torch.float16)
        v_out = k_out.clone()
        ops.pq_gather_rows(t["k_codes"], t["v_codes"], t["k_cents"], t["v_cents"], k_out, v_out, t0=t0, t1=t1, k_res=t["k_res"], v_res=t["v_res"],
                           r=r, resid_start=rs)
        torch.cuda.synchronize()
        return k_out.view(torch.int16), v_out.view(torch.int16)

    for t0, t1 in ((37, 171), (0, T)):
        for rs, r in GATHER_RINGS:
            what = f"gather {wname} far strides [{t0}, {t1}) ring ({rs}, {r})"
            n = (t1 - t0) + r
            (tk, tv), (tk2, tv2) = twin_call(t0, t1, rs, r), twin_call(t0, t1, rs, r)
            assert ops.pq_gather_rows(kc_far, vc_far, t["k_cents"], t["v_cents"], ko_far, vo_far, t0=t0, t1=t1, k_res=kw_far, v_res=vw_far, r=r,
                                      resid_start=rs) == n
            torch.cuda.synchronize()
            for side, tw, tw2, g, codes, cents, res in (("K", tk, tk2, ko_far, "k_codes", "k_cents", "k_res"), ("V", tv, tv2, vo_far, "v_codes", "v_cents", "v_res")):
                want = B.gather_ref(oracle, inp[codes], inp[cents], inp[res], t0, t1, r, rs)
                twn = _host(tw)
                assert np.array_equal(twn[:, :, :n], want.view(np.int16)), f"{what} {side}: the twin is not pq_decode of the codes, then the ring rows"
                assert (twn[:, :, n:] == S16).all(), f"{what} {side}: rows past {n} were written"
                assert torch.equal(tw, tw2) and torch.equal(g.view(torch.int16), tw), f"{what} {side}: the far call differs from its compact twin"
            _reset(ko_far, vo_far)
    # the codes and the window are read only; with the views back to the sentinel nothing else was written
    assert _bits(kc_far) == _bits(t["k_codes"]) and _bits(vc_far) == _bits(t["v_codes"])
    assert _bits(kw_far) == _bits(t["k_res"]) and _bits(vw_far) == _bits(t["v_res"])
    _reset(kc_far, vc_far, kw_far, vw_far)
    assert BA.only_sentinel(far[0]) and BA.only_sentinel(far[1])


# --------------------------------------------------------------------------------------- 5. pq_encode_into, uint16 pages ---
@pytest.mark.parametrize("which,bs,nhk,n", [("small", 2, 2, 200), ("bulk", 2, 2, 980)])
def test_wide_encode_into_far_pages(which, bs, nhk, n, env, oracle, far):
    """pq_encode_into at C = 1024 (the wide cache's flush) into uint16 K pages and transposed V pages named by far ids, at the
    sizes of test_encode_into_far_pages; the twin's pools start as the sentinel word too, so partly written pages compare byte
    for byte."""
    torch, ops = env
    from million_amd import _lib as L
    d, M, C, ps, tok0 = 128, 64, 1024, 64, 37
    Bp = ps * M * 2
    npg = max(BA.TABLE[2], -(-(tok0 + n) // ps))
    c = synth.encode_case(60 + n, bs, nhk, n, d, M, C)
    X, cents = _cu(torch, c["X"]), _cu(torch, c["cents"])
    ids_c = np.arange(bs * nhk * npg).reshape(bs, nhk, npg)
    fid, tab_far = _far_table(torch, ids_c, Bp, 31)
    assert BA.sensitive_rows(fid[ids_c], Bp, 31, 2).all()
    tab_c = _cu(torch, ids_c.astype(np.int32))
    kbig, vbig = BA.pool_view(far[0], Bp, (ps, M), code_bytes=2), BA.pool_view(far[1], Bp, (M, ps), code_bytes=2)
    kc, vc = _sentinel_pool(torch, torch.uint16, ids_c.size, ps, M), _sentinel_pool(torch, torch.uint16, ids_c.size, M, ps)
    for kpool, vpool, tab in ((kc, vc, tab_c), (kbig, vbig, tab_far)):
        kw = dict(token_start=tok0, n=n, page_ids=tab, page_size=ps)
        ops.pq_encode_into(X, cents, kpool, layout=L.MILLION_CODES_KPAGES, **kw)
        ops.pq_encode_into(X, cents, vpool, layout=L.MILLION_CODES_VPAGES, **kw)
    torch.cuda.synchronize()
    gold = oracle.pq_encode(c["X"], c["cents"])
    assert gold.dtype == np.uint16 and gold.max() >= 256
    want = np.full((bs, nhk, npg * ps, M), BA.SENTINEL16, np.uint16)
    want[:, :, tok0:tok0 + n] = gold
    got_k, got_v = _from_pools(_host(kc), _host(vc), ids_c, npg * ps)
    np.testing.assert_array_equal(got_k, want)
    np.testing.assert_array_equal(got_v, want)
    BA.assert_only_these_pages(kbig, fid, kc, far[0], f"wide encode {which} K pages")
    BA.assert_only_these_pages(vbig, fid, vc, far[1], f"wide encode {which} V pages")


def test_wide_encode_into_far_rowmajor_strides(env, oracle, far):
    """A row-major uint16 destination whose batch stride in bytes, and a source whose batch stride in elements, put request 1
    past byte 2^32."""
    torch, ops = env
    bs, nhk, n, d, M, C, tok0, Tcap = 2, 2, 200, 128, 64, 1024, 37, 300
    c = synth.encode_case(91, bs, nhk, n, d, M, C)
    X, cents = _cu(torch, c["X"]), _cu(torch, c["cents"])
    x_far = BA.far_view(far[0], (bs, nhk, n, d), (BA.far_stride(nhk * n * d), n * d, d, 1), torch.float16)
    dst_far = BA.far_view(far[1], (bs, nhk, Tcap, M), ((BA.HI + 64) // 2, Tcap * M, M, 1), torch.uint16)
    assert dst_far.stride(0) * 2 > 2 ** 32
    _fill(x_far, X)
    twin = _sentinel_pool(torch, torch.uint16, bs, nhk, Tcap, M)
    ops.pq_encode_into(X, cents, twin, token_start=tok0, n=n)
    ops.pq_encode_into(x_far, cents, dst_far, token_start=tok0, n=n)
    torch.cuda.synchronize()
    want = np.full((bs, nhk, Tcap, M), BA.SENTINEL16, np.uint16)
    want[:, :, tok0:tok0 + n] = oracle.pq_encode(c["X"], c["cents"])
    np.testing.assert_array_equal(_host(twin), want)
    assert _bits(dst_far) == _bits(twin)
    assert _bits(x_far) == _bits(X)
    _reset(dst_far, x_far)
    assert BA.only_sentinel(far[0]) and BA.only_sentinel(far[1])


# ------------------------------------------------------------------------------------------ 6. prompt attention with lse ---
@pytest.mark.parametrize("form", ["dense", "dev_spans", "noncausal"])
@pytest.mark.parametrize("d", [128, 64])
def test_prefill_lse_far_strides(d, form, env, far):
    """The inputs and strides of test_prefill_far_strides through million_prefill_attn_lse (other kernel instances): `out` is
    bitwise the far call without lse, the lse bitwise the twin's and within lse_ref.LSE_TOL of fp64.  noncausal: the block
    route's call over a past block."""
    torch, ops = env
    bs, nh, nhk, n = 2, 4, 2, 257
    rs_ = np.random.RandomState(40 + d)
    q, k, v = (rs_.standard_normal((bs, h, n, d)).astype(np.float16) for h in (nh, nhk, nhk))
    qn, kn = nh * n * d, nhk * n * d
    sb = BA.far_stride(qn + 2 * kn)
    assert sb + qn + 2 * kn <= BA.FLAT_BYTES // 2
    mk = lambda flat, off, heads: BA.far_view(flat[2 * off:], (bs, heads, n, d), (sb, n * d, d, 1), torch.float16)
    q_far, k_far, v_far, out_far = mk(far[0], 0, nh), mk(far[0], qn, nhk), mk(far[0], qn + kn, nhk), mk(far[1], 0, nh)
    tq, tk, tv = _cu(torch, q), _cu(torch, k), _cu(torch, v)
    _fill(q_far, tq); _fill(k_far, tk); _fill(v_far, tv)
    spans = [[257, 257, 0, 0], [100, 190, 90, 0]]
    ds = torch.tensor(spans, dtype=torch.int32, device="cuda") if form == "dev_spans" else None
    causal = form != "noncausal"

    def call(q_, k_, v_, out, lse=True):
        res = ops.prefill_attn(q_, k_, v_, out=out, dev_spans=ds, causal=causal, return_lse=lse)
        torch.cuda.synchronize()
        return res

    new_out = lambda: torch.full((bs, nh, n, d), float("nan"), dtype=torch.float16, device="cuda")
    (twin, twin_l), (twin2, twin2_l) = call(tq, tk, tv, new_out()), call(tq, tk, tv, new_out())
    plain = call(q_far, k_far, v_far, out_far, lse=False)
    assert plain.data_ptr() == out_far.data_ptr() and out_far.stride(0) > 2 ** 31
    plain_bits = _bits(plain)
    _reset(out_far)
    got, got_l = call(q_far, k_far, v_far, out_far)
    assert _bits(got) == plain_bits, "out with lse differs from the far call without it"

    if form == "dev_spans":
        refs = [B.prefill_ref(q[b:b + 1, :, :nq_], k[b:b + 1, :, :nkv_], v[b:b + 1, :, :nkv_], q_pos0=p0) for b, (nq_, nkv_, p0, _) in enumerate(spans)]
    else:
        refs = None
        gold, gold_l = B.prefill_ref(q, k, v, 0, causal)

    def vs(o, what):
        if refs is None:
            return _heads(o, gold, what)
        for b, (nq_, _, _, _) in enumerate(spans):
            _heads(o[b:b + 1, :, :nq_], refs[b][0], f"{what} request {b}")
            assert not o[b, :, nq_:].any()

    def vs_l(l, what):
        if refs is None:
            return _lse_close(l, gold_l, what)
        for b, (nq_, _, _, _) in enumerate(spans):
            _lse_close(l[b:b + 1, :, :nq_], refs[b][1], f"{what} request {b}")

    vs(twin, f"prefill lse d={d} {form} twin")
    vs_l(twin_l, f"prefill lse d={d} {form} twin lse")
    _same(got, twin, twin2, f"prefill lse far strides d={d} {form} out", vs)
    _same(got_l, twin_l, twin2_l, f"prefill lse far strides d={d} {form} lse", vs_l)
    _reset(q_far, k_far, v_far, out_far)
    assert BA.only_sentinel(far[0]) and BA.only_sentinel(far[1])


# ----------------------------------------------------------------------------------------------- 7. merges over far views ---
def _far_rows(torch, flat, off_elems, shape):
    """A (bs, heads, n, d) fp16 view with dense requests whose batch stride is BA.far_stride: request 1 past byte 2^32."""
    bs, h, n, d = shape
    return BA.far_view(flat[2 * off_elems:], shape, (BA.far_stride(h * n * d), n * d, d, 1), torch.float16)


@pytest.mark.parametrize("d", [128, 64])
@pytest.mark.parametrize("P", [3, 8])
def test_attn_merge_far_views(P, d, env, far):
    """attn_merge with every part's out in the first buffer and the result in the second, all with batch stride far_stride; a
    second call writes the result over part 0 (`out` aliasing a part)."""
    torch, ops = env
    bs, nh, n_q = 2, 8, 5
    rs_ = np.random.RandomState(P * 1000 + d)
    outs = [rs_.standard_normal((bs, nh, n_q, d)).astype(np.float16) for _ in range(P)]
    lses = [(3 * rs_.standard_normal((bs, nh, n_q))).astype(np.float32) for _ in range(P)]
    lses[1][0, 0, :2] = -np.inf      # a part that saw no key in some rows
    blk = nh * n_q * d
    t_o, t_l = [_cu(torch, o) for o in outs], [_cu(torch, l) for l in lses]
    parts_far = [_fill(_far_rows(torch, far[0], i * blk, (bs, nh, n_q, d)), t_o[i]) for i in range(P)]
    res_far = _far_rows(torch, far[1], 0, (bs, nh, n_q, d))
    assert all(p.stride(0) * 2 > 2 ** 32 for p in parts_far + [res_far])

    def call(parts, out):
        o, l = ops.attn_merge(parts, t_l, out=out, return_lse=True)
        torch.cuda.synchronize()
        return o, l

    new_out = lambda: torch.full((bs, nh, n_q, d), float("nan"), dtype=torch.float16, device="cuda")
    (twin, twin_l), (twin2, twin2_l) = call(t_o, new_out()), call(t_o, new_out())
    got, got_l = call(parts_far, res_far)
    assert got.data_ptr() == res_far.data_ptr()
    gold, gold_l = lse_ref.merge(outs, lses)
    vs, vs_l = (lambda o, what: _heads(o, gold, what)), (lambda l, what: _lse_close(l, gold_l, what))
    vs(twin, f"merge P={P} d={d} twin")
    vs_l(twin_l, f"merge P={P} d={d} twin lse")
    _same(got, twin, twin2, f"merge far views P={P} d={d} out", vs)
    _same(got_l, twin_l, twin2_l, f"merge far views P={P} d={d} lse", vs_l)
    for i in range(P):      # the parts are read only
        assert _bits(parts_far[i]) == _bits(t_o[i])
    # out = part 0, in place
    al, al_l = call(parts_far, parts_far[0])
    assert al.data_ptr() == parts_far[0].data_ptr()
    _same(al, twin, twin2, f"merge far views P={P} d={d}, out aliasing part 0", vs)
    _same(al_l, twin_l, twin2_l, f"merge far views P={P} d={d}, out aliasing part 0, lse", vs_l)
    _reset(res_far, *parts_far)
    assert BA.only_sentinel(far[0]) and BA.only_sentinel(far[1])


def _merge_inputs(seed, bs, nh, nhk, n, rows, d):
    rs_ = np.random.RandomState(seed)
    f = lambda *s: rs_.standard_normal(s).astype(np.float16)
    return dict(q=f(bs, nh, n, d), k=f(bs, nhk, rows, d), v=f(bs, nhk, rows, d), out_a=f(bs, nh, n, d),
                lse_a=(3 * rs_.standard_normal((bs, nh, n))).astype(np.float32))


def _merge_far(torch, ops, far, inp, op, ref, what):
    """q and out_a in the first buffer, out in the second, all with batch stride far_stride; k / v rows and lse_a compact."""
    shape = inp["q"].shape
    blk = shape[1] * shape[2] * shape[3]
    t = {k: _cu(torch, v) for k, v in inp.items()}
    q_far, a_far = (_fill(_far_rows(torch, far[0], i * blk, shape), t[nm]) for i, nm in enumerate(("q", "out_a")))
    o_far = _far_rows(torch, far[1], 0, shape)
    assert q_far.stride(0) * 2 > 2 ** 32

    def call(q, out_a, out):
        o, l = op(q, t["k"], t["v"], out_a, t["lse_a"], out=out, return_lse=True)
        torch.cuda.synchronize()
        return o, l

    new_out = lambda: torch.full(shape, float("nan"), dtype=torch.float16, device="cuda")
    (twin, twin_l), (twin2, twin2_l) = call(t["q"], t["out_a"], new_out()), call(t["q"], t["out_a"], new_out())
    got, got_l = call(q_far, a_far, o_far)
    assert got.data_ptr() == o_far.data_ptr()
    gold, gold_l = ref
    vs, vs_l = (lambda o, w_: _heads(o, gold, w_)), (lambda l, w_: _lse_close(l, gold_l, w_))
    vs(twin, f"{what} twin")
    vs_l(twin_l, f"{what} twin lse")
    _same(got, twin, twin2, f"{what} out", vs)
    _same(got_l, twin_l, twin2_l, f"{what} lse", vs_l)
    assert _bits(q_far) == _bits(t["q"]) and _bits(a_far) == _bits(t["out_a"])
    _reset(q_far, a_far, o_far)
    assert BA.only_sentinel(far[0]) and BA.only_sentinel(far[1])


@pytest.mark.parametrize("tree", [False, True], ids=["chain", "tree"])
def test_attn_block_merge_far_views(tree, env, far):
    """attn_block_merge (the chain) and its dev_mask form (a token tree) with q, out_a and out far-strided."""
    torch, ops = env
    bs, nh, nhk, n, d = 2, 8, 2, 16, 128
    inp = _merge_inputs(7 + tree, bs, nh, nhk, n, n, d)
    if tree:
        masks = np.stack([VT.ancestor_masks(VT.random_tree(seed, n)) for seed in (2, 3)]).astype(np.int32)
        ref = VT.tree_block_merge(inp["q"], inp["k"], inp["v"], inp["out_a"], inp["lse_a"], masks)
        dm = _cu(torch, masks)
        op = lambda *a, **kw: ops.attn_block_merge(*a, dev_mask=dm, **kw)
    else:
        ref = VM.block_merge(inp["q"], inp["k"], inp["v"], inp["out_a"], inp["lse_a"])
        op = ops.attn_block_merge
    _merge_far(torch, ops, far, inp, op, ref, f"block merge far views tree={tree}")


@pytest.mark.parametrize("n", [1, 16])
def test_attn_sink_merge_far_views(n, env, far):
    """attn_sink_merge with q, out_a and out far-strided."""
    torch, ops = env
    bs, nh, nhk, s_cap, d = 2, 8, 2, 7, 128
    inp = _merge_inputs(20 + n, bs, nh, nhk, n, s_cap, d)
    ref = sink_model.sink_merge(inp["q"], inp["k"], inp["v"], inp["out_a"], inp["lse_a"])
    _merge_far(torch, ops, far, inp, ops.attn_sink_merge, ref, f"sink merge far views n={n}")


# ------------------------------------------------------------------------------------------- 8. the block route end to end ---
@pytest.mark.parametrize("wide", [False, True], ids=["u8", "u16"])
def test_chunk_attn_blocks_far_pages(wide, env, oracle, far):
    """ops.pq_chunk_attn_blocks over far paged pools: T = 633 in blocks of 64 tokens is ten blocks and the chunk - more than
    eight parts, so both merge levels run; out, workspace and lse are the caller's."""
    torch, ops = env
    bs, nhk, npg = BA.TABLE
    d, M, G, ps, r, cap, rstart, n_q, blk = 128, 64, 4, 64, 40, 64, 50, 16, 64
    C, cb = (1024, 2) if wide else (256, 1)
    nh, T, Bp = G * nhk, npg * ps - 7, ps * M * cb
    st = chunk_state(np.random.RandomState(800 + wide), bs, nh, nhk, d, M, C, n_q, T, r, cap, rstart, True)
    if wide:
        rs_ = np.random.RandomState(801)
        st["k_codes"], st["v_codes"] = (rs_.randint(0, C, (bs, nhk, T, M)).astype(np.uint16) for _ in range(2))
    plan = ops.chunk_blocks_plan(T, r, True, blk)
    assert len(plan["parts"]) > 8 and len(plan["groups"]) > 1
    kpool_c, vpool_c, ids_c = _pools(st["k_codes"], st["v_codes"], ps)
    fid, tab_far = _far_table(torch, ids_c, Bp, 83)
    kpc, vpc = _cu(torch, kpool_c), _cu(torch, vpool_c)
    kbig, vbig = _far_pools(torch, far, ps, M, kpc, vpc, fid, code_bytes=cb)
    tab_c = _cu(torch, ids_c.astype(np.int32))
    t = {k: _cu(torch, v) for k, v in st.items() if isinstance(v, np.ndarray)}
    if wide:
        kt, vt = t["k_cents"], t["v_cents"]
    else:
        kt, vt = ops.prepare_cents(t["k_cents"], cache=False), ops.prepare_cents(t["v_cents"], cache=False)
    need = ops.chunk_blocks_workspace_bytes(bs, nh, nhk, n_q, d, cap, blk)

    def call(kpool, vpool, tab):
        out = torch.full((bs, nh, n_q, d), float("nan"), dtype=torch.float16, device="cuda")
        lse = torch.full((bs, nh, n_q), float("nan"), dtype=torch.float32, device="cuda")
        ws = torch.zeros(need, dtype=torch.uint8, device="cuda")
        res = ops.pq_chunk_attn_blocks(t["q"], t["k_ch"], t["v_ch"], kpool, vpool, kt, vt, t["k_res"], t["v_res"], r, M=M, C=C, n_tokens=T,
                                       resid_start=rstart, k_page_ids=tab, v_page_ids=tab, page_size=ps, out=out, workspace=ws, lse=lse,
                                       block_tokens=blk)
        torch.cuda.synchronize()
        assert res[0] is out and res[1] is lse
        return out, lse

    (twin, twin_l), (twin2, twin2_l), (got, got_l) = call(kpc, vpc, tab_c), call(kpc, vpc, tab_c), call(kbig, vbig, tab_far)
    gold, gold_l = B.route_ref(oracle, st)
    vs = lambda o, what: B.check_bar(o.float().cpu().numpy(), gold, what)
    vs_l = lambda l, what: B.check_lse(l.cpu().numpy(), gold_l, what)
    vs(twin, f"block route wide={wide} twin")
    vs_l(twin_l, f"block route wide={wide} twin lse")
    _same(got, twin, twin2, f"block route far pages wide={wide} out", vs)
    _same(got_l, twin_l, twin2_l, f"block route far pages wide={wide} lse", vs_l)
    BA.assert_only_these_pages(kbig, fid, kpc, far[0], f"block route wide={wide} K pool")
    BA.assert_only_these_pages(vbig, fid, vpc, far[1], f"block route wide={wide} V pool")


# ------------------------------------------------------------------------- 9. a wide PagedPQCache whose pools pass 4 GiB ---
def _slot_bits16(torch, cache, b):
    """test_big_address_gpu._slot_bits over uint16 pools (gathered as int16: the same bits): lengths rows, both windows, the K
    and V codes of the slot's T tokens in every layer through its tables, and the ids of its live pages."""
    T, ps = int(cache._T_a[0, b]), cache.page_size
    n_live = -(-T // ps)
    ids = cache._page_ids_all[:, b, :, :n_live].long()
    nl, nhk = ids.shape[:2]
    k = cache.key_page_pool.view(torch.int16)[ids.reshape(-1)].reshape(nl, nhk, n_live * ps, cache.M)[:, :, :T]
    v = cache.value_page_pool.view(torch.int16)[ids.reshape(-1)].reshape(nl, nhk, n_live, cache.M, ps).permute(0, 1, 2, 4, 3).reshape(nl, nhk, n_live * ps, cache.M)[:, :, :T]
    return (dict(lengths=_bits(cache._lengths_all[:, b]), k_win=_bits(cache._kres_all[:, b]), v_win=_bits(cache._vres_all[:, b]),
                 k_codes=_bits(k), v_codes=_bits(v)), k.cpu().numpy().view(np.uint16), v.cpu().numpy().view(np.uint16), ids.cpu().numpy())


def test_wide_paged_cache_pools_past_4gib(env, oracle, flat_store):
    """A PagedPQCache at nbits = 10 (uint16 codes, M 64, page size 128: 16 KiB pages, paging on demand) whose K and V pools are
    4 GiB + 64 pages each, against a compact twin of the same geometry - test_paged_cache_pools_past_4gib with the wide cache's
    life: page ids are burnt through page_manager.allocate_pages so that the prompts' pages straddle id 2^31 / 16384 and the
    first flush's pages straddle 2^32 / 16384.  After prefill_request, decode across one flush with host lengths, release(1) and
    a new prompt in slot 1: outputs, lengths rows, windows and the slots' codes read through their tables are the twin's, bit
    for bit; the twin's codes are oracle.pq_encode's and its last decode step is within the bar of wide_model.decode_attn.  The
    far buffers are dropped first, so no more than about 9 GiB is live at a time."""
    torch, ops = env
    from million_amd.pq_cache import PagedPQCache
    flat_store.drop()
    free = torch.cuda.mem_get_info()[0]
    if free < NEED_FREE:
        pytest.skip(f"{free / 2 ** 30:.1f} GiB of device memory free, the cache's pools want {NEED_FREE >> 30} GiB")
    nl, bs, nh, nhk, d, M, nbits, ps, cap, n_prompt, n_dec, n_again = 2, 2, 8, 2, 128, 64, 10, 128, 128, 300, 129, 200
    C, Bp = 2 ** nbits, ps * M * 2
    assert Bp == 16 << 10
    lo_id, hi_id = 2 ** 31 // Bp, 2 ** 32 // Bp
    pages_cap = -(-(hi_id + 64 + 1) // (nl * bs * nhk))
    assert nl * bs * nhk * pages_cap > hi_id + 64
    rs_ = np.random.RandomState(2025)
    f = lambda *s_: rs_.standard_normal(s_).astype(np.float16)
    N = n_prompt + n_dec
    K, V, ck, cv = f(nl, bs, nhk, N, d), f(nl, bs, nhk, N, d), f(M, C, d // M), f(M, C, d // M)
    K2, V2 = f(nl, 1, nhk, n_again, d), f(nl, 1, nhk, n_again, d)
    qp, qd, qp2 = f(1, nh, n_prompt, d), f(n_dec, nl, bs, nh, 1, d), f(1, nh, n_again, d)
    geom = dict(bs=bs, nh=nh, num_key_value_heads=nhk, M=M, layer_num=nl, nbits=nbits, dtype=torch.uint16, d=d, page_size=ps,
                extended_residual_size=cap, preallocate=False, device="cuda")
    caches = {"far": PagedPQCache(max_tokens=pages_cap * ps, **geom), "twin": PagedPQCache(max_tokens=8 * ps, **geom)}
    far_c = caches["far"]
    assert far_c.key_page_pool.dtype == torch.uint16 and far_c.key_page_pool.numel() * 2 > 2 ** 32 + 64 * Bp
    assert far_c.key_page_pool.shape[0] == nl * bs * nhk * pages_cap
    for c in caches.values():
        c.set_cent(_cu(torch, ck), _cu(torch, cv))
    pm = far_c.page_manager

    def burn_to(next_id):
        lowest = min(pm.free_pages)
        assert lowest <= next_id
        pm.allocate_pages(next_id - lowest)
        assert min(pm.free_pages) == next_id

    def same_state(what, rows_of):
        """rows_of[b]: oracle.pq_encode's (K, V) codes (nl, nh_k, >= T, M) of the rows slot b was given.  -> the far ids of
        every slot's live pages."""
        far_ids = []
        for b in range(bs):
            (sf, _, _, idf), (st, kt, vt, _) = _slot_bits16(torch, far_c, b), _slot_bits16(torch, caches["twin"], b)
            for nm in sf:
                assert sf[nm] == st[nm], f"{what}: slot {b}: {nm} of the cache past 4 GiB differs from the twin's"
            T = kt.shape[2]
            assert T == int(caches["twin"]._T_a[0, b]) == int(far_c._T_a[0, b])
            for nm, got, want in (("K", kt, rows_of[b][0][:, :, :T]), ("V", vt, rows_of[b][1][:, :, :T])):
                bad = np.argwhere((got != want).any(axis=-1))
                assert bad.size == 0, (f"{what}: slot {b}: the twin's {nm} codes are not the oracle's at {len(bad)} (layer, kv head, token), "
                                       f"first {bad[0].tolist()}, last {bad[-1].tolist()}")
            far_ids.append(idf)
        return far_ids

    # the oracle's codes of every row a slot is ever given, encoded once (a code depends on its row and the codebook alone)
    enc = lambda X, cents: oracle.pq_encode(X.reshape(-1, *X.shape[-3:]), cents).reshape(*X.shape[:-1], M)
    Kc, Vc, K2c, V2c = enc(K, ck), enc(V, cv), enc(K2, ck), enc(V2, cv)
    assert Kc.dtype == np.uint16 and min(a.max() for a in (Kc, Vc, K2c, V2c)) >= 256
    first = {b: (Kc[:, b], Vc[:, b]) for b in range(bs)}
    # phase 1: the prompts; the pages of slot 0 straddle byte 2^31 of the pools
    burn_to(lo_id - 3)
    outs_p = {name: [] for name in caches}
    for name, c in caches.items():
        for b in range(bs):
            for l in range(nl):
                outs_p[name].append(c.prefill_request(b, _cu(torch, qp), _cu(torch, K[l, b:b + 1, :, :n_prompt]), _cu(torch, V[l, b:b + 1, :, :n_prompt]), l).clone())
    torch.cuda.synchronize()
    assert _bits(torch.stack(outs_p["far"])) == _bits(torch.stack(outs_p["twin"])), "prefill outputs differ from the twin's"
    ids1 = np.concatenate([i.ravel() for i in same_state("prefill", first)])
    assert ids1.min() < lo_id <= ids1.max() < hi_id, (ids1.min(), ids1.max())
    # phase 2: decode until the window has flushed once; the flush's pages straddle byte 2^32
    burn_to(hi_id - 3)
    outs = {name: [] for name in caches}
    for i in range(n_dec):
        for l in range(nl):
            t = n_prompt + i
            for name, c in caches.items():
                outs[name].append(c.decoding_with_pages(_cu(torch, qd[i, l]), _cu(torch, K[l, :, :, t:t + 1]), _cu(torch, V[l, :, :, t:t + 1]), l).clone())
    torch.cuda.synchronize()
    assert ops.tail_faults() == 0
    assert _bits(torch.stack(outs["far"])) == _bits(torch.stack(outs["twin"])), "decode outputs differ from the twin's"
    T, r = n_prompt + ps, n_dec - ps
    for c in caches.values():
        assert c._T_a.tolist() == [[T] * bs] * nl and c._r_a.tolist() == [[r] * bs] * nl
    ids2 = np.concatenate([i[:, :, -1].ravel() for i in same_state("decode across a flush", first)])      # the page the flush filled
    assert ids2.min() < hi_id <= ids2.max(), (ids2.min(), ids2.max())
    for l in range(nl):      # the twin's last step against the model: codes of T tokens, the r window rows behind them
        gold, _ = W.decode_attn(qd[n_dec - 1, l], Kc[l, :, :, :T], Vc[l, :, :, :T], ck, cv, K[l, :, :, T:T + r], V[l, :, :, T:T + r], r)
        _heads(outs["twin"][-nl + l], gold, f"wide cache twin, last decode step, layer {l}")
    # phase 3: slot 1 ends; a new prompt takes the slot (the pages it returns, or fresh ones)
    outs_r = {name: [] for name in caches}
    for name, c in caches.items():
        c.release(1)
        for l in range(nl):
            outs_r[name].append(c.prefill_request(1, _cu(torch, qp2), _cu(torch, K2[l]), _cu(torch, V2[l]), l).clone())
    torch.cuda.synchronize()
    assert _bits(torch.stack(outs_r["far"])) == _bits(torch.stack(outs_r["twin"])), "the new prompt's outputs differ from the twin's"
    for c in caches.values():
        assert c._T_a.tolist() == [[T, n_again]] * nl and c._r_a.tolist() == [[r, 0]] * nl
    ids3 = same_state("release + a new prompt", {0: first[0], 1: (K2c[:, 0], V2c[:, 0])})
    # the slots' tables held ids on both sides of both boundaries, so none of this passed on low ids alone
    seen = np.concatenate([ids1, ids2] + [i.ravel() for i in ids3])
    assert (seen < lo_id).any() and ((seen >= lo_id) & (seen < hi_id)).any() and (seen >= hi_id).any()
    for c in caches.values():
        c.cleanup()
    caches.clear()
    del pm, c, far_c
    gc.collect()
    torch.cuda.empty_cache()
