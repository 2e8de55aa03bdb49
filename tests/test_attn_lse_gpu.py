"""GPU tests of the log-sum-exp surface: million_pq_decode_attn_lse on every case of the poisoned-memory matrix, chunk attention
with lse, million_attn_merge, split-and-merge at the op level, SharedPrefix and its refusals.  References: tests/lse_ref.py (fp64).

Bars.  lse: 1e-3 absolute in natural-log units (lse_ref.LSE_TOL).  `out` of an lse entry: bitwise the entry's without it.  The
merge kernel: one fp16 rounding of the fp64 merge (2^-10 relative per element), lse_out within 1e-5.  Merged attentions against
the whole context's fp64 `out`: the project's per-head rel-L2 < 1e-3 (decode_poison.head_err).

SharedPrefix runs at d 128 / M 64 / C 256 and at d 64 / M 32 / C 256: PagedPQCache takes 256 centroids only (nbits = 8), so the
second geometry keeps its d and M and cannot have 128 centroids."""
import ctypes
import dataclasses
import zlib

import numpy as np
import pytest

from tests import cache_life_model as CL
from tests import decode_poison as P
from tests import lse_ref as R
from tests import test_chunk_attn_gpu as CG

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def env():
    import torch
    assert torch.cuda.is_available(), "GPU tests need an MI355X"
    from million_amd import ops, _lib
    return torch, ops, _lib.load(), _lib


def _bits(a):
    a = np.ascontiguousarray(a)
    return a.view({2: np.uint16, 4: np.uint32}[a.dtype.itemsize])


# ---------------------------------------------------------------- a. the poisoned-memory matrix through the lse entry --------
def run_lse(c, arrs, torch, ops, lib, L):
    """decode_poison.run through million_pq_decode_attn_lse (k_new = v_new = NULL without an append), lse pre-filled with NaN."""
    cu = lambda a: None if a is None else torch.from_numpy(np.ascontiguousarray(a)).cuda()
    ptr = lambda t: None if t is None else t.data_ptr()
    t = {k: cu(v) for k, v in arrs.items() if isinstance(v, np.ndarray)}
    kp, vp = ops.prepare_cents(t["k_cents"], cache=False), ops.prepare_cents(t["v_cents"], cache=False)
    out = torch.full_like(t["q"], float("nan"))
    lse = torch.full((c.bs, c.nh), float("nan"), dtype=torch.float32, device="cuda")
    desc = P.make_desc(c, L)
    if c.dev:
        desc.dev_lengths = t["lengths"].data_ptr()
    ws = ops.attn_workspace(desc, t["q"].device)
    ids = t.get("ids")
    kids, vids = (ids if c.kl == "paged" else None), (ids if c.vl == "paged" else None)
    lib.million_set_force_generic(c.policy)
    try:
        rc = lib.million_pq_decode_attn_lse(ctypes.byref(desc), ptr(t["q"]), ptr(t.get("k_new")) if c.append else None,
                                            ptr(t.get("v_new")) if c.append else None, ptr(t["k_codes"]), ptr(t["v_codes"]),
                                            ptr(kids), ptr(vids), ptr(kp), ptr(vp), ptr(t["k_res"]), ptr(t["v_res"]), ptr(out),
                                            ptr(lse), ptr(ws), ws.numel(), torch.cuda.current_stream().cuda_stream)
        torch.cuda.synchronize()
    finally:
        lib.million_set_force_generic(0)
    assert rc == 0, f"{c.name}: rc={rc} {lib.million_last_error()}"
    res = {"out": out.cpu().numpy(), "lse": lse.cpu().numpy(), "k_res": t["k_res"].cpu().numpy(), "v_res": t["v_res"].cpu().numpy()}
    if c.dev:
        res["lengths"] = t["lengths"].cpu().numpy()
    return res


@pytest.mark.parametrize("cname", [c.name for c in P.CASES])
def test_decode_lse_matrix(cname, env, oracle):
    torch, ops, lib, L = env
    c = P.BY_NAME[cname]
    built = P.build(c)
    old = P.run(c, built["clean"], torch, ops, lib, L)
    clean = run_lse(c, built["clean"], torch, ops, lib, L)
    pois = run_lse(c, built["poisoned"], torch, ops, lib, L)
    for nm in ("out", "k_res", "v_res"):
        assert np.array_equal(_bits(clean[nm]), _bits(old[nm])), f"{cname}: {nm} differs from the entry without lse"
    if c.dev:
        assert np.array_equal(clean["lengths"], old["lengths"])
    _, ref = R.decode_ref(c, built, oracle)
    err = np.abs(clean["lse"].astype(np.float64) - ref)
    print(f"{cname}: lse max abs error {err.max():.3e}")
    assert np.isfinite(clean["lse"]).all() and err.max() < R.LSE_TOL, f"{cname}: lse off by {err.max():.3e} at {np.unravel_index(err.argmax(), err.shape)}"
    assert ops.tail_faults() == 0
    assert np.array_equal(_bits(pois["lse"]), _bits(clean["lse"])), f"{cname}: the poisoned copy's lse differs from the clean copy's"
    assert np.array_equal(_bits(pois["out"]), _bits(clean["out"]))


# ---------------------------------------------------------------- b. nothing to attend to -----------------------------------
@pytest.mark.parametrize("cname", ["lean-d128-M64-ps64-C256", "stream-M64-C256", "tile-d64-M32-ps32-C256", "scalar-d128-M64-C256"])
def test_decode_lse_of_an_empty_request(cname, env, oracle):
    """Device lengths, two requests, the second at {0, 0, 0} and no append: its lse is -inf and its out 0; the first is untouched."""
    torch, ops, lib, L = env
    c = dataclasses.replace(P.BY_NAME[cname], bs=2, dev=True, gap=0, append=False)
    built = P.build(c)
    arrs = dict(built["clean"])
    arrs["lengths"] = arrs["lengths"].copy()
    arrs["lengths"][1, :3] = 0
    got = run_lse(c, arrs, torch, ops, lib, L)
    assert np.all(np.isneginf(got["lse"][1])), got["lse"][1]
    assert np.all(_bits(got["out"][1]) == 0)
    ref_o, ref_l = R.decode_ref(c, built, oracle)
    assert np.abs(got["lse"][0] - ref_l[0]).max() < R.LSE_TOL
    assert P.head_err(got["out"][:1], ref_o[:1]).max() < P.REL_TOL
    assert ops.tail_faults() == 0


# ---------------------------------------------------------------- c. chunk attention ----------------------------------------
def _chunk_run(torch, ops, oracle, st, M, C, layout, ps, lse, dev_n_q=None):
    dev = lambda a: None if a is None else torch.from_numpy(np.ascontiguousarray(a)).cuda()
    T = st["k_codes"].shape[2]
    kp, vp = ops.prepare_cents(dev(st["k_cents"]), cache=False), ops.prepare_cents(dev(st["v_cents"]), cache=False)
    kw = {}
    if layout == "paged":
        vpool, ids = oracle.v_rowmajor_to_pool(st["v_codes"], ps)
        kpool, _ = oracle.k_rowmajor_to_pool(st["k_codes"], ps)
        if ids.shape[2] == 0:
            ids = np.zeros(ids.shape[:2] + (1,), np.int64)
        ids_t = dev(ids.astype(np.int32))
        k_codes, v_codes = dev(kpool), dev(vpool)
        kw = dict(k_page_ids=ids_t, v_page_ids=ids_t, page_size=ps)
    else:
        k_codes, v_codes = dev(st["k_codes"]), dev(st["v_codes"])
    if dev_n_q is not None:
        kw["dev_n_q"] = dev(np.asarray(dev_n_q, np.int32))
    bs, nh, n_q, _ = st["q"].shape
    if lse:
        kw["lse"] = torch.full((bs, nh, n_q), float("nan"), dtype=torch.float32, device="cuda")
    res = ops.pq_chunk_attn(dev(st["q"]), dev(st["k_ch"]), dev(st["v_ch"]), k_codes, v_codes, kp, vp, dev(st["k_res"]),
                            dev(st["v_res"]), st["r"], M=M, C=C, n_tokens=T, resid_start=st["rs"], **kw)
    torch.cuda.synchronize()
    return (res[0].cpu().numpy(), res[1].cpu().numpy()) if lse else res.cpu().numpy()


# (d, M, C, G, n_q, T, window, chunk, layout, ps)
CHUNK = [
    (128, 64, 256, 4, 16, 4097, "wrap", True, "paged", 64),        # several splits, paged
    (128, 32, 128, 8, 65, 63, "17", True, "paged", 32),            # one split
    (64, 16, 256, 4, 3, 1000, "wrap", False, "rowmajor", 0),
    (128, 64, 256, 4, 65, 0, "0", True, "rowmajor", 0),            # chunk only
    (128, 64, 256, 4, 3, 0, "0", False, "rowmajor", 0),            # no chunk, no window: -inf
]


@pytest.mark.parametrize("case", CHUNK, ids=["-".join(map(str, c)) for c in CHUNK])
def test_chunk_lse(case, env, oracle):
    torch, ops, lib, L = env
    d, M, C, G, n_q, T, win, chunk, layout, ps = case
    r, rstart = {"0": (0, 0), "17": (17, 0), "wrap": (100, 90)}[win]
    st = CG._state(np.random.RandomState(zlib.crc32(repr(case).encode())), 1, G * 2, 2, d, M, C, n_q, T, r, 128, rstart, chunk)
    old = _chunk_run(torch, ops, oracle, st, M, C, layout, ps, lse=False)
    out, lse = _chunk_run(torch, ops, oracle, st, M, C, layout, ps, lse=True)
    assert np.array_equal(_bits(out), _bits(old)), f"{case}: out differs from the entry without lse"
    ref_o, ref_l = R.chunk_ref(oracle, st)
    if T == 0 and r == 0 and not chunk:
        assert np.all(np.isneginf(lse)) and np.all(_bits(out) == 0)
        return
    err = np.abs(lse.astype(np.float64) - ref_l)
    print(f"{case}: lse max abs error {err.max():.3e}")
    assert np.isfinite(lse).all() and err.max() < R.LSE_TOL, f"{case}: lse off by {err.max():.3e}"
    CG._check(out, ref_o, str(case))


@pytest.mark.parametrize("T", [1000, 63])      # several splits (the merge kernel writes the rows), one split
def test_chunk_lse_ragged_rows(T, env, oracle):
    """dev_n_q = (2, 0) at n_q = 3: the rows past a request's count give -inf (their out is zeros already)."""
    torch, ops, lib, L = env
    d, M, C, G, n_q = 128, 64, 256, 4, 3
    st = CG._state(np.random.RandomState(77 + T), 2, G * 2, 2, d, M, C, n_q, T, 17, 128, 120, True)
    n_valid = (2, 0)
    old = _chunk_run(torch, ops, oracle, st, M, C, "paged", 64, lse=False, dev_n_q=n_valid)
    out, lse = _chunk_run(torch, ops, oracle, st, M, C, "paged", 64, lse=True, dev_n_q=n_valid)
    assert np.array_equal(_bits(out), _bits(old))
    ref_o, ref_l = R.chunk_ref(oracle, st, n_valid)
    assert np.all(np.isneginf(lse[0, :, 2:])) and np.all(np.isneginf(lse[1])), lse
    assert np.all(_bits(out[0, :, 2:]) == 0) and np.all(_bits(out[1]) == 0)
    assert np.abs(lse[0, :, :2].astype(np.float64) - ref_l[0, :, :2]).max() < R.LSE_TOL
    CG._check(out[0, :, :2], ref_o[0, :, :2], "ragged")


# ---------------------------------------------------------------- d. the merge kernel ---------------------------------------
def _merge_parts(rs, bs, nh, n_q, d, P_):
    """Values in [0.5, 2): a merged element is then a normal fp16 number, where one rounding is 2^-11 relative."""
    outs = [(0.5 + 1.5 * rs.random_sample((bs, nh, n_q, d))).astype(np.float16) for _ in range(P_)]
    lses = [(3.0 * rs.standard_normal((bs, nh, n_q))).astype(np.float32) for _ in range(P_)]
    return outs, lses


def _check_merge(got_o, got_l, outs, lses, what):
    ref_o, ref_l = R.merge(outs, lses)
    nan = np.isnan(ref_l)
    assert np.array_equal(np.isnan(got_l), nan) and np.array_equal(np.isnan(got_o.astype(np.float32)).all(axis=-1), nan), what
    ok = ~nan
    fin = ok & np.isfinite(ref_l)
    assert np.array_equal(np.isneginf(got_l[ok]), np.isneginf(ref_l[ok])), what
    assert np.abs(got_l[fin].astype(np.float64) - ref_l[fin]).max(initial=0) <= 1e-5, what
    g, r_ = got_o[ok].astype(np.float64), ref_o[ok]
    assert np.all(np.abs(g - r_) <= 2.0 ** -10 * np.abs(r_)), f"{what}: out off by {np.max(np.abs(g - r_) / np.maximum(np.abs(r_), 1e-30)):.3e} relative"


@pytest.mark.parametrize("shape", [(3, 5, 1, 64, 2), (2, 8, 9, 128, 3), (2, 7, 9, 128, 3), (1, 8, 4, 128, 8), (1, 4, 1, 128, 1)],
                         ids=lambda s: "x".join(map(str, s)))
def test_attn_merge_against_the_formula(shape, env):
    torch, ops, lib, L = env
    bs, nh, n_q, d, P_ = shape
    outs, lses = _merge_parts(np.random.RandomState(sum(shape)), bs, nh, n_q, d, P_)
    cu = lambda a: torch.from_numpy(a).cuda()
    o, l = ops.attn_merge([cu(a) for a in outs], [cu(a) for a in lses], return_lse=True)
    torch.cuda.synchronize()
    _check_merge(o.cpu().numpy(), l.cpu().numpy(), outs, lses, str(shape))


def test_attn_merge_views_alias_and_special_rows(env):
    torch, ops, lib, L = env
    bs, nh, n_q, d = 3, 4, 5, 128
    outs, lses = _merge_parts(np.random.RandomState(5), bs, nh, n_q, d, 3)
    lses[0][0, 0, :] = -np.inf                      # one part -inf
    for l in lses:
        l[1, 1, 2] = -np.inf                        # all parts -inf
    lses[2][2, 3, 4] = np.nan                       # a NaN lse
    lses[1][0, 2, 1] = -np.inf
    outs[1][0, 2, 1] = np.float16("nan")            # a -inf part's out is never used, whatever it holds
    cu = lambda a: torch.from_numpy(np.ascontiguousarray(a)).cuda()
    # part 0 as a transposed view: stored (n_q, nh, bs, d) / (n_q, nh, bs), seen as (bs, nh, n_q, d) / (bs, nh, n_q)
    p0 = cu(outs[0].transpose(2, 1, 0, 3)).permute(2, 1, 0, 3)
    l0 = cu(lses[0].transpose(2, 1, 0)).permute(2, 1, 0)
    assert not p0.is_contiguous() and p0.shape == (bs, nh, n_q, d)
    p1 = cu(outs[1])
    parts_o, parts_l = [p0, p1, cu(outs[2])], [l0, cu(lses[1]), cu(lses[2])]
    ref_inputs = ([a.copy() for a in outs], [a.copy() for a in lses])
    ref_inputs[0][1][0, 2, 1] = 0                   # (the formula's stand-in for "not used")
    o, l = ops.attn_merge(parts_o, parts_l, out=p1, return_lse=True)      # out aliases part 1
    torch.cuda.synchronize()
    assert o.data_ptr() == p1.data_ptr()
    _check_merge(o.cpu().numpy(), l.cpu().numpy(), ref_inputs[0], ref_inputs[1], "views / alias / special rows")
    got = o.cpu().numpy()
    assert np.all(_bits(got[1, 1, 2]) == 0) and np.isneginf(l.cpu().numpy()[1, 1, 2])
    bad = cu(np.zeros((bs, nh, n_q, d + 4), np.float16))[..., 4:]      # rows 8 bytes off a 16-byte boundary, 132 elements apart
    with pytest.raises(RuntimeError, match="aligned|stride"):
        ops.attn_merge([cu(outs[0]), bad], parts_l[:2])


# ---------------------------------------------------------------- e. split and merge at the op level -------------------------
@pytest.mark.parametrize("cname", ["lean-d128-M64-ps64-C256", "scalar-d64-M32-C128"])
@pytest.mark.parametrize("cuts", [(333,), (333, 777)], ids=["two-parts", "three-parts"])
def test_split_context_merges_to_the_whole(cname, cuts, env, oracle):
    """The geometry of two matrix cases with row-major codes (a token range is a slice): the parts [0, T1) .. without a window
    and the last part [Tk, T) + window + appended row, merged, against the whole context's fp64 out."""
    torch, ops, lib, L = env
    base = P.BY_NAME[cname]
    c = dataclasses.replace(base, kl="row", vl="row", dev=False, gap=0, append=True)
    built = P.build(c)
    cl = built["clean"]
    cu = lambda a: torch.from_numpy(np.ascontiguousarray(a)).cuda()
    q, kc, vc = cu(cl["q"]), cu(built["k_codes"]), cu(built["v_codes"])
    kp, vp = ops.prepare_cents(cu(cl["k_cents"]), cache=False), ops.prepare_cents(cu(cl["v_cents"]), cache=False)
    k_res, v_res = cu(cl["k_res"]), cu(cl["v_res"])
    edges = (0,) + cuts + (c.T,)
    outs, lses = [], []
    ops.set_force_generic(c.policy)
    try:
        for i, (a, b) in enumerate(zip(edges[:-1], edges[1:])):
            last = i == len(edges) - 2
            kw = dict(k_new=cu(cl["k_new"]), v_new=cu(cl["v_new"])) if last else {}
            o, l = ops.pq_decode_attn(q, kc[:, :, a:b], vc[:, :, a:b], kp, vp, k_res, v_res, c.r if last else 0, M=c.M, C=c.C,
                                      n_tokens=b - a, resid_start=c.rs, return_lse=True, **kw)
            outs.append(o)
            lses.append(l)
            ref_l = R.decode_ref(c, built, oracle, tokens=slice(a, b), window=last)[1]
            assert np.abs(l.cpu().numpy()[:, :, 0] - ref_l).max() < R.LSE_TOL, f"part {i}"
        torch.cuda.synchronize()
    finally:
        ops.set_force_generic(0)
    merged, l_all = ops.attn_merge(outs, lses, return_lse=True)
    torch.cuda.synchronize()
    ref_o, ref_l = R.decode_ref(c, built, oracle)
    e = P.head_err(merged.cpu().numpy(), ref_o)
    print(f"{cname} {cuts}: worst head {e.max():.3e}, merged lse error {np.abs(l_all.cpu().numpy()[:, :, 0] - ref_l).max():.3e}")
    assert e.max() < P.REL_TOL, f"worst head {e.max():.3e}"
    assert np.abs(l_all.cpu().numpy()[:, :, 0] - ref_l).max() < R.LSE_TOL
    assert ops.tail_faults() == 0


# ---------------------------------------------------------------- f. SharedPrefix -------------------------------------------
NH, NHK, LAYERS, PS, CAP, N_CONT, PROMPT = 8, 2, 2, 64, 128, 3, 300


def _caches(torch, d, M, cents=None, cont_M=None):
    from million_amd.pq_cache import PagedPQCache
    from tests import synth
    mk = lambda bs, m: PagedPQCache(bs=bs, nh=NH, num_key_value_heads=NHK, M=m, layer_num=LAYERS, d=d, page_size=PS,
                                    extended_residual_size=CAP, max_tokens=1024)
    prefix, cont = mk(1, M), mk(N_CONT, cont_M or M)
    cent = lambda seed, m: torch.from_numpy(synth.encode_case(seed, 1, NHK, 1, d, m, 256)["cents"])
    prefix.set_cent(cent(4400, M), cent(4401, M))
    cont.set_cent(*(cents or (cent(4400, cont_M or M), cent(4401, cont_M or M))))
    return prefix, cont


def _rows(torch, rs, bs, n, d):
    f = lambda h: torch.from_numpy(rs.standard_normal((bs, h, n, d)).astype(np.float16)).cuda()
    return f(NH), f(NHK), f(NHK)


def _fill_prefix(torch, prefix, rs, d):
    for l in range(LAYERS):
        prefix.prefill(*_rows(torch, rs, 1, PROMPT, d), l)
    for _ in range(5):
        for l in range(LAYERS):
            prefix.decoding_with_pages(*_rows(torch, rs, 1, 1, d), l)


def _slot_keys(oracle, cache, snap, l, b):
    """K, V (nh_k, n, d) fp64 of what slot b of layer l holds on the device: its codes through its page table, then its ring."""
    T, r, rs_ = int(snap["T_a"][l, b]), int(snap["r_a"][l, b]), int(snap["rs_a"][l, b])      # (the mirror: host-length steps do not move the device rows)
    ks, vs = [], []
    if T:
        kc, vc = CL.gather_codes(snap, l, b, T, cache.page_size)
        ks.append(oracle.pq_decode(kc[None], cache.key_cent.cpu().numpy())[0].astype(np.float64))
        vs.append(oracle.pq_decode(vc[None], cache.value_cent.cpu().numpy())[0].astype(np.float64))
    ring = (rs_ + np.arange(r)) % cache.extended_residual_size
    ks.append(snap["k_res"][l, b].view(np.float16)[:, ring].astype(np.float64))
    vs.append(snap["v_res"][l, b].view(np.float16)[:, ring].astype(np.float64))
    return np.concatenate(ks, axis=1), np.concatenate(vs, axis=1)


def _check_step(oracle, prefix, cont, l, q, out, what):
    """out (n, nh, 1, d) against the fp64 softmax over [prefix slot 0; continuation slot b] as both caches hold them now (the
    continuation's window holds the step's new row)."""
    ps_, cs_ = CL.snapshot(prefix), CL.snapshot(cont)
    Kp, Vp = _slot_keys(oracle, prefix, ps_, l, 0)
    qn, on = q.cpu().numpy(), out.cpu().numpy()
    for b in range(cont.bs):
        Kc, Vc = _slot_keys(oracle, cont, cs_, l, b)
        K, V = np.concatenate([Kp, Kc], axis=1)[None], np.concatenate([Vp, Vc], axis=1)[None]
        ref, _ = R.attend(qn[b:b + 1], K, V)
        e = P.head_err(on[b:b + 1], ref)
        assert np.isfinite(on[b]).all() and e.max() < P.REL_TOL, f"{what}: slot {b}: worst head {e.max():.3e}"


@pytest.mark.parametrize("d,M,dev", [(128, 64, False), (64, 32, True)], ids=["d128-M64-C256", "d64-M32-C256-devlen"])
def test_shared_prefix_decode_and_extend(d, M, dev, env, oracle):
    torch, ops, lib, L = env
    from million_amd.shared_prefix import SharedPrefix
    rs = np.random.RandomState(d + M)
    prefix, cont = _caches(torch, d, M)
    _fill_prefix(torch, prefix, rs, d)
    sp = SharedPrefix(prefix, 0, cont)
    assert (sp.T, sp.r) == (PROMPT, 5)
    frozen = prefix.host_state()
    allocs = lambda: torch.cuda.memory_stats()["allocation.all.allocated"]
    for step in range(CAP + 2):
        for l in range(LAYERS):
            q, k, v = _rows(torch, rs, N_CONT, 1, d)
            before = allocs()
            out = sp.decoding(q, k, v, l, use_dev_lengths=dev)
            if step == 1:      # the second call of a layer allocates nothing
                assert allocs() == before, f"layer {l}: {allocs() - before} allocations in the second decoding call"
            if step in (0, 1, CAP - 1, CAP, CAP + 1):
                torch.cuda.synchronize()
                _check_step(oracle, prefix, cont, l, q, out, f"step {step} layer {l}")
    assert int(cont._T_a[0, 0]) == PS and int(cont._r_a[0, 0]) == CAP + 2 - PS      # one continuation flush was crossed
    assert all(np.array_equal(a, b) for a, b in zip(prefix.host_state(), frozen))
    # a fresh continuation slot: a question of 5 rows asked of the document, then 3 decode steps of every slot
    cont.release(1)
    n = 5
    for l in range(LAYERS):
        q, k, v = _rows(torch, rs, 1, n, d)
        out = sp.extend_request(1, q, k, v, l)
        torch.cuda.synchronize()
        ps_ = CL.snapshot(prefix)
        Kp, Vp = _slot_keys(oracle, prefix, ps_, l, 0)
        kn, vn = k.cpu().numpy()[0].astype(np.float64), v.cpu().numpy()[0].astype(np.float64)
        on, qn = out.cpu().numpy(), q.cpu().numpy()
        for i in range(n):      # row i sees the prefix and the block's rows 0 .. i
            K, V = np.concatenate([Kp, kn[:, :i + 1]], axis=1)[None], np.concatenate([Vp, vn[:, :i + 1]], axis=1)[None]
            ref, _ = R.attend(qn[:, :, i:i + 1], K, V)
            e = P.head_err(on[:, :, i:i + 1], ref)
            assert e.max() < P.REL_TOL, f"extend_request layer {l} row {i}: worst head {e.max():.3e}"
    assert int(cont._T_a[0, 1]) == n and int(cont._r_a[0, 1]) == 0
    if not dev:      # the steps so far ran on host lengths, which leave the device rows alone: bring them up to the mirror
        for l in range(LAYERS):
            cont._sync_lengths(l)
    for step in range(3):
        for l in range(LAYERS):
            q, k, v = _rows(torch, rs, N_CONT, 1, d)
            out = sp.decoding(q, k, v, l, use_dev_lengths=True)      # the slots are at different lengths now
            torch.cuda.synchronize()
            _check_step(oracle, prefix, cont, l, q, out, f"after extend: step {step} layer {l}")
    assert ops.tail_faults() == 0


def test_extend_request_with_lse_on_an_empty_slot_leaves_prefill_requests_state(env):
    """return_lse on an empty slot goes through chunk attention instead of the prompt kernel: same pages, codes, lengths."""
    torch, ops, lib, L = env
    d, M = 128, 64
    a, b = _caches(torch, d, M)[1], _caches(torch, d, M)[1]
    rs = np.random.RandomState(9)
    for l in range(LAYERS):
        q, k, v = _rows(torch, rs, 1, 70, d)
        o1 = a.extend_request(2, q, k, v, l)
        o2, lse = b.extend_request(2, q, k, v, l, return_lse=True)
        assert lse.shape == (1, NH, 70) and torch.isfinite(lse).all()
        assert ((o1.float() - o2.float()).norm() / o1.float().norm()).item() < 2e-3      # two kernels, each within 1e-3 of the truth
    torch.cuda.synchronize()
    sa, sb = CL.snapshot(a), CL.snapshot(b)
    for nm in ("lengths", "T_a", "r_a", "rs_a", "page_ids", "k_pool", "v_pool", "k_res", "v_res"):
        assert np.array_equal(sa[nm], sb[nm]), nm
    assert all(np.array_equal(x, y) for x, y in zip(a.host_state(), b.host_state()))


# ---------------------------------------------------------------- g. refusals -----------------------------------------------
def test_shared_prefix_refusals(env):
    torch, ops, lib, L = env
    from million_amd.shared_prefix import SharedPrefix
    from tests import synth
    d, M = 128, 64
    rs = np.random.RandomState(1)
    same = lambda s0, s1: all(np.array_equal(x, y) for x, y in zip(s0, s1))

    def refused(make, prefix, cont, match):
        s0, s1 = prefix.host_state(), cont.host_state()
        with pytest.raises(RuntimeError, match=match):
            make()
        assert same(prefix.host_state(), s0) and same(cont.host_state(), s1), "a refused call moved a host mirror"

    other = tuple(torch.from_numpy(synth.encode_case(s, 1, NHK, 1, d, M, 256)["cents"]) for s in (5500, 5501))
    prefix, cont = _caches(torch, d, M, cents=other)
    _fill_prefix(torch, prefix, rs, d)
    refused(lambda: SharedPrefix(prefix, 0, cont), prefix, cont, "codebooks")
    _, cont32 = _caches(torch, d, M, cont_M=32)
    refused(lambda: SharedPrefix(prefix, 0, cont32), prefix, cont32, "differ in M")
    # a prefix slot that decoded a step after construction
    _, cont = _caches(torch, d, M)
    sp = SharedPrefix(prefix, 0, cont)
    q, k, v = _rows(torch, rs, N_CONT, 1, d)
    sp.decoding(q, k, v, 0)
    for l in range(LAYERS):
        prefix.decoding_with_pages(*_rows(torch, rs, 1, 1, d), l)
    refused(lambda: sp.decoding(q, k, v, 1), prefix, cont, "moved")
    refused(lambda: sp.extend_request(0, *_rows(torch, rs, 1, 4, d), 0), prefix, cont, "moved")
    # a prefix mid-step: layer 0 has decoded, layer 1 has not
    prefix.decoding_with_pages(*_rows(torch, rs, 1, 1, d), 0)
    _, cont2 = _caches(torch, d, M)
    refused(lambda: SharedPrefix(prefix, 0, cont2), prefix, cont2, "mid-step")
    torch.cuda.synchronize()
