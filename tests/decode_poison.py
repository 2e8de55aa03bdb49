"""Poisoned-memory parity matrix of million_pq_decode_attn / million_pq_decode_attn_append: the case table, the builders and
one runner, shared by test_decode_poison_gpu.py, test_decode_poison_host.py and lds_poison_child.py.

Every case builds two copies of the same valid data:
  clean     - everything outside the live data is zero (code bytes past T, unused pool pages, page-table entries past the
              live pages, window rows outside the ring's span);
  poisoned  - code bytes of tokens >= T (last live page, row-major tensors past T, pages between the device length and the
              host bound) and pool pages no live entry names are 0xFF; page-table entries past the live pages name a 0xFF page
              (always an id inside the pool); window rows outside [resid_start, resid_start + r) - the row a fused append is
              about to write included - are fp16 NaN; out is NaN before every call.
At C = 256, 0xFF is a valid code: a leak then gives a finite but wrong answer, which only the exact comparison of the two runs
catches.  Checks (check_case): the kernel kind, the clean run against the fp64 oracle (whole tensor and every head), the
poisoned run bitwise equal to the clean one, the fused append's window row, the rest of the window and the device lengths."""
from __future__ import annotations

import ctypes
import zlib
from dataclasses import dataclass

import numpy as np

REL_TOL = 1e-3        # test_gpu_parity.py
MEAN_ABS_TOL = 1e-3
EXTRA_PAGES = 3       # pool pages that no live entry names


@dataclass(frozen=True)
class Case:
    name: str
    d: int
    M: int
    C: int
    G: int                 # query heads per kv head
    kind: int              # million_attn_kernel_kind under `policy`
    policy: int = 0        # million_set_force_generic
    bs: int = 1
    nhk: int = 2
    kl: str = "paged"      # K codes: "paged" pool or "row"-major tensor
    vl: str = "paged"      # V codes: "paged", "row" (transposed into the workspace by the call) or "dense" (v_pages_dense)
    ps: int = 64
    i64: bool = False
    T: int = 1000          # quantised tokens (the device length when dev)
    gap: int = 0           # dev: the host bound is T + gap
    r: int = 17
    rs: int = 0            # ring start
    cap: int = 128
    dev: bool = False      # device-resident lengths
    append: bool = False   # fused append of one window row

    @property
    def nh(self):
        return self.G * self.nhk

    @property
    def T_host(self):
        return self.T + (self.gap if self.dev else 0)

    @property
    def n_live(self):      # live pages per (b, kv head)
        return -(-self.T // self.ps)

    @property
    def n_pages_cap(self):      # two table entries past the host bound's pages
        return -(-self.T_host // self.ps) + 2

    @property
    def T_cap(self):            # rows of a row-major code tensor
        return self.T_host + 64

    @property
    def n_pool(self):
        return self.bs * self.nhk * self.n_live + EXTRA_PAGES

    @property
    def paged(self):
        return self.kl == "paged" or self.vl in ("paged", "dense")


def _c(name, d, M, C, G, kind, **kw):
    return Case(name, d, M, C, G, kind, **kw)


# (a launch splits and its merge runs at every one of these contexts: >= 8 pages per (b, kv head) on a 256-CU chip)
CASES = [
    # lean kernel (csrc/attn_lean.h): policy 0, kind 1
    _c("lean-d128-M64-ps64-C256", 128, 64, 256, 4, 1, bs=2, T=1000),
    _c("lean-d128-M64-ps64-C128", 128, 64, 128, 4, 1, bs=2, T=2500, r=100, rs=90, dev=True, gap=200, append=True, i64=True),
    _c("lean-d128-M64-ps128-C256", 128, 64, 256, 3, 1, ps=128, T=3333, r=40, rs=110, i64=True),
    _c("lean-d128-M64-ps128-C128", 128, 64, 128, 4, 1, ps=128, T=1000, append=True),
    _c("lean-d128-M32-ps64-C256", 128, 32, 256, 2, 1, T=2500, r=60, rs=100, dev=True, gap=100),
    _c("lean-d128-M32-ps64-C128", 128, 32, 128, 4, 1, T=1000, r=1, rs=127),
    _c("lean-d128-M32-ps128-C256", 128, 32, 256, 4, 1, ps=128, T=1000, r=0),
    _c("lean-d128-M32-ps128-C128", 128, 32, 128, 1, 1, ps=128, T=3333, r=100, rs=60, append=True, i64=True),
    _c("lean-d64-M64-C256", 64, 64, 256, 4, 1, T=1000),
    _c("lean-d64-M64-C128", 64, 64, 128, 4, 1, ps=128, T=2500, r=100, rs=90, dev=True, gap=300, append=True),
    _c("lean-d64-M32-C256", 64, 32, 256, 2, 1, T=3333, r=5),
    _c("lean-d64-M32-C128", 64, 32, 128, 4, 1, T=1000, r=120, rs=30, append=True),
    _c("lean-d64-M16-C256", 64, 16, 256, 4, 1, ps=128, T=1000),
    _c("lean-d64-M16-C128", 64, 16, 128, 3, 1, T=2500, r=64, rs=100, dev=True, gap=64, append=True, i64=True),
    # query-head parts (virtual kv heads) with device lengths and the fused append
    _c("parts-d64-M32-G7-C128", 64, 32, 128, 7, 1, T=1000, r=50, rs=100, dev=True, gap=300, append=True),
    _c("parts-d64-M64-G8-C256", 64, 64, 256, 8, 1, ps=128, T=2500, r=100, rs=90, dev=True, gap=100, append=True, i64=True),
    _c("parts-d128-M16-G8-C128", 128, 16, 128, 8, 1, T=1000, r=30, rs=110, dev=True, gap=200, append=True),
    # two launches in one call (16 + 4 query heads)
    _c("groups-d128-M64-G20-C256", 128, 64, 256, 20, 1, T=1000, r=70, rs=100, dev=True, gap=150, append=True),
    _c("groups-d128-M32-G20-C128", 128, 32, 128, 20, 1, T=2500, r=17, rs=120, dev=True, gap=64, append=True),
    # streaming kernel: policy 16 keeps the lean kernel's shapes on it
    _c("stream-M64-C256", 128, 64, 256, 4, 1, policy=16, T=2500),
    _c("stream-M64-C128", 128, 64, 128, 4, 1, policy=16, T=1000, r=100, rs=90, dev=True, gap=200, append=True),
    _c("stream-M32-C256", 128, 32, 256, 8, 1, policy=16, T=3333, r=40, i64=True),
    _c("stream-M32-C128", 128, 32, 128, 2, 1, policy=16, T=2500, append=True),
    _c("stream-M16-C256", 128, 16, 256, 4, 1, policy=16, T=1000),
    _c("stream-M16-C128", 128, 16, 128, 4, 1, policy=16, T=2500, r=100, rs=90, dev=True, gap=100),
    # tile kernel
    _c("tile-d64-M32-ps32-C256", 64, 32, 256, 4, 3, ps=32, T=1000),
    _c("tile-d64-M16-ps32-C128", 64, 16, 128, 4, 3, ps=32, T=2500, r=100, rs=90, dev=True, gap=100, append=True),
    _c("tile-T0-d128-M64-C256", 128, 64, 256, 4, 3, T=0, r=30, rs=120, append=True),
    # row-major code layouts
    _c("rowkv-d128-M64-C256", 128, 64, 256, 4, 2, kl="row", vl="row", T=1000),
    _c("rowkv-d128-M64-C128", 128, 64, 128, 4, 2, kl="row", vl="row", T=2500, r=100, rs=90, dev=True, gap=100, append=True),
    _c("rowkv-d64-M16-C128", 64, 16, 128, 4, 2, kl="row", vl="row", T=1000, r=40),
    _c("rowK-pagedV-d128-M64-C128", 128, 64, 128, 4, 1, kl="row", T=1000, r=40, rs=100),
    _c("rowK-pagedV-d128-M32-C256", 128, 32, 256, 4, 1, kl="row", ps=128, T=2500, i64=True, append=True),
    _c("denseV-d128-M64-C128", 128, 64, 128, 4, 1, kl="row", vl="dense", T=1000, r=100, rs=90, append=True),
    _c("denseV-d64-M32-C256", 64, 32, 256, 4, 1, kl="row", vl="dense", T=2500),
    # scalar kernel
    _c("scalar-d128-M64-C256", 128, 64, 256, 4, 0, policy=1, T=1000),
    _c("scalar-d64-M32-C128", 64, 32, 128, 4, 0, policy=1, T=2500, r=100, rs=90, dev=True, gap=100, append=True),
    _c("scalar-pagedK-rowV-d128-M64-C256", 128, 64, 256, 4, 0, vl="row", T=1000, r=40, rs=100),
]
BY_NAME = {c.name: c for c in CASES}


def make_desc(c: Case, lib_types):
    """The million_attn_desc of a case (dev_lengths left NULL: the runner sets it)."""
    d = lib_types.AttnDesc()
    d.struct_size = ctypes.sizeof(lib_types.AttnDesc)
    d.bs, d.nh, d.nh_k, d.d, d.M, d.C = c.bs, c.nh, c.nhk, c.d, c.M, c.C
    d.n_tokens, d.r, d.resid_start, d.resid_cap = c.T_host, c.r, c.rs, c.cap
    d.resid_stride_b, d.resid_stride_h = c.nhk * c.cap * c.d, c.cap * c.d
    d.k_layout = lib_types.MILLION_KV_PAGED if c.kl == "paged" else lib_types.MILLION_KV_ROWMAJOR
    d.v_layout = lib_types.MILLION_KV_PAGED if c.vl in ("paged", "dense") else lib_types.MILLION_KV_ROWMAJOR
    d.v_pages_dense = int(c.vl == "dense")
    if c.paged:
        d.page_size, d.n_pages_cap, d.page_ids_i64 = c.ps, c.n_pages_cap, int(c.i64)
    row = (c.nhk * c.T_cap * c.M, c.T_cap * c.M)
    if c.kl == "row":
        d.k_stride_b, d.k_stride_h = row
    else:
        d.k_pool_pages = c.n_pool
    if c.vl == "row":
        d.v_stride_b, d.v_stride_h = row
    elif c.vl == "paged":
        d.v_pool_pages = c.n_pool
    return d


def build(c: Case, src: dict | None = None) -> dict:
    """Both copies of a case's data plus the live masks: {"clean": {...}, "poisoned": {...}, "live": {...}, "codes": ...}.
    Arrays: q, k_cents, v_cents, k_codes, v_codes, ids (paged sides; None otherwise), k_res, v_res, k_new, v_new (append),
    lengths (dev).  live[name] is True where the two copies must agree.
    src: the valid data from elsewhere (tests/decode_inputs.py: an input family) instead of this function's own N(0, 1) draws:
    q (bs, nh, 1, d), k_cents, v_cents, row-major k_codes / v_codes (bs, nh_k, T, M), k_res / v_res of cap rows and, for an
    appending case, k_new / v_new; layouts, poison and masks are built around it as around the draws."""
    rs_ = np.random.RandomState(zlib.crc32(c.name.encode()))
    f = lambda *s: rs_.standard_normal(s).astype(np.float16)
    bs, nhk, T, M, ps = c.bs, c.nhk, c.T, c.M, c.ps
    base = dict(q=f(bs, c.nh, 1, c.d), k_cents=f(M, c.C, c.d // M), v_cents=f(M, c.C, c.d // M))
    kcodes = rs_.randint(0, c.C, (bs, nhk, T, M)).astype(np.uint8)
    vcodes = rs_.randint(0, c.C, (bs, nhk, T, M)).astype(np.uint8)
    kres, vres = f(bs, nhk, c.cap, c.d), f(bs, nhk, c.cap, c.d)
    if c.append:
        base["k_new"], base["v_new"] = f(bs, nhk, 1, c.d), f(bs, nhk, 1, c.d)
    if src is not None:
        for nm in base:
            assert src[nm].shape == base[nm].shape and src[nm].dtype == base[nm].dtype, nm
            base[nm] = src[nm]
        for nm, own in (("k_codes", kcodes), ("v_codes", vcodes), ("k_res", kres), ("v_res", vres)):
            assert src[nm].shape == own.shape and src[nm].dtype == own.dtype, nm
        kcodes, vcodes, kres, vres = src["k_codes"], src["v_codes"], src["k_res"], src["v_res"]
    clean, pois, live = dict(base), dict(base), {}

    # window: valid rows of the ring; everything else 0 / NaN
    ring = (c.rs + np.arange(c.r)) % c.cap
    wl = np.zeros(c.cap, bool)
    wl[ring] = True
    wmask = np.broadcast_to(wl[None, None, :, None], kres.shape)
    for nm, w in (("k_res", kres), ("v_res", vres)):
        clean[nm] = np.where(wmask, w, np.float16(0))
        pois[nm] = np.where(wmask, w, np.float16("nan"))
        live[nm] = wmask.copy()

    # physical pages: live pages of (b, kv head) pairs, then the extra pages, shuffled (page order must not matter)
    n_lp = bs * nhk * c.n_live
    perm = np.random.RandomState(7 + n_lp).permutation(c.n_pool)      # perm[phys] = logical page
    inv = np.argsort(perm)                                          # inv[logical] = phys
    spare = [int(inv[n_lp + e]) for e in range(EXTRA_PAGES) if inv[n_lp + e] != 0]      # 0xFF pages with a non-zero id

    def pool(codes, transposed):
        shp = (c.n_pool, M, ps) if transposed else (c.n_pool, ps, M)
        pc, pp, lv = np.zeros(shp, np.uint8), np.full(shp, 0xFF, np.uint8), np.zeros(shp, bool)
        for b in range(bs):
            for h in range(nhk):
                for j in range(c.n_live):
                    ph = int(inv[(b * nhk + h) * c.n_live + j])
                    blk = codes[b, h, j * ps:(j + 1) * ps]
                    n = blk.shape[0]
                    if transposed:
                        pc[ph, :, :n] = pp[ph, :, :n] = blk.T
                        lv[ph, :, :n] = True
                    else:
                        pc[ph, :n] = pp[ph, :n] = blk
                        lv[ph, :n] = True
        return pc, pp, lv

    def dense(codes):
        n = bs * nhk * c.n_pages_cap
        pc, pp, lv = np.zeros((n, M, 64), np.uint8), np.full((n, M, 64), 0xFF, np.uint8), np.zeros((n, M, 64), bool)
        for b in range(bs):
            for h in range(nhk):
                for j in range(c.n_live):
                    blk = codes[b, h, j * 64:(j + 1) * 64].T
                    pg = (b * nhk + h) * c.n_pages_cap + j
                    pc[pg, :, :blk.shape[1]] = pp[pg, :, :blk.shape[1]] = blk
                    lv[pg, :, :blk.shape[1]] = True
        return pc, pp, lv

    def rowmajor(codes):
        shp = (bs, nhk, c.T_cap, M)
        pc, pp, lv = np.zeros(shp, np.uint8), np.full(shp, 0xFF, np.uint8), np.zeros(shp, bool)
        pc[:, :, :T] = pp[:, :, :T] = codes
        lv[:, :, :T] = True
        return pc, pp, lv

    for nm, codes, layout in (("k_codes", kcodes, c.kl), ("v_codes", vcodes, c.vl)):
        if layout == "row":
            clean[nm], pois[nm], live[nm] = rowmajor(codes)
        elif layout == "dense":
            clean[nm], pois[nm], live[nm] = dense(codes)
        else:
            clean[nm], pois[nm], live[nm] = pool(codes, nm == "v_codes")

    if c.kl == "paged" or c.vl == "paged":
        ids_c = np.zeros((bs, nhk, c.n_pages_cap), np.int64)
        ids_p = np.zeros_like(ids_c)
        lv = np.zeros(ids_c.shape, bool)
        for b in range(bs):
            for h in range(nhk):
                for j in range(c.n_pages_cap):
                    if j < c.n_live:
                        ids_c[b, h, j] = ids_p[b, h, j] = inv[(b * nhk + h) * c.n_live + j]
                        lv[b, h, j] = True
                    else:      # past the live pages: page 0 when clean, a 0xFF page (in the pool) when poisoned
                        ids_p[b, h, j] = spare[(b + h + j) % len(spare)]
        dt = np.int64 if c.i64 else np.int32
        clean["ids"], pois["ids"], live["ids"] = ids_c.astype(dt), ids_p.astype(dt), lv
    else:
        clean["ids"] = pois["ids"] = None

    if c.dev:
        ln = np.zeros((bs, 4), np.int32)
        ln[:, 0], ln[:, 1], ln[:, 2] = T, c.r, c.rs
        clean["lengths"], pois["lengths"] = ln, ln.copy()
    return {"clean": clean, "poisoned": pois, "live": live, "k_codes": kcodes, "v_codes": vcodes}


def gold(c: Case, built: dict, oracle) -> np.ndarray:
    """fp64 oracle: the ring's valid rows in order (np.roll), plus the appended row."""
    cl = built["clean"]
    kw = np.roll(cl["k_res"], -c.rs, axis=2)[:, :, :c.r]
    vw = np.roll(cl["v_res"], -c.rs, axis=2)[:, :, :c.r]
    if c.append:
        kw, vw = np.concatenate([kw, cl["k_new"]], axis=2), np.concatenate([vw, cl["v_new"]], axis=2)
    r = kw.shape[2]
    if r == 0:      # the oracle wants at least one window row (never read at r = 0)
        kw = vw = np.zeros((c.bs, c.nhk, 1, c.d), np.float16)
    return oracle.decode_attn(cl["q"], built["k_codes"], built["v_codes"], cl["k_cents"], cl["v_cents"], kw, vw, r)


def kernel_kind(c: Case, lib, lib_types) -> int:
    """million_attn_kernel_kind under the case's policy (host logic: no launch, no GPU)."""
    desc = make_desc(c, lib_types)
    if c.dev:
        desc.dev_lengths = 4096      # only its being set matters to the planner; it is never read on the host
    lib.million_set_force_generic(c.policy)
    try:
        return int(lib.million_attn_kernel_kind(ctypes.byref(desc)))
    finally:
        lib.million_set_force_generic(0)


def run(c: Case, arrs: dict, torch, ops, lib, lib_types) -> dict:
    """One call on one copy.  Returns out, k_res, v_res (after the call) and lengths (dev) as numpy arrays."""
    cu = lambda a: None if a is None else torch.from_numpy(np.ascontiguousarray(a)).cuda()
    ptr = lambda t: None if t is None else t.data_ptr()
    t = {k: cu(v) for k, v in arrs.items() if isinstance(v, np.ndarray)}
    kp = ops.prepare_cents(t["k_cents"], cache=False)
    vp = ops.prepare_cents(t["v_cents"], cache=False)
    out = torch.full_like(t["q"], float("nan"))
    desc = make_desc(c, lib_types)
    if c.dev:
        desc.dev_lengths = t["lengths"].data_ptr()
    ws = ops.attn_workspace(desc, t["q"].device)
    ids = t.get("ids")
    kids = ids if c.kl == "paged" else None
    vids = ids if c.vl == "paged" else None
    stream = torch.cuda.current_stream().cuda_stream
    lib.million_set_force_generic(c.policy)
    try:
        if c.append:
            rc = lib.million_pq_decode_attn_append(ctypes.byref(desc), ptr(t["q"]), ptr(t["k_new"]), ptr(t["v_new"]),
                                                   ptr(t["k_codes"]), ptr(t["v_codes"]), ptr(kids), ptr(vids), ptr(kp), ptr(vp),
                                                   ptr(t["k_res"]), ptr(t["v_res"]), ptr(out), ptr(ws), ws.numel(), stream)
        else:
            rc = lib.million_pq_decode_attn(ctypes.byref(desc), ptr(t["q"]), ptr(t["k_codes"]), ptr(t["v_codes"]), ptr(kids),
                                            ptr(vids), ptr(kp), ptr(vp), ptr(t["k_res"]), ptr(t["v_res"]), ptr(out), ptr(ws),
                                            ws.numel(), stream)
        torch.cuda.synchronize()
    finally:
        lib.million_set_force_generic(0)
    assert rc == 0, f"{c.name}: rc={rc} {lib.million_last_error()}"
    res = {"out": out.cpu().numpy(), "k_res": t["k_res"].cpu().numpy(), "v_res": t["v_res"].cpu().numpy()}
    if c.dev:
        res["lengths"] = t["lengths"].cpu().numpy()
    return res


def head_err(out, gold) -> np.ndarray:
    """||out - gold||_2 / ||gold||_2 over d for every (b, h) of a decode step's (bs, nh, 1, d) output: (bs, nh)."""
    out, gold = np.asarray(out, np.float64), np.asarray(gold, np.float64)
    return (np.linalg.norm(out - gold, axis=-1) / np.maximum(np.linalg.norm(gold, axis=-1), 1e-300))[:, :, 0]


def _bits(a):
    return np.ascontiguousarray(a).view(np.uint16)


def check_case(c: Case, torch, ops, lib, lib_types, oracle) -> dict:
    """Every assertion of the matrix for one case; returns a few numbers for reports."""
    got = kernel_kind(c, lib, lib_types)
    assert got == c.kind, f"{c.name}: kernel kind {got}, expected {c.kind}"
    built = build(c)
    clean = run(c, built["clean"], torch, ops, lib, lib_types)
    pois = run(c, built["poisoned"], torch, ops, lib, lib_types)
    g = gold(c, built, oracle)
    o = clean["out"].astype(np.float64)
    assert np.isfinite(o).all(), f"{c.name}: clean run not finite"
    rel = np.linalg.norm(o - g) / max(np.linalg.norm(g), 1e-30)
    mae = np.abs(o - g).mean()
    assert rel < REL_TOL and mae < MEAN_ABS_TOL, f"{c.name}: clean run vs oracle rel={rel:.3e} mean_abs={mae:.3e}"
    e = head_err(o, g)      # and every head on its own
    b_, h_ = np.unravel_index(np.argmax(e), e.shape)
    assert e[b_, h_] < REL_TOL, (f"{c.name}: clean run, worst head (b={b_}, h={h_}) rel-L2 {e[b_, h_]:.3e} >= {REL_TOL:g}; "
                                 f"{int((e >= REL_TOL).sum())} of {e.size} heads fail (whole tensor {rel:.3e})")
    po = pois["out"]
    n_bad = int((~np.isfinite(po.astype(np.float32))).sum())
    assert n_bad == 0, f"{c.name}: poisoned run has {n_bad} non-finite outputs"
    n_diff = int((_bits(po) != _bits(clean["out"])).sum())
    assert n_diff == 0, (f"{c.name}: poisoned run differs from the clean run in {n_diff} outputs "
                         f"(max abs {np.abs(po.astype(np.float64) - o).max():.3e})")
    if c.append:
        row = (c.rs + c.r) % c.cap
        for run_, src in ((clean, built["clean"]), (pois, built["poisoned"])):
            for nm, new in (("k_res", "k_new"), ("v_res", "v_new")):
                after, before = _bits(run_[nm]), _bits(src[nm])
                assert np.array_equal(after[:, :, row], _bits(src[new])[:, :, 0]), f"{c.name}: {nm} row {row} is not the new row"
                keep = np.ones(c.cap, bool)
                keep[row] = False
                assert np.array_equal(after[:, :, keep], before[:, :, keep]), f"{c.name}: {nm} changed outside row {row}"
    else:
        for run_, src in ((clean, built["clean"]), (pois, built["poisoned"])):
            for nm in ("k_res", "v_res"):
                assert np.array_equal(_bits(run_[nm]), _bits(src[nm])), f"{c.name}: {nm} written without an append"
    if c.dev:
        for run_, src in ((clean, built["clean"]), (pois, built["poisoned"])):
            want = src["lengths"].copy()
            want[:, 1] += 1 if c.append else 0
            assert np.array_equal(run_["lengths"], want), f"{c.name}: lengths {run_['lengths'].tolist()} != {want.tolist()}"
    faults = ops.tail_faults()
    assert faults == 0, f"{c.name}: {faults} split merges gave up"
    return {"rel": float(rel), "mean_abs": float(mae), "worst_head": float(e[b_, h_])}
