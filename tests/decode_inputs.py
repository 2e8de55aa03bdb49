"""Decode-step attention on the input families of tests/flash_inputs.py: the generator, the per-head bar, the case lists and a
numpy model of the lean / streaming kernels' arithmetic (csrc/attn_lean.h, attn_stream.h, attn_front.h, attn_tail.h).
Not collected: test_decode_numerics_host.py and test_decode_numerics_gpu.py import it.

The key axis of a decode step is [T codes | r window rows from rstart in a ring of cap | the appended row, if any]: the chunk
axis of flash_inputs.chunk_inputs at n_q = 1, whose one chunk row is the row a fused append writes.  The arrays are the ones
decode_poison.build draws from its own RNG, so every case of decode_poison.CASES - every kernel form, layout, id width and length
mode - runs on any family (build(c, src=...)).

The bar: rel-L2 < 1e-3 of the fp64 oracle for every (b, h) on its own (check_heads), beside the whole-tensor bars."""
import numpy as np

from tests import decode_poison as P
from tests import flash_inputs as F

PEAKS = F.DECODE_PEAKS
NAMES = list(F.FAMILIES) + ["peak:" + p for p in PEAKS]      # what section (a) of the GPU file runs on every one of its cases
CUS = 256            # compute units of an MI355X: the split policy (mfma_splits) deals about one workgroup to each


# ---------------------------------------------------------------- inputs ------------------------------------------------
def decode_inputs(name, bs, nh, nh_k, d, M, C, T, r, cap, rstart, append, peak=None):
    """q (bs, nh, 1, d), k_cents, v_cents (M, C, d / M), row-major k_codes / v_codes (bs, nh_k, T, M), k_res / v_res (bs, nh_k,
    cap, d) with the r valid rows at ring positions rstart .., k_new / v_new (bs, nh_k, 1, d; None without append) of family
    `name`, or of gauss1 with one dominating key (peak, one of PEAKS).  "st": the chunk_inputs state, for flash_inputs' models."""
    st = F.chunk_inputs(name, bs, nh, nh_k, d, M, C, 1, T, r, cap, rstart, bool(append), peak=peak)
    out = {nm: st[nm] for nm in ("q", "k_cents", "v_cents", "k_codes", "v_codes", "k_res", "v_res")}
    out.update(k_new=st["k_ch"], v_new=st["v_ch"], peak_at=st["peak_at"], st=st)
    return out


def split_name(name):
    """"peak:x" -> ("gauss1", "x"); a family -> (family, None)."""
    return ("gauss1", name[5:]) if name.startswith("peak:") else (name, None)


def has_peak(c, peak):
    """Whether case c has the segment peak `peak` lies in."""
    if peak in ("code_first", "code_last"):
        return c.T > 0
    if peak == "window_wrap":
        return 0 < c.cap - c.rs < c.r
    return peak is None or (peak == "appended" and c.append)


def for_case(name, c):
    """The inputs of family / peak `name` at the shape of decode_poison case c."""
    fam, peak = split_name(name)
    return decode_inputs(fam, c.bs, c.nh, c.nhk, c.d, c.M, c.C, c.T, c.r, c.cap, c.rs, c.append, peak=peak)


def keys(oracle, c, src, b=0):
    """(K, V) fp16 (nh_k, T + r (+ 1), d) of request b over the key axis, as the kernels see them: decoded codes, window rows in
    ring order, the appended row."""
    ring = (c.rs + np.arange(c.r)) % c.cap
    out = []
    for codes, cents, res, new in ((src["k_codes"], src["k_cents"], src["k_res"], src["k_new"]),
                                   (src["v_codes"], src["v_cents"], src["v_res"], src["v_new"])):
        parts = ([oracle.pq_decode(codes[b:b + 1], cents)[0]] if c.T else []) + [res[b][:, ring]] + ([new[b]] if c.append else [])
        out.append(np.concatenate(parts, axis=1).astype(np.float16))
    return out


def request(src, b):
    """The inputs of request b alone."""
    return {nm: (a[b:b + 1] if isinstance(a, np.ndarray) and nm not in ("k_cents", "v_cents") else a) for nm, a in src.items()
            if nm != "st"}


def gold(oracle, c, src):
    """fp64 oracle.decode_attn of the inputs themselves (what decode_poison.gold computes from a built case), for the requests
    src holds."""
    ring = (c.rs + np.arange(c.r)) % c.cap
    kw, vw = src["k_res"][:, :, ring], src["v_res"][:, :, ring]
    if c.append:
        kw, vw = np.concatenate([kw, src["k_new"]], axis=2), np.concatenate([vw, src["v_new"]], axis=2)
    r = kw.shape[2]
    if r == 0:      # the oracle wants at least one window row (never read at r = 0)
        kw = vw = np.zeros((src["q"].shape[0], c.nhk, 1, c.d), np.float16)
    return oracle.decode_attn(src["q"], src["k_codes"], src["v_codes"], src["k_cents"], src["v_cents"], kw, vw, r)


# ---------------------------------------------------------------- the bar -----------------------------------------------
def check_heads(out, gold_, what, name="gauss1"):
    """Every (b, h) within REL_TOL of fp64, the whole-tensor bars as before (mean-abs in units of the family's V scale).  One
    DECNUM line: worst head, 99th percentile, whole tensor."""
    fam, _ = split_name(name)
    return F.check_rows(out, gold_, what, unit=F.v_unit(fam), tag="DECNUM", each="head")


def whole_tensor_ok(out, gold_, unit=1.0):
    """The bars the decode tests had before: one norm over the whole output, and the mean absolute error."""
    out, gold_ = np.asarray(out, np.float64), np.asarray(gold_, np.float64)
    rel = np.linalg.norm(out - gold_) / max(np.linalg.norm(gold_), 1e-300)
    return rel < F.REL_TOL and np.abs(out - gold_).mean() / unit < F.MEAN_ABS_TOL


# ---------------------------------------------------------------- cases -------------------------------------------------
# (a) every family and peak on one case per kernel form
SECTION_A = ["lean-d128-M64-ps64-C128", "lean-d128-M32-ps64-C256", "lean-d64-M64-C128", "lean-d64-M32-C128", "lean-d64-M16-C128",
             "parts-d64-M32-G7-C128", "groups-d128-M64-G20-C256", "stream-M64-C128", "stream-M32-C256", "stream-M16-C128",
             "tile-d64-M16-ps32-C128", "scalar-d64-M32-C128"]
SECTION_B_NAMES = ["gauss4", "sink_local"]                                  # (b) on every case of decode_poison.CASES
# (c) many (request, kv head) pairs, one split each: a wave streams T / 8 keys under one lazy reference
MANY_PAIRS = dict(T=4096, r=100, cap=128, rs=60, G=4, nhk=8, d=128, M=64, C=256, ps=64)
MANY_PAIRS_NAMES = ["gauss4", "descending"]      # (descending last: the flush check of the host file reuses it)
# (d) every grouping of query heads: (form, d, M, policy)
GROUPINGS = [1, 2, 3, 4, 5, 6, 7, 8, 9, 12, 13, 16]
GROUP_FORMS = [("lean", 128, 64, 0), ("stream", 128, 64, 16), ("parts-d64", 64, 32, 0), ("parts-m16", 128, 16, 0)]
GROUP_NAMES = ["gauss4", "peak:last_head", "peak:head0"]
# (e) one ragged launch with device lengths: (T, r) per request
RAGGED_T = [0, 1, 31, 32, 33, 63, 64, 65, 511, 512, 513, 1023, 1025]
RAGGED_R = [1, 0, 127, 128, 1, 0, 127, 128, 0, 1, 128, 127, 1]            # (request 0 has no codes: it needs a window row)
RAGGED_START = [0, 5, 100, 17, 127, 0, 64, 1, 33, 90, 127, 3, 60]


def many_pairs_case(policy, cus=CUS):
    m = MANY_PAIRS
    return P.Case(f"pairs-{'stream' if policy else 'lean'}", m["d"], m["M"], m["C"], m["G"], 1, policy=policy, bs=-(-cus // m["nhk"]),
                  nhk=m["nhk"], ps=m["ps"], T=m["T"], r=m["r"], rs=m["rs"], cap=m["cap"])


def group_case(form, d, M, policy, G):
    return P.Case(f"G{G}-{form}", d, M, 256, G, 1, policy=policy, bs=3, nhk=2, T=1000, r=100, rs=90, cap=128)


def group_inputs(name, c):
    """gauss4, or gauss1 with a dominating key (the last key of the code segment) that only ONE query head sees: the last head of
    every group ("peak:last_head") or head 0 ("peak:head0") keeps its structured channels, the others' are zeroed."""
    if not name.startswith("peak:"):
        return for_case(name, c)
    src = for_case("peak:code_last", c)
    q = src["q"].copy().reshape(c.bs, c.nhk, c.G, 1, c.d)
    keep = c.G - 1 if name == "peak:last_head" else 0
    q[:, :, [g for g in range(c.G) if g != keep], :, :c.d // 2] = 0
    src["q"] = q.reshape(c.bs, c.nh, 1, c.d)
    return src


RAGGED_TMAX = max(RAGGED_T)


def ragged_inputs(name="gauss4"):
    """One batch, request i of which uses the first RAGGED_T[i] codes and RAGGED_R[i] window rows from RAGGED_START[i] (every
    row of the ring is a valid draw)."""
    return decode_inputs(name, len(RAGGED_T), 8, 2, 128, 64, 256, RAGGED_TMAX, 128, 128, 0, False)


def ragged_case(i, policy):
    """Request i as the launch sees it: its own lengths on the device, the batch's bound on the host."""
    return P.Case(f"ragged{i}", 128, 64, 256, 4, 1, policy=policy, bs=len(RAGGED_T), nhk=2, T=RAGGED_T[i], gap=RAGGED_TMAX - RAGGED_T[i],
                  r=RAGGED_R[i], rs=RAGGED_START[i], cap=128, dev=True)


def ragged_request(src, i, policy):
    """(case, inputs) of request i: the batch's arrays with the codes cut to the request's length."""
    c = ragged_case(i, policy)
    one = dict(src, k_codes=src["k_codes"][:, :, :c.T], v_codes=src["v_codes"][:, :, :c.T])
    return c, one


# ---------------------------------------------------------------- the arithmetic model ---------------------------------
def launches(c):
    """The launches of a call as the planner forms them (million_api.hip attn_impl, attn_mfma.hip mfma_hparts / plan_attn_mfma):
    [(heads of a kv head group that share a workgroup ..., unit, pairs)]: a list of (head lists, tokens per unit, workgroup pairs
    of the launch).  Groups above 16 heads run as launches of 16 + the rest; 5 .. 16 heads run as parts (virtual kv heads of at
    most 4) on the lean kernel's d = 64 forms and the streaming kernel's M = 16 form, as one workgroup on the streaming kernel's
    other forms.  The tile and scalar kernels (no lazy reference) are modelled as the streaming kernel."""
    out, g0 = [], 0
    while g0 < c.G:
        n = min(c.G - g0, 16)
        lean_off = bool(c.policy & 16)
        parts = -(-n // 4) if (n > 4 and (c.d == 64 or c.M == 16) and not lean_off) else 1
        gp = -(-n // parts)
        lean = gp <= 4 and c.ps >= 64 and not lean_off and (c.d == 64 or c.M in (64, 32))
        groups = [list(range(g0 + i * gp, g0 + min(n, (i + 1) * gp))) for i in range(parts)]
        out.append((groups, 64 if lean else 32, c.bs * c.nhk * parts))
        g0 += n
    return out


def mfma_splits(T, pairs, cap, cus=CUS):
    """attn_mfma.hip mfma_splits for T <= 16384 * splits: about one workgroup per CU, a split at least 512 tokens long."""
    ns = min(-(-cus // pairs), 64, -(-T // 512) if T > 0 else 1)
    ns = max(1, min(ns, -(-T // 32) if T > 0 else 1))
    return max(ns, -(-cap // 128))


def _p16(p, flush):
    h = p.astype(np.float16)
    if flush:      # the defect the flush check is about: an fp16-subnormal operand read as zero
        h = np.where(p < np.float32(2.0 ** -14), np.float16(0), h)
    return h.astype(np.float32)


def model_workgroups(q, K, V, T, *, unit, ps, ns, flush=False):
    """One (request, kv head) of the lean (unit = 64) or streaming (unit = 32) kernel for the query heads q (G, d) fp16 that share a
    workgroup; K, V (T + r, d) fp16 over [codes | window rows in order, the appended one last].  -> (G, d) fp16.
      * 8 waves per split.  Units are dealt by page, strided (attn_front.h): wave w of split s owns the unit at token
        ((j ppr + w / upp) ns + s) ps + (w % upp) unit in round j (upp = ps / unit units per page, ppr = 8 / upp);
      * window row j goes to split j % ns, and a split's rows go to its waves in runs of 16; a wave runs its window tile first,
        with the exact maximum as reference (softmax_online);
      * code units: raw fp32 scores; the reference moves (for every head of the workgroup) only when some head's score exceeds
        its reference by 2^3 in the scaled domain (thr = (m + 8) / c), to max(m, c max x); p = exp2(fma(x, c, -m)), rounded to
        fp16 for the value product, accumulated in fp32; l from the unrounded p;
      * wave partials merged in fp32 (weights exp2(m_w - max)), then the split partials the same way; one division; fp16."""
    G, d = q.shape
    c = np.float32(F.LOG2E / np.sqrt(d))
    inv_c = np.float32(1.0) / c
    n_keys = K.shape[0]
    S = F._f32(q) @ F._f32(K).T                               # (G, keys) raw scores, fp32 accumulation
    V32 = F._f32(V)
    upp, ninf = ps // unit, np.float32(-np.inf)
    ppr = 8 // upp
    parts = []
    for s in range(ns):
        rows = np.arange(s, n_keys - T, ns)
        wm, wl, wO = [], [], []
        for w in range(8):
            m, l, O = np.full(G, ninf, np.float32), np.zeros(G, np.float32), np.zeros((G, d), np.float32)
            idx = T + rows[16 * w:16 * w + 16]
            if len(idx):
                sc = S[:, idx] * c
                m = sc.max(axis=1)
                pr = F._exp2(sc - m[:, None])
                l = pr.sum(axis=1, dtype=np.float32)
                O = _p16(pr, flush) @ V32[idx]
            t0 = ((w // upp) * ns + s) * ps + (w % upp) * unit
            for tu in range(t0, T, ns * ppr * ps):
                x = S[:, tu:min(tu + unit, T)]
                mx = x.max(axis=1)
                if (mx > (m + np.float32(8)) * inv_c).any():
                    m_new = np.maximum(m, mx * c)
                    alpha = F._exp2(m - np.where(m_new > ninf, m_new, np.float32(0)))
                    O, l, m = O * alpha[:, None], l * alpha, m_new
                pr = F._exp2(F._fma(x, c, np.where(m > ninf, -m, np.float32(0))[:, None]))
                l = l + pr.sum(axis=1, dtype=np.float32)
                O = O + _p16(pr, flush) @ V32[tu:tu + x.shape[1]]
            wm.append(m), wl.append(l), wO.append(O)
        parts.append(_merge(np.array(wm), np.array(wl), np.array(wO)))
    m, l, O = parts[0] if ns == 1 else _merge(*(np.array(x) for x in zip(*parts)))
    with np.errstate(divide="ignore", invalid="ignore"):
        return np.where(l[:, None] > 0, O * (np.float32(1) / l)[:, None], np.float32(0)).astype(np.float16)


def _merge(m, l, O):
    """(n, G), (n, G), (n, G, d) partials -> one: weights exp2(m_i - max m) in fp32 (merge_and_publish, tail_merge_head)."""
    mx = m.max(axis=0)
    f = F._exp2(m - np.where(mx > -np.inf, mx, np.float32(0))[None])
    return mx, (f * l).sum(axis=0, dtype=np.float32), (f[:, :, None] * O).sum(axis=0, dtype=np.float32)


def model_heads(oracle, c, src, heads, b=0, flush=False, cus=CUS):
    """The model for the query heads `heads` (indices within the whole nh) of request b of case c: every workgroup that holds one
    of them is run (its heads share the reference's moves).  -> {head: (d,) fp16}"""
    K, V = keys(oracle, c, src, b)
    T_host = c.T_host
    out = {}
    for h in heads:
        hk, g = divmod(h, c.G)
        for groups, unit, pairs in launches(c):
            for grp in groups:
                if g in grp and h not in out:
                    ns = mfma_splits(T_host, pairs, c.cap, cus)
                    o = model_workgroups(src["q"][b, [hk * c.G + x for x in grp], 0], K[hk], V[hk], c.T, unit=unit,
                                         ps=c.ps if c.paged else 64, ns=ns, flush=flush)
                    for x, row in zip(grp, o):
                        out.setdefault(hk * c.G + x, row)
    return {h: out[h] for h in heads}
