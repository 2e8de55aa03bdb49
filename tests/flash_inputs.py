"""Inputs, references and arithmetic models for the flash family (csrc/prefill.hip, csrc/chunk_attn.hip, csrc/flash_tile.h).
Not collected: test_flash_numerics_host.py and test_flash_numerics_gpu.py import it.

Every input family has the same form, so that one description serves prompt attention (K given as rows) and chunk attention
(the first T keys exist only as PQ codes):

    logit(i, j) = q_i . k_j / sqrt(d) = a * t_j + noise(i, j)

The first d / 2 channels (S) carry the structure: q = a u there (u a fixed pattern of +-1, the same for every row) and k_j = t_j u,
t_j the key's *level*, one of a finite set.  The other channels (N) carry independent gaussian noise.  A family without
structure (gauss, outlier_channels) uses all d channels for noise.  For the code segment of chunk attention a structured
subspace reserves one code per level (its centroid is level * the matching sub-vector of u) and a noise subspace holds random
centroids addressed by random codes.

The bar: the project's rel-L2 < 1e-3, applied to every output row (row_err) and, as before, to the whole tensor."""
import numpy as np

from tests.test_chunk_attn_gpu import model as chunk_model      # the fp64 model of chunk attention (and oracle.pq_decode)

REL_TOL = 1e-3
MEAN_ABS_TOL = 1e-3
LOG2E = 1.4426950408889634

# name -> (family, argument, power of two on V)
FAMILIES = {
    "gauss1": ("gauss", 1, 0), "gauss2": ("gauss", 2, 0), "gauss4": ("gauss", 4, 0), "gauss8": ("gauss", 8, 0),
    "outlier4": ("outlier_channels", 4, 0), "sink_local": ("sink_local", None, 0),
    "stair5": ("staircase", 5, 0), "stair9": ("staircase", 9, 0), "descending": ("descending", None, 0),
    "gauss4-v*2^10": ("gauss", 4, 10), "gauss4-v*2^-6": ("gauss", 4, -6),
}
PEAKS = ("code_first", "code_last", "window_wrap", "chunk_row")
DECODE_PEAKS = ("code_first", "code_last", "window_wrap", "appended")      # tests/decode_inputs.py: the row a fused append writes

SINK_NATS = 8.0           # sink_local: key 0 lies this far above the noise, and the ramp climbs as far over the last 64 keys
PEAK_NATS = 16.0          # peak_in: the dominating key
DESC_LO, DESC_HI = 11.0, 19.0      # descending: later keys lie this many log2 units below key 0 (+- noise: 10 .. 20)
DESC_LEVELS = 64


def v_unit(name):
    """The scale of V (and so of the output) in family `name`: the mean-abs bar is in these units."""
    return 2.0 ** FAMILIES[name][2] if name in FAMILIES else 1.0


# ---------------------------------------------------------------- families ----------------------------------------------
def _spec(name, n_keys, d, peak_at=None):
    """-> dict(a, levels (n_keys,) fp16 values, n_struct channels, sq, sk (d,) noise stds of q and k, v_mean).
    peak_at: key index of a dominating key (peak_in families, built on gauss(1))."""
    kind, arg, _ = FAMILIES[name] if name in FAMILIES else ("peak", None, 0)
    ns = d // 2
    gain = ns / np.sqrt(d)                      # logit per unit of a * t
    sp = dict(a=0.0, levels=np.zeros(n_keys, np.float16), ns=0, sq=np.ones(d), sk=np.ones(d), v_mean=0.0)
    if kind == "gauss":
        sp["sq"][:] = sp["sk"][:] = np.sqrt(arg)
    elif kind == "outlier_channels":            # 90 % of the logit variance in two channels
        L = float(arg)
        hot, cold = (0.9 * d * L * L / 2) ** 0.25, (0.1 * d * L * L / (d - 2)) ** 0.25
        sp["sq"][:] = sp["sk"][:] = cold
        sp["sq"][[5, d - 3]] = sp["sk"][[5, d - 3]] = hot
    else:
        sp["ns"] = ns
        sp["sq"][:ns] = sp["sk"][:ns] = 0.0
        sp["sq"][ns:] = sp["sk"][ns:] = (d / (d - ns)) ** 0.25      # noise logits of standard deviation 1
        t = np.zeros(n_keys)
        if kind == "sink_local":
            sp["a"] = 1.0
            nr = min(64, n_keys - 1)
            t[n_keys - nr:] = SINK_NATS * np.arange(1, nr + 1) / nr / gain
            t[0] = SINK_NATS / gain
        elif kind == "staircase":               # levels 0.5 h are exact; a carries the step
            sp["a"] = arg / LOG2E / gain / 0.5
            t = 0.5 * (np.arange(n_keys) // 32)
        elif kind == "descending":
            sp["a"] = 1.0
            sp["sq"][ns:] = sp["sk"][ns:] = (0.1 / LOG2E) ** 0.5 * (d / (d - ns)) ** 0.25      # noise of 0.1 log2 units
            lv = np.random.RandomState(1234).randint(0, DESC_LEVELS, n_keys)
            t = -(DESC_LO + (DESC_HI - DESC_LO) * lv / (DESC_LEVELS - 1)) / LOG2E / gain
            t[0] = 0.0
            sp["v_mean"] = 1.0                  # V with a common component: a flushed probability then shows in the output
        elif kind == "peak":
            sp["a"] = 1.0
            t[peak_at] = PEAK_NATS / gain
        sp["levels"] = t.astype(np.float16)
    sp["a"] = float(np.float16(sp["a"]))
    return sp


def _u(d, ns):
    u = np.zeros(d)
    u[:ns] = np.where(np.random.RandomState(77).randint(0, 2, ns) > 0, 1.0, -1.0)
    return u


def _seed(name, *shape):
    import zlib
    return zlib.crc32(repr((name,) + shape).encode())


def _q(rs, sp, bs, nh, n_q, d):
    return (rs.standard_normal((bs, nh, n_q, d)) * sp["sq"] + sp["a"] * _u(d, sp["ns"])).astype(np.float16)


def prefill_inputs(name, bs, nh, nh_k, n_q, n_kv, d):
    """fp16 q (bs, nh, n_q, d), k, v (bs, nh_k, n_kv, d) of family `name` (a key of FAMILIES)."""
    rs = np.random.RandomState(_seed(name, bs, nh, nh_k, n_q, n_kv, d))
    sp = _spec(name, n_kv, d)
    q = _q(rs, sp, bs, nh, n_q, d)
    k = rs.standard_normal((bs, nh_k, n_kv, d)) * sp["sk"] + sp["levels"].astype(np.float64)[:, None] * _u(d, sp["ns"])
    v = (rs.standard_normal((bs, nh_k, n_kv, d)) + sp["v_mean"]) * v_unit(name)
    return q, k.astype(np.float16), v.astype(np.float16)


def chunk_inputs(name, bs, nh, nh_k, d, M, C, n_q, T, r, cap, rstart, chunk, peak=None):
    """The state dict of test_chunk_attn_gpu._state / _run for family `name` over the concatenated key axis [T codes | r window
    rows from rstart in a ring of cap | the chunk's n_q rows].  peak: one of PEAKS (name is then ignored: gauss(1) plus one
    dominating key in that segment; "appended": the first chunk row - at n_q = 1 the row a decode step appends)."""
    n_c = n_q if chunk else 0
    n_keys = T + r + n_c
    at = None
    if peak is not None:
        name = "peak_in:" + peak
        at = {"code_first": min(5, T - 1), "code_last": T - 1, "window_wrap": T + (cap - rstart), "chunk_row": T + r + n_q // 2,
              "appended": T + r}[peak]
        assert 0 <= at < n_keys and (peak != "window_wrap" or (0 < cap - rstart < r)), "the shape has no such segment"
    rs = np.random.RandomState(_seed(name, bs, nh, nh_k, d, M, C, n_q, T, r, cap, rstart, chunk))
    sp = _spec(name, n_keys, d, at)
    dm, ns, u, vu = d // M, sp["ns"], _u(d, sp["ns"]), v_unit(name)
    lv = sp["levels"].astype(np.float64)
    st = dict(q=_q(rs, sp, bs, nh, n_q, d), r=r, rs=rstart, peak_at=at)
    # codes: a structured subspace keeps one code per level, from C - 1 downwards (its other centroids are noise nobody addresses)
    vals = np.unique(lv[:T])
    assert len(vals) <= C, f"{len(vals)} levels in the code segment, {C} codes"
    k_cents = rs.standard_normal((M, C, dm)) * sp["sk"].reshape(M, 1, dm)
    k_codes = rs.randint(0, C, (bs, nh_k, T, M))
    for m in range(ns // dm):
        k_cents[m, C - len(vals):] = vals[:, None] * u[m * dm:(m + 1) * dm]
        k_codes[:, :, :, m] = C - len(vals) + np.searchsorted(vals, lv[:T])
    st["k_cents"], st["k_codes"] = k_cents.astype(np.float16), k_codes.astype(np.uint8)
    st["v_cents"] = ((rs.standard_normal((M, C, dm)) + sp["v_mean"]) * vu).astype(np.float16)
    st["v_codes"] = rs.randint(0, C, (bs, nh_k, T, M)).astype(np.uint8)
    rows = lambda n, lev: (rs.standard_normal((bs, nh_k, n, d)) * sp["sk"] + lev[:, None] * u).astype(np.float16)
    vrows = lambda n: ((rs.standard_normal((bs, nh_k, n, d)) + sp["v_mean"]) * vu).astype(np.float16)
    ring = (rstart + np.arange(r)) % cap
    st["k_res"], st["v_res"] = rows(cap, np.zeros(cap)), vrows(cap)
    st["k_res"][:, :, ring] = rows(r, lv[T:T + r])
    st["k_win"], st["v_win"] = st["k_res"][:, :, ring], st["v_res"][:, :, ring]
    st["k_ch"], st["v_ch"] = (rows(n_q, lv[T + r:]), vrows(n_q)) if chunk else (None, None)
    return st


def chunk_keys(oracle, st):
    """(K, V) fp16 over the concatenated key axis and the number of past keys, for the arithmetic models."""
    T = st["k_codes"].shape[2]
    ks = ([oracle.pq_decode(st["k_codes"], st["k_cents"])] if T else []) + [st["k_win"]] + ([st["k_ch"]] if st["k_ch"] is not None else [])
    vs = ([oracle.pq_decode(st["v_codes"], st["v_cents"])] if T else []) + [st["v_win"]] + ([st["v_ch"]] if st["v_ch"] is not None else [])
    return (np.concatenate(ks, axis=2).astype(np.float16), np.concatenate(vs, axis=2).astype(np.float16),
            T + st["k_win"].shape[2])


def chunk_gold(oracle, st, rows=None):
    return chunk_model(oracle, st["q"], st["k_codes"], st["v_codes"], st["k_cents"], st["v_cents"], st["k_win"], st["v_win"],
                       st["k_ch"], st["v_ch"], rows=rows)


# ---------------------------------------------------------------- reference and metric ------------------------------------
def visible(n_q, n_kv, q_pos0=0, causal=True, rows=None):
    """(rows, n_kv) bool: key j is visible to query row i iff not causal or j <= q_pos0 + i."""
    rows = np.arange(n_q) if rows is None else np.asarray(rows)
    if not causal:
        return np.ones((len(rows), n_kv), bool)
    return np.arange(n_kv)[None, :] <= (q_pos0 + rows)[:, None]


def logits(q, k, rows=None):
    """fp64 q . k / sqrt(d): (bs, nh, rows, n_kv)."""
    nh, nh_k = q.shape[1], k.shape[1]
    qq = q.astype(np.float64) if rows is None else q[:, :, rows].astype(np.float64)
    kk = np.repeat(k.astype(np.float64), nh // nh_k, axis=1)
    return qq @ kk.transpose(0, 1, 3, 2) / np.sqrt(q.shape[3])


def prefill_gold(q, k, v, q_pos0=0, causal=True, rows=None, sliced=False):
    """fp64 prompt attention with GQA: q (bs, nh, n_q, d), k / v (bs, nh_k, n_kv, d) -> (bs, nh, rows, d).  rows: the query rows to
    evaluate (default all); sliced: q holds only those rows already.  Every row must see a key."""
    nh, nh_k = q.shape[1], k.shape[1]
    rows_ = np.arange(q.shape[2]) if rows is None else np.asarray(rows)
    vis = visible(None, k.shape[2], q_pos0, causal, rows_)
    out = np.zeros(q.shape[:2] + (len(rows_), q.shape[3]))
    for b in range(q.shape[0]):
        for h in range(nh):
            qr = q[b, h] if sliced else q[b, h, rows_]
            s = qr.astype(np.float64) @ k[b, h * nh_k // nh].astype(np.float64).T / np.sqrt(q.shape[3])
            s = np.where(vis, s, -np.inf)
            p = np.exp(s - s.max(axis=1, keepdims=True))
            out[b, h] = (p @ v[b, h * nh_k // nh].astype(np.float64)) / p.sum(axis=1, keepdims=True)
    return out


def row_err(out, gold):
    """||out_row - gold_row||_2 / ||gold_row||_2 over d, for every (b, h, i)."""
    out, gold = np.asarray(out, np.float64), np.asarray(gold, np.float64)
    return np.linalg.norm(out - gold, axis=-1) / np.maximum(np.linalg.norm(gold, axis=-1), 1e-300)


def check_rows(out, gold, what="", rows=None, unit=1.0, tol=REL_TOL, tag="FLASHNUM", each="row"):
    """Every output row within `tol` of gold, beside the whole-tensor bars (rel-L2 < REL_TOL, mean-abs < MEAN_ABS_TOL in units of
    `unit`, the scale of V).  rows: the query indices of axis 2 when only sampled rows are compared (for the message).
    Prints (one line, prefixed by `tag`; each: what a row of this output is called) and returns (worst row, 99th-percentile row,
    whole tensor)."""
    out, gold = np.asarray(out, np.float64), np.asarray(gold, np.float64)
    assert out.shape == gold.shape, f"{what}: shape {out.shape} vs {gold.shape}"
    assert np.isfinite(out).all(), f"{what}: non-finite output"
    e = row_err(out, gold)
    rel = np.linalg.norm(out - gold) / max(np.linalg.norm(gold), 1e-300)
    mae = np.abs(out - gold).mean() / unit
    b, h, i = np.unravel_index(np.argmax(e), e.shape)
    worst, p99 = float(e[b, h, i]), float(np.percentile(e, 99))
    print(f"{tag} {what}: worst {each} {worst:.2e} p99 {p99:.2e} whole {rel:.2e}")
    qi = i if rows is None else int(np.asarray(rows)[i])
    assert worst < tol, (f"{what}: worst {each} (b={b}, h={h}, i={qi}) rel-L2 {worst:.3e} >= {tol:g}; "
                         f"{int((e >= tol).sum())} of {e.size} {each}s fail (99th percentile {p99:.3e}, whole tensor {rel:.3e})")
    assert rel < REL_TOL and mae < MEAN_ABS_TOL, f"{what}: whole tensor rel={rel:.3e} mean_abs={mae:.3e}"
    return worst, p99, rel


def ideal(gold):
    """The best any kernel can do: the fp64 result rounded to fp16."""
    return np.asarray(gold).astype(np.float16)


# ---------------------------------------------------------------- arithmetic models ------------------------------------
# numpy restatements of what the d = 128 kernels compute for ONE query head: q (n_q, d) fp16, k / v (n_kv, d) fp16, vis (n_q, n_kv)
# bool, tiles = [(key0, key1)] in the order the kernel walks them.  fp32 where the kernel is fp32 (products accumulate in
# fp32; numpy's summation order differs from the MFMA's, which is the same class of error), fp16 where it rounds to fp16.
def prefill_tiles(n_kv, step=64):
    return [(j, min(j + step, n_kv)) for j in range(0, n_kv, step)]


def chunk_tiles(T, r, n_c, step=64):
    """A tile holds one source: codes, window, chunk."""
    out, base = [], 0
    for n in (T, r, n_c):
        out += [(base + j, base + min(j + step, n)) for j in range(0, n, step)]
        base += n
    return out


def _f32(x):
    return np.asarray(x, np.float32)


def _fma(a, b, c):
    """fp32 a * b + c with one rounding (the fp64 product of two fp32 numbers is exact)."""
    return (a.astype(np.float64) * np.float64(b) + c.astype(np.float64)).astype(np.float32)


def _exp2(x):
    with np.errstate(under="ignore"):
        return np.exp2(x.astype(np.float64)).astype(np.float32)


def model_plain(q, k, v, vis, tiles):
    """prefill_attn_kernel / chunk_attn_kernel (flash_tile.h): fp32 scores of the unscaled fp16 q, the scale applied in fp32 inside
    the exponent's fused multiply-add, online maximum per tile, P rounded to fp16 for the value product, l summed in fp32 from
    the unrounded P, O / l rounded to fp16."""
    c = np.float32(LOG2E / np.sqrt(q.shape[1]))
    n_q, d = q.shape
    O, l, m = np.zeros((n_q, d), np.float32), np.zeros(n_q, np.float32), np.full(n_q, -np.inf, np.float32)
    q32, v32 = _f32(q), _f32(v)
    for j0, j1 in tiles:
        sc = np.where(vis[:, j0:j1], q32 @ _f32(k[j0:j1]).T, np.float32(-np.inf))
        m_new = np.maximum(m, sc.max(axis=1) * c)
        m_safe = np.where(m_new > -np.inf, m_new, np.float32(0))
        alpha = _exp2(m - m_safe)
        O, l, m = O * alpha[:, None], l * alpha, m_new
        p = _exp2(_fma(sc, c, -m_safe[:, None]))
        l = l + p.sum(axis=1, dtype=np.float32)
        O = O + _f32(p.astype(np.float16)) @ v32[j0:j1]
    with np.errstate(divide="ignore", invalid="ignore"):
        return np.where(l[:, None] > 0, O / l[:, None], np.float32(0)).astype(np.float16)


def model_pipelined(q, k, v, vis, n_kv_tiles=None, scaled_q=False):
    """prefill_attn_pipe_kernel: 32-key halves; the scores of a half are accumulated from -reference, so the accumulator is the
    exponent's argument; the reference is lazy: it moves (for all 32 rows of a wave) only when a row of the wave sees a score
    more than 2^8 above its reference, so P <= 2^8 (exact in fp16's range).
    scaled_q = False: the kernel as it is: unscaled fp16 q, raw-score accumulator, p = exp2(c * (s - reference)).
    scaled_q = True:  the form it replaced: qf = fp16(q * c) and p = exp2(accumulator) - one more rounding of Q, which makes the
                      score error proportional to the score."""
    c = np.float32(LOG2E / np.sqrt(q.shape[1]))
    n_q, d = q.shape
    pad = (-n_q) % 32                      # rows past the end repeat the last one (prefill_q_row)
    idx = np.r_[np.arange(n_q), np.full(pad, n_q - 1)]
    q32 = _f32(q)[idx]
    vis = vis[idx]
    if scaled_q:
        q32, cs, thr = _f32((q32 * c).astype(np.float16)), np.float32(1), np.float32(8)
    else:
        cs, thr = c, np.float32(8) / c
    n = len(idx)
    O, l = np.zeros((n, d), np.float32), np.zeros(n, np.float32)
    m_ref, neg = np.full(n, -np.inf, np.float32), np.zeros(n, np.float32)
    has_ref = np.zeros(n, bool)
    v32 = _f32(v)
    for j0, j1 in prefill_tiles(k.shape[0], 32):
        s = (q32 @ _f32(k[j0:j1]).T + neg[:, None]).astype(np.float32)      # relative to the current reference
        s = np.where(vis[:, j0:j1], s, np.float32(-np.inf))
        mx = s.max(axis=1)
        trig = mx > np.where(has_ref, thr, np.float32(-np.inf))
        move = np.repeat(trig.reshape(-1, 32).any(axis=1), 32)
        m_new = np.where(move, np.maximum(m_ref, mx - neg), m_ref)
        m_safe = np.where(m_new > -np.inf, m_new, np.float32(0))
        alpha = np.where(move, _exp2((m_ref - m_safe) * cs), np.float32(1))
        O, l = O * alpha[:, None], l * alpha
        s = np.where(move[:, None], s + (-m_safe - neg)[:, None], s)
        neg = np.where(move, -m_safe, neg)
        m_ref, has_ref = m_new, has_ref | move
        p = _exp2(s * cs)
        l = l + p.sum(axis=1, dtype=np.float32)
        O = O + _f32(p.astype(np.float16)) @ v32[j0:j1]
    with np.errstate(divide="ignore", invalid="ignore"):
        out = np.where(l[:, None] > 0, O / l[:, None], np.float32(0)).astype(np.float16)
    return out[:n_q]


def model_heads(fn, q, k, v, vis, heads, *a, **kw):
    """A model over the query heads `heads` of batch 0: (len(heads), n_q, d) fp16."""
    G = q.shape[1] // k.shape[1]
    return np.stack([fn(q[0, h], k[0, h // G], v[0, h // G], vis, *a, **kw) for h in heads])
