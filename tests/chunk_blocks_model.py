"""fp64 / numpy models of the block route of chunk attention (ops.pq_chunk_attn_blocks), of
million_prefill_attn_lse and of million_pq_gather_rows.  Not collected: test_chunk_blocks_host.py, test_prefill_lse_gpu.py,
test_gather_rows_gpu.py and test_chunk_blocks_gpu.py import it.

A chunk state is the dict of tests/test_chunk_attn_gpu._state / tests/flash_inputs.chunk_inputs: q, k_codes / v_codes
(bs, nh_k, T, M), k_cents / v_cents (M, C, d_m), the window buffers k_res / v_res with r rows from rs, those rows in ring order
(k_win / v_win), the chunk k_ch / v_ch or None."""
import numpy as np

from tests import lse_ref


# ---------------------------------------------------------------- prompt attention with lse --------------------------------
def prefill_ref(q, k, v, q_pos0=0, causal=True):
    """fp64 (out (bs, nh, n_q, d), lse (bs, nh, n_q)) of prompt attention with GQA; a row without a key: out 0, lse -inf."""
    bs, nh, n_q, d = q.shape
    nh_k, n_kv = k.shape[1], k.shape[2]
    G = nh // nh_k
    out, lse = np.zeros((bs, nh, n_q, d)), np.full((bs, nh, n_q), -np.inf)
    vis = np.ones((n_q, n_kv), bool) if not causal else np.arange(n_kv)[None, :] <= (q_pos0 + np.arange(n_q))[:, None]
    for b in range(bs):
        for h in range(nh):
            s = q[b, h].astype(np.float64) @ k[b, h // G].astype(np.float64).T / np.sqrt(d)
            s = np.where(vis, s, -np.inf)
            out[b, h], lse[b, h] = lse_ref.softmax_state(s, v[b, h // G].astype(np.float64))
    return out, lse


# ---------------------------------------------------------------- page pools of any code type ------------------------------
def to_pools(k_codes, v_codes, ps, extra_pages=3, seed=5, fill=0):
    """Row-major codes (bs, nh_k, T, M) -> (K pool (n_pool, ps, M), V pool (n_pool, M, ps) transposed, int32 ids (bs, nh_k, n_pages))
    with `extra_pages` unused pages and the physical pages shuffled; page tails past T and the unused pages hold `fill`.  The
    table has one entry more than the codes need (never to be read): it names an unused page."""
    bs, nhk, T, M = k_codes.shape
    n_pg = (T + ps - 1) // ps
    n_pool = bs * nhk * n_pg + extra_pages
    kpool = np.full((n_pool, ps, M), fill, k_codes.dtype)
    vpool = np.full((n_pool, M, ps), fill, v_codes.dtype)
    perm = np.random.RandomState(seed).permutation(n_pool)
    ids = np.zeros((bs, nhk, n_pg + 1), np.int32)
    i = 0
    for b in range(bs):
        for h in range(nhk):
            for pg in range(n_pg):
                pid = perm[i]
                i += 1
                ids[b, h, pg] = pid
                n = min(ps, T - pg * ps)
                kpool[pid, :n] = k_codes[b, h, pg * ps:pg * ps + n]
                vpool[pid, :, :n] = v_codes[b, h, pg * ps:pg * ps + n].T
            ids[b, h, n_pg] = perm[n_pool - 1]      # an unused page
    return kpool, vpool, ids


def from_pools(kpool, vpool, ids, T):
    """The codes read back through the table: (k_codes, v_codes) (bs, nh_k, T, M)."""
    bs, nhk = ids.shape[:2]
    ps, M = kpool.shape[1], kpool.shape[2]
    kc, vc = np.zeros((bs, nhk, T, M), kpool.dtype), np.zeros((bs, nhk, T, M), vpool.dtype)
    for b in range(bs):
        for h in range(nhk):
            for t0 in range(0, T, ps):
                n = min(ps, T - t0)
                kc[b, h, t0:t0 + n] = kpool[ids[b, h, t0 // ps], :n]
                vc[b, h, t0:t0 + n] = vpool[ids[b, h, t0 // ps], :, :n].T
    return kc, vc


def gather_ref(oracle, codes, cents, res, t0, t1, r, rs):
    """fp16 rows [dequant(codes[t0:t1]); the r ring rows of res from rs]: (bs, nh_k, (t1 - t0) + r, d)."""
    bs, nhk = codes.shape[:2]
    d = cents.shape[0] * cents.shape[2]
    parts = []
    if t1 > t0:
        parts.append(np.asarray(oracle.pq_decode(np.ascontiguousarray(codes[:, :, t0:t1]), cents)).astype(np.float16))
    if r:
        parts.append(res[:, :, (rs + np.arange(r)) % res.shape[2]])
    return np.concatenate(parts, axis=2) if parts else np.zeros((bs, nhk, 0, d), np.float16)


# ---------------------------------------------------------------- the route ------------------------------------------------
def keys_of_state(oracle, st):
    """fp64 (K_past, V_past) (bs, nh_k, T + r, d): the dequantised codes, then the window rows in ring order."""
    T = st["k_codes"].shape[2]
    ks = ([np.asarray(oracle.pq_decode(st["k_codes"], st["k_cents"]), np.float64)] if T else []) + [st["k_win"].astype(np.float64)]
    vs = ([np.asarray(oracle.pq_decode(st["v_codes"], st["v_cents"]), np.float64)] if T else []) + [st["v_win"].astype(np.float64)]
    return np.concatenate(ks, axis=2), np.concatenate(vs, axis=2)


def part_refs(oracle, st, plan):
    """fp64 (out, lse) of every part of a plan (ops.chunk_blocks_plan) on a chunk state."""
    T = st["k_codes"].shape[2]
    Kp, Vp = keys_of_state(oracle, st)
    res = []
    for part in plan["parts"]:
        if part[0] == "chunk":
            res.append(prefill_ref(st["q"], st["k_ch"], st["v_ch"], 0, True))
        else:
            _, t0, t1, r_here = part
            sel = np.r_[np.arange(t0, t1), T + np.arange(r_here)]
            res.append(lse_ref.attend(st["q"], Kp[:, :, sel], Vp[:, :, sel]))
    return res


def _merge_f32(outs, lses):
    """million_attn_merge's arithmetic: fp16 outs, fp32 lses -> fp32 accumulation, out rounded once to fp16, lse fp32."""
    outs = [np.asarray(o, np.float16).astype(np.float32) for o in outs]
    lses = [np.asarray(l, np.float32) for l in lses]
    Ls = np.stack(lses)
    Lm = Ls.max(axis=0)
    Lf = np.where(np.isfinite(Lm), Lm, np.float32(0))
    with np.errstate(invalid="ignore", over="ignore", under="ignore"):
        w = np.where(np.isfinite(Ls), np.exp(Ls - Lf, dtype=np.float32), np.float32(0))
    W = w.sum(axis=0, dtype=np.float32)
    num = np.zeros_like(outs[0])
    for i, o in enumerate(outs):
        num = num + w[i][..., None] * np.where(w[i][..., None] > 0, o, np.float32(0))
    with np.errstate(invalid="ignore", divide="ignore"):
        out = np.where(W[..., None] > 0, num / np.where(W > 0, W, np.float32(1))[..., None], np.float32(0)).astype(np.float16)
        lse = np.where(W > 0, Lf + np.log(np.where(W > 0, W, np.float32(1)), dtype=np.float32), np.float32(-np.inf)).astype(np.float32)
    return out, lse


def emulate_route(oracle, st, plan):
    """The roundings of the route on exact parts: every part's fp64 out rounded to fp16 and its lse to fp32, merged as the plan's
    groups say in fp32 with the merged out rounded to fp16 - the intermediate merges of a plan of more than one group too.
    -> (out fp16, lse fp32).  What a route with exact kernels gives: the part of the error the design itself makes."""
    q = st["q"]
    bs, nh, n_q, d = q.shape
    parts = [(o.astype(np.float16), l.astype(np.float32)) for o, l in part_refs(oracle, st, plan)]
    if not parts:
        return np.zeros((bs, nh, n_q, d), np.float16), np.full((bs, nh, n_q), -np.inf, np.float32)
    tops = []
    for group in plan["groups"]:
        if len(group) == 1:
            tops.append(parts[group[0]])
        else:
            tops.append(_merge_f32([parts[i][0] for i in group], [parts[i][1] for i in group]))
    if len(tops) == 1:
        return tops[0]
    return _merge_f32([t[0] for t in tops], [t[1] for t in tops])


def route_ref(oracle, st):
    """fp64 (out, lse) of the unsplit attention of a chunk state (lse_ref.chunk_ref)."""
    return lse_ref.chunk_ref(oracle, st)


def check_bar(out, gold, what, rel_tol=1e-3, mae_tol=1e-3):
    """The project's attention bar on the whole tensor; prints the figures, returns rel-L2."""
    out, gold = np.asarray(out, np.float64), np.asarray(gold, np.float64)
    assert out.shape == gold.shape, f"{what}: shape {out.shape} vs {gold.shape}"
    assert np.isfinite(out).all(), f"{what}: non-finite output"
    rel = np.linalg.norm(out - gold) / max(np.linalg.norm(gold), 1e-30)
    mae = np.abs(out - gold).mean()
    print(f"BLOCKS {what}: rel {rel:.2e} mean_abs {mae:.2e}")
    assert rel < rel_tol and mae < mae_tol, f"{what}: rel={rel:.3e} mean_abs={mae:.3e}"
    return rel


def check_lse(lse, gold, what, tol=lse_ref.LSE_TOL):
    """-inf exactly where gold is -inf, within tol elsewhere."""
    lse, gold = np.asarray(lse, np.float64), np.asarray(gold, np.float64)
    assert lse.shape == gold.shape, f"{what}: lse shape {lse.shape} vs {gold.shape}"
    dead = np.isneginf(gold)
    assert np.array_equal(np.isneginf(lse), dead), f"{what}: lse is not -inf exactly where no key is seen"
    err = float(np.abs(lse[~dead] - gold[~dead]).max()) if (~dead).any() else 0.0
    print(f"BLOCKS {what}: lse max abs err {err:.2e}")
    assert np.isfinite(lse[~dead]).all() and err < tol, f"{what}: lse max abs err {err:.3e} >= {tol:g}"
    return err
