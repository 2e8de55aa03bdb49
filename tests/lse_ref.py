"""fp64 references of the log-sum-exp surface (include/million_hip.h, "Log-sum-exp"): (out, lse) of a decode case built by
tests/decode_poison.py, (out, lse) of a chunk-attention state in the form of test_chunk_attn_gpu.py, and the merge of partial
attentions.  lse = ln sum_j exp(q . k_j / sqrt(d)) over the keys a row attends to, -inf where there is none (out = 0).
Shared by test_attn_lse_host.py and test_attn_lse_gpu.py."""
from __future__ import annotations

import numpy as np

LSE_TOL = 1e-3      # absolute, natural-log units: the project's 1e-3 applied to the softmax denominator


def softmax_state(s, V):
    """s (n_rows, n_keys) fp64 scaled scores (-inf = masked), V (n_keys, d): (out (n_rows, d), lse (n_rows,))."""
    n = s.shape[0]
    if s.shape[1] == 0:
        return np.zeros((n, V.shape[1])), np.full(n, -np.inf)
    m = s.max(axis=1, keepdims=True)
    ms = np.where(np.isfinite(m), m, 0.0)
    p = np.exp(s - ms)
    l = p.sum(axis=1, keepdims=True)
    with np.errstate(divide="ignore", invalid="ignore"):
        out = np.where(l > 0, (p @ V) / np.where(l > 0, l, 1.0), 0.0)
        lse = np.where(l[:, 0] > 0, ms[:, 0] + np.log(np.where(l[:, 0] > 0, l[:, 0], 1.0)), -np.inf)
    return out, lse


def keys_of_decode(c, built, oracle, tokens=None, window=True):
    """K, V (bs, nh_k, n, d) fp64 of a decode_poison case: the codes of `tokens` (a slice; default all T), then - window=True -
    the ring's valid rows in order and the appended row, as decode_poison.gold takes them."""
    cl = built["clean"]
    sl = slice(0, c.T) if tokens is None else tokens
    kc, vc = built["k_codes"][:, :, sl], built["v_codes"][:, :, sl]
    parts_k, parts_v = [], []
    if kc.shape[2]:
        parts_k.append(oracle.pq_decode(kc, cl["k_cents"]).astype(np.float64))
        parts_v.append(oracle.pq_decode(vc, cl["v_cents"]).astype(np.float64))
    if window:
        parts_k.append(np.roll(cl["k_res"], -c.rs, axis=2)[:, :, :c.r].astype(np.float64))
        parts_v.append(np.roll(cl["v_res"], -c.rs, axis=2)[:, :, :c.r].astype(np.float64))
        if c.append:
            parts_k.append(cl["k_new"].astype(np.float64))
            parts_v.append(cl["v_new"].astype(np.float64))
    if not parts_k:
        z = np.zeros((c.bs, c.nhk, 0, c.d))
        return z, z
    return np.concatenate(parts_k, axis=2), np.concatenate(parts_v, axis=2)


def attend(q, K, V):
    """q (bs, nh, n_q, d), K / V (bs, nh_k, n, d) fp64, no mask: (out (bs, nh, n_q, d), lse (bs, nh, n_q))."""
    bs, nh, n_q, d = q.shape
    G = nh // K.shape[1]
    out, lse = np.zeros((bs, nh, n_q, d)), np.zeros((bs, nh, n_q))
    for b in range(bs):
        for h in range(nh):
            s = q[b, h].astype(np.float64) @ K[b, h // G].T / np.sqrt(d)
            out[b, h], lse[b, h] = softmax_state(s, V[b, h // G])
    return out, lse


def decode_ref(c, built, oracle, tokens=None, window=True):
    """(out (bs, nh, 1, d), lse (bs, nh)) of a decode_poison case (or of a part of its keys: see keys_of_decode)."""
    K, V = keys_of_decode(c, built, oracle, tokens, window)
    out, lse = attend(built["clean"]["q"], K, V)
    return out, lse[:, :, 0]


def chunk_ref(oracle, st, n_valid=None):
    """(out (bs, nh, n_q, d), lse (bs, nh, n_q)) of a chunk state of test_chunk_attn_gpu._state: codes, the window rows in ring
    order, the chunk causally (when the state has one).  n_valid: per request, the rows of a ragged call (dev_n_q): the rows
    past it are out = 0, lse = -inf, and chunk keys past it are not seen."""
    q = st["q"]
    bs, nh, n_q, d = q.shape
    nhk = st["k_res"].shape[1]
    G = nh // nhk
    T = st["k_codes"].shape[2]
    Kc = oracle.pq_decode(st["k_codes"], st["k_cents"]).astype(np.float64) if T else np.zeros((bs, nhk, 0, d))
    Vc = oracle.pq_decode(st["v_codes"], st["v_cents"]).astype(np.float64) if T else np.zeros((bs, nhk, 0, d))
    out, lse = np.zeros((bs, nh, n_q, d)), np.full((bs, nh, n_q), -np.inf)
    for b in range(bs):
        nv = n_q if n_valid is None else int(n_valid[b])
        ks, vs = [Kc[b], st["k_win"][b].astype(np.float64)], [Vc[b], st["v_win"][b].astype(np.float64)]
        n_c = 0
        if st["k_ch"] is not None:
            ks.append(st["k_ch"][b, :, :nv].astype(np.float64))
            vs.append(st["v_ch"][b, :, :nv].astype(np.float64))
            n_c = nv
        K, V = np.concatenate(ks, axis=1), np.concatenate(vs, axis=1)
        n_past = K.shape[1] - n_c
        for h in range(nh):
            s = q[b, h, :nv].astype(np.float64) @ K[h // G].T / np.sqrt(d)
            if n_c:
                s[:, n_past:] = np.where(np.arange(n_c)[None, :] <= np.arange(nv)[:, None], s[:, n_past:], -np.inf)
            out[b, h, :nv], lse[b, h, :nv] = softmax_state(s, V[h // G])
    return out, lse


def merge(outs, lses):
    """The merge formula: outs[i] (..., d), lses[i] (...) -> (out, lse_out).  L = max lse_i, w_i = exp(lse_i - L) (0 for -inf),
    out = sum w_i out_i / sum w_i, lse_out = L + ln sum w_i; every part -inf: out 0, lse -inf; a NaN lse_i: the row is NaN."""
    outs = [np.asarray(o, np.float64) for o in outs]
    lses = [np.asarray(l, np.float64) for l in lses]
    Ls = np.stack(lses)
    nan = np.isnan(Ls).any(axis=0)
    L = np.max(np.where(np.isnan(Ls), -np.inf, Ls), axis=0)
    Lf = np.where(np.isfinite(L), L, 0.0)
    with np.errstate(invalid="ignore", divide="ignore"):
        w = np.where(np.isfinite(Ls), np.exp(Ls - Lf), 0.0)
        W = w.sum(axis=0)
        num = sum(w[i][..., None] * np.where(w[i][..., None] > 0, outs[i], 0.0) for i in range(len(outs)))
        out = np.where(W[..., None] > 0, num / np.where(W > 0, W, 1.0)[..., None], 0.0)
        lse = np.where(W > 0, Lf + np.log(np.where(W > 0, W, 1.0)), -np.inf)
    out = np.where(nan[..., None], np.nan, out)
    lse = np.where(nan, np.nan, lse)
    return out, lse


def lse_model_f32(q, K, scale_log2e=None, block=64):
    """What a kernel's arithmetic gives for the lse of one head: q (d,), K (n, d) fp16 values.  fp32 scores, online maximum in
    the scaled exp2 domain over blocks of `block` keys, probabilities rounded to fp16 before they are summed in fp32 (the value
    product's operand format feeds the denominator), lse = (m + log2 l) ln 2 in fp32."""
    d = q.shape[0]
    c = np.float32(1.4426950408889634 / np.sqrt(d)) if scale_log2e is None else np.float32(scale_log2e)
    s = (K.astype(np.float32) @ q.astype(np.float32)).astype(np.float32) * c
    m, l = np.float32(-np.inf), np.float32(0)
    for i in range(0, s.shape[0], block):
        sb = s[i:i + block]
        m_new = np.maximum(m, sb.max())
        if np.isfinite(m):
            l = np.float32(l * np.exp2(m - m_new, dtype=np.float32))
        p = np.exp2(sb - m_new, dtype=np.float32).astype(np.float16).astype(np.float32)
        l = np.float32(l + p.sum(dtype=np.float32))
        m = m_new
    if not l > 0:
        return -np.inf
    return float(np.float32(np.float32(m + np.log2(l, dtype=np.float32)) * np.float32(0.6931471805599453)))
