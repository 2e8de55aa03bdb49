"""fp64 numpy model of chunk attention over PQ codes of any width (million_pq_chunk_attn / million_pq_chunk_attn_wide): n_q query
rows of every request against [dequantised codes (wide_model.decode) ; window rows in ring order ; the chunk, causally], the
output and the natural-log lse.  The attention is the formula of tests/test_chunk_attn_gpu.py's model, with the lse beside it.
The reference of tests/test_chunk_wide_gpu.py.

Shapes: q (bs, nh, n_q, d); codes (bs, nh_k, T_cap, M); cents (M, C, d_m); window (bs, nh_k, cap, d) read as a ring of r rows from
`start`; k_chunk / v_chunk (bs, nh_k, n_q, d) or None (every row sees the past only).  T, r, start, n_q: ints, or one per request.
Rows at or past a request's n_q: zeros and lse -inf, as the kernel stores them; so is a row that sees no key."""
import numpy as np

from tests import wide_model as W


def chunk_attn(q, k_codes, v_codes, k_cents, v_cents, k_res, v_res, r, *, T=None, start=0, k_chunk=None, v_chunk=None, n_q=None):
    """-> out (bs, nh, n_q, d) fp64, lse (bs, nh, n_q) fp64."""
    q = np.asarray(q, dtype=np.float64)
    bs, nh, nq_all, d = q.shape
    nhk = k_res.shape[1]
    G = nh // nhk
    per = lambda x, default: [int(v) for v in np.broadcast_to(np.asarray(default if x is None else x), (bs,))]
    Ts, rs, ss, nqs = per(T, k_codes.shape[2]), per(r, 0), per(start, 0), per(n_q, nq_all)
    out, lse = np.zeros((bs, nh, nq_all, d)), np.full((bs, nh, nq_all), -np.inf)
    for b in range(bs):
        n = nqs[b]
        if n == 0:
            continue
        K = [W.decode(k_codes[b, :, :Ts[b]], k_cents), W.ring_rows(k_res[b], rs[b], ss[b])]
        V = [W.decode(v_codes[b, :, :Ts[b]], v_cents), W.ring_rows(v_res[b], rs[b], ss[b])]
        n_c = 0
        if k_chunk is not None:
            K.append(np.asarray(k_chunk[b, :, :n], dtype=np.float64))
            V.append(np.asarray(v_chunk[b, :, :n], dtype=np.float64))
            n_c = n
        K, V = np.concatenate(K, axis=1), np.concatenate(V, axis=1)
        n_past = K.shape[1] - n_c
        if K.shape[1] == 0:
            continue
        for h in range(nh):
            s = q[b, h, :n] @ K[h // G].T / np.sqrt(np.float64(d))
            if n_c:
                j = np.arange(n_c)[None, :]
                s[:, n_past:] = np.where(j <= np.arange(n)[:, None], s[:, n_past:], -np.inf)
            m = s.max(axis=1, keepdims=True)
            p = np.exp(s - m)
            l = p.sum(axis=1, keepdims=True)
            out[b, h, :n] = (p @ V[h // G]) / l
            lse[b, h, :n] = (m + np.log(l))[:, 0]
    return out, lse


def head_errors(got, ref):
    """(rel-L2, mean-abs) of every (b, head) over its (n_q, d) block: two (bs, nh) arrays (a zero reference: absolute L2)."""
    return W.head_errors(got, ref)


def lse_error(got, ref):
    """Worst |got - ref| over the rows whose reference is finite; the others must be -inf in both."""
    got, ref = np.asarray(got, dtype=np.float64), np.asarray(ref, dtype=np.float64)
    none = np.isneginf(ref)
    assert np.array_equal(np.isneginf(got), none), "lse: -inf rows differ from the model's"
    return float(np.abs(got[~none] - ref[~none]).max()) if (~none).any() else 0.0
