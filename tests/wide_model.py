"""fp64 numpy model of the decode step over PQ codes of any width (uint8 or uint16): decode through the codebook, softmax over
[K^ ; window rows in ring order ; appended row], the output and the natural-log lse.  The reference of tests/test_attn_wide_*.py and
tests/test_cache_wide_gpu.py; checked against the oracle's own forms in tests/test_attn_wide_host.py.

Shapes: q (bs, nh, 1, d) or (bs, nh, d); codes (bs, nh_k, T, M); cents (M, C, d_m); window (bs, nh_k, cap, d) read as a ring of r
rows from `start`; k_new / v_new (bs, nh_k, 1, d) or None.  T, r, start: ints, or one per request."""
import numpy as np


def decode(codes, cents):
    """(bs, nh_k, T, M) codes -> (bs, nh_k, T, d) fp64: out[..., m d_m + k] = cents[m, code_m, k]."""
    codes, cents = np.asarray(codes), np.asarray(cents, dtype=np.float64)
    M, C, dm = cents.shape
    assert codes.shape[-1] == M and (codes.size == 0 or int(codes.max()) < C)
    return cents[np.arange(M), codes.astype(np.int64)].reshape(*codes.shape[:-1], M * dm)


def ring_rows(res, r, start):
    """The r live rows of one request's window (nh_k, cap, d), oldest first."""
    cap = res.shape[1]
    return np.asarray(res, dtype=np.float64)[:, (start + np.arange(r)) % cap]


def attend(q, K, V):
    """q (nh, d), K / V (nh_k, n, d) fp64 -> out (nh, d), lse (nh,); nothing to attend to: zeros and -inf."""
    nh, d = q.shape
    G = nh // K.shape[0]
    if K.shape[1] == 0:
        return np.zeros((nh, d)), np.full(nh, -np.inf)
    Kg, Vg = np.repeat(K, G, axis=0), np.repeat(V, G, axis=0)
    s = np.einsum("hd,hnd->hn", q, Kg) / np.sqrt(np.float64(d))
    m = s.max(axis=-1, keepdims=True)
    p = np.exp(s - m)
    l = p.sum(axis=-1, keepdims=True)
    return np.einsum("hn,hnd->hd", p / l, Vg), (m + np.log(l))[:, 0]


def decode_attn(q, k_codes, v_codes, k_cents, v_cents, k_res, v_res, r, *, T=None, start=0, k_new=None, v_new=None):
    """-> out (bs, nh, 1, d) fp64, lse (bs, nh) fp64.  T: tokens of the code tensors that are live (None: all of them)."""
    q = np.asarray(q, dtype=np.float64)
    if q.ndim == 4:
        q = q[:, :, 0]
    bs, nh, d = q.shape
    per = lambda x: [int(v) for v in np.broadcast_to(np.asarray(k_codes.shape[2] if x is None else x), (bs,))]
    Ts, rs, ss = per(T), per(r), per(start)
    out, lse = np.empty((bs, nh, d)), np.empty((bs, nh))
    for b in range(bs):
        K = [decode(k_codes[b, :, :Ts[b]], k_cents), ring_rows(k_res[b], rs[b], ss[b])]
        V = [decode(v_codes[b, :, :Ts[b]], v_cents), ring_rows(v_res[b], rs[b], ss[b])]
        if k_new is not None:
            K.append(np.asarray(k_new[b], dtype=np.float64))
            V.append(np.asarray(v_new[b], dtype=np.float64))
        out[b], lse[b] = attend(q[b], np.concatenate(K, axis=1), np.concatenate(V, axis=1))
    return out[:, :, None], lse


def head_errors(got, ref):
    """(rel-L2, mean-abs) of every head: got, ref (bs, nh, 1, d) -> two (bs, nh) arrays (a zero reference head: absolute L2)."""
    got, ref = np.asarray(got, dtype=np.float64).reshape(ref.shape), np.asarray(ref, dtype=np.float64)
    num = np.sqrt(((got - ref) ** 2).sum(axis=(-1, -2)))
    den = np.sqrt((ref ** 2).sum(axis=(-1, -2)))
    return num / np.where(den > 0, den, 1.0), np.abs(got - ref).mean(axis=(-1, -2))
