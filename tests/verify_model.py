"""Numpy models of draft verification (include/million_hip.h, "Draft verification"): the block-merge formula of
million_attn_block_merge in fp64, million_window_commit from its closed form, and the rule the closed form must equal - a_b
single decode steps, "if the window is full, flush the oldest page; append".  Shared by test_verify_host.py and
test_verify_gpu.py."""
from __future__ import annotations

import numpy as np


def block_merge(q, k, v, out_a, lse_a, n_valid=None):
    """q, out_a (bs, nh, n, d), k, v (bs, nh_k, n, d), lse_a (bs, nh, n): (out (bs, nh, n, d), lse (bs, nh, n)), fp64.
    Row i < n_valid[b] sees the block keys j <= i: s_j = q_i . k_j / sqrt(d), L = max(lse_a, max s_j), w = exp(lse_a - L) (0 for
    -inf), p_j = exp(s_j - L), out = (w out_a + sum p_j v_j) / (w + sum p_j), lse = L + ln(w + sum p_j); a NaN lse_a: a NaN
    row.  Rows at or past n_valid[b]: out = 0, lse = -inf, whatever the inputs hold there."""
    bs, nh, n, d = q.shape
    G = nh // k.shape[1]
    out, lse = np.zeros((bs, nh, n, d)), np.full((bs, nh, n), -np.inf)
    for b in range(bs):
        nb = n if n_valid is None else max(0, min(n, int(n_valid[b])))
        for h in range(nh):
            K, V = k[b, h // G].astype(np.float64), v[b, h // G].astype(np.float64)
            for i in range(nb):
                la = float(lse_a[b, h, i])
                if np.isnan(la):
                    out[b, h, i], lse[b, h, i] = np.nan, np.nan
                    continue
                s = q[b, h, i].astype(np.float64) @ K[:i + 1].T / np.sqrt(d)
                L = max(la, s.max())
                w = np.exp(la - L) if np.isfinite(la) else 0.0
                p = np.exp(s - L)
                den = w + p.sum()
                past = w * out_a[b, h, i].astype(np.float64) if w > 0 else 0.0
                out[b, h, i] = (past + p @ V[:i + 1]) / den
                lse[b, h, i] = L + np.log(den)
    return out, lse


def _ring(r, start, cap):
    """A window of r live rows from slot `start`: ring[slot] = ("w", j) for the j-th oldest row, None for a dead slot."""
    ring = [None] * cap
    for j in range(r):
        ring[(start + j) % cap] = ("w", j)
    return ring


def commit_closed(T, r, start, a, ps, cap, ring=None, rows=None):
    """million_window_commit of one (layer, request): (T', r', start', coded, ring').  coded: {token: source row} for the rows
    that became codes; ring': the window's slots afterwards.  Source rows are `ring`'s entries (default ("w", j)) and rows[i]
    (default ("n", i)).  Closed form: S = [window in ring order; new rows], F = ceil((r + a - cap) / ps) if r + a > cap else 0,
    f = F ps; S[0, f) -> tokens [T, T + f); new row i with r + i >= f -> slot (start + r + i) % cap; T += f, r += a - f,
    start = (start + f) % cap."""
    ring = list(_ring(r, start, cap) if ring is None else ring)
    rows = [("n", i) for i in range(a)] if rows is None else rows
    S = [ring[(start + j) % cap] for j in range(r)] + [rows[i] for i in range(a)]
    F = -(-(r + a - cap) // ps) if r + a > cap else 0
    f = F * ps
    coded = {T + j: S[j] for j in range(f)}
    for i in range(a):
        if r + i >= f:
            ring[(start + r + i) % cap] = rows[i]
    return T + f, r + a - f, (start + f) % cap, coded, ring


def commit_sequential(T, r, start, a, ps, cap, ring=None, rows=None):
    """The same through a single decode steps: if r == cap, the oldest ps rows become tokens [T, T + ps) and the window moves
    on; then the new row goes to slot (start + r) % cap."""
    ring = list(_ring(r, start, cap) if ring is None else ring)
    rows = [("n", i) for i in range(a)] if rows is None else rows
    coded = {}
    for i in range(a):
        if r == cap:
            for t in range(ps):
                coded[T + t] = ring[(start + t) % cap]
            T, r, start = T + ps, r - ps, (start + ps) % cap
        ring[(start + r) % cap] = rows[i]
        r += 1
    return T, r, start, coded, ring


def live_ring(ring, r, start, cap):
    """{slot: row} of the r live slots from `start`."""
    return {(start + j) % cap: ring[(start + j) % cap] for j in range(r)}
