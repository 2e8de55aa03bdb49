"""fp64 models of the sink rows (include/million_hip.h, "Sink rows"): million_attn_sink_merge's formula restated in numpy, and a
per-request model of a PagedPQCache with sink_tokens = S - what a request's attention sees is
    [its exact sink rows; the dequantised codes of the rows behind them; the window rows; the new rows]
with the softmax of tests/lse_ref.py over all of it.  numpy only.  Shared by test_attn_sink_host.py, test_attn_sink_gpu.py and
test_cache_sink_gpu.py."""
from __future__ import annotations

import numpy as np

from tests import lse_ref as R

S_CAP_MAX = 64


def clamp(x, bound):
    return min(max(int(x), 0), bound)


def sink_merge(q, k_sink, v_sink, out_a, lse_a, s_valid=None, n_valid=None):
    """q (bs, nh, n, d), k_sink / v_sink (bs, nh_k, s_cap, d), out_a (bs, nh, n, d), lse_a (bs, nh, n) -> (out, lse_out) fp64.
    s_valid / n_valid: per request, the live sink rows / query rows (any int: clamped as the kernel clamps them; None: all).
    Row by row, the header's formula: L = max(lse_a, max_j s_j), w = exp(lse_a - L), p_j = exp(s_j - L),
    out = (w out_a + sum p_j v_j) / (w + sum p_j), lse_out = L + ln(w + sum p_j); rows past n_valid: zeros, -inf; a NaN lse_a: NaN."""
    q, k_sink, v_sink, out_a, lse_a = (np.asarray(x, np.float64) for x in (q, k_sink, v_sink, out_a, lse_a))
    bs, nh, n, d = q.shape
    s_cap = k_sink.shape[2]
    G = nh // k_sink.shape[1]
    out, lse = np.zeros((bs, nh, n, d)), np.full((bs, nh, n), -np.inf)
    for b in range(bs):
        sb = s_cap if s_valid is None else clamp(s_valid[b], s_cap)
        nb = n if n_valid is None else clamp(n_valid[b], n)
        for h in range(nh):
            K, V = k_sink[b, h // G, :sb], v_sink[b, h // G, :sb]
            for i in range(nb):
                la = lse_a[b, h, i]
                if np.isnan(la):
                    out[b, h, i], lse[b, h, i] = np.nan, np.nan
                    continue
                s = K @ q[b, h, i] / np.sqrt(d)
                L = max(la, s.max()) if sb else la
                Ls = L if np.isfinite(L) else 0.0
                w = np.exp(la - Ls) if la > -np.inf else 0.0
                p = np.exp(s - Ls)
                den = w + p.sum()
                num = (w * out_a[b, h, i] if w > 0 else 0.0) + p @ V
                if den > 0:
                    out[b, h, i], lse[b, h, i] = num / den, Ls + np.log(den)
    return out, lse


class Request:
    """One request of one layer of a cache with sink_tokens = S: every K / V row it was given, in order ((nh_k, rows, d) fp16),
    and s, the sink rows it keeps - min(S, n) of a first store step of n rows, 0 when its first token came by a decode step.
    The cache holds T codes (of rows s .. s + T) and the rows from s + T on exactly (window, new rows)."""

    def __init__(self, S, nh_k, d):
        self.S, self.s = S, 0
        self.k, self.v = np.zeros((nh_k, 0, d), np.float16), np.zeros((nh_k, 0, d), np.float16)

    @property
    def seen(self):
        return self.k.shape[1]

    def store(self, k, v):
        """prefill / extend: n rows (nh_k, n, d).  The first store step of an empty request takes the sinks."""
        if self.seen == 0:
            self.s = min(self.S, k.shape[1])
        self.append(k, v)

    def append(self, k, v):
        """Decode steps / committed draft rows: never sinks."""
        self.k, self.v = np.concatenate([self.k, k], axis=1), np.concatenate([self.v, v], axis=1)

    def copy(self):
        c = Request(self.S, *self.k.shape[::2])
        c.s, c.k, c.v = self.s, self.k.copy(), self.v.copy()
        return c

    def keys(self, deq_k, deq_v, extra_k=None, extra_v=None):
        """K, V (nh_k, rows, d) fp64 as the attention sees them: deq_k / deq_v (nh_k, T, d) are the dequantised codes of the
        cache's T coded tokens (rows s .. s + T of the request); extra: rows not stored yet (a chunk, a draft)."""
        T = deq_k.shape[1]
        parts_k = [self.k[:, :self.s], deq_k, self.k[:, self.s + T:]] + ([] if extra_k is None else [extra_k])
        parts_v = [self.v[:, :self.s], deq_v, self.v[:, self.s + T:]] + ([] if extra_v is None else [extra_v])
        return (np.concatenate([np.asarray(p, np.float64) for p in parts_k], axis=1),
                np.concatenate([np.asarray(p, np.float64) for p in parts_v], axis=1))


def attend_rows(q, K, V, mask=None):
    """q (nh, n, d), K / V (nh_k, rows, d) fp64, mask (n, rows) bool (True: row i sees key j; None: all) -> out (nh, n, d),
    lse (nh, n): lse_ref.softmax_state per head."""
    nh, n, d = q.shape
    G = nh // K.shape[0]
    out, lse = np.zeros((nh, n, d)), np.zeros((nh, n))
    for h in range(nh):
        s = np.asarray(q[h], np.float64) @ K[h // G].T / np.sqrt(d)
        if mask is not None:
            s = np.where(mask, s, -np.inf)
        out[h], lse[h] = R.softmax_state(s, V[h // G])
    return out, lse


def causal_tail_mask(n, rows):
    """n new rows at the end of `rows` keys: row i sees everything before the block and the block's rows j <= i."""
    m = np.ones((n, rows), bool)
    m[:, rows - n:] = np.arange(n)[None, :] <= np.arange(n)[:, None]
    return m


def tree_tail_mask(parents, rows):
    """A draft tree at the end of `rows` keys: node i sees everything before the block, its ancestors and itself."""
    n = len(parents)
    m = np.ones((n, rows), bool)
    blk = np.zeros((n, n), bool)
    for i in range(n):
        j = i
        while j >= 0:
            blk[i, j] = True
            j = parents[j]
    m[:, rows - n:] = blk
    return m


def errors(got, want):
    """(rel-L2, mean-abs) of got against want over finite reference entries."""
    got, want = np.asarray(got, np.float64), np.asarray(want, np.float64)
    return float(np.linalg.norm(got - want) / max(np.linalg.norm(want), 1e-30)), float(np.abs(got - want).mean())
