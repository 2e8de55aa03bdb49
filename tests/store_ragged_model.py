"""A numpy statement of million_pq_store_ragged's per-request rule (include/million_hip.h): the clamps, the source order
(window rows in ring order, then the new rows), the destination tokens, the lengths advance.  No arithmetic: the codes are the
oracle's (oracle.pq_encode of the source rows in this order).  tests/test_store_ragged_host.py checks it against hand-written
expectations and the oracle's paging policy; tests/test_store_ragged_gpu.py compares the kernel with it."""
import numpy as np

# the common case table of the GPU tests: bs = 4, nh_k = 2, resid_cap = 64, n_bound = 70; rows (T, r, start, n)
CAP, N_BOUND, NH_K, CAP_TOK = 64, 70, 2, 256
CASES = [(70, 40, 50, 30),      # the ring wraps, T is not page-aligned, 70 source rows cross a 64-row block and several pages
         (32, 17, 3, 0),        # a non-participant holding a live window
         (0, 0, 0, 9),          # an empty slot
         (64, 64, 0, 70)]       # a full window and a full chunk
# untrusted rows: every clamp at once; the last rows past the page table; T past it altogether; a non-participant by clamping
UNTRUSTED = [(-5, 1000, 64, 1000), (250, 0, 0, 20), (10 ** 9, -3, -1, 5), (40, 10, 70, -4)]


def clamp(row, *, cap_tok, resid_cap, n_bound):
    """(T, r, start, n) as the kernels read it."""
    T, r, start, n = (int(x) for x in row)
    T = min(max(T, 0), cap_tok)
    r = min(max(r, 0), resid_cap)
    start = start if 0 <= start < resid_cap else 0
    n = min(max(n, 0), n_bound)
    return T, r, start, n


class Plan:
    """One request's part in a call.  live = False: it takes no part (nothing read, nothing written, its row stays).
    src: the source rows in order, ("win", ring row) or ("new", row); tokens[j]: the destination token of source row j;
    kept[j]: False where the token's page lies past the table and the store is dropped; T_after: word 0 after the advance."""

    def __init__(self, row, *, page_size, n_pages_cap, resid_cap, n_bound):
        cap_tok = page_size * n_pages_cap
        self.T, self.r, self.start, self.n = clamp(row, cap_tok=cap_tok, resid_cap=resid_cap, n_bound=n_bound)
        self.live = self.n > 0
        self.src, self.tokens, self.kept, self.T_after = [], np.zeros(0, np.int64), np.zeros(0, bool), None
        if not self.live:
            return
        self.src = [("win", (self.start + j) % resid_cap) for j in range(self.r)] + [("new", j) for j in range(self.n)]
        self.tokens = self.T + np.arange(self.r + self.n)
        self.kept = self.tokens // page_size < n_pages_cap
        self.T_after = min(self.T + self.r + self.n, cap_tok)

    def pages_written(self, page_size):
        return sorted({int(t) // page_size for t in self.tokens[self.kept]})

    def rows_of(self, win_b, new_b):
        """The source rows in model order: win_b (nh_k, resid_cap, d), new_b (nh_k, n_bound, d) -> (nh_k, r + n, d)."""
        return np.stack([(win_b if kind == "win" else new_b)[:, i] for kind, i in self.src], axis=1)


def plans(rows, **geom):
    return [Plan(row, **geom) for row in rows]


def advance(lengths, dev_n, **geom):
    """The (bs, 4) lengths array after the call: rows of live requests advanced, word 3 and the other rows untouched."""
    out = np.array(lengths, dtype=np.int32, copy=True)
    for b, row in enumerate(out):
        p = Plan((row[0], row[1], row[2], dev_n[b]), **geom)
        if p.live:
            out[b, :3] = (p.T_after, 0, 0)
    return out


def scatter(k_pool, v_pool, ids, b, plan, k_codes, v_codes):
    """Write request b's codes (nh_k, rows, M) into numpy pools (K (n_pool, page_size, M), V (n_pool, M, page_size)) in place."""
    ps = k_pool.shape[1]
    for j in np.nonzero(plan.kept)[0]:
        t = int(plan.tokens[j])
        for h in range(ids.shape[1]):
            pid = ids[b, h, t // ps]
            k_pool[pid, t % ps, :] = k_codes[h, j]
            v_pool[pid, :, t % ps] = v_codes[h, j]
