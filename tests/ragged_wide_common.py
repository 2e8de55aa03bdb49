"""What the tests of the wide one-launch flush and ragged store share (tests/test_flush_wide_gpu.py, test_ragged_wide_gpu.py,
test_flush_wide_host.py, test_ragged_wide_host.py): the geometry, the three code formats, a numpy statement of
million_pq_flush_wide's per-request rule (the ragged store's is tests/store_ragged_model.py), and numpy page pools that take
codes the way the kernels store them - uint16 pages, or packed pages through tests/packed_model.py.  No arithmetic: codes are
oracle.pq_encode's."""
import numpy as np

from tests import packed_model as P

BS, NH, NHK, LAYERS, PS, CAP, MAX_TOKENS = 3, 8, 2, 2, 32, 64, 512
NPC = MAX_TOKENS // PS
CAP_TOK = NPC * PS
FORMATS = [(128, 64, 10), (128, 32, 12), (64, 32, 9)]      # (d, M, nbits): d_m 2 / 4, hb 2 / 4
FILL = 0xA5
INT_MAX = 2 ** 31 - 1


def clamp_row(row):
    """(T, r, start) as load_len_row reads it."""
    T, r, st = (int(x) for x in row[:3])
    return min(max(T, 0), CAP_TOK), min(max(r, 0), CAP), st if 0 <= st < CAP else 0


class FlushPlan:
    """One request's part in a flush of n rows with device lengths: live = False, it takes no part.  ring: the window rows read,
    in order; tokens: their destination tokens; kept: False where the token lies past the table; after: words 0 .. 2 afterwards."""

    def __init__(self, row, n, min_r):
        self.T, self.r, self.start = clamp_row(row)
        self.live = self.r >= min_r
        self.ring = (self.start + np.arange(n)) % CAP
        self.tokens = self.T + np.arange(n)
        self.kept = self.tokens < CAP_TOK
        self.after = (min(self.T + n, CAP_TOK), max(self.r - n, 0), (self.start + n) % CAP) if self.live else tuple(int(x) for x in row[:3])


def fill_pools(n_pool, M, C, packed):
    """numpy K and V pools holding 0xA5 in every byte."""
    if packed:
        return [np.full((n_pool, P.page_bytes(PS, M, C)), FILL, np.uint8) for _ in range(2)]
    return np.full((n_pool, PS, M), FILL * 0x101, np.uint16), np.full((n_pool, M, PS), FILL * 0x101, np.uint16)


def put(pools, ids_b, tokens, kept, k_codes, v_codes, M, C, packed):
    """Codes (nh_k, rows, M) of one request at `tokens` (kept ones only) into numpy pools in place, through its page ids (nh_k, NPC)."""
    for j in np.nonzero(kept)[0]:
        t = int(tokens[j])
        for h in range(ids_b.shape[0]):
            pid = ids_b[h, t // PS]
            if packed:
                P.put_tokens(pools[0][pid], "k", [t % PS], k_codes[h, j][None], PS, M, C)
                P.put_tokens(pools[1][pid], "v", [t % PS], v_codes[h, j][None], PS, M, C)
            else:
                pools[0][pid, t % PS, :] = k_codes[h, j]
                pools[1][pid, :, t % PS] = v_codes[h, j]


def codes_of(pools, ids_b, t0, t1, M, C, packed):
    """The codes (nh_k, t1 - t0, M) uint16 a request reaches through its page ids at tokens [t0, t1): K and V."""
    kp, vp = (P.unpack(pools[0], "k", PS, M, C), P.unpack(pools[1], "v", PS, M, C)) if packed else pools
    tok = np.arange(t0, t1)
    k = np.stack([kp[ids_b[h, tok // PS], tok % PS] for h in range(ids_b.shape[0])])
    v = np.stack([vp[ids_b[h, tok // PS], :, tok % PS] for h in range(ids_b.shape[0])])
    return k, v


def to_dev(torch, a):
    """numpy -> cuda, uint16 included."""
    a = np.ascontiguousarray(a)
    if a.dtype == np.uint16:
        return torch.from_numpy(a.view(np.int16)).cuda().view(torch.uint16)
    return torch.from_numpy(a).cuda()


def to_np(torch, t):
    """cuda -> numpy, uint16 included."""
    if t.dtype == torch.uint16:
        return t.view(torch.int16).cpu().numpy().view(np.uint16)
    return t.cpu().numpy()
