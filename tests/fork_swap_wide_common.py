"""What the tests of fork and swap over wide code pages share (tests/test_fork_swap_wide_host.py, test_swap_wide_gpu.py,
test_fork_wide_gpu.py): the geometry of tests/ragged_wide_common.py with short page-table rows, the formats, and cache arrays that
hold the same codes - oracle.pq_encode of random rows - in a uint16 pool and in a packed pool behind one scattered table; and, for the
cache-level GPU tests, seeded request rows, caches over them and decode steps through million_amd.paged_turns."""
import numpy as np

from tests import cache_swap_model as SM
from tests import cache_swap_wide_model as WM
from tests import packed_model as P
from tests import ragged_wide_common as R

LAYERS, BS, NHK, NH, CAP, NPC = R.LAYERS, R.BS, R.NHK, R.NH, R.CAP, 4
FORMATS = R.FORMATS + [(64, 16, 10)]      # (d, M, nbits); (64, 16, 10): a token's row of the K high plane is 4 bytes
NAMES = ("page_ids", "k_pool", "v_pool", "k_resid", "v_resid", "lengths")
to_dev, to_np = R.to_dev, R.to_np


def tables(seed, d, M, C, ps, oracle, garbage=True, extra=7):
    """{"u16": [ids, k_pool, v_pool, k_res, v_res, lengths], "packed": the same over packed pools}.  garbage: the uint16 words carry
    bits above log2 C, and at C = 512 / 2048 both pools carry the field's top bit: no reader sees either."""
    rs = np.random.RandomState(seed)
    n_tab = LAYERS * BS * NHK * NPC
    n_pool = n_tab + extra
    ids = rs.permutation(n_pool)[:n_tab].reshape(LAYERS, BS, NHK, NPC).astype(np.int32)
    cents = rs.standard_normal((M, C, d // M)).astype(np.float16)
    rows = rs.standard_normal((1, 2, n_pool * ps, d)).astype(np.float16)
    codes = oracle.pq_encode(rows, cents)[0].astype(np.uint16)      # (2, n_pool * ps, M)
    assert (codes >= 256).any() and codes.max() < C
    k16 = codes[0].reshape(n_pool, ps, M).copy()
    v16 = codes[1].reshape(n_pool, ps, M).transpose(0, 2, 1).copy()
    if garbage and C < (1 << (8 + P.hi_bits(C))):
        for a in (k16, v16):
            a |= (rs.randint(0, 2, a.shape) * C).astype(np.uint16)
    kp, vp = P.pack(k16, "k", C), P.pack(v16, "v", C)
    if garbage:
        for a in (k16, v16):
            a |= (rs.randint(0, 16, a.shape) << 12).astype(np.uint16)
    kr = rs.standard_normal((LAYERS, BS, NHK, CAP, d)).astype(np.float16).view(np.int16)
    vr = rs.standard_normal((LAYERS, BS, NHK, CAP, d)).astype(np.float16).view(np.int16)
    ln = rs.randint(1, 200, (LAYERS, BS, 4)).astype(np.int32)
    return dict(u16=[ids, k16, v16, kr, vr, ln], packed=[ids.copy(), kp, vp, kr.copy(), vr.copy(), ln.copy()])


def layout(table, ps, M, d, C, layers=LAYERS, bound=NPC):
    """Offsets of the entries' blobs one behind the other, sized by the clamped values; the total."""
    sizes = [layers * NHK * WM.row_bytes(*SM.clamp_entry(e, page_size=ps, n_pages_bound=bound, resid_cap=CAP)[1:3], ps, M, d, C) for e in table]
    offs = np.concatenate([[0], np.cumsum(sizes)]).astype(np.int64)
    return offs[:-1].copy(), int(offs[-1])


# ---------------------------------------------------------------- the cache, through paged_turns (GPU tests) ---------------
PS, N_PROMPT, FIRST, STEPS = 32, 69, 30, 40      # 69 coded tokens; the window (64 rows) is flushed in front of decode step 65: FIRST + 35


class World:
    """Rows of two requests, seeded standard-normal fp16, per format."""
    _memo = {}

    def __new__(cls, d, M, nbits):
        key = (d, M, nbits)
        if key not in cls._memo:
            self = object.__new__(cls)
            rs = np.random.RandomState(500 + nbits)
            h = lambda *s: rs.standard_normal(s).astype(np.float16)
            self.d, self.M, self.nbits, self.C = d, M, nbits, 2 ** nbits
            self.ck, self.cv = h(M, self.C, d // M), h(M, self.C, d // M)
            self.K, self.V, self.Q = (h(LAYERS, 1, n, N_PROMPT + 2 * CAP + 8, d) for n in (NHK, NHK, NH))
            cls._memo[key] = self
        return cls._memo[key]


def new_cache(torch, w, packed, preallocate):
    from million_amd.pq_cache import PagedPQCache
    c = PagedPQCache(bs=BS, nh=NH, num_key_value_heads=NHK, M=w.M, layer_num=LAYERS, d=w.d, page_size=PS, extended_residual_size=CAP,
                     max_tokens=512, nbits=w.nbits, dtype=torch.uint16, packed=packed, preallocate=preallocate, device="cuda")
    c.set_cent(to_dev(torch, w.ck), to_dev(torch, w.cv))
    return c


def prefill(torch, cache, w, b, n=N_PROMPT):
    for l in range(LAYERS):
        cache.prefill_request(b, *(to_dev(torch, A[l][:, :, :n]) for A in (w.Q, w.K, w.V)), l)


def decode(torch, cache, w, pos, steps):
    """`steps` decode steps through paged_turns.decode with device lengths; slot b is fed the rows at pos[b] + step (None: the
    slot idles on row 0, its output is not kept, and it is released afterwards if it was empty before).  Returns {b: [per step, per layer int16 bits]}."""
    from million_amd import paged_turns
    outs = {b: [] for b, p in enumerate(pos) if p is not None}
    empty = [b for b, p in enumerate(pos) if p is None and not cache._T_a[:, b].any() and not cache._r_a[:, b].any()]
    for s in range(steps):
        for l in range(LAYERS):
            pick = lambda A: torch.cat([to_dev(torch, A[l][:, :, (0 if p is None else p + s)][:, :, None]) for p in pos])
            o = paged_turns.decode(cache, pick(w.Q), pick(w.K), pick(w.V), l, use_dev_lengths=True)
            for b in outs:
                outs[b].append(o[b].view(torch.int16).cpu().numpy().copy())
    torch.cuda.synchronize()
    for b in empty:      # an idle slot that was empty is empty again
        cache.release(b)
    return outs


def same_bits(a, b):
    return len(a) == len(b) and all(np.array_equal(x, y) for x, y in zip(a, b))
