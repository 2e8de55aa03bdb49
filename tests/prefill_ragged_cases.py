"""Shapes, batches and inputs of the ragged prompt-attention tests (million_prefill_desc.dev_spans, csrc/prefill.hip).
Not collected: test_prefill_ragged_host.py and test_prefill_ragged_gpu.py import it.

The shapes are the smallest that cross every edge of the kernels: 64-key tiles, 32-key halves (the pipelined form), 32-row
waves and query blocks of 256 / hpw rows - bounds of 200 rows at G = nh / nh_k in {4, 8} (blocks of 64 / 32 rows) and of 300
rows at G in {1, 3} (blocks of 256 rows), two kv heads.  A request is (n_q, n_kv, q_pos0): the words 0 .. 2 of its device row."""
import functools

import numpy as np

from tests import flash_inputs as F

NH_K = 2
GROUPS = [(4, 200), (8, 200), (1, 300), (3, 300)]                      # (G, bound of n_q and n_kv)
GROUP_IDS = [f"G{g}-bound{n}" for g, n in GROUPS]
FORMS = [(128, 0), (128, 64), (64, 0)]                                 # (d, million_set_force_generic policy)
FORM_IDS = ["pipelined", "plain", "d64"]
FORM_NAME = dict(zip(FORMS, FORM_IDS))
# The families of the fp64 comparisons, and the one every bit-for-bit test draws its data from.  Rows of two or three keys
# have no averaging: the fp16 roundings of P and of the output alone come to 2^-11 = 4.9e-4 in the worst row, and the fp32
# models of both loops stay at or below half the bar on these two families (tests/test_prefill_ragged_host.py; the gaussian
# families with wider logits land at 5.2e-4 .. 5.6e-4 in single rows of the pipelined model and are not used).
FAMILIES = ["sink_local", "descending"]
BASE = "sink_local"

# name -> (causal, requests by bound)
BATCHES = {
    # full, one past a tile, a whole tile, one row, nothing
    "edges": (True, {200: [(200, 200, 0), (65, 65, 0), (64, 64, 0), (1, 1, 0), (0, 0, 0)],
                     300: [(300, 300, 0), (257, 257, 0), (256, 256, 0), (65, 65, 0), (1, 1, 0), (0, 0, 0)]}),
    # a chunk behind cached rows; a whole wave; one short of a tile; keys that end before the diagonals
    "offsets": (True, {200: [(33, 150, 117), (32, 200, 0), (63, 63, 0), (200, 31, 0)],
                       300: [(33, 250, 217), (256, 300, 0), (63, 63, 0), (290, 31, 0)]}),
    # every key: key counts one past a tile and one past a half tile, rows without any key
    "noncausal": (False, {200: [(200, 200, 0), (40, 129, 0), (1, 65, 0), (77, 33, 0), (50, 0, 0)],
                          300: [(300, 300, 0), (40, 129, 0), (257, 65, 0), (77, 33, 0), (50, 0, 0)]}),
    # the poison test's: key counts one past a tile edge (65) and one past a half-tile edge (33), rows without any key
    "poison": (True, {200: [(200, 200, 0), (65, 65, 0), (33, 33, 0), (120, 97, 40), (0, 0, 0), (50, 0, 0)],
                      300: [(300, 300, 0), (65, 65, 0), (33, 33, 0), (270, 97, 40), (0, 0, 0), (50, 0, 0)]}),
}


def requests(batch, bound):
    """-> (causal, [(n_q, n_kv, q_pos0)])"""
    causal, by_bound = BATCHES[batch]
    return causal, by_bound[bound]


def spans(reqs, word3=0):
    """The device rows of a batch: int32 (bs, 4)."""
    return np.array([[a, b, c, word3] for a, b, c in reqs], dtype=np.int32)


@functools.lru_cache(maxsize=None)
def inputs(name, bs, G, bound, d):
    """fp16 q (bs, G * NH_K, bound, d), k, v (bs, NH_K, bound, d) of family `name`: request b owns the first n_q_b rows of q[b]
    and the first n_kv_b rows of k[b], v[b].  Shared, read-only."""
    q, k, v = F.prefill_inputs(name, bs, G * NH_K, NH_K, bound, bound, d)
    for a in (q, k, v):
        a.setflags(write=False)
    return q, k, v


def live(req):
    """Does the request produce output rows that are not zeros?"""
    return req[0] > 0 and req[1] > 0


def request_inputs(q, k, v, b, req):
    n_q, n_kv, _ = req
    return q[b:b + 1, :, :n_q], k[b:b + 1, :, :n_kv], v[b:b + 1, :, :n_kv]


@functools.lru_cache(maxsize=None)
def gold(name, batch, G, bound, d):
    """fp64 per request: a list with one (1, nh, n_q_b, d) array per request (None for a request without live rows)."""
    causal, reqs = requests(batch, bound)
    q, k, v = inputs(name, len(reqs), G, bound, d)
    return [F.prefill_gold(*request_inputs(q, k, v, b, r), r[2], causal) if live(r) else None for b, r in enumerate(reqs)]
