"""Numpy models of draft verification over a tree (include/million_hip.h, "Draft verification": million_attn_tree_merge,
million_window_commit_rows): the ancestor masks, the block merge with the visibility set taken from a mask word, the commit of
chosen rows, and the trees the tests run on.  Shared by test_verify_tree_host.py and test_verify_tree_gpu.py; the chain's models
are verify_model's."""
from __future__ import annotations

import numpy as np

from tests import verify_model as VM


def ancestor_masks(parents):
    """int32 (n,): bit j of word i is set when j is i or an ancestor of i.  Written apart from million_amd.spec_tree: by walking
    up from every node."""
    masks = np.zeros(len(parents), np.int32)
    for i in range(len(parents)):
        j = i
        while j >= 0:
            masks[i] |= 1 << j
            j = int(parents[j])
    return masks


def sanitise(mask, i):
    """What the kernel makes of word `mask` of row i: bits 0 .. i kept, bit i set - (mask & ((2 << i) - 1)) | (1 << i)."""
    return ((int(mask) & 0xFFFFFFFF) & ((2 << i) - 1)) | (1 << i)


def chain_of(parents, node):
    chain = []
    while node >= 0:
        chain.append(int(node))
        node = int(parents[node])
    return chain[::-1]


def tree_block_merge(q, k, v, out_a, lse_a, masks, n_valid=None):
    """verify_model.block_merge with row i of request b seeing the block keys j whose bit is set in sanitise(masks[b, i], i),
    in ascending order of j.  masks (bs, n) integers.  Rows at or past n_valid[b]: out = 0, lse = -inf."""
    bs, nh, n, d = q.shape
    G = nh // k.shape[1]
    out, lse = np.zeros((bs, nh, n, d)), np.full((bs, nh, n), -np.inf)
    for b in range(bs):
        nb = n if n_valid is None else max(0, min(n, int(n_valid[b])))
        for i in range(nb):
            m = sanitise(masks[b][i], i)
            see = [j for j in range(nb) if (m >> j) & 1]
            for h in range(nh):
                K, V = k[b, h // G][see].astype(np.float64), v[b, h // G][see].astype(np.float64)
                la = float(lse_a[b, h, i])
                if np.isnan(la):
                    out[b, h, i], lse[b, h, i] = np.nan, np.nan
                    continue
                s = q[b, h, i].astype(np.float64) @ K.T / np.sqrt(d)
                L = max(la, s.max())
                w = np.exp(la - L) if np.isfinite(la) else 0.0
                p = np.exp(s - L)
                den = w + p.sum()
                past = w * out_a[b, h, i].astype(np.float64) if w > 0 else 0.0
                out[b, h, i] = (past + p @ V) / den
                lse[b, h, i] = L + np.log(den)
    return out, lse


def clamp_row(x, n_bound):
    return max(0, min(n_bound - 1, int(x)))


def commit_rows(T, r, start, a, ps, cap, rows, n_bound, ring=None):
    """million_window_commit_rows of one (layer, request): verify_model.commit_sequential - a single decode steps - over the
    gathered rows ("n", clamp(rows[i])) for i < a.  (T', r', start', coded, ring') as verify_model's."""
    picked = [("n", clamp_row(rows[i], n_bound)) for i in range(a)]
    return VM.commit_sequential(T, r, start, a, ps, cap, ring=ring, rows=picked)


# ---------------------------------------------------------------- trees ---------------------------------------------------------
def random_tree(seed, n):
    """n parents in topological order; seed % 4 picks the family: 0 a chain, 1 a star (every node a root), 2 uniform random
    parents in [-1, i), 3 a deep spine with a bush under node 0 whose last node is a leaf under node 0."""
    rs = np.random.RandomState(seed)
    kind = seed % 4
    if kind == 0:
        return [i - 1 for i in range(n)]
    if kind == 1:
        return [-1] * n
    if kind == 2:
        return [int(rs.randint(-1, i)) for i in range(n)]
    ps = [-1]
    for i in range(1, n):
        ps.append(0 if (i == n - 1 or i % 3 == 0) else i - 1 if (i - 1) % 3 else max(0, i - 2))
    return ps


TREE_SIZES = (1, 2, 5, 16)
TREE_SEEDS = tuple(range(8))


def tree_set():
    """[(seed, n, parents)]: every family at every size."""
    return [(seed, n, random_tree(seed, n)) for n in TREE_SIZES for seed in TREE_SEEDS]


def depth(parents, i):
    return len(chain_of(parents, i))


def children(parents, i):
    return [j for j, p in enumerate(parents) if p == i]


def binary_tree(n):
    """Node i hangs under (i - 1) // 2: a heap-shaped binary tree."""
    return [(i - 1) // 2 if i else -1 for i in range(n)]


def random_path(rs, parents, n_live):
    """A random valid path of the tree below n_live, the empty path included: walk from a random root through random children,
    stopping at a random depth."""
    path, level = [], [i for i in range(n_live) if parents[i] == -1]
    while level and rs.randint(0, 4):
        node = int(level[rs.randint(len(level))])
        path.append(node)
        level = [j for j in children(parents, node) if j < n_live]
    return path
