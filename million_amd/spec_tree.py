"""Host helpers for draft trees (PagedPQCache.verify(tree=) / commit(path=)): pure numpy.

A tree of n <= 16 nodes is a sequence of parent indices in topological order: parents[i] in [-1, i), -1 marks a root, several
roots are allowed.  Node i sits at row i of the verified block."""
from __future__ import annotations

import numpy as np

MAX_NODES = 16


def check_parents(parents, n=None):
    """The parents as a list of ints, or ValueError: n entries (when given), at most 16, each in [-1, i)."""
    ps = [int(x) for x in parents]
    if n is not None and len(ps) != n:
        raise ValueError(f"a tree of {n} nodes takes {n} parents, got {len(ps)}")
    if len(ps) > MAX_NODES:
        raise ValueError(f"a tree of {len(ps)} nodes (at most {MAX_NODES})")
    for i, p in enumerate(ps):
        if not -1 <= p < i:
            raise ValueError(f"parents[{i}] = {p}: a parent precedes its child (-1 .. {i - 1})")
    return ps


def ancestor_masks(parents) -> np.ndarray:
    """int32 (n,): bit j of word i is set when node j is node i or one of its ancestors - the rows that row i of the block sees
    (ops.attn_block_merge(dev_mask=)).  A chain gives (2 << i) - 1, a forest of single nodes 1 << i."""
    ps = check_parents(parents)
    masks = np.zeros(len(ps), np.int32)
    for i, p in enumerate(ps):
        masks[i] = (1 << i) | (int(masks[p]) if p >= 0 else 0)
    return masks


def chain_of(parents, node):
    """The root-to-node path of `node`, the node included."""
    chain = []
    while node >= 0:
        chain.append(int(node))
        node = int(parents[node])
    return chain[::-1]


def is_path(parents, path, n_live=None) -> bool:
    """Whether `path` is empty or a chain of the tree from a root: parents[path[0]] == -1, parents[path[k]] == path[k - 1], and
    every node below n_live (default: the tree's size)."""
    n_live = len(parents) if n_live is None else n_live
    prev = -1
    for node in path:
        if not 0 <= node < n_live or int(parents[node]) != prev:
            return False
        prev = node
    return True


def greedy_path(parents, draft_ids, target_ids, n_live, prev_target):
    """The longest chain of the tree that greedy acceptance keeps, as a list of node indices: a node is accepted when its parent
    is (a root always has an accepted parent: the sequence so far) and its draft token equals the target model's token at its
    parent - target_ids[parent], or prev_target, the token the previous step's target produced, for a root.  Only nodes below
    n_live take part.  Among chains of equal length the one whose last node has the lowest index wins."""
    ps = check_parents(parents)
    n_live = max(0, min(int(n_live), len(ps)))
    depth = [0] * n_live      # accepted nodes on the chain to node i, 0: not accepted
    best = -1
    for i in range(n_live):
        p = ps[i]
        if p >= 0 and not depth[p]:
            continue
        if int(draft_ids[i]) != (int(target_ids[p]) if p >= 0 else int(prev_target)):
            continue
        depth[i] = (depth[p] if p >= 0 else 0) + 1
        if best < 0 or depth[i] > depth[best]:
            best = i
    return chain_of(ps, best) if best >= 0 else []
