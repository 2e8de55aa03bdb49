"""numpy fp32 restatement of the PQ-training contract of include/million_hip.h ("PQ codebook training").  Test code only.

Assign goes through oracle.pq_encode (the bit-exact definition of the encoder); the chunked sums go through np.add.at on
float32 arrays, which applies its updates one by one in index order (an unbuffered sequential fp32 sum); the split rule is a
plain Python loop.  tests/test_train_gpu.py compares million_pq_train with this bit for bit."""
import numpy as np

from oracle import oracle as O

TRAIN_CHUNK = 4096
SPLIT_EPS = 1.0 / 1024.0


def init_from_rows(X, M, rows):
    """Centroid c of every subspace = the sub-vector of row rows[c]."""
    X = np.asarray(X, dtype=np.float32)
    n, d = X.shape
    dm = d // M
    return np.ascontiguousarray(X[np.asarray(rows)].reshape(len(rows), M, dm).transpose(1, 0, 2))


def assign(X, cents):
    """codes (n, M) and the fp32 minimum distances (n, M): e = x - c, sq = e * e, sequential fp32 sum over k."""
    X = np.ascontiguousarray(X, dtype=np.float32)
    cents = np.ascontiguousarray(cents, dtype=np.float32)
    n, d = X.shape
    M, C, dm = cents.shape
    codes = O.pq_encode(X[None, None], cents)[0, 0].astype(np.int64)
    picked = cents[np.arange(M)[None, :], codes]                     # (n, M, dm)
    e = X.reshape(n, M, dm) - picked
    sq = e * e
    dist = sq[..., 0].copy()
    for k in range(1, dm):
        dist = dist + sq[..., k]
    return codes, dist


def update(X, codes, C):
    """Chunked sums and counts: (sums (M, C, dm) fp32, counts (M, C) int32)."""
    X = np.ascontiguousarray(X, dtype=np.float32)
    n, d = X.shape
    M = codes.shape[1]
    dm = d // M
    Xs = X.reshape(n, M, dm)
    total = None
    counts = np.zeros((M, C), dtype=np.int32)
    for r0 in range(0, n, TRAIN_CHUNK):
        r1 = min(r0 + TRAIN_CHUNK, n)
        part = np.zeros((M, C, dm), dtype=np.float32)
        for m in range(M):
            np.add.at(part[m], codes[r0:r1, m], Xs[r0:r1, m])         # in row order, one fp32 add each, from +0.0
            counts[m] += np.bincount(codes[r0:r1, m], minlength=C).astype(np.int32)
        total = part if total is None else total + part               # chunk sums in chunk order
    return total, counts


def divide(sums, counts, prev):
    """centroid = sum / (float)count; an empty cluster keeps `prev` here and is overwritten by split()."""
    cents = np.array(prev, dtype=np.float32, copy=True)
    nz = counts > 0
    cents[nz] = sums[nz] / counts[nz].astype(np.float32)[:, None]
    return cents


def split(cents, counts, eps=SPLIT_EPS):
    """faiss's empty-cluster split, deterministic: ascending c, donor = largest count (lowest index), in place."""
    hi = np.float32(1.0) + np.float32(eps)
    lo = np.float32(1.0) - np.float32(eps)
    M, C, dm = cents.shape
    n_split = 0
    for m in range(M):
        for c in range(C):
            if counts[m, c] != 0:
                continue
            donor = int(np.argmax(counts[m]))                          # first maximum: the lowest index
            v = cents[m, donor].copy()
            for k in range(dm):
                a, b = (hi, lo) if k % 2 == 0 else (lo, hi)
                cents[m, c, k] = v[k] * a
                cents[m, donor, k] = v[k] * b
            counts[m, c] = counts[m, donor] // 2
            counts[m, donor] -= counts[m, c]
            n_split += 1
    return n_split


def lloyd(X, cents0, niter, eps=SPLIT_EPS):
    """niter rounds of assign -> update -> split from the (M, C, dm) table cents0.
    Returns (cents fp32, counts int32, objectives list of float: fp64 sums of the fp32 minimum distances)."""
    cents = np.array(cents0, dtype=np.float32, copy=True)
    C = cents.shape[1]
    objs, counts = [], None
    for _ in range(niter):
        codes, dist = assign(X, cents)
        objs.append(float(dist.astype(np.float64).sum()))
        sums, counts = update(X, codes, C)
        cents = divide(sums, counts, cents)
        split(cents, counts, eps)
    return cents, counts, objs
