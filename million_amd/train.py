"""PQ codebook training on the GPU: the first step of samples -> train -> .pq.pt -> encode -> attend.

Drop-in for the reference's `train_pq(X, M, nbits, niter=25)` (scripts/utils/pq_utils.py:586-609), which wraps faiss-cpu's
`IndexPQ.train`: one independent Lloyd k-means per subspace.  All arithmetic runs in libmillion_hip.so
(`million_pq_train`, contract in include/million_hip.h); the host only subsamples, draws the initial rows and holds memory.
Parity with faiss is not pinned: faiss is not installed where this project runs, and its empty-cluster split draws the
donor at random (here: the largest cluster, lowest index on ties).  `train_opq` is out of scope.
"""
from __future__ import annotations

import ctypes
from typing import Optional

import numpy as np
import torch

from . import _lib as L
from .ops import _need_cuda, _ptr, _stream

TRAIN_CHUNK = 4096      # kTrainChunk of csrc/train.hip
SPLIT_EPS = 1.0 / 1024.0


def _desc(n: int, d: int, M: int, C: int, niter: int, x_is_f32: bool, x_stride_n: int, eps: float = SPLIT_EPS) -> L.TrainDesc:
    desc = L.TrainDesc()
    desc.struct_size = ctypes.sizeof(L.TrainDesc)
    desc.n, desc.d, desc.M, desc.C, desc.niter = n, d, M, C, niter
    desc.x_is_f32, desc.x_stride_n, desc.eps = int(x_is_f32), x_stride_n, eps
    return desc


def workspace_bytes(n: int, d: int, M: int, C: int) -> int:
    """The formula of million_pq_train_workspace_bytes (tests/test_train_host.py holds the two together): the transposed
    codes (M, n), the chunk partials (S, M, C, d_m + 1) and one fp64 objective partial per assign workgroup, each rounded
    up to 256 bytes."""
    up = lambda v: (v + 255) // 256 * 256
    dm = d // M
    S = (n + TRAIN_CHUNK - 1) // TRAIN_CHUNK
    n_obj = ((n + 63) // 64) * (((M + 3) // 4 + 3) // 4)
    return up(M * n * (1 if C <= 256 else 2)) + up(S * M * C * (dm + 1) * 4) + up(n_obj * 8)


def kmeans_pq(X: torch.Tensor, M: int, C: int, niter: int, *, init_rows: Optional[torch.Tensor] = None,
              cents_init: Optional[torch.Tensor] = None, workspace: Optional[torch.Tensor] = None,
              out: Optional[torch.Tensor] = None, counts: Optional[torch.Tensor] = None,
              objective: Optional[torch.Tensor] = None, eps: float = SPLIT_EPS):
    """million_pq_train on device tensors.  X (n, d) fp32 or fp16 with contiguous rows; exactly one of init_rows (C int32)
    and cents_init ((M, C, d_m) fp32).  Returns (cents (M, C, d_m) fp32, counts (M, C) int32, objective (niter,) fp64), all
    on X's device; nothing is synchronised.  workspace / out / counts / objective: preallocated buffers (a captured graph
    must pass them all: nothing is allocated then)."""
    _need_cuda(X, init_rows, cents_init, workspace, out, counts, objective)
    if X.dim() != 2 or X.stride(1) != 1 or X.dtype not in (torch.float32, torch.float16):
        raise RuntimeError("train: X must be (n, d) fp32 or fp16 with contiguous rows")
    n, d = X.shape
    if M <= 0 or d % M:
        raise RuntimeError(f"train: d={d} is not a multiple of M={M}")
    dm = d // M
    if init_rows is not None and (init_rows.dtype != torch.int32 or not init_rows.is_contiguous() or init_rows.numel() != C):
        raise RuntimeError("train: init_rows must be C contiguous int32 row indices")
    if cents_init is not None and (cents_init.dtype != torch.float32 or not cents_init.is_contiguous()
                                   or tuple(cents_init.shape) != (M, C, dm)):
        raise RuntimeError("train: cents_init must be a contiguous fp32 (M, C, d_m) table")
    lib = L.load()
    desc = _desc(n, d, M, C, niter, X.dtype == torch.float32, X.stride(0), eps)
    need = lib.million_pq_train_workspace_bytes(ctypes.byref(desc))
    dev = X.device
    if workspace is None and need:
        workspace = torch.empty(need, dtype=torch.uint8, device=dev)
    if out is None:
        out = torch.empty(M, C, dm, dtype=torch.float32, device=dev)
    if counts is None:
        counts = torch.empty(M, C, dtype=torch.int32, device=dev)
    if objective is None:
        objective = torch.empty(max(niter, 0), dtype=torch.float64, device=dev)
    for t, shape, dt in ((out, (M, C, dm), torch.float32), (counts, (M, C), torch.int32), (objective, (niter,), torch.float64)):
        if tuple(t.shape) != shape or t.dtype != dt or not t.is_contiguous():
            raise RuntimeError(f"train: output buffer must be contiguous {dt} {shape}")
    L.check(lib.million_pq_train(ctypes.byref(desc), X.data_ptr(), _ptr(init_rows), _ptr(cents_init), out.data_ptr(),
                                 counts.data_ptr(), objective.data_ptr(), _ptr(workspace),
                                 0 if workspace is None else workspace.numel() * workspace.element_size(), _stream()),
            "million_pq_train")
    return out, counts, objective


def train_pq(X, M: int, nbits: int, niter: int = 25, *, seed: int = 1234, max_points_per_centroid: int = 256,
             return_stats: bool = False):
    """Drop-in for the reference's train_pq: X (n, d) -> fp32 (M, 2**nbits, d // M) codebook.

    X is what the reference takes - an (n, d) numpy array (`read_fvecs` output), trained on the current device and returned
    as a CPU tensor like there - or a device tensor (fp32 / fp16), whose codebook stays on its device.  A CPU torch tensor
    is refused: there is no CPU path.  More than max_points_per_centroid * 2**nbits points are subsampled on the host the
    way faiss does (a seeded permutation, its first rows); the C initial rows come from the same seeded CPU generator.
    return_stats: also a dict with the per-iteration objective (list of float) and the final counts (M, C)."""
    from_numpy = isinstance(X, np.ndarray)
    if from_numpy:
        if not torch.cuda.is_available():
            raise RuntimeError("train_pq needs a GPU (no CPU fallback)")
        X = torch.from_numpy(np.ascontiguousarray(X, dtype=np.float32)).cuda()
    if not isinstance(X, torch.Tensor):
        raise RuntimeError("train_pq: X must be an (n, d) numpy array or a device tensor")
    _need_cuda(X)
    if X.dim() != 2:
        raise RuntimeError(f"train_pq: X must be (n, d), got {tuple(X.shape)}")
    n, d = X.shape
    assert d > M and d % M == 0, "d must be divisible by M"      # the reference's own check (pq_utils.py:598)
    C = 2 ** nbits
    if n < C:
        raise RuntimeError(f"train_pq: {n} points cannot seed {C} centroids")
    if X.dtype not in (torch.float32, torch.float16):
        X = X.float()
    gen = torch.Generator(device="cpu")
    gen.manual_seed(seed)
    if n > max_points_per_centroid * C:
        keep = torch.randperm(n, generator=gen)[: max_points_per_centroid * C]
        X = X[keep.to(X.device)]
        n = X.shape[0]
    X = X.contiguous()
    init_rows = torch.randperm(n, generator=gen)[:C].to(torch.int32).to(X.device)
    cents, counts, objective = kmeans_pq(X, M, C, niter, init_rows=init_rows)
    if from_numpy:
        cents = cents.cpu()
    if return_stats:
        return cents, {"objective": objective.cpu().tolist(), "counts": counts.cpu(), "n_train": n}
    return cents
