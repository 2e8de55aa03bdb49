#!/usr/bin/env python3
"""Timing of PQ codebook training at the headline shape: N = 65536, d = 128, M = 64, C = 256, niter = 25.

  python tools/train_bench.py [--out profiles/train_pq.txt] [--host-iters 2] [--reps 5]

Prints (and writes to --out):
  * the whole million_pq_train call (HIP events, median of --reps) and the time per iteration;
  * the three kernels of an iteration (torch.profiler device times, mean over the call's launches), and the assign kernel's
    share of the vector-ALU roofline it is bound by (csrc/train.hip: 6 vector instructions per centroid test at d_m = 2,
    one 64-lane instruction per 4 cycles per SIMD, CUs x 4 SIMDs at the device's clock);
  * the same iterations as dense torch ops on the host (assign: ((x - c) ** 2).sum(-1).argmin in chunks; update: index_add_
    and bincount), at most 16 threads.  faiss, which the reference trains with, is not installed where this project runs:
    this is the only baseline at hand.  The host leg runs --host-iters iterations (every iteration costs the same) and is
    scaled to niter."""
import argparse
import sys
import time
from pathlib import Path

import torch

sys.path.insert(0, str(Path(__file__).resolve().parents[1]))
from million_amd import train  # noqa: E402

N, D, M, C, NITER = 65536, 128, 64, 256, 25


def mixture(n, d, gen, n_modes=64, spread=0.35):
    modes = torch.randn(n_modes, d, generator=gen) * 2.0
    return modes[torch.randint(0, n_modes, (n,), generator=gen)] + spread * torch.randn(n, d, generator=gen)


def host_iteration(X, cents):
    """One Lloyd iteration as dense torch ops on the host (no empty-cluster split: timing only)."""
    n, d = X.shape
    m, c, dm = cents.shape
    Xs = X.reshape(n, m, 1, dm)
    codes = torch.empty(n, m, dtype=torch.long)
    step = max(1, (1 << 24) // (m * c * dm))      # ~64 MB of differences per chunk
    for i0 in range(0, n, step):
        e = Xs[i0:i0 + step] - cents[None]
        codes[i0:i0 + step] = (e * e).sum(-1).argmin(-1)
    new = torch.zeros_like(cents)
    for j in range(m):
        sums = torch.zeros(c, dm).index_add_(0, codes[:, j], X[:, j * dm:(j + 1) * dm])
        cnt = torch.bincount(codes[:, j], minlength=c).clamp_(min=1).float()
        new[j] = sums / cnt[:, None]
    return new


def main(argv=None) -> int:
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--host-iters", type=int, default=2)
    ap.add_argument("--reps", type=int, default=5)
    args = ap.parse_args(argv)
    lines = []

    def say(s):
        print(s, flush=True)
        lines.append(s)

    dev = torch.device("cuda", 0)
    gen = torch.Generator().manual_seed(0)
    X = mixture(N, D, gen)
    rows = torch.randperm(N, generator=gen)[:C].to(torch.int32)
    Xd, rows_d = X.to(dev), rows.to(dev)
    ws = torch.empty(train.workspace_bytes(N, D, M, C), dtype=torch.uint8, device=dev)
    out = torch.empty(M, C, D // M, device=dev)
    counts = torch.empty(M, C, dtype=torch.int32, device=dev)
    obj = torch.empty(NITER, dtype=torch.float64, device=dev)

    def run():
        train.kmeans_pq(Xd, M, C, NITER, init_rows=rows_d, workspace=ws, out=out, counts=counts, objective=obj)

    run()
    torch.cuda.synchronize()
    ts = []
    for _ in range(args.reps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        run()
        b.record()
        torch.cuda.synchronize()
        ts.append(a.elapsed_time(b))
    ts.sort()
    gpu_ms = ts[len(ts) // 2]
    o = obj.cpu().tolist()
    say(f"== python3 tools/train_bench.py   (N={N} d={D} M={M} C={C} niter={NITER}, fp32 samples)")
    say(f"million_pq_train, {NITER} iterations : {gpu_ms:9.3f} ms  ({gpu_ms / NITER:.3f} ms per iteration; median of {args.reps}, "
        f"min {ts[0]:.3f}, max {ts[-1]:.3f})")
    say(f"objective: {o[0]:.6g} -> {o[-1]:.6g}; smallest cluster {int(counts.min())} points")

    # per-kernel device times of one call
    from torch.profiler import ProfilerActivity, profile
    with profile(activities=[ProfilerActivity.CUDA]) as prof:
        run()
        torch.cuda.synchronize()
    per = {}
    for ev in prof.events():
        for key in ("kmeans_assign", "kmeans_update", "kmeans_finish", "kmeans_gather"):
            if key in ev.name:
                per.setdefault(key, []).append(ev.device_time if hasattr(ev, "device_time") else ev.cuda_time)
    props = torch.cuda.get_device_properties(dev)
    clock_hz = getattr(props, "clock_rate", 2400000) * 1e3      # kHz
    for key, v in per.items():
        say(f"  {key:14s}: {len(v):3d} launches, mean {sum(v) / len(v):8.1f} us, min {min(v):8.1f} us")
    if "kmeans_assign" in per:
        us = sum(per["kmeans_assign"]) / len(per["kmeans_assign"])
        tests = N * M * C
        peak = props.multi_processor_count * 4 * 64 / 4 * clock_hz      # lane-instructions per second
        floor_us = tests * 6 / peak * 1e6
        say(f"  assign: {tests / us / 1e6:.2f} T(centroid tests)/s; vector-ALU floor at 6 instructions per test, {props.multi_processor_count} CUs, "
            f"{clock_hz / 1e9:.2f} GHz: {floor_us:.1f} us -> {100 * floor_us / us:.0f}% of the roofline "
            f"(derived before measuring: ~0.2 ms per iteration for assign, about half of that for update)")

    # host baseline
    if args.host_iters < 1:
        return 0
    torch.set_num_threads(min(16, torch.get_num_threads()))
    cents = X[rows.long()].reshape(C, M, D // M).transpose(0, 1).contiguous()
    host_iteration(X[:4096], cents)      # warm the thread pool
    t0 = time.perf_counter()
    for _ in range(args.host_iters):
        cents = host_iteration(X, cents)
    host_s = (time.perf_counter() - t0) / args.host_iters
    say(f"host, dense torch ops, {torch.get_num_threads()} threads : {host_s * 1e3:9.1f} ms per iteration (mean of {args.host_iters}), "
        f"{host_s * NITER:.1f} s for {NITER} iterations -> GPU {host_s * NITER * 1e3 / gpu_ms:.0f}x")
    if args.out:
        Path(args.out).parent.mkdir(parents=True, exist_ok=True)
        Path(args.out).write_text("\n".join(lines) + "\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())
