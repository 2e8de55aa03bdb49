#!/usr/bin/env python3
"""Timing of the prompt-attention kernel (csrc/prefill.hip) against torch's scaled_dot_product_attention on the same
fp16 tensors (the reference's recipe: repeat_kv + SDPA, pq_utils.py:249-260), HIP events, median of repeats.
FLOPs = 4 d nh x (number of unmasked (query, key) pairs) = 2 d nh n (n + 1) for a causal prompt of n tokens.

  python tools/prefill_bench.py                     the lockstep shapes against torch SDPA
  python tools/prefill_bench.py --ragged [--out F]  four prompts of 32K / 24K / 8K / 1K tokens at the Llama-3.1-8B shape (32 query
      heads, 8 kv heads, d = 128) in ONE ragged launch (dev_spans), against (a) the lockstep launch padded to 4 x 32K and (b) the
      four batch-1 lockstep calls issued back to back; rounds alternate the three, TFLOP/s counts the unmasked pairs of the four
      prompts in all three (the padded launch computes more pairs than it is credited with)."""
import argparse
import sys
from pathlib import Path

import torch

sys.path.insert(0, str(Path(__file__).resolve().parents[1]))
from million_amd import ops  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--ragged", action="store_true")
ap.add_argument("--rounds", type=int, default=5)
ap.add_argument("--out", default=None)
args = ap.parse_args()
dev = torch.device("cuda", 0)


def timeit(fn, reps=8):
    for _ in range(2):
        fn()
    torch.cuda.synchronize()
    ts = []
    for _ in range(reps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        torch.cuda.synchronize()
        ts.append(a.elapsed_time(b))
    ts.sort()
    return ts[len(ts) // 2]


def ragged():
    nh, nhk, d, lens = 32, 8, 128, [32768, 24576, 8192, 1024]
    bs, n = len(lens), max(lens)
    q = torch.randn(bs, nh, n, d, device=dev).half()
    k = torch.randn(bs, nhk, n, d, device=dev).half()
    v = torch.randn(bs, nhk, n, d, device=dev).half()
    out = torch.empty_like(q)
    spans = torch.tensor([[x, x, 0, 0] for x in lens], dtype=torch.int32, device=dev)
    flops = sum(2.0 * d * nh * x * (x + 1) for x in lens)

    def four():
        for b, x in enumerate(lens):
            ops.prefill_attn(q[b:b + 1, :, :x], k[b:b + 1, :, :x], v[b:b + 1, :, :x], out=out[b:b + 1, :, :x])
    forms = [("ragged launch (dev_spans)", lambda: ops.prefill_attn(q, k, v, out=out, dev_spans=spans)),
             ("(a) lockstep, padded to 4 x 32K", lambda: ops.prefill_attn(q, k, v, out=out)),
             ("(b) four batch-1 lockstep calls", four)]
    ms = [[] for _ in forms]
    for _ in range(args.rounds):
        for i, (_, fn) in enumerate(forms):
            ms[i].append(timeit(fn, reps=5))
    lines = [f"prompts {lens} nh={nh} nh_k={nhk} d={d}: {flops / 1e12:.2f} TFLOP of unmasked pairs (padded: "
             f"{bs * 2.0 * d * nh * n * (n + 1) / 1e12:.2f}); {args.rounds} rounds alternating the three forms, median of 5 per round"]
    for (name, _), m in zip(forms, ms):
        best = min(m)
        lines.append(f"{name:34s} best {best:8.3f} ms  {flops / best / 1e9:7.1f} TFLOP/s   rounds {' '.join('%.3f' % x for x in m)} ms "
                     f"(band {flops / max(m) / 1e9:.1f} .. {flops / best / 1e9:.1f} TFLOP/s)")
    lines.append(f"ragged / (a) {min(ms[0]) / min(ms[1]):.3f} of the time   ragged / (b) {min(ms[0]) / min(ms[2]):.3f} of the time")
    print("\n".join(lines), flush=True)
    if args.out:
        Path(args.out).write_text("\n".join(lines) + "\n")


if args.ragged:
    ragged()
    sys.exit(0)

for (bs, nh, nhk, n) in ((1, 32, 8, 4096), (1, 32, 8, 32768), (1, 32, 32, 4096), (1, 32, 32, 32768), (1, 32, 8, 131072)):
    d = 128
    q = torch.randn(bs, nh, n, d, device=dev).half()
    k = torch.randn(bs, nhk, n, d, device=dev).half()
    v = torch.randn(bs, nhk, n, d, device=dev).half()
    flops = 2.0 * d * nh * bs * n * (n + 1)
    ms = timeit(lambda: ops.prefill_attn(q, k, v))
    line = f"bs={bs} nh={nh} nh_k={nhk} n={n:6d}: prefill.hip {ms:9.3f} ms  {flops / ms / 1e9:7.1f} TFLOP/s ({flops / ms / 1e9 / 2500 * 100:4.1f}% of 2.5 PF dense fp16)"
    if n <= 32768:
        G = nh // nhk

        def sdpa():
            kk, vv = (k.repeat_interleave(G, dim=1), v.repeat_interleave(G, dim=1)) if G > 1 else (k, v)
            return torch.nn.functional.scaled_dot_product_attention(q, kk, vv, is_causal=True)
        ms2 = timeit(sdpa, reps=4)
        line += f" | repeat_kv + torch SDPA {ms2:9.3f} ms  {flops / ms2 / 1e9:7.1f} TFLOP/s"
    print(line, flush=True)
    del q, k, v
    torch.cuda.empty_cache()
