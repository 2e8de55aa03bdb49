"""One decode step of n continuations of one long prompt, two routes ("Log-sum-exp, merge, SharedPrefix"):

  fork     the prompt in slot 0 of an on-demand PagedPQCache, forked into the other n - 1 slots (shared code pages), ONE
           decode launch per layer over the n slots: every slot streams the whole prompt
  shared   SharedPrefix: the prompt in a cache of its own, the continuations in a second cache; three launches per layer
           (chunk attention of the n queries over the prompt, the continuations' decode launch, the merge): the prompt is
           read once

Llama-3.1-8B shape: 32 / 8 heads, d 128, M 64, C 256, pages of 64 tokens, a window of 128 rows, `--layers` rotating layers.
The prompt is encoded into the pages without its attention pass (the store step of prefill: the bench times decode steps).
Per (prompt, n): the per-layer step time of each route, microseconds, as
  device_us  HIP events around `--sweeps` sweeps over the layers queued behind ~50 ms of other work, so that the host is ahead
             of the device and the figure is the device's alone
  eager_us   the same sweeps issued on an idle device: what a Python loop without a captured graph sees (host-bound when the
             launches are shorter than their issue)
each the median of `--rounds` rounds, the routes alternating within a round.  `crossover`: the smallest measured n at which the
shared route's device time is below the fork route's (null: none).  One JSON line.

  python tools/shared_prefix_bench.py [--prompts 32768 131072] [--n 4 8 16] [--layers 32] [--sweeps 3] [--rounds 3]"""
from __future__ import annotations

import argparse
import json
import sys
from pathlib import Path

sys.path.insert(0, str(Path(__file__).resolve().parents[1]))

import torch  # noqa: E402

from million_amd.pq_cache import PagedPQCache  # noqa: E402
from million_amd.shared_prefix import SharedPrefix  # noqa: E402

NH, NHK, D, M, C, PS, CAP = 32, 8, 128, 64, 256, 64, 128


def _median(xs):
    xs = sorted(xs)
    return xs[len(xs) // 2]


def _cache(bs, layers, max_tokens, cents):
    c = PagedPQCache(bs=bs, nh=NH, num_key_value_heads=NHK, M=M, layer_num=layers, d=D, page_size=PS, extended_residual_size=CAP,
                     max_tokens=max_tokens, preallocate=False, device="cuda")
    c.set_cent(*cents)
    return c


def _encode_prompt(cache, k, v):
    for l in range(cache.layer_num):
        cache._store(k, v, l, k.size(2), 0, all_rows=True)      # prefill_request without the prompt's attention pass


def _busy(x):
    """~50 ms of device work the timed launches queue behind."""
    for _ in range(40):
        x = x @ x
    return x


def _time(step, layers, sweeps, busy):
    """(device_us, eager_us) per layer of step(l) over `sweeps` sweeps of the layers."""
    out = []
    for behind in (True, False):
        torch.cuda.synchronize()
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        if behind:
            _busy(busy)
        a.record()
        for _ in range(sweeps):
            for l in range(layers):
                step(l)
        b.record()
        b.synchronize()
        out.append(a.elapsed_time(b) * 1e3 / (sweeps * layers))
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--prompts", type=int, nargs="*", default=[32768, 131072])
    ap.add_argument("--n", type=int, nargs="*", default=[4, 8, 16])
    ap.add_argument("--layers", type=int, default=32)
    ap.add_argument("--sweeps", type=int, default=3)
    ap.add_argument("--rounds", type=int, default=3)
    a = ap.parse_args()
    assert torch.cuda.is_available(), "shared_prefix_bench needs the GPU (no CPU timing)"
    assert (2 * a.rounds + 2) * a.sweeps < CAP, "the windows must not flush inside the timed steps"
    g = torch.Generator(device="cuda").manual_seed(0)
    rnd = lambda *s: torch.randn(*s, device="cuda", generator=g).half()
    cents = (rnd(M, C, D // M), rnd(M, C, D // M))
    busy = rnd(8192, 8192) * 0.01
    res = dict(nh=NH, nh_k=NHK, d=D, M=M, C=C, page_size=PS, resid_cap=CAP, layers=a.layers, sweeps=a.sweeps, rounds=a.rounds, cases=[])
    for T in a.prompts:
        k, v = rnd(1, NHK, T, D), rnd(1, NHK, T, D)
        prefix = _cache(1, a.layers, T + 1024, cents)
        _encode_prompt(prefix, k, v)
        cross = None
        for n in a.n:
            forked = _cache(n, a.layers, T + 1024, cents)
            _encode_prompt(forked, k, v)
            forked.fork(0, list(range(1, n)))
            sp = SharedPrefix(prefix, 0, _cache(n, a.layers, 1024, cents))
            q, kn, vn = rnd(n, NH, 1, D), rnd(n, NHK, 1, D), rnd(n, NHK, 1, D)
            out_f = torch.empty_like(q)
            sides = dict(fork=lambda l: forked.decoding_with_pages(q, kn, vn, l, out=out_f, use_dev_lengths=True),
                         shared=lambda l: sp.decoding(q, kn, vn, l, use_dev_lengths=True))
            for step in sides.values():      # warm-up: workspaces, buffers, code caches
                for l in range(a.layers):
                    step(l)
            t = {s: [] for s in sides}
            for _ in range(a.rounds):
                for s, step in sides.items():
                    t[s].append(_time(step, a.layers, a.sweeps, busy))
            case = dict(prompt=T, n=n)
            for s in sides:
                case[s] = dict(device_us=round(_median([x[0] for x in t[s]]), 2), eager_us=round(_median([x[1] for x in t[s]]), 2),
                               device_rounds=[round(x[0], 2) for x in t[s]])
            case["shared_over_fork_device"] = round(case["shared"]["device_us"] / case["fork"]["device_us"], 3)
            if cross is None and case["shared"]["device_us"] < case["fork"]["device_us"]:
                cross = n
            res["cases"].append(case)
            print(json.dumps(case), file=sys.stderr, flush=True)
            del forked, sp
            torch.cuda.empty_cache()
        res.setdefault("crossover", {})[str(T)] = cross
        del prefix
        torch.cuda.empty_cache()
    from million_amd import ops
    res["tail_faults"] = ops.tail_faults()
    print(json.dumps(res), flush=True)


if __name__ == "__main__":
    main()
