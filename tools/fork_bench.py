"""Forking a request of a PagedPQCache (PagedPQCache.fork -> ops.cache_fork, ONE launch) against the only routes there were:
encoding the prompt again (prefill_request) and a torch indexed copy of the pools, windows and lengths rows.

Llama-3.1-8B shape: 32 layers, 8 kv heads (32 query heads), d 128, M 64, pages of 64 tokens, a window of 128 rows; the source
holds a 32K-token prompt and a half-full window (64 decode steps).  Measured, each as the median of `--reps` calls per round,
`--rounds` rounds interleaved A B A B ... in one process (device time: HIP events around the call; host: perf_counter around
the call on an idle device):

  copy1 / copy3    fork into 1 / 3 slots of a preallocated cache (COPY: every live page is copied)
  torch1 / torch3  the same result through torch: int64 gathers of the page ids, pool[dst_ids] = pool[src_ids], slice copies
                   of the windows and lengths rows - all layers at once, the fewest launches torch allows
  share1 / share3  fork into 1 / 3 slots of an on-demand cache (SHARE: table rows, the partial tail page, the window)
  prefill          prefill_request of the same prompt into an empty slot, all layers (what a second request cost)

Bytes are read + written (pages of both sides, both windows); GB/s from the device time; `hbm_fraction` against the 8 TB/s HBM
peak of an MI355X.  One JSON line.

  python tools/fork_bench.py [--tokens 32768] [--reps 10] [--rounds 3]"""
from __future__ import annotations

import argparse
import json
import sys
import time
from pathlib import Path

sys.path.insert(0, str(Path(__file__).resolve().parents[1]))

import torch  # noqa: E402

from million_amd.pq_cache import PagedPQCache  # noqa: E402

LAYERS, NH, NHK, D, M, C, PS, CAP = 32, 32, 8, 128, 64, 256, 64, 128
HBM_PEAK = 8.0e12
BS = 4


def _median(xs):
    xs = sorted(xs)
    return xs[len(xs) // 2]


def _time(fn, reset, reps):
    """(median host microseconds to issue, median device microseconds to finish) of fn(); reset() runs before each call,
    outside both measurements."""
    reset()
    fn()
    host, dev = [], []
    for _ in range(reps):
        reset()
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        fn()
        host.append((time.perf_counter() - t0) * 1e6)
        torch.cuda.synchronize()
        reset()
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        b.synchronize()
        dev.append(a.elapsed_time(b) * 1e3)
    return _median(host), _median(dev)


def _filled(preallocate, tokens, prompt, cents, rows):
    """A cache whose slot 0 holds the prompt and 64 window rows; the other slots are empty."""
    cache = PagedPQCache(bs=BS, nh=NH, num_key_value_heads=NHK, M=M, layer_num=LAYERS, d=D, page_size=PS, extended_residual_size=CAP,
                         max_tokens=tokens + 1024, preallocate=preallocate, device="cuda")
    cache.set_cent(*cents)
    q, k, v = prompt
    for l in range(LAYERS):
        cache.prefill_request(0, q, k, v, l)
    qd, kd, vd = rows
    for _ in range(CAP // 2):
        for l in range(LAYERS):
            cache.decoding_with_pages(qd, kd, vd, l, use_dev_lengths=True)
    for b in range(1, BS):
        cache.release(b)
    torch.cuda.synchronize()
    return cache


def _torch_route(cache, src, dsts):
    """What a user could do without the call: the same bytes through torch indexing (a preallocated cache)."""
    n = -(-int(cache._T_a[0, src]) // PS)
    ids = cache._page_ids_all
    si = ids[:, src, :, :n].reshape(-1).long()
    for b in dsts:
        di = ids[:, b, :, :n].reshape(-1).long()
        cache.key_page_pool[di] = cache.key_page_pool[si]
        cache.value_page_pool[di] = cache.value_page_pool[si]
        cache._kres_all[:, b] = cache._kres_all[:, src]
        cache._vres_all[:, b] = cache._vres_all[:, src]
        cache._lengths_all[:, b] = cache._lengths_all[:, src]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--tokens", type=int, default=32768)
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--rounds", type=int, default=3)
    a = ap.parse_args()
    assert torch.cuda.is_available(), "fork_bench needs the GPU (no CPU timing)"
    g = torch.Generator(device="cuda").manual_seed(0)
    rnd = lambda *s: torch.randn(*s, device="cuda", generator=g).half()
    cents = (rnd(M, C, D // M), rnd(M, C, D // M))
    prompt = (rnd(1, NH, a.tokens, D), rnd(1, NHK, a.tokens, D), rnd(1, NHK, a.tokens, D))
    rows = (rnd(BS, NH, 1, D), rnd(BS, NHK, 1, D), rnd(BS, NHK, 1, D))
    pre = _filled(True, a.tokens, prompt, cents, rows)
    dem = _filled(False, a.tokens, prompt, cents, rows)
    T = int(pre._T_a[0, 0])
    n_live, tail = -(-T // PS), T % PS
    page_pair, win_pair = 2 * PS * M, 2 * CAP * D * 2
    per_dst = dict(copy=LAYERS * NHK * (n_live * page_pair + win_pair), share=LAYERS * NHK * ((page_pair if tail else 0) + win_pair))

    def releaser(cache, dsts):
        def reset():
            for b in dsts:
                cache.release(b)
        return reset

    # the torch route and the call leave the same bytes (one destination, checked once)
    pre.fork(0, 1)
    _torch_route(pre, 0, [2])
    ids = pre._page_ids_all[:, :, :, :n_live].long()
    same = all(bool(torch.equal(p[ids[:, 1]], p[ids[:, 2]])) for p in (pre.key_page_pool, pre.value_page_pool)) and \
        bool(torch.equal(pre._kres_all[:, 1], pre._kres_all[:, 2]) and torch.equal(pre._lengths_all[:, 1], pre._lengths_all[:, 2]))
    pre.release(1)
    pre._lengths_all[:, 2].zero_()

    def prefill():
        for l in range(LAYERS):
            dem.prefill_request(1, *prompt, l)

    sides = {}
    for n, dsts in ((1, [1]), (3, [1, 2, 3])):
        sides[f"copy{n}"] = (lambda dsts=dsts: pre.fork(0, dsts), releaser(pre, dsts), n * per_dst["copy"])
        sides[f"torch{n}"] = (lambda dsts=dsts: _torch_route(pre, 0, dsts), lambda: None, n * per_dst["copy"])
        sides[f"share{n}"] = (lambda dsts=dsts: dem.fork(0, dsts), releaser(dem, dsts), n * per_dst["share"])
    sides["prefill"] = (prefill, releaser(dem, [1]), 0)
    res = {s: [] for s in sides}
    for _ in range(a.rounds):
        for s, (fn, reset, _) in sides.items():
            res[s].append(_time(fn, reset, a.reps if s != "prefill" else 2))
            reset()
    out = dict(layers=LAYERS, nh_k=NHK, d=D, M=M, page_size=PS, resid_cap=CAP, T=T, r=int(pre._r_a[0, 0]), reps=a.reps,
               torch_route_equals_fork=same)
    for s, (_, _, nbytes) in sides.items():
        hs, ds = [round(r[0], 1) for r in res[s]], [round(r[1], 1) for r in res[s]]
        e = dict(device_us=dict(rounds=ds, median=_median(ds)), host_issue_us=dict(rounds=hs, median=_median(hs)))
        if nbytes:
            e["bytes_moved"] = 2 * nbytes
            e["GBps"] = round(2 * nbytes / (_median(ds) * 1e-6) / 1e9, 1)
            e["hbm_fraction"] = round(2 * nbytes / (_median(ds) * 1e-6) / HBM_PEAK, 3)
        out[s] = e
    for n in (1, 3):
        out[f"copy{n}_over_torch{n}_device"] = round(out[f"copy{n}"]["device_us"]["median"] / out[f"torch{n}"]["device_us"]["median"], 3)
    print(json.dumps(out), flush=True)


if __name__ == "__main__":
    main()
