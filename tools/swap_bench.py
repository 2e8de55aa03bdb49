"""Swapping a request of a PagedPQCache out to host memory and back in (PagedPQCache.swap_out / swap_in -> ops.cache_swap, ONE
pack or unpack launch per range of layers) against the routes there were: gathering and scattering the same bytes with torch
indexing on the device, and release + prefill_request of the same prompt.

Llama-3.1-8B shape: 32 layers, 8 kv heads (32 query heads), d 128, M 64, pages of 64 tokens, a window of 128 rows; slot 0 holds a
32K-token prompt and a half-full window (64 decode steps).  Measured, each as the median of its calls per round, `--rounds`
rounds interleaved in one process:

  pack / unpack      the launch alone, all layers into / out of one device blob (device time: HIP events around the call)
  torch_gather       the same bytes through torch: an int64 gather of the page ids, pool[ids] per side, the window rows in ring
  torch_scatter      order per side; and back: pool[ids] = pages per side, the window rows, the lengths rows - all layers at once,
                     the fewest launches torch allows (device time)
  swap_out / swap_in end to end: pack ranges into the staging buffer, copies to / from the pinned blob, the final
                     synchronisation (host time, perf_counter; the device is idle before the call)
  prefill            release + prefill_request of the same prompt, all layers (host time with a final synchronisation)

Bytes are read + written for the device routes (GB/s against the 8 TB/s HBM peak) and the blob's bytes once for the host link
(GB/s of the swap_out / swap_in wall time: the link rate with everything else on top).  One JSON line.
The run ends with an assertion error unless, in every round, pack <= torch_gather and unpack <= torch_scatter.  As measured
(profiles/cache_swap.txt): pack 369.5 / 368.6 / 364.6 us against 392.4 / 384.2 / 385.6 us; unpack 374.7 / 376.3 / 378.0 us against
2657.7 / 2666.6 / 2657.6 us.

  python tools/swap_bench.py [--tokens 32768] [--reps 10] [--rounds 3] [--staging-mib 64]"""
from __future__ import annotations

import argparse
import json
import sys
import time
from pathlib import Path

sys.path.insert(0, str(Path(__file__).resolve().parents[1]))

import torch  # noqa: E402

from million_amd import _lib as L  # noqa: E402
from million_amd import ops  # noqa: E402
from million_amd.pq_cache import PagedPQCache  # noqa: E402

LAYERS, NH, NHK, D, M, C, PS, CAP = 32, 32, 8, 128, 64, 256, 64, 128
HBM_PEAK = 8.0e12
BS = 2


def _median(xs):
    xs = sorted(xs)
    return xs[len(xs) // 2]


def _device_us(fn, reps):
    fn()
    out = []
    for _ in range(reps):
        torch.cuda.synchronize()
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        b.synchronize()
        out.append(a.elapsed_time(b) * 1e3)
    return _median(out)


def _host_us(fn, reps, reset=lambda: None):
    out = []
    for _ in range(reps):
        reset()
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        out.append((time.perf_counter() - t0) * 1e6)
    return _median(out)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--tokens", type=int, default=32768)
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--staging-mib", type=int, default=64)
    a = ap.parse_args()
    assert torch.cuda.is_available(), "swap_bench needs the GPU (no CPU timing)"
    g = torch.Generator(device="cuda").manual_seed(0)
    rnd = lambda *s: torch.randn(*s, device="cuda", generator=g).half()
    cache = PagedPQCache(bs=BS, nh=NH, num_key_value_heads=NHK, M=M, layer_num=LAYERS, d=D, page_size=PS, extended_residual_size=CAP,
                         max_tokens=a.tokens + 1024, preallocate=True, device="cuda")
    cache.set_cent(rnd(M, C, D // M), rnd(M, C, D // M))
    prompt = (rnd(1, NH, a.tokens, D), rnd(1, NHK, a.tokens, D), rnd(1, NHK, a.tokens, D))
    for l in range(LAYERS):
        cache.prefill_request(0, *prompt, l)
    rows = (rnd(BS, NH, 1, D), rnd(BS, NHK, 1, D), rnd(BS, NHK, 1, D))
    for _ in range(CAP // 2):
        for l in range(LAYERS):
            cache.decoding_with_pages(*rows, l, use_dev_lengths=True)
    cache.release(1)
    torch.cuda.synchronize()
    T, r, st = int(cache._T_a[0, 0]), int(cache._r_a[0, 0]), int(cache._rs_a[0, 0])
    n_live = -(-T // PS)
    rb = ops.cache_swap_row_bytes(T, r, PS, M, D)
    blob_bytes = LAYERS * NHK * rb
    staging = a.staging_mib << 20

    # ---- the launches alone
    blob = torch.empty(blob_bytes, dtype=torch.uint8, device="cuda")
    offs = torch.zeros(1, dtype=torch.int64, device="cuda")
    arrays = (cache._page_ids_all, cache.key_page_pool, cache.value_page_pool, cache._kres_all, cache._vres_all, cache._lengths_all)
    t_out = torch.tensor([[0, T, r, st]], dtype=torch.int32, device="cuda")
    t_in = torch.tensor([[1, T, r, st]], dtype=torch.int32, device="cuda")
    pack = lambda: ops.cache_swap(L.MILLION_SWAP_PACK, *arrays, t_out, offs, blob, n_pages_bound=n_live)
    unpack = lambda: ops.cache_swap(L.MILLION_SWAP_UNPACK, *arrays, t_in, offs, blob, n_pages_bound=n_live)

    # ---- the same bytes through torch indexing
    ring = (st + torch.arange(r, device="cuda")) % CAP
    held = {}

    def torch_gather():
        ids = cache._page_ids_all[:, 0, :, :n_live].reshape(-1).long()
        held["k"], held["v"] = cache.key_page_pool[ids], cache.value_page_pool[ids]
        held["kw"], held["vw"] = cache._kres_all[:, 0][:, :, ring], cache._vres_all[:, 0][:, :, ring]

    def torch_scatter():
        ids = cache._page_ids_all[:, 1, :, :n_live].reshape(-1).long()
        cache.key_page_pool[ids] = held["k"]
        cache.value_page_pool[ids] = held["v"]
        cache._kres_all[:, 1][:, :, ring] = held["kw"]
        cache._vres_all[:, 1][:, :, ring] = held["vw"]
        cache._lengths_all[:, 1] = cache._lengths_all[:, 0]

    # the routes leave the same bytes (checked once; T is a multiple of the page size here, so the gather needs no tail mask)
    pack()
    torch_gather()
    rows_ = blob.view(LAYERS * NHK, rb)
    pb = n_live * PS * M
    same = (torch.equal(rows_[:, :pb], held["k"].view(LAYERS * NHK, pb)) and torch.equal(rows_[:, pb:2 * pb], held["v"].view(LAYERS * NHK, pb))
            and torch.equal(rows_[:, 2 * pb:2 * pb + 2 * r * D], held["kw"].contiguous().view(torch.uint8).view(LAYERS * NHK, -1))) if T % PS == 0 else None
    unpack()
    ids = cache._page_ids_all[:, :, :, :n_live].long()
    same_back = all(bool(torch.equal(p[ids[:, 0]], p[ids[:, 1]])) for p in (cache.key_page_pool, cache.value_page_pool)) and \
        bool(torch.equal(cache._kres_all[:, 1][:, :, ring], cache._kres_all[:, 0][:, :, ring]))
    cache._lengths_all[:, 1].zero_()

    # ---- end to end
    snap = {}

    def swap_out():
        snap["s"] = cache.swap_out(0, release=False, staging_bytes=staging)

    def swap_in():
        cache.swap_in(1, snap["s"], staging_bytes=staging)

    def prefill():
        cache.release(1)
        for l in range(LAYERS):
            cache.prefill_request(1, *prompt, l)

    res = {k: [] for k in ("pack", "torch_gather", "unpack", "torch_scatter", "swap_out", "swap_in", "prefill")}
    few = max(3, a.reps // 2)
    for _ in range(a.rounds):
        res["pack"].append(_device_us(pack, a.reps))
        res["torch_gather"].append(_device_us(torch_gather, few))
        res["unpack"].append(_device_us(unpack, a.reps))
        res["torch_scatter"].append(_device_us(torch_scatter, few))
        cache._lengths_all[:, 1].zero_()
        res["swap_out"].append(_host_us(swap_out, few))
        res["swap_in"].append(_host_us(swap_in, few, reset=lambda: cache.release(1)))
        res["prefill"].append(_host_us(prefill, 2))
        cache.release(1)
    out = dict(layers=LAYERS, nh_k=NHK, d=D, M=M, page_size=PS, resid_cap=CAP, T=T, r=r, start=st, reps=a.reps, blob_bytes=blob_bytes,
               staging_bytes=staging, pinned=bool(snap["s"].blob.is_pinned()), pack_equals_torch_gather=same, unpack_restores_slot=same_back)
    for k, v in res.items():
        e = dict(us=dict(rounds=[round(x, 1) for x in v], median=round(_median(v), 1)))
        if k in ("pack", "unpack", "torch_gather", "torch_scatter"):
            e["bytes_moved"] = 2 * blob_bytes
            e["TBps"] = round(2 * blob_bytes / (_median(v) * 1e-6) / 1e12, 3)
            e["hbm_fraction"] = round(2 * blob_bytes / (_median(v) * 1e-6) / HBM_PEAK, 3)
        elif k != "prefill":
            e["link_GBps"] = round(blob_bytes / (_median(v) * 1e-6) / 1e9, 1)
        out[k] = e
    out["pack_not_slower_than_torch_every_round"] = all(p <= t for p, t in zip(res["pack"], res["torch_gather"]))
    out["unpack_not_slower_than_torch_every_round"] = all(p <= t for p, t in zip(res["unpack"], res["torch_scatter"]))
    out["device_share_of_swap_out"] = round(_median(res["pack"]) / _median(res["swap_out"]), 3)
    out["device_share_of_swap_in"] = round(_median(res["unpack"]) / _median(res["swap_in"]), 3)
    print(json.dumps(out), flush=True)
    assert out["pack_not_slower_than_torch_every_round"] and out["unpack_not_slower_than_torch_every_round"]


if __name__ == "__main__":
    main()
