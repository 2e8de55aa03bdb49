"""Fork and swap of a request of a wide PagedPQCache (nbits 10 / 12, uint16 or packed pages) through million_amd.paged_turns
(ops.cache_fork_wide, ops.cache_swap_wide: ONE launch, blob format 2) against the routes there were: torch indexing over the same
pages and windows, and the prompt pass (prefill_request) that a fork or a swap-in replaces.

Llama-3.1-8B shape: 32 layers, 8 kv heads (32 query heads), d 128, pages of 64 tokens, a window of 128 rows; slot 0 holds a
32K-token prompt and a half-full window (64 decode steps).  Per configuration - (M 64, C 1024) and (M 32, C 4096), packed and
uint16 - each figure is the median of its calls per round, `--rounds` rounds interleaved A B A B ... in one process:

  fork             paged_turns.fork into one slot of a preallocated cache (COPY: every live page; device time, HIP events)
  torch_copy       the same result through torch: pool[dst_ids] = pool[src_ids] per side, the windows, the lengths rows
  pack / unpack    the swap launch alone, all layers into / out of one device blob (device time)
  torch_gather     the same pages and window rows through torch indexing, in the POOL's format: pool[ids] per side, and back:
  torch_scatter    pool[ids] = pages (a uint16 pool moves 16 bits per code here, the blob 10 or 12)
  swap_out / swap_in  end to end through a 64 MiB staging buffer and a pinned blob (host time with the final synchronisation);
                   link_GBps: the blob's bytes over that time
  prefill          release + prefill_request of the same prompt, all layers (host time with a final synchronisation)
  link             a plain device-to-pinned-host copy of 256 MiB: the link rate of this run.  A uint16 cache's own page bytes are
                   16 / (8 + h) of its blob's page bytes: `u16_pages_at_link_us` is the time those bytes alone would need at
                   that rate - derived, not measured - beside the measured swap_out of the uint16 cache.

No ratio is asserted: the line says which route was faster.  One JSON line per configuration.

  python tools/fork_swap_wide_bench.py [--tokens 32768] [--reps 5] [--rounds 3] [--configs 64x10,32x12]"""
from __future__ import annotations

import argparse
import json
import sys
import time
from pathlib import Path

sys.path.insert(0, str(Path(__file__).resolve().parents[1]))

import torch  # noqa: E402

from million_amd import _lib as L  # noqa: E402
from million_amd import ops, paged_turns  # noqa: E402
from million_amd.pq_cache import PagedPQCache  # noqa: E402

LAYERS, NH, NHK, D, PS, CAP, BS = 32, 32, 8, 128, 64, 128, 3
STAGING = 64 << 20


def _median(xs):
    xs = sorted(xs)
    return xs[len(xs) // 2]


def _device_us(fn, reps, reset=lambda: None):
    reset()
    fn()
    out = []
    for _ in range(reps):
        reset()
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


def _link_GBps(reps):
    n = 256 << 20
    dev, host = torch.empty(n, dtype=torch.uint8, device="cuda"), torch.empty(n, dtype=torch.uint8, pin_memory=True)
    us = _host_us(lambda: host.copy_(dev, non_blocking=True), reps)
    return n / (us * 1e-6) / 1e9


def run(M, nbits, packed, a):
    C = 2 ** nbits
    g = torch.Generator(device="cuda").manual_seed(0)
    rnd = lambda *s: torch.randn(*s, device="cuda", generator=g).half()
    cache = PagedPQCache(bs=BS, nh=NH, num_key_value_heads=NHK, M=M, layer_num=LAYERS, d=D, page_size=PS, extended_residual_size=CAP,
                         max_tokens=a.tokens + 1024, nbits=nbits, dtype=torch.uint16, packed=packed, preallocate=True, device="cuda")
    cache.set_cent(rnd(M, C, D // M), rnd(M, C, D // M))
    prompt = (rnd(1, NH, a.tokens, D), rnd(1, NHK, a.tokens, D), rnd(1, NHK, a.tokens, D))
    for l in range(LAYERS):
        cache.prefill_request(0, *prompt, l)
    rows = (rnd(BS, NH, 1, D), rnd(BS, NHK, 1, D), rnd(BS, NHK, 1, D))
    for _ in range(CAP // 2):
        for l in range(LAYERS):
            paged_turns.decode(cache, *rows, l, use_dev_lengths=True)
    for b in (1, 2):
        cache.release(b)
    torch.cuda.synchronize()
    T, r, st = int(cache._T_a[0, 0]), int(cache._r_a[0, 0]), int(cache._rs_a[0, 0])
    n_live = -(-T // PS)
    rb = ops.cache_swap_row_bytes_wide(T, r, PS, M, D, C)
    blob_bytes = LAYERS * NHK * rb
    page_pool = cache.key_page_pool[0].numel() * cache.key_page_pool.element_size()      # bytes of a page as the pool holds it
    pool_bytes = LAYERS * NHK * (2 * n_live * page_pool + 4 * r * D)
    fork_bytes = LAYERS * NHK * (2 * n_live * page_pool + 4 * CAP * D)
    kw = dict(C=C, packed=packed, page_size=PS, M=M)
    arrays = (cache._page_ids_all, cache.key_page_pool, cache.value_page_pool, cache._kres_all, cache._vres_all, cache._lengths_all)
    signed = lambda t: t.view(torch.int16) if t.dtype == torch.uint16 else t      # torch indexes int16, not uint16
    kp, vp = signed(cache.key_page_pool), signed(cache.value_page_pool)

    # ---- fork and its torch route (slot 0 -> 1 and -> 2): the same bytes, checked once
    def torch_copy(dst=2):
        si = cache._page_ids_all[:, 0, :, :n_live].reshape(-1).long()
        di = cache._page_ids_all[:, dst, :, :n_live].reshape(-1).long()
        kp[di] = kp[si]
        vp[di] = vp[si]
        cache._kres_all[:, dst] = cache._kres_all[:, 0]
        cache._vres_all[:, dst] = cache._vres_all[:, 0]
        cache._lengths_all[:, dst] = cache._lengths_all[:, 0]

    paged_turns.fork(cache, 0, 1)
    torch_copy()
    ids = cache._page_ids_all[:, :, :, :n_live].long()
    fork_same = all(bool(torch.equal(p[ids[:, 1]], p[ids[:, 2]])) for p in (kp, vp)) and bool(
        torch.equal(cache._kres_all[:, 1], cache._kres_all[:, 2]) and torch.equal(cache._lengths_all[:, 1], cache._lengths_all[:, 2]))
    cache.release(1)
    cache._lengths_all[:, 2].zero_()

    # ---- the swap launches alone and their torch routes
    blob = torch.empty(blob_bytes, dtype=torch.uint8, device="cuda")
    offs = torch.zeros(1, dtype=torch.int64, device="cuda")
    t_out = torch.tensor([[0, T, r, st]], dtype=torch.int32, device="cuda")
    t_in = torch.tensor([[1, T, r, st]], dtype=torch.int32, device="cuda")
    pack = lambda: ops.cache_swap_wide(L.MILLION_SWAP_PACK, *arrays, t_out, offs, blob, n_pages_bound=n_live, **kw)
    unpack = lambda: ops.cache_swap_wide(L.MILLION_SWAP_UNPACK, *arrays, t_in, offs, blob, n_pages_bound=n_live, **kw)
    ring = (st + torch.arange(r, device="cuda")) % CAP
    held = {}

    def torch_gather():
        i = cache._page_ids_all[:, 0, :, :n_live].reshape(-1).long()
        held["k"], held["v"] = kp[i], vp[i]
        held["kw"], held["vw"] = cache._kres_all[:, 0][:, :, ring], cache._vres_all[:, 0][:, :, ring]

    def torch_scatter():
        i = cache._page_ids_all[:, 1, :, :n_live].reshape(-1).long()
        kp[i] = held["k"]
        vp[i] = held["v"]
        cache._kres_all[:, 1][:, :, ring] = held["kw"]
        cache._vres_all[:, 1][:, :, ring] = held["vw"]
        cache._lengths_all[:, 1] = cache._lengths_all[:, 0]

    snap = {}

    def swap_out():
        snap["s"] = paged_turns.swap_out(cache, 0, release=False, staging_bytes=STAGING)

    def swap_in():
        paged_turns.swap_in(cache, 1, snap["s"], staging_bytes=STAGING)

    def prefill():
        cache.release(1)
        for l in range(LAYERS):
            cache.prefill_request(1, *prompt, l)

    names = ("fork", "torch_copy", "pack", "torch_gather", "unpack", "torch_scatter", "swap_out", "swap_in", "prefill", "link_GBps")
    res = {k: [] for k in names}
    for _ in range(a.rounds):
        res["fork"].append(_device_us(lambda: paged_turns.fork(cache, 0, 1), a.reps, reset=lambda: cache.release(1)))
        cache.release(1)
        res["torch_copy"].append(_device_us(torch_copy, a.reps))
        cache._lengths_all[:, 2].zero_()
        res["pack"].append(_device_us(pack, a.reps))
        res["torch_gather"].append(_device_us(torch_gather, a.reps))
        res["unpack"].append(_device_us(unpack, a.reps))
        res["torch_scatter"].append(_device_us(torch_scatter, a.reps))
        cache._lengths_all[:, 1].zero_()
        res["swap_out"].append(_host_us(swap_out, a.reps))
        res["swap_in"].append(_host_us(swap_in, a.reps, reset=lambda: cache.release(1)))
        res["prefill"].append(_host_us(prefill, 2))
        cache.release(1)
        res["link_GBps"].append(_link_GBps(a.reps))
    med = {k: _median(v) for k, v in res.items()}
    out = dict(M=M, C=C, packed=packed, layers=LAYERS, nh_k=NHK, d=D, page_size=PS, resid_cap=CAP, T=T, r=r, start=st, reps=a.reps,
               blob_bytes=blob_bytes, pool_format_bytes=pool_bytes, fork_bytes_moved=2 * fork_bytes, torch_copy_equals_fork=fork_same,
               pinned=bool(snap["s"].blob.is_pinned()))
    for k in names:
        out[k] = dict(rounds=[round(x, 1) for x in res[k]], median=round(med[k], 1))
    out["fork"]["TBps"] = round(2 * fork_bytes / (med["fork"] * 1e-6) / 1e12, 3)
    out["pack"]["TBps"] = round((pool_bytes + blob_bytes) / (med["pack"] * 1e-6) / 1e12, 3)
    out["unpack"]["TBps"] = round((pool_bytes + blob_bytes) / (med["unpack"] * 1e-6) / 1e12, 3)
    for k in ("swap_out", "swap_in"):
        out[k]["link_GBps"] = round(blob_bytes / (med[k] * 1e-6) / 1e9, 1)
    out["fork_over_torch_copy"] = round(med["fork"] / med["torch_copy"], 3)
    out["fork_over_prefill"] = round(med["fork"] / med["prefill"], 5)
    out["pack_over_torch_gather"] = round(med["pack"] / med["torch_gather"], 3)
    out["unpack_over_torch_scatter"] = round(med["unpack"] / med["torch_scatter"], 3)
    out["swap_in_over_prefill"] = round(med["swap_in"] / med["prefill"], 4)
    if not packed:      # derived: the uint16 page bytes (and the same windows) at the link rate of this run
        out["u16_pages_at_link_us"] = round(pool_bytes / (med["link_GBps"] * 1e9) * 1e6, 1)
        out["swap_out_over_u16_pages_at_link"] = round(med["swap_out"] / out["u16_pages_at_link_us"], 3)
    print(json.dumps(out), flush=True)
    del cache, prompt, blob, held, snap
    torch.cuda.empty_cache()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--tokens", type=int, default=32768)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--configs", default="64x10,32x12", help="M x nbits, comma separated")
    a = ap.parse_args()
    assert torch.cuda.is_available(), "fork_swap_wide_bench needs the GPU (no CPU timing)"
    for cfg in a.configs.split(","):
        M, nbits = (int(x) for x in cfg.split("x"))
        for packed in (True, False):
            run(M, nbits, packed, a)


if __name__ == "__main__":
    main()
