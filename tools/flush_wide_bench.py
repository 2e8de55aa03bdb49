"""The window flush and the ragged store of a wide paged cache (nbits 9 .. 12, uint16 or packed pages), new route against old,
in one process, at the Llama-3.1-8B shape: 8 kv heads, 32 query heads, d 128, pages of 64 tokens, a window of 128 rows.

(a) The flush alone, 64 rows, at (M 64, C 1024), (M 32, C 4096), (M 64, C 512), uint16 and packed, 1 and 8 requests in lockstep:
    NEW  ops.pq_flush_wide with device lengths (min_r = the window), its advance launch included;
    OLD  what PagedPQCache._flush_wide issues: two ops.pq_encode_into / pq_encode_into_packed launches with host values plus
         ops.lengths_advance.
    Each route is captured into a graph behind a copy that puts the lengths rows back (so every replay flushes; the copy alone is
    measured too) and replayed `--reps` times between two events; `--rounds` such windows per route, alternating NEW OLD NEW OLD.
    Reported: every window, the median, the lowest and highest window, and the condition of DESIGN.md 4.19 - NEW's highest window
    below OLD's lowest.  The pools of the two routes are compared bit for bit first.
(b) Whole steps: all layers of paged_turns.decode (NEW) and of PagedPQCache.decoding_with_pages (OLD) on a cache of `--layers`
    layers holding `--tokens` tokens, one graph per step kind (the lengths rows put back inside the graph), flush step over plain
    step as bench.py reports it for uint8.
(c) The ragged store: ONE ops.pq_store_ragged_wide call against the host-driven per-slot encodes, at the requests of
    tools/store_bench.py, device time between events.

One JSON line per measurement.  python tools/flush_wide_bench.py [--reps 50] [--rounds 5] [--layers 8] [--tokens 4096] [--skip abc]"""
from __future__ import annotations

import argparse
import json
import sys
from pathlib import Path

sys.path.insert(0, str(Path(__file__).resolve().parents[1]))

import numpy as np  # noqa: E402
import torch  # noqa: E402

from million_amd import _lib as L  # noqa: E402
from million_amd import ops, paged_turns  # noqa: E402
from million_amd.pq_cache import PagedPQCache  # noqa: E402

NH, NHK, D, PS, CAP = 32, 8, 128, 64, 128
FORMATS = [(64, 10), (32, 12), (64, 9)]      # (M, nbits)
STORE_REQUESTS = [(8192, 77, 100, 2048), (4096, 128, 64, 64), (0, 0, 0, 512), (1024, 50, 7, 0)]      # tools/store_bench.py: (T, r, start, n)


def _median(xs):
    xs = sorted(xs)
    return xs[len(xs) // 2]


def _windows(graphs, reps, rounds):
    """{name: [microseconds per replay, one per window]}: the graphs take turns, one window of `reps` replays each per round."""
    for g in graphs.values():
        for _ in range(5):
            g.replay()
    torch.cuda.synchronize()
    out = {name: [] for name in graphs}
    for _ in range(rounds):
        for name, g in graphs.items():
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            for _ in range(reps):
                g.replay()
            b.record()
            b.synchronize()
            out[name].append(round(a.elapsed_time(b) * 1e3 / reps, 2))
    return out


def _capture(fn):
    fn()
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        fn()
    return g


def _summary(ws):
    return dict(windows=ws, median=_median(ws), low=min(ws), high=max(ws))


def _pools(n_pool, M, C, packed, dev):
    if packed:
        return [torch.zeros(n_pool, ops.packed_page_bytes(PS, M, C), dtype=torch.uint8, device=dev) for _ in range(2)]
    return [torch.zeros(n_pool, PS, M, dtype=torch.uint16, device=dev), torch.zeros(n_pool, M, PS, dtype=torch.uint16, device=dev)]


def flush_alone(a, dev, g):
    for M, nbits in FORMATS:
        C = 2 ** nbits
        kc, vc = (torch.randn(M, C, D // M, device=dev, generator=g).half() for _ in range(2))
        for packed in (False, True):
            for bs in (1, 8):
                T, start, npc = 4096 + 45, 40, 80
                n_pool = bs * NHK * npc
                ids = torch.randperm(n_pool, device=dev, generator=g).to(torch.int32).reshape(bs, NHK, npc)
                kres, vres = (torch.randn(bs, NHK, CAP, D, device=dev, generator=g).half() for _ in range(2))
                rows0 = torch.tensor([[T, CAP, start, 0]] * bs, dtype=torch.int32, device=dev)
                lengths = {s: rows0.clone() for s in ("new", "old", "copy")}
                pools = {s: _pools(n_pool, M, C, packed, dev) for s in ("new", "old")}
                enc = ops.pq_encode_into_packed if packed else ops.pq_encode_into

                def new():
                    lengths["new"].copy_(rows0)
                    ops.pq_flush_wide(kres, vres, kc, vc, *pools["new"], ids, n=PS, page_size=PS, dev_lengths=lengths["new"], min_r=CAP, packed=packed)

                def old():
                    lengths["old"].copy_(rows0)
                    kw = dict(token_start=T, n=PS, page_ids=ids, page_size=PS, x_row_start=start, x_row_mod=CAP)
                    enc(kres, kc, pools["old"][0], layout=L.MILLION_CODES_KPAGES, **kw)
                    enc(vres, vc, pools["old"][1], layout=L.MILLION_CODES_VPAGES, **kw)
                    ops.lengths_advance(lengths["old"], PS, CAP)

                graphs = dict(new=_capture(new), old=_capture(old), copy=_capture(lambda: lengths["copy"].copy_(rows0)))
                for gr in graphs.values():
                    gr.replay()
                torch.cuda.synchronize()
                same = all(torch.equal(x.view(torch.uint8), y.view(torch.uint8)) for x, y in zip(pools["new"], pools["old"])) and \
                    torch.equal(lengths["new"][:, :3], lengths["old"][:, :3]) and lengths["new"][0, :3].tolist() == [T + PS, CAP - PS, (start + PS) % CAP]
                ws = _windows(graphs, a.reps, a.rounds)
                tests = PS * NHK * 2 * M * C * bs
                floor_us = tests * (9 if D // M == 4 else 6) / 39e12 * 1e6
                print(json.dumps(dict(what="flush_alone", M=M, C=C, packed=packed, requests=bs, bitwise_equal=bool(same),
                                      new_us=_summary(ws["new"]), old_us=_summary(ws["old"]), lengths_copy_us=_summary(ws["copy"]),
                                      new_over_old=round(_median(ws["new"]) / _median(ws["old"]), 3),
                                      new_faster_beyond_spread=bool(max(ws["new"]) < min(ws["old"])),
                                      centroid_tests=tests, derived_floor_us=round(floor_us, 1))), flush=True)


def whole_steps(a, dev, g):
    for M, nbits in FORMATS:
        C = 2 ** nbits
        for packed in (False, True):
            for bs in (1, 8):
                cache = PagedPQCache(bs=bs, nh=NH, num_key_value_heads=NHK, M=M, layer_num=a.layers, d=D, page_size=PS, extended_residual_size=CAP,
                                     max_tokens=a.tokens + 1024, nbits=nbits, dtype=torch.uint16, packed=packed, device=dev)
                cache.set_cent(*(torch.randn(M, C, D // M, device=dev, generator=g).half() for _ in range(2)))
                cache._kres_all.copy_(torch.randn(cache._kres_all.shape, device=dev, generator=g).half())
                cache._vres_all.copy_(torch.randn(cache._vres_all.shape, device=dev, generator=g).half())
                q = torch.randn(bs, NH, 1, D, device=dev, generator=g).half()
                k, v = (torch.randn(bs, NHK, 1, D, device=dev, generator=g).half() for _ in range(2))
                out = torch.empty_like(q)
                full = np.full((a.layers, bs), 1)
                states = {"plain": (full * a.tokens, full * (CAP - PS), full * a.tokens, full * 0),
                          "flush": (full * a.tokens, full * CAP, full * a.tokens, full * 0)}      # (seen, r, T, start)
                rows = {kind: torch.tensor([[a.tokens, int(st[1][0, 0]), 0, 0]] * (a.layers * bs), dtype=torch.int32, device=dev).view(a.layers, bs, 4)
                        for kind, st in states.items()}

                def step(kind, new):
                    def fn():
                        cache.set_host_state(states[kind])
                        cache._lengths_all.copy_(rows[kind])
                        for l in range(a.layers):
                            if new:
                                paged_turns.decode(cache, q, k, v, l, out=out, use_dev_lengths=True)
                            else:
                                cache.decoding_with_pages(q, k, v, l, out=out, use_dev_lengths=True)
                    return fn

                graphs = {f"{route}_{kind}": _capture(step(kind, route == "new")) for route in ("new", "old") for kind in ("plain", "flush")}
                ws = _windows(graphs, max(a.reps // 5, 5), a.rounds)
                med = {name: _median(x) for name, x in ws.items()}
                print(json.dumps(dict(what="whole_step", M=M, C=C, packed=packed, requests=bs, layers=a.layers, tokens=a.tokens,
                                      **{name + "_us": _summary(x) for name, x in ws.items()},
                                      new_flush_over_plain=round(med["new_flush"] / med["new_plain"], 3),
                                      old_flush_over_plain=round(med["old_flush"] / med["old_plain"], 3))), flush=True)
                del cache, graphs
                torch.cuda.empty_cache()


def ragged_store(a, dev, g):
    bs, n_bound, npc = len(STORE_REQUESTS), max(r[3] for r in STORE_REQUESTS), 192
    for M, nbits in FORMATS[:2]:
        C = 2 ** nbits
        kc, vc = (torch.randn(M, C, D // M, device=dev, generator=g).half() for _ in range(2))
        for packed in (False, True):
            n_pool = bs * NHK * npc
            ids = torch.randperm(n_pool, device=dev, generator=g).to(torch.int32).reshape(bs, NHK, npc)
            kres, vres = (torch.randn(bs, NHK, CAP, D, device=dev, generator=g).half() for _ in range(2))
            k_new, v_new = (torch.randn(bs, NHK, n_bound, D, device=dev, generator=g).half() for _ in range(2))
            rows0 = torch.tensor([[T, r, s, 0] for T, r, s, _ in STORE_REQUESTS], dtype=torch.int32, device=dev)
            lengths = {s: rows0.clone() for s in ("new", "old")}
            dev_n = torch.tensor([r[3] for r in STORE_REQUESTS], dtype=torch.int32, device=dev)
            after = [torch.tensor([[T + r + n, 0, 0, 0]], dtype=torch.int32) for T, r, _, n in STORE_REQUESTS]
            pools = {s: _pools(n_pool, M, C, packed, dev) for s in ("new", "old")}
            enc = ops.pq_encode_into_packed if packed else ops.pq_encode_into

            def new():
                ops.pq_store_ragged_wide(k_new, v_new, kres, vres, kc, vc, *pools["new"], ids, lengths["new"], dev_n, M=M, C=C, page_size=PS, packed=packed)

            def old():
                for b, (T, r, s, n) in enumerate(STORE_REQUESTS):
                    if n == 0:
                        continue
                    sl = slice(b, b + 1)
                    kw = dict(page_ids=ids[sl], page_size=PS)
                    for x_win, x_new, cents, pool, lay in ((kres, k_new, kc, pools["old"][0], L.MILLION_CODES_KPAGES), (vres, v_new, vc, pools["old"][1], L.MILLION_CODES_VPAGES)):
                        if r:
                            enc(x_win[sl], cents, pool, layout=lay, token_start=T, n=r, x_row_start=s, x_row_mod=CAP, **kw)
                        enc(x_new[sl, :, :n], cents, pool, layout=lay, token_start=T + r, n=n, **kw)
                    lengths["old"][sl].copy_(after[b])

            res = {"new": [], "old": []}
            for name, fn in (("new", new), ("old", old)):
                lengths[name].copy_(rows0)
                fn()
            torch.cuda.synchronize()
            same = all(torch.equal(x.view(torch.uint8), y.view(torch.uint8)) for x, y in zip(pools["new"], pools["old"])) and torch.equal(lengths["new"], lengths["old"])
            for _ in range(a.rounds):
                for name, fn in (("new", new), ("old", old)):
                    xs = []
                    for _ in range(max(a.reps // 10, 3)):
                        lengths[name].copy_(rows0)
                        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                        e0.record()
                        fn()
                        e1.record()
                        e1.synchronize()
                        xs.append(e0.elapsed_time(e1) * 1e3)
                    res[name].append(round(_median(xs), 1))
            print(json.dumps(dict(what="ragged_store", M=M, C=C, packed=packed, requests=STORE_REQUESTS, bitwise_equal=bool(same),
                                  new_device_us=_summary(res["new"]), old_device_us=_summary(res["old"]),
                                  new_over_old=round(_median(res["new"]) / _median(res["old"]), 3))), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=50)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--layers", type=int, default=8)
    ap.add_argument("--tokens", type=int, default=4096)
    ap.add_argument("--skip", default="")
    a = ap.parse_args()
    assert torch.cuda.is_available(), "flush_wide_bench needs the GPU (no CPU timing)"
    dev = torch.device("cuda")
    g = torch.Generator(device=dev).manual_seed(0)
    for tag, fn in (("a", flush_alone), ("b", whole_steps), ("c", ragged_store)):
        if tag not in a.skip:
            fn(a, dev, g)


if __name__ == "__main__":
    main()
