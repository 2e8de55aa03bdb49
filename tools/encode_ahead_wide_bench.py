"""Encode-ahead on a wide paged cache (nbits 9 .. 12, uint16 or packed pages) against the in-line flush, in one process, at the
Llama-3.1-8B shape: 32 layers, 8 kv heads, 32 query heads, d 128, pages of 64 tokens, a window of 128 rows.

Per (M, C) in (64, 1024), (32, 4096), (64, 512), uint16 and packed, 1 and 8 requests, `--tokens` tokens per request:
  * whole steps, every layer, one graph per step kind with the lengths rows and the host mirror put back inside the graph:
      plain     paged_turns.decode, no window full;
      flush     the in-line flush step: paged_turns.decode without begin_step - the route without this feature, the reference;
      commit    paged_turns.begin_step ('commit': one lengths_advance) + decode;
      pre/S     paged_turns.begin_step ('pre' / 'pre0' with encode_ahead_steps = S, for every S of --spreads; "default" is the
                cache's own rule) + decode: the step that carries a group's encode-ahead launches on the side stream;
    replayed `--reps` times between two events, `--rounds` windows per graph, the graphs taking turns (plain flush commit pre ..
    plain flush ..): medians, and lowest / highest window as the run-to-run spread of the same run;
  * the encode-ahead launch of all layers alone (ops.pq_flush_wide, advance=False), warm and back to back, per pairs_in_flight
    of --in-flight (0: the library's rule);
  * per spread S the two claims: (a) the worst step of a flush period (max of pre/S and commit) against the in-line flush step,
    (b) the sum over one period of page_size steps - (page_size - 1 - S) plain + S pre/S + commit against (page_size - 1) plain +
    flush - each "beyond the spread": the highest window of the one below the lowest window of the other.

One JSON line per measurement.
python tools/encode_ahead_wide_bench.py [--tokens 4096] [--layers 32] [--reps 10] [--rounds 5] [--spreads default,1,8,32] [--in-flight 0]
                                        [--formats 0,1,2] [--requests 1,8]"""
from __future__ import annotations

import argparse
import json
import sys
from pathlib import Path

sys.path.insert(0, str(Path(__file__).resolve().parents[1]))

import numpy as np  # noqa: E402
import torch  # noqa: E402

from million_amd import ops, paged_turns  # noqa: E402
from million_amd.pq_cache import PagedPQCache  # noqa: E402

NH, NHK, D, PS, CAP = 32, 8, 128, 64, 128
FORMATS = [(64, 10), (32, 12), (64, 9)]      # (M, nbits)


def _median(xs):
    xs = sorted(xs)
    return xs[len(xs) // 2]


def _summary(ws):
    return dict(median=_median(ws), low=min(ws), high=max(ws))


def _windows(graphs, reps, rounds):
    """{name: [microseconds per replay, one per window]}: the graphs take turns, one window of `reps` replays each per round."""
    for g in graphs.values():
        for _ in range(3):
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
            out[name].append(round(a.elapsed_time(b) * 1e3 / reps, 1))
    return out


def _capture(fn):
    fn()
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        fn()
    return g


def one_shape(a, dev, gen, M, nbits, packed, bs):
    C, nl = 2 ** nbits, a.layers
    cache = PagedPQCache(bs=bs, nh=NH, num_key_value_heads=NHK, M=M, layer_num=nl, d=D, page_size=PS, extended_residual_size=CAP,
                         max_tokens=a.tokens + 1024, nbits=nbits, dtype=torch.uint16, packed=packed, device=dev)
    cache.set_cent(*(torch.randn(M, C, D // M, device=dev, generator=gen).half() for _ in range(2)))
    cache._kres_all.copy_(torch.randn(cache._kres_all.shape, device=dev, generator=gen).half())
    cache._vres_all.copy_(torch.randn(cache._vres_all.shape, device=dev, generator=gen).half())
    q = torch.randn(bs, NH, 1, D, device=dev, generator=gen).half()
    k, v = (torch.randn(bs, NHK, 1, D, device=dev, generator=gen).half() for _ in range(2))
    out = torch.empty_like(q)
    full = np.full((nl, bs), 1)
    base = (full * a.tokens, full * 0, full * a.tokens, full * 0, full * 0)      # (seen, r, T, start, flags)

    def rows_of(state):
        r = np.broadcast_to(np.asarray(state[1]).reshape(nl, -1), (nl, bs))
        t = np.stack([full * a.tokens, r, full * 0, full * 0], axis=2).astype(np.int32)
        return torch.from_numpy(np.ascontiguousarray(t)).to(dev)

    keep = []      # the rows a graph copies from live as long as the graphs do

    def step(state, begin):
        rows = rows_of(state)
        keep.append(rows)

        def fn():
            cache.set_host_state(state)
            cache._lengths_all.copy_(rows)
            if begin:
                paged_turns.begin_step(cache, use_dev_lengths=True)
            for l in range(nl):
                paged_turns.decode(cache, q, k, v, l, out=out, use_dev_lengths=True)
        return fn

    graphs, spreads = {}, {}
    states = dict(cache.capture_states(base))
    states["plain"] = (base[0], [CAP - PS] * nl, base[2], base[3], [1] * nl)      # a window of page_size rows, as behind a flush
    graphs["plain"] = _capture(step(states["plain"], False))
    graphs["flush"] = _capture(step(states["flush"], False))
    graphs["commit"] = _capture(step(states["commit"], True))
    for sp in a.spreads.split(","):
        cache.encode_ahead_steps = None if sp == "default" else int(sp)
        groups = cache._ea_groups()
        kind, state = cache.capture_states(base)[1]
        assert kind in ("pre", "pre0")
        cache.set_host_state(state)
        assert paged_turns.next_step_kind(cache) == kind
        if len(groups) in spreads.values():
            continue      # the same grouping as a spread already captured
        spreads[sp] = len(groups)
        graphs[f"pre/{sp}"] = _capture(step(state, True))
    cache.encode_ahead_steps = None
    for name, gr in graphs.items():      # every graph does what its name says: the device rows after one replay
        gr.replay()
        torch.cuda.synchronize()
        rows = cache._lengths_all.cpu().numpy()
        moved = name in ("flush", "commit")
        r0 = {"plain": CAP - PS, "flush": CAP, "commit": CAP}.get(name, cache.encode_ahead_at())
        assert (rows[:, :, 0] == a.tokens + (PS if moved else 0)).all() and (rows[:, :, 1] == r0 - (PS if moved else 0) + 1).all(), (name, rows[0])
        assert (rows[:, :, 2] == (PS if moved else 0)).all(), (name, rows[0])
    ws = _windows(graphs, a.reps, a.rounds)
    rec = dict(what="steps", M=M, C=C, packed=packed, requests=bs, layers=nl, tokens=a.tokens,
               **{name + "_us": _summary(x) for name, x in ws.items()})
    print(json.dumps(rec), flush=True)
    plain, flush, commit = ws["plain"], ws["flush"], ws["commit"]
    inline_sum = [(PS - 1) * p + f for p, f in zip(plain, flush)]
    for sp, n in spreads.items():
        pre = ws[f"pre/{sp}"]
        worst = [max(p, c) for p, c in zip(pre, commit)]
        ea_sum = [(PS - 1 - n) * p + n * e + c for p, e, c in zip(plain, pre, commit)]
        print(json.dumps(dict(what="claims", M=M, C=C, packed=packed, requests=bs, tokens=a.tokens, spread=sp, pre_steps=n,
                              layers_per_pre_step=-(-nl // n), pre_over_plain=round(_median(pre) / _median(plain), 3),
                              commit_over_plain=round(_median(commit) / _median(plain), 3), flush_over_plain=round(_median(flush) / _median(plain), 3),
                              worst_step_us=_summary(worst), inline_flush_us=_summary(flush), a_worst_step_shorter_beyond_spread=bool(max(worst) < min(flush)),
                              period_us=_summary([round(x, 1) for x in ea_sum]), inline_period_us=_summary([round(x, 1) for x in inline_sum]),
                              period_over_inline=round(_median(ea_sum) / _median(inline_sum), 4),
                              b_period_not_longer_beyond_spread=bool(min(ea_sum) <= max(inline_sum)))), flush=True)
    # the encode-ahead launch of every layer alone, warm, back to back
    alone = {}
    for pif in a.in_flight.split(","):
        def launch(pif=int(pif)):
            ops.pq_flush_wide(cache._kres_all, cache._vres_all, cache.key_cent, cache.value_cent, cache.key_page_pool, cache.value_page_pool,
                              cache._page_ids_all, n=PS, page_size=PS, token_start=a.tokens, x_row_start=0, packed=packed, advance=False,
                              pairs_in_flight=pif or None)
        alone[f"in_flight={pif}"] = _capture(launch)

    def inline(layered):      # the 16-wave flush of every layer, host lengths: one layered call, or the in-line route's call per layer
        kw = dict(n=PS, page_size=PS, token_start=a.tokens, x_row_start=0, packed=packed)
        if layered:
            return lambda: ops.pq_flush_wide(cache._kres_all, cache._vres_all, cache.key_cent, cache.value_cent, cache.key_page_pool,
                                             cache.value_page_pool, cache._page_ids_all, **kw)
        return lambda: [ops.pq_flush_wide(cache._kres_all[l], cache._vres_all[l], cache.key_cent, cache.value_cent, cache.key_page_pool,
                                          cache.value_page_pool, cache._page_ids_all[l], **kw) for l in range(nl)]
    alone["flush_16_wave_layered"] = _capture(inline(True))
    alone["flush_16_wave_per_layer"] = _capture(inline(False))
    ws = _windows(alone, a.reps, a.rounds)
    print(json.dumps(dict(what="encode_ahead_launch_alone", M=M, C=C, packed=packed, requests=bs, layers=nl,
                          **{name + "_us": _summary(x) for name, x in ws.items()})), flush=True)
    del cache, graphs, alone, keep
    torch.cuda.empty_cache()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--tokens", type=int, default=4096)
    ap.add_argument("--layers", type=int, default=32)
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--spreads", default="default,1,8,32")
    ap.add_argument("--in-flight", dest="in_flight", default="0")
    ap.add_argument("--formats", default="0,1,2")
    ap.add_argument("--requests", default="1,8")
    a = ap.parse_args()
    assert torch.cuda.is_available(), "encode_ahead_wide_bench needs the GPU (no CPU timing)"
    dev = torch.device("cuda")
    gen = torch.Generator(device=dev).manual_seed(0)
    for fi in a.formats.split(","):
        M, nbits = FORMATS[int(fi)]
        for packed in (False, True):
            for bs in (int(x) for x in a.requests.split(",")):
                one_shape(a, dev, gen, M, nbits, packed, bs)


if __name__ == "__main__":
    main()
