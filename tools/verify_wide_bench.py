"""Draft verification on wide caches (million_amd.paged_turns.verify / commit, nbits 10 and 12, uint16 and packed pages) per layer,
on one cache state, as replayed graphs, interleaved.

  python tools/verify_wide_bench.py [--rounds 11] [--inner 10] [--quick]

Per shape (Llama-3.1-8B: 32 query heads over 8 kv heads, d 128; 32K and 4K tokens; (M 64, C 1024) and (M 32, C 4096); uint16 and
packed; 1 and 8 requests) and n in {2, 4, 8, 16} draft rows, up to four graphs of `inner` back-to-back calls are captured once and
replayed in turn, `rounds` times; the figure is the median replay time over inner (HIP events around the replay), the spread
max - min of the rounds:
  heads      paged_turns.verify(route="heads"): one launch of the wide decode kernel over the 4 n rows of a kv head as query heads,
             then ops.attn_block_merge; the kernel has 16 score columns, so the route (and this graph) exists for n <= 4 only
  chunk      paged_turns.verify(route="chunk"): the chunk attention of the format with the rows as chunk + the staging copies
  decode_n   n one-token decode launches without append: what a caller without verify pays for n tokens
  decode_1   one such launch (the line --decode-only repeats on any tree)
One JSON line per shape and n; profiles/verify_wide.txt keeps a run.

  python tools/verify_wide_bench.py --decode-only
The one-token decode launch at G = 4 alone, every shape: it touches nothing this tool's other modes need, so the same file run on
the parent commit's tree, in a process of its own, is the reference for "the existing instances are untouched".

  python tools/verify_wide_bench.py --commit
ops.window_commit_wide of 4 rows over 32 layers behind a copy that restores the lengths rows, minus that copy alone, in a state in
which no request flushes and in one in which every request does, against what a caller had before: 32 paged_turns.flush launches
(ops.pq_flush_wide with device lengths, gated by min_r) plus the copies of the rows into the windows."""
from __future__ import annotations

import argparse
import json
import sys
from pathlib import Path

sys.path.insert(0, str(Path(__file__).resolve().parents[1]))

import torch  # noqa: E402

from million_amd import ops  # noqa: E402
from million_amd.pq_cache import PagedPQCache  # noqa: E402

D, PS, CAP, R, RS, NH, NHK = 128, 64, 128, 77, 100, 32, 8
CODES = ((64, 10), (32, 12))      # (M, nbits)


def _cache(bs, M, nbits, packed, layers, T, r, rs, max_tokens):
    dev = torch.device("cuda")
    g = torch.Generator(device=dev).manual_seed(0)
    C = 2 ** nbits
    cache = PagedPQCache(bs=bs, nh=NH, num_key_value_heads=NHK, M=M, layer_num=layers, d=D, page_size=PS, extended_residual_size=CAP,
                         max_tokens=max_tokens, nbits=nbits, dtype=torch.uint16, packed=packed)
    cache.set_cent(torch.randn(M, C, D // M, device=dev, generator=g).half(), torch.randn(M, C, D // M, device=dev, generator=g).half())
    # the state is written, not computed: random codes in every page (packed: random bytes - every field is masked with C - 1),
    # random window rows, the lengths of a request T tokens in
    for pool in (cache.key_page_pool, cache.value_page_pool):
        if packed:
            pool.copy_(torch.randint(0, 256, pool.shape, device=dev, dtype=torch.uint8, generator=g))
        else:
            pool.view(torch.int16).copy_(torch.randint(0, C, pool.shape, device=dev, dtype=torch.int16, generator=g))
    cache._kres_all.copy_(torch.randn(cache._kres_all.shape, device=dev, generator=g).half())
    cache._vres_all.copy_(torch.randn(cache._vres_all.shape, device=dev, generator=g).half())
    cache._T_a[:], cache._r_a[:], cache._rs_a[:], cache._seen_a[:] = T, r, rs, T + r
    for l in range(layers):
        cache._sync_lengths(l)
    return cache, g


def _graph(fn, inner):
    for _ in range(3):
        fn()
    torch.cuda.synchronize()
    gr = torch.cuda.CUDAGraph()
    with torch.cuda.graph(gr):
        for _ in range(inner):
            fn()
    gr.replay()
    torch.cuda.synchronize()
    return gr


def _interleaved_us(graphs, rounds, inner):
    """({name: median us per call}, {name: max - min over the rounds}): the graphs replayed in turn, `rounds` times."""
    times = {k: [] for k in graphs}
    for _ in range(rounds):
        for k, gr in graphs.items():
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            gr.replay()
            b.record()
            b.synchronize()
            times[k].append(a.elapsed_time(b) * 1e3 / inner)
    med = lambda v: sorted(v)[len(v) // 2]
    return {k: round(med(v), 2) for k, v in times.items()}, {k: round(max(v) - min(v), 2) for k, v in times.items()}


def _decode_fn(cache, q1, ws):
    fmt = cache._fmt
    return lambda: fmt.decode_pages(q1, cache.key_page_pool, cache.value_page_pool, *cache._cents(), cache.key_residual_cache[0],
                                    cache.value_residual_cache[0], R, M=cache.M, C=cache.C, page_ids=cache.page_ids[0], n_tokens=cache.max_tokens,
                                    resid_start=RS, page_size=PS, dev_lengths=cache.lengths[0], workspace=ws)


def run_decode_only(M, nbits, packed, T, bs, rounds, inner):
    cache, g = _cache(bs, M, nbits, packed, 1, T, R, RS, T + 1024)
    q1 = torch.randn(bs, NH, 1, D, device=cache.device, generator=g).half()
    ws = torch.zeros(ops.decode_wide_workspace_bytes(q1, cache.key_residual_cache[0], M=M, C=cache.C, page_size=PS), dtype=torch.uint8, device=cache.device)
    fn = _decode_fn(cache, q1, ws)
    us, spread = _interleaved_us({"decode_1": _graph(fn, inner), "decode_1_again": _graph(fn, inner)}, rounds, inner)
    return dict(decode_only=True, bs=bs, M=M, C=cache.C, packed=packed, T=T, us=us, spread_us=spread)


def run_attention(M, nbits, packed, T, bs, n, rounds, inner):
    from million_amd import paged_turns
    cache, g = _cache(bs, M, nbits, packed, 1, T, R, RS, T + 1024)
    dev = cache.device
    q = torch.randn(bs, NH, n, D, device=dev, generator=g).half()
    k = torch.randn(bs, NHK, n, D, device=dev, generator=g).half()
    v = torch.randn(bs, NHK, n, D, device=dev, generator=g).half()
    q1 = q[:, :, :1].contiguous()
    ws = torch.zeros(ops.decode_wide_workspace_bytes(q1, cache.key_residual_cache[0], M=M, C=cache.C, page_size=PS), dtype=torch.uint8, device=dev)
    one = _decode_fn(cache, q1, ws)
    fns = {"chunk": lambda: paged_turns.verify(cache, q, k, v, 0, route="chunk"),
           "decode_n": lambda: [one() for _ in range(n)],
           "decode_1": one}
    has_heads = n * NH // NHK <= cache.VERIFY_WIDE_HEADS_ROWS
    oc, rel = fns["chunk"]().float(), None
    if has_heads:
        fns["heads"] = lambda: paged_turns.verify(cache, q, k, v, 0, route="heads")
        rel = ((fns["heads"]().float() - oc).norm() / oc.norm()).item()
    torch.cuda.synchronize()
    rec = cache._verify_rec      # (kept: the captured launches read its dev_n)
    graphs = {name: _graph(fn, inner) for name, fn in fns.items()}
    us, spread = _interleaved_us(graphs, rounds, inner)
    faults = ops.tail_faults()
    assert faults == 0 and rec is not None, f"{faults} split merges gave up"
    out = dict(bs=bs, M=M, C=cache.C, packed=packed, T=T, r=R, n=n, rows_per_kv_head=n * NH // NHK, default_route=cache._verify_route(n), us=us,
               spread_us=spread, chunk_over_decode_n=round(us["chunk"] / us["decode_n"], 3))
    if has_heads:
        out.update(heads_over_chunk=round(us["heads"] / us["chunk"], 3), heads_over_decode_n=round(us["heads"] / us["decode_n"], 3),
                   rel_heads_vs_chunk=float(f"{rel:.2e}"))
    return out


def run_commit(M, nbits, packed, rounds, inner, layers=32, bs=1, n=4):
    out = {}
    for tag, r in (("no_flush", 40), ("flush", CAP - 2)):
        cache, g = _cache(bs, M, nbits, packed, layers, 4096, r, RS, 8192)
        dev = cache.device
        shape = (layers, bs, NHK, 16, D)
        ks, vs = torch.randn(shape, device=dev, generator=g).half(), torch.randn(shape, device=dev, generator=g).half()
        dev_n = torch.full((bs,), n, dtype=torch.int32, device=dev)
        saved = cache._lengths_all.clone()
        cents = cache._cents()[0]

        def reset():
            cache._lengths_all.copy_(saved)

        def commit():
            reset()
            ops.window_commit_wide(ks, vs, cache._kres_all, cache._vres_all, *cents, cache.key_page_pool, cache.value_page_pool,
                                   cache._page_ids_all, cache._lengths_all, dev_n, n_bound=n, packed=packed)

        def per_layer():      # what a caller had: a flush launch per layer where the n rows do not fit (gated on the device), then the rows
            reset()
            for l in range(layers):
                ops.pq_flush_wide(cache.key_residual_cache[l], cache.value_residual_cache[l], *cents, cache.key_page_pool, cache.value_page_pool,
                                  cache.page_ids[l], n=PS, page_size=PS, dev_lengths=cache.lengths[l], min_r=CAP - n + 1, packed=packed)
                cache.key_residual_cache[l][:, :, :n].copy_(ks[l, :, :, :n])
                cache.value_residual_cache[l][:, :, :n].copy_(vs[l, :, :, :n])
        graphs = {"commit": _graph(commit, inner), "per_layer": _graph(per_layer, inner), "reset": _graph(reset, inner)}
        us, spread = _interleaved_us(graphs, rounds, inner)
        graphs["commit"].replay()
        torch.cuda.synchronize()
        out[tag] = dict(r=r, n_accept=n, us=us, spread_us=spread, window_commit_wide_us=round(us["commit"] - us["reset"], 2),
                        per_layer_us=round(us["per_layer"] - us["reset"], 2), lengths_after=cache._lengths_all[0, 0].tolist())
    return dict(commit=True, layers=layers, bs=bs, M=M, C=2 ** nbits, packed=packed, **out)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=11)
    ap.add_argument("--inner", type=int, default=10)
    ap.add_argument("--quick", action="store_true", help="32K, one request, (M 64, C 1024) packed only")
    ap.add_argument("--decode-only", action="store_true", help="the one-token decode launch alone (runs on the parent commit too)")
    ap.add_argument("--commit", action="store_true", help="window_commit_wide over 32 layers against per-layer flushes")
    a = ap.parse_args()
    assert torch.cuda.is_available(), "verify_wide_bench needs the GPU (no CPU timing)"
    shapes = [(M, nbits, packed, T, bs) for T in (32768, 4096) for M, nbits in CODES for packed in (False, True) for bs in (1, 8)]
    if a.quick:
        shapes = [s for s in shapes if s == (64, 10, True, 32768, 1)]
    if a.commit:
        for M, nbits in CODES:
            for packed in (False, True):
                print(json.dumps(run_commit(M, nbits, packed, a.rounds, a.inner)), flush=True)
        return
    for M, nbits, packed, T, bs in shapes:
        if a.decode_only:
            print(json.dumps(run_decode_only(M, nbits, packed, T, bs, a.rounds, a.inner)), flush=True)
            continue
        for n in (2, 4, 8, 16):
            print(json.dumps(run_attention(M, nbits, packed, T, bs, n, a.rounds, a.inner)), flush=True)


if __name__ == "__main__":
    main()
