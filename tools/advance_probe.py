#!/usr/bin/env python3
"""Development probe: what does the window-length advance at the end of a fused-append launch with device-resident lengths cost?
(attn_tail.h, "Window-length advance"; profiles/ab_decode_advance.txt).  Times ONE captured graph of 32 x reps launches per call
form (HIP events around a replay, after a warm replay), forms interleaved, at least three rounds:
    plain          million_pq_decode_attn, host lengths, n_tokens = T                      (bench.py's roofline region)
    append         ..._append (new K/V row attended to and stored), host lengths
    devlen         plain + device-resident lengths, n_tokens = the cache's bound
    append+devlen  the step's own form (PagedPQCache.decoding_with_pages)
Unlike tools/mode_probe.py the append+devlen graph holds NOTHING but the attention launches: r starts at --r and grows by one
per launch of a layer (reps launches per layer and replay: it stays far below the 128-row window), and the lengths of every
layer are put back between replays, outside the timed events, by one copy of the cache's _lengths_all.
The library is the one MILLION_HIP_LIB names (tools/ab_build.py 64 = no advance at all), or the in-tree one:
    python tools/advance_probe.py --bs 1 --json out.jsonl ; MILLION_HIP_LIB=build/ab/libmillion_exp64.so python tools/advance_probe.py ...
    python tools/advance_probe.py --summary out.jsonl      (medians, bands and the differences between the libraries)
"""
import argparse
import json
import os
import statistics
import sys
from pathlib import Path

ap = argparse.ArgumentParser()
ap.add_argument("--bs", type=int, default=1)
ap.add_argument("--ctx", type=int, default=32768)
ap.add_argument("--M", type=int, default=64)
ap.add_argument("--layers", type=int, default=32)
ap.add_argument("--reps", type=int, default=8)
ap.add_argument("--r", type=int, default=30)
ap.add_argument("--rounds", type=int, default=3)
ap.add_argument("--tag", default=None, help="name of this library in the record (default: the file name MILLION_HIP_LIB names)")
ap.add_argument("--json", default=None, help="append one JSON line per form to this file")
ap.add_argument("--summary", default=None, help="read such a file and print medians, bands and differences; runs nothing")
a = ap.parse_args()

STEP = "append+devlen (step form)"


def summarise(path):
    recs = [json.loads(x) for x in Path(path).read_text().splitlines() if x.strip()]
    by = {}
    for r_ in recs:
        by.setdefault((r_["bs"], r_["lib"], r_["form"]), []).extend(r_["us"])
    for bs in sorted({k[0] for k in by}):
        print(f"bs={bs}: us per launch, every reading of every process of a library pooled: median (min .. max) [readings]")
        libs = sorted({k[1] for k in by if k[0] == bs})
        for lib in libs:
            for form in [f for (b_, l_, f) in by if b_ == bs and l_ == lib]:
                v = by[(bs, lib, form)]
                print(f"  {lib:28s} {form:28s} {statistics.median(v):7.2f} ({min(v):6.2f} .. {max(v):6.2f}) [{len(v)}]")
        for lib in libs:
            if (bs, lib, STEP) in by and (bs, lib, "plain") in by:
                pl = by[(bs, lib, "plain")]
                print(f"  {lib:28s} step form - plain: {statistics.median(by[(bs, lib, STEP)]) - statistics.median(pl):+6.2f} us"
                      f"   (plain band {min(pl):.2f} .. {max(pl):.2f}, spread {max(pl) - min(pl):.2f})")


if a.summary:
    summarise(a.summary)
    sys.exit(0)

import torch  # noqa: E402

sys.path.insert(0, str(Path(__file__).resolve().parents[1]))
from million_amd import ops  # noqa: E402
from million_amd.pq_cache import PagedPQCache  # noqa: E402

dev = torch.device("cuda", 0)
bs, nh, nhk, d, M, C, ps, cap, layers = a.bs, 32, 8, 128, a.M, 256, 64, 128, a.layers
T0 = a.ctx
assert a.r + a.reps < cap, "r must stay below the window over the graph's launches"
cache = PagedPQCache(bs=bs, nh=nh, num_key_value_heads=nhk, M=M, layer_num=layers, d=d, page_size=ps, extended_residual_size=cap,
                     max_tokens=T0 + 600, device=dev)
g = torch.Generator(device="cpu").manual_seed(1)
cache.set_cent(torch.randn(M, C, d // M, generator=g).half().to(dev), torch.randn(M, C, d // M, generator=g).half().to(dev))
cache.key_page_pool.copy_(torch.randint(0, C, cache.key_page_pool.shape, dtype=torch.uint8, device=dev))
cache.value_page_pool.copy_(torch.randint(0, C, cache.value_page_pool.shape, dtype=torch.uint8, device=dev))
for l in range(layers):
    cache.key_residual_cache[l].copy_(torch.randn(cache.key_residual_cache[l].shape, device=dev).half())
    cache.value_residual_cache[l].copy_(torch.randn(cache.value_residual_cache[l].shape, device=dev).half())
state = ([T0 + a.r] * layers, [a.r] * layers, [T0] * layers, [0] * layers)
cache.set_host_state(state)
q = [torch.randn(bs, nh, 1, d, device=dev).half() for _ in range(layers)]
kn = [torch.randn(bs, nhk, 1, d, device=dev).half() for _ in range(layers)]
vn = [torch.randn(bs, nhk, 1, d, device=dev).half() for _ in range(layers)]
outs = [torch.empty(bs, nh, 1, d, device=dev, dtype=torch.float16) for _ in range(layers)]
cache.decoding_with_pages(q[0], kn[0], vn[0], 0, out=outs[0], use_dev_lengths=False)      # allocates the workspace
cache.set_host_state(state)
for l in range(layers):
    cache._sync_lengths(l)
saved = cache._lengths_all.clone()
kp, vp = cache._kprep, cache._vprep


def call(l, append, devlen):
    ops.pq_decode_attn(q[l], cache.key_page_pool, cache.value_page_pool, kp, vp, cache.key_residual_cache[l],
                       cache.value_residual_cache[l], a.r, M=M, C=C, n_tokens=cache.max_tokens if devlen else T0, resid_start=0,
                       k_page_ids=cache.page_ids[l], v_page_ids=cache.page_ids[l], page_size=ps, out=outs[l],
                       dev_lengths=cache.lengths[l] if devlen else None, workspace=cache._ws,
                       **(dict(k_new=kn[l], v_new=vn[l]) if append else {}))


forms = {"plain": (False, False), "append": (True, False), "devlen": (False, True), STEP: (True, True)}
graphs = {}
for name, (ap_, dl_) in forms.items():
    for l in range(layers):
        call(l, ap_, dl_)
    torch.cuda.synchronize()
    cache._lengths_all.copy_(saved)
    gr = torch.cuda.CUDAGraph()
    with torch.cuda.graph(gr):      # nothing but the launches
        for rep in range(a.reps):
            for l in range(layers):
                call(l, ap_, dl_)
    graphs[name] = gr
n = a.reps * layers
res = {k: [] for k in graphs}
for rnd in range(a.rounds + 1):      # round 0 warms
    for name, gr in graphs.items():
        cache._lengths_all.copy_(saved)      # outside the timed events
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        gr.replay()
        e1.record()
        torch.cuda.synchronize()
        if rnd:
            res[name].append(e0.elapsed_time(e1) * 1e3 / n)
r_end = cache._lengths_all[:, :, 1].cpu().numpy()
faults = ops.tail_faults()
tag = a.tag or os.path.basename(os.environ.get("MILLION_HIP_LIB", "in-tree"))
print(f"{tag}: bs={bs} T={T0} M={M} r={a.r}: one graph of {n} launches per form, us per launch ({a.rounds} rounds, forms interleaved);"
      f" r after the last step-form replay: {int(r_end.min())}..{int(r_end.max())}; tail_faults {faults}")
for name, v in res.items():
    print(f"  {name:28s} " + "  ".join(f"{x:7.2f}" for x in v) + f"   median {statistics.median(v):7.2f}")
    if a.json:
        with open(a.json, "a") as fh:
            fh.write(json.dumps({"lib": tag, "bs": bs, "T": T0, "M": M, "form": name, "us": v, "r_end": [int(r_end.min()), int(r_end.max())],
                                 "tail_faults": faults}) + "\n")
