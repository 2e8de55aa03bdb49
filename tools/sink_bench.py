#!/usr/bin/env python3
"""What the sink rows cost a decode step (PagedPQCache(sink_tokens=S), ops.attn_sink_merge) -> profiles/attn_sink.txt.

Per layer, at the Llama-3.1-8B shape (32 query heads on 8 kv heads, d = 128, M = 64 / 8 bits, 32 layers), 32K coded tokens, 1 and 8
requests, S in {1, 4, 64}:
  step     one decode step of the cache with device lengths, all layers in one hipGraph, replayed: time / layers
  eager    the same step launched from Python (host clock around the steps, ended by a synchronise)
  sink     ops.attn_sink_merge alone, one launch per layer in one hipGraph, replayed: time / layers
The time WITHOUT sinks is taken three times: from a checkout of the parent commit with its own library (--parent DIR:
`git archive <parent> | tar -x -C DIR`, then `python -m million_amd.build` in DIR), from this tree with sink_tokens=0 in a process
that holds nothing else ("alone": the parent's conditions), and from this tree with sink_tokens=0 beside the caches and graphs of
the other variants - in worker processes that alternate between the trees, in alternating order, so that all see the same box in
the same minutes.  Inside a worker the variants alternate window by window.  A window is `--steps` replays between two device events; the table gives the median over all windows of all
rounds and the lowest and highest window.  No GPU: the tool fails, it measures nothing on a CPU.

    python tools/sink_bench.py --parent build/parent --out profiles/attn_sink.txt
"""
import argparse
import json
import statistics
import subprocess
import sys
import time
from pathlib import Path

HERE = Path(__file__).resolve().parents[1]
NH, NHK, D, M, C, PS, CAP, R0 = 32, 8, 128, 64, 256, 64, 128, 17


def worker(a):
    sys.path.insert(0, str(Path(a.root).resolve()))
    import inspect
    import numpy as np
    import torch
    from million_amd import ops
    from million_amd.pq_cache import PagedPQCache
    assert torch.cuda.is_available(), "sink_bench measures on the GPU only"
    assert Path(inspect.getfile(PagedPQCache)).resolve().is_relative_to(Path(a.root).resolve())
    has_sinks = "sink_tokens" in inspect.signature(PagedPQCache.__init__).parameters
    rs = np.random.RandomState(5)
    cents = [torch.from_numpy(rs.standard_normal((M, C, D // M)).astype(np.float16)).cuda() for _ in range(2)]
    L = a.layers
    res = {}
    for bs in a.bs:
        variants = [0] + (list(a.sinks) if has_sinks else [])
        runs = {}
        qs = [torch.randn(bs, NH, 1, D, device="cuda").half() for _ in range(L)]
        kn = [torch.randn(bs, NHK, 1, D, device="cuda").half() for _ in range(L)]
        vn = [torch.randn(bs, NHK, 1, D, device="cuda").half() for _ in range(L)]
        for S in variants:
            c = PagedPQCache(bs=bs, nh=NH, num_key_value_heads=NHK, M=M, layer_num=L, d=D, page_size=PS, extended_residual_size=CAP,
                             max_tokens=a.ctx + 1024, **({"sink_tokens": S} if S else {}))
            c.set_cent(*cents)
            c.key_page_pool.random_(0, 256)
            c.value_page_pool.random_(0, 256)
            c._kres_all.normal_()
            c._vres_all.normal_()
            c.set_host_state(([a.ctx + R0] * L, [R0] * L, [a.ctx] * L, [0] * L))
            for l in range(L):
                c._sync_lengths(l)
            if S:
                c._ksink_all.normal_()
                c._vsink_all.normal_()
                c._note_sinks(slice(None), slice(None), S)
            outs = [torch.empty(bs, NH, 1, D, device="cuda", dtype=torch.float16) for _ in range(L)]

            def step(c=c, outs=outs):
                for l in range(L):
                    c.decoding_with_pages(qs[l], kn[l], vn[l], l, out=outs[l], use_dev_lengths=True)

            st, rows = c.host_state(), c._lengths_all.clone()
            step()      # eager once: workspace, lse buffer, code objects
            torch.cuda.synchronize()
            c.set_host_state(st)
            g = torch.cuda.CUDAGraph()
            with torch.cuda.graph(g):
                step()
            c.set_host_state(st)
            runs[f"step S={S}"] = (g, c, rows, st, step)
            if S:
                lse = [torch.randn(bs, NH, 1, device="cuda") for _ in range(L)]
                gs = torch.cuda.CUDAGraph()

                def sink_only(c=c, outs=outs, lse=lse):
                    for l in range(L):
                        ops.attn_sink_merge(qs[l], c._ksink_all[l], c._vsink_all[l], outs[l], lse[l], dev_s=c._sink_all[l], out=outs[l],
                                            lse_out=lse[l])

                sink_only()
                torch.cuda.synchronize()
                with torch.cuda.graph(gs):
                    sink_only()
                runs[f"sink S={S}"] = (gs, None, None, None, None)
        times = {k: [] for k in runs}
        times.update({k.replace("step", "eager"): [] for k in runs if k.startswith("step")})
        ev = lambda: torch.cuda.Event(enable_timing=True)
        for w in range(a.windows + 1):      # window 0 warms every graph up and is dropped
            for name, (g, c, rows, st, step) in runs.items():
                if c is not None:
                    c._lengths_all.copy_(rows)      # the window grows by one row per replay: every window starts at r = 17
                e0, e1 = ev(), ev()
                e0.record()
                for _ in range(a.steps):
                    g.replay()
                e1.record()
                torch.cuda.synchronize()
                if w:
                    times[name].append(e0.elapsed_time(e1) * 1e3 / (a.steps * L))
                if c is not None and w <= a.eager_windows:
                    c._lengths_all.copy_(rows)
                    c.set_host_state(st)
                    torch.cuda.synchronize()
                    t0 = time.perf_counter()
                    for _ in range(a.steps):
                        step()
                    torch.cuda.synchronize()
                    if w:
                        times[name.replace("step", "eager")].append((time.perf_counter() - t0) * 1e6 / (a.steps * L))
                    c.set_host_state(st)
        res[str(bs)] = times
        del runs
        torch.cuda.empty_cache()
    print("SINK_BENCH " + json.dumps({"root": a.tag, "times_us_per_layer": res}), flush=True)


def fmt(xs):
    return f"{statistics.median(xs):8.2f}  [{min(xs):7.2f} .. {max(xs):7.2f}]  n={len(xs)}" if xs else "     not measured"


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--parent", default=None, help="a checkout of the parent commit with its library built")
    ap.add_argument("--out", default=None)
    ap.add_argument("--bs", type=int, nargs="+", default=[1, 8])
    ap.add_argument("--sinks", type=int, nargs="*", default=[1, 4, 64])
    ap.add_argument("--ctx", type=int, default=32768)
    ap.add_argument("--layers", type=int, default=32)
    ap.add_argument("--steps", type=int, default=50, help="replays per window (the window fills: at most 111)")
    ap.add_argument("--windows", type=int, default=12)
    ap.add_argument("--eager-windows", type=int, default=3)
    ap.add_argument("--rounds", type=int, default=2, help="worker processes per tree, alternating")
    ap.add_argument("--worker", action="store_true")
    ap.add_argument("--root", default=str(HERE))
    ap.add_argument("--tag", default="this")
    a = ap.parse_args()
    if a.steps > CAP - R0:
        ap.error(f"--steps at most {CAP - R0}")
    if a.worker:
        return worker(a)
    # "alone": this tree measured as the parent is - one cache, one graph in the process - so that the two compare like with like
    # (the worker with every variant keeps four caches and seven graphs alive between the windows of sink_tokens=0)
    trees = ([("parent", str(Path(a.parent).resolve()))] if a.parent else []) + [("alone", str(HERE)), ("this", str(HERE))]
    merged = {tag: {} for tag, _ in trees}
    for rnd in range(a.rounds):
        for tag, root in (trees if rnd % 2 == 0 else trees[::-1]):      # the order alternates too: neither tree is always second
            cmd = [sys.executable, str(Path(__file__).resolve()), "--worker", "--root", root, "--tag", tag, "--ctx", str(a.ctx),
                   "--layers", str(a.layers), "--steps", str(a.steps), "--windows", str(a.windows), "--eager-windows", str(a.eager_windows),
                   "--bs", *map(str, a.bs), "--sinks", *map(str, a.sinks if tag == "this" else [])]
            out = subprocess.run(cmd, cwd=root, capture_output=True, text=True, timeout=900)
            if out.returncode != 0:
                sys.stderr.write(out.stdout + out.stderr)
                raise SystemExit(f"sink_bench: the worker of tree '{tag}' failed ({out.returncode}); nothing is reported")
            line = [x for x in out.stdout.splitlines() if x.startswith("SINK_BENCH ")][-1]
            for bs, times in json.loads(line[len("SINK_BENCH "):])["times_us_per_layer"].items():
                for k, v in times.items():
                    merged[tag].setdefault(bs, {}).setdefault(k, []).extend(v)
            print(f"round {rnd} tree {tag}: done", flush=True)
    lines = [f"tools/sink_bench.py: us per layer, median [lowest .. highest window]; {a.layers} layers, nh {NH} / nh_k {NHK}, d {D}, M {M}, "
             f"{a.ctx} coded tokens, window {R0} .. {R0 + a.steps} of {CAP} rows; {a.steps} replays (steps) per window, {a.rounds} worker "
             f"processes per tree, alternating" + ("" if a.parent else "; NO parent tree given: its rows are not measured")]
    for bs in map(str, a.bs):
        lines.append(f"\nbs = {bs}")
        this = merged["this"].get(bs, {})
        par = merged.get("parent", {}).get(bs, {})
        for kind in ("step", "eager"):
            lines.append(f"  {kind + ', parent commit, no sinks':42s} {fmt(par.get(f'{kind} S=0', []))}")
            lines.append(f"  {kind + ', this tree alone, sink_tokens=0':42s} {fmt(merged['alone'].get(bs, {}).get(f'{kind} S=0', []))}")
            lines.append(f"  {kind + ', this tree, sink_tokens=0':42s} {fmt(this.get(f'{kind} S=0', []))}")
            for S in a.sinks:
                xs, base = this.get(f"{kind} S={S}", []), this.get(f"{kind} S=0", [])
                extra = f"   +{statistics.median(xs) - statistics.median(base):.2f} over sink_tokens=0" if xs and base else ""
                lines.append(f"  {kind + f', this tree, sink_tokens={S}':42s} {fmt(xs)}{extra}")
        for S in a.sinks:
            lines.append(f"  {f'sink launch alone, S={S}':42s} {fmt(this.get(f'sink S={S}', []))}")
    text = "\n".join(lines) + "\n"
    print(text)
    if a.out:
        Path(a.out).parent.mkdir(parents=True, exist_ok=True)
        Path(a.out).write_text(text)


if __name__ == "__main__":
    main()
