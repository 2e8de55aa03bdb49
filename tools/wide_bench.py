#!/usr/bin/env python3
"""One decode layer-call over uint16 PQ codes, three routes -> profiles/attn_wide.txt.

At the Llama-3.1-8B shape (32 query heads on 8 kv heads, d = 128), 32K coded tokens, a window of 17 rows, 1 and 8 requests, for the
code configurations (M 64, C 1024), (M 32, C 4096), (M 64, C 512):
  (a) wide     ops.pq_decode_attn_wide: the fused launch over the uint16 pages (csrc/attn_wide.hip)
  (b) dequant  what a user of these codes had before it: ops.pq_decode of the K and V codes, torch.cat with the window rows (as
               PagedPQCache.update / DynamicPQCache.update return them), repeat_kv, torch scaled_dot_product_attention
  (c) uint8    for context only: ops.pq_decode_attn at the same M with C = 256 (uint8 pages, codebooks in LDS)
Every route is captured in a hipGraph of its own after an eager warm-up; the routes alternate window by window in one process, a
window is `--steps` replays between two device events, window 0 is dropped.  Reported: the median window, the lowest and the
highest (the run-to-run spread), (a)'s achieved fraction of the HBM peak counted on code bytes alone (2 sides x bs x nh_k x T x M
x 2 bytes; the table gathers hit L2 / the Infinity Cache and are not counted), and whether (a) beats (b) by more than the
spread - (b)'s lowest window above (a)'s highest.  No GPU: the tool fails, it measures nothing on a CPU.

    python tools/wide_bench.py --out profiles/attn_wide.txt
"""
import argparse
import statistics
import sys
from pathlib import Path

HERE = Path(__file__).resolve().parents[1]
sys.path.insert(0, str(HERE))
NH, NHK, D, PS, CAP, R = 32, 8, 128, 64, 128, 17
HBM_PEAK = 8.0e12      # bytes / s, MI355X data sheet


def fmt(xs):
    return f"{statistics.median(xs):9.1f}  [{min(xs):8.1f} .. {max(xs):8.1f}]"


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--out", default=None)
    ap.add_argument("--bs", type=int, nargs="+", default=[1, 8])
    ap.add_argument("--ctx", type=int, default=32768)
    ap.add_argument("--steps", type=int, default=20, help="replays per window")
    ap.add_argument("--windows", type=int, default=8)
    a = ap.parse_args()
    import torch
    import torch.nn.functional as F
    from million_amd import ops
    assert torch.cuda.is_available(), "wide_bench measures on the GPU only"
    T, G = a.ctx, NH // NHK
    npc = -(-T // PS)
    lines = [f"tools/wide_bench.py: us per layer-call, median [lowest .. highest window]; nh {NH} / nh_k {NHK}, d {D}, {T} coded tokens, "
             f"window {R} of {CAP} rows, pages of {PS}; {a.steps} replays per window, {a.windows} windows per route, routes alternating; "
             f"HBM peak taken as {HBM_PEAK / 1e12:.1f} TB/s"]
    verdicts = []
    for bs in a.bs:
        for M, C in ((64, 1024), (32, 4096), (64, 512)):
            dm = D // M
            q = torch.randn(bs, NH, 1, D, device="cuda").half()
            kres, vres = torch.randn(bs, NHK, CAP, D, device="cuda").half(), torch.randn(bs, NHK, CAP, D, device="cuda").half()
            kc, vc = torch.randn(M, C, dm, device="cuda").half(), torch.randn(M, C, dm, device="cuda").half()
            n_pool = bs * NHK * npc
            ids = torch.randperm(n_pool, device="cuda").to(torch.int32).view(bs, NHK, npc)
            kp = torch.randint(0, C, (n_pool, PS, M), device="cuda", dtype=torch.int16).view(torch.uint16)
            vp = torch.randint(0, C, (n_pool, M, PS), device="cuda", dtype=torch.int16).view(torch.uint16)
            k_rows = torch.randint(0, C, (bs, NHK, T, M), device="cuda", dtype=torch.int16).view(torch.uint16)      # route (b): row-major codes
            v_rows = torch.randint(0, C, (bs, NHK, T, M), device="cuda", dtype=torch.int16).view(torch.uint16)
            kc8, vc8 = kc[:, :256].contiguous(), vc[:, :256].contiguous()
            kprep, vprep = ops.prepare_cents(kc8), ops.prepare_cents(vc8)
            kp8 = torch.randint(0, 256, (n_pool, PS, M), device="cuda", dtype=torch.uint8)
            vp8 = torch.randint(0, 256, (n_pool, M, PS), device="cuda", dtype=torch.uint8)
            outs = {k: torch.empty_like(q) for k in "ac"}
            ws = torch.zeros(ops.decode_wide_workspace_bytes(q, kres, M=M, C=C, page_size=PS), dtype=torch.uint8, device="cuda")
            ws8 = torch.zeros(ops.decode_workspace_bytes(q, kres, nh_k=NHK, M=M, C=256), dtype=torch.uint8, device="cuda")

            def wide():
                ops.pq_decode_attn_wide(q, kp, vp, kc, vc, kres, vres, R, n_tokens=T, page_ids=ids, page_size=PS, out=outs["a"], workspace=ws)

            def dequant():
                K = torch.cat([ops.pq_decode(k_rows, kc), kres[:, :, :R]], dim=2)
                V = torch.cat([ops.pq_decode(v_rows, vc), vres[:, :, :R]], dim=2)
                rep = lambda x: x[:, :, None].expand(bs, NHK, G, T + R, D).reshape(bs, NH, T + R, D)      # repeat_kv
                return F.scaled_dot_product_attention(q, rep(K), rep(V))

            def uint8():
                ops.pq_decode_attn(q, kp8, vp8, kprep, vprep, kres, vres, R, M=M, C=256, n_tokens=T, k_page_ids=ids, v_page_ids=ids,
                                   page_size=PS, out=outs["c"], workspace=ws8)

            graphs = {}
            for name, fn in (("a wide", wide), ("b dequant", dequant), ("c uint8", uint8)):
                fn()
                torch.cuda.synchronize()
                g = torch.cuda.CUDAGraph()
                with torch.cuda.graph(g):
                    fn()
                graphs[name] = g
            times = {k: [] for k in graphs}
            for w in range(a.windows + 1):      # window 0 warms every graph up and is dropped
                for name, g in graphs.items():
                    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                    e0.record()
                    for _ in range(a.steps):
                        g.replay()
                    e1.record()
                    torch.cuda.synchronize()
                    if w:
                        times[name].append(e0.elapsed_time(e1) * 1e3 / a.steps)
            ta, tb, tc = (times[k] for k in ("a wide", "b dequant", "c uint8"))
            code_bytes = 2 * bs * NHK * T * M * 2
            frac = code_bytes / (statistics.median(ta) * 1e-6) / HBM_PEAK
            beats = min(tb) > max(ta)
            verdicts.append(beats)
            lines += [f"\nbs = {bs}, M = {M}, C = {C} (d_m = {dm}; splits per (b, kv head): "
                      f"{ops.attn_wide_splits(ops.wide_attn_desc('wide_bench', q, kp, vp, kc, vc, kres, vres, R, T, ids, PS, 0, None))})",
                      f"  (a) wide fused launch            {fmt(ta)}   {frac * 100:5.1f} % of the HBM peak on {code_bytes / 2 ** 20:.0f} MiB of code bytes",
                      f"  (b) pq_decode + cat + SDPA       {fmt(tb)}   (b) / (a) = {statistics.median(tb) / statistics.median(ta):.2f}",
                      f"  (c) uint8 launch, C = 256        {fmt(tc)}   (a) / (c) = {statistics.median(ta) / statistics.median(tc):.2f}  (not gated)",
                      f"  (a) beats (b) by more than the spread: {'yes' if beats else 'NO'}"]
            del graphs, k_rows, v_rows, kp, vp, kp8, vp8
            torch.cuda.empty_cache()
    lines.append(f"\nthe condition - (a) beats (b) at every measured shape by more than the run-to-run spread: "
                 f"{'met' if all(verdicts) else 'NOT met at ' + str(verdicts.count(False)) + ' of ' + str(len(verdicts)) + ' shapes'}")
    text = "\n".join(lines) + "\n"
    print(text)
    if a.out:
        Path(a.out).parent.mkdir(parents=True, exist_ok=True)
        Path(a.out).write_text(text)


if __name__ == "__main__":
    main()
