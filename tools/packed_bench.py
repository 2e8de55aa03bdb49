#!/usr/bin/env python3
"""One decode layer-call over packed code pages against the same call over uint16 pages -> profiles/attn_packed.txt.

tools/wide_bench.py's shapes and method: the Llama-3.1-8B shape (32 query heads on 8 kv heads, d = 128), 32K coded tokens, a window
of 17 rows, 1 and 8 requests, the code configurations (M 64, C 1024), (M 32, C 4096), (M 64, C 512):
  (w) wide     ops.pq_decode_attn_wide over uint16 pools (csrc/attn_wide.hip, the instances every earlier build has)
  (p) packed   ops.pq_decode_attn_packed over the packed pools that hold the same codes (ops.pq_pack_pages of (w)'s pools)
Both are captured in a hipGraph of their own after an eager warm-up and alternate window by window in one process; a window is
`--steps` replays between two device events, window 0 is dropped.  The two outputs are compared bit for bit first.  Reported: the
median window with the lowest and the highest (the run-to-run spread), (p) / (w) of the medians, whether the two ranges overlap,
and the pool bytes of both.  No bar is set here: the feature stands on its memory.  No GPU: the tool fails.

    python tools/packed_bench.py --out packed_bench.txt      (profiles/attn_packed.txt, part B, holds a run's output)
"""
import argparse
import statistics
import sys
from pathlib import Path

HERE = Path(__file__).resolve().parents[1]
sys.path.insert(0, str(HERE))
NH, NHK, D, PS, CAP, R = 32, 8, 128, 64, 128, 17


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
    from million_amd import ops
    assert torch.cuda.is_available(), "packed_bench measures on the GPU only"
    T = a.ctx
    npc = -(-T // PS)
    lines = [f"tools/packed_bench.py: us per layer-call, median [lowest .. highest window]; nh {NH} / nh_k {NHK}, d {D}, {T} coded tokens, "
             f"window {R} of {CAP} rows, pages of {PS}; {a.steps} replays per window, {a.windows} windows per route, routes alternating"]
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
            kpk, vpk = ops.pq_pack_pages(kp, side="k", C=C), ops.pq_pack_pages(vp, side="v", C=C)
            outs = {k: torch.empty_like(q) for k in "wp"}
            ws = torch.zeros(ops.decode_wide_workspace_bytes(q, kres, M=M, C=C, page_size=PS), dtype=torch.uint8, device="cuda")

            def wide():
                ops.pq_decode_attn_wide(q, kp, vp, kc, vc, kres, vres, R, n_tokens=T, page_ids=ids, page_size=PS, out=outs["w"], workspace=ws)

            def packed():
                ops.pq_decode_attn_packed(q, kpk, vpk, kc, vc, kres, vres, R, n_tokens=T, page_ids=ids, page_size=PS, out=outs["p"], workspace=ws)

            graphs = {}
            for name, fn in (("w", wide), ("p", packed)):
                fn()
                torch.cuda.synchronize()
                g = torch.cuda.CUDAGraph()
                with torch.cuda.graph(g):
                    fn()
                graphs[name] = g
            same = torch.equal(outs["w"].view(torch.int16), outs["p"].view(torch.int16))
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
            tw, tp = times["w"], times["p"]
            apart = min(tp) > max(tw) or min(tw) > max(tp)
            ratio = statistics.median(tp) / statistics.median(tw)
            u16_bytes, pk_bytes = 2 * kp.numel() * 2, 2 * kpk.numel()
            lines += [f"\nbs = {bs}, M = {M}, C = {C} (d_m = {dm}, {ops.packed_hi_bits(C)} high bits per code); outputs bitwise equal: {'yes' if same else 'NO'}",
                      f"  (w) uint16 pages   {fmt(tw)}   pools {u16_bytes / 2 ** 20:7.1f} MiB",
                      f"  (p) packed pages   {fmt(tp)}   pools {pk_bytes / 2 ** 20:7.1f} MiB  ({pk_bytes / u16_bytes:.4f} of (w)'s)",
                      f"  (p) / (w) = {ratio:.3f}; the two ranges {'lie apart: packed is ' + ('slower' if ratio > 1 else 'faster') + ' by more than the spread' if apart else 'overlap: no difference beyond the spread'}"]
            del graphs, kp, vp, kpk, vpk
            torch.cuda.empty_cache()
    text = "\n".join(lines) + "\n"
    print(text)
    if a.out:
        Path(a.out).parent.mkdir(parents=True, exist_ok=True)
        Path(a.out).write_text(text)


if __name__ == "__main__":
    main()
