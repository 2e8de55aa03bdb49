#!/usr/bin/env python3
"""A block of n_q new tokens against 32K tokens of uint16 PQ codes, three routes -> profiles/chunk_attn_wide.txt.

At the Llama-3.1-8B shape (32 query heads on 8 kv heads, d = 128), one request, 32K coded tokens in pages of 64, an empty window,
the block attended causally, for the code configurations (M 64, C 1024) and (M 32, C 4096) and n_q in {1, 16, 64, 2048}:
  (a) wide     ops.pq_chunk_attn_wide: the launch over the uint16 pages and its merge (csrc/chunk_attn_wide.hip)
  (b) dequant  what these codes had before it: ops.pq_decode of the K and V codes, torch.cat with the block's rows (what
               DynamicPQCache.update returns), ops.prefill_attn(q_pos0 = T) - an O(T) fp16 transient on every call
  (c) uint8    for context only: ops.pq_chunk_attn at the same M with C = 256 (uint8 pages, codebooks in LDS)
Every route is captured in a hipGraph of its own after an eager warm-up; the routes alternate window by window in one process, a
window is `--steps` replays between two device events (a quarter of them at n_q = 2048), window 0 is dropped.  Reported: the
median window, the lowest and the highest (the run-to-run spread), and whether (a) beats (b) by more than the spread - (b)'s
lowest window above (a)'s highest - which is the condition at n_q in {1, 16, 64}; n_q = 2048 is reported without one (every
query block dequantises the past again: the gain there is the absent transient, not time).  No GPU: the tool fails.

    python tools/chunk_wide_bench.py --out chunk_wide_bench.txt        # section 1 of profiles/chunk_attn_wide.txt
"""
import argparse
import statistics
import sys
from pathlib import Path

HERE = Path(__file__).resolve().parents[1]
sys.path.insert(0, str(HERE))
NH, NHK, D, PS, CAP = 32, 8, 128, 64, 128
GATED = (1, 16, 64)


def fmt(xs):
    return f"{statistics.median(xs):10.1f}  [{min(xs):9.1f} .. {max(xs):9.1f}]"


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--out", default=None)
    ap.add_argument("--n-q", type=int, nargs="+", default=[1, 16, 64, 2048])
    ap.add_argument("--ctx", type=int, default=32768)
    ap.add_argument("--steps", type=int, default=20, help="replays per window")
    ap.add_argument("--windows", type=int, default=8)
    a = ap.parse_args()
    import torch
    from million_amd import ops
    assert torch.cuda.is_available(), "chunk_wide_bench measures on the GPU only"
    T, bs = a.ctx, 1
    npc = -(-T // PS)
    lines = [f"tools/chunk_wide_bench.py: us per layer-call, median [lowest .. highest window]; 1 request, nh {NH} / nh_k {NHK}, d {D}, "
             f"{T} coded tokens in pages of {PS}, empty window, the block attended causally; {a.steps} replays per window "
             f"({max(a.steps // 4, 1)} at n_q = 2048), {a.windows} windows per route, routes alternating"]
    verdicts = {}
    for M, C in ((64, 1024), (32, 4096)):
        dm = D // M
        kres, vres = torch.zeros(bs, NHK, CAP, D, device="cuda").half(), torch.zeros(bs, NHK, CAP, D, device="cuda").half()
        kc, vc = torch.randn(M, C, dm, device="cuda").half(), torch.randn(M, C, dm, device="cuda").half()
        n_pool = bs * NHK * npc
        ids = torch.randperm(n_pool, device="cuda").to(torch.int32).view(bs, NHK, npc)
        kp = torch.randint(0, C, (n_pool, PS, M), device="cuda", dtype=torch.int16).view(torch.uint16)
        vp = torch.randint(0, C, (n_pool, M, PS), device="cuda", dtype=torch.int16).view(torch.uint16)
        k_rows = torch.randint(0, C, (bs, NHK, T, M), device="cuda", dtype=torch.int16).view(torch.uint16)      # route (b): row-major codes
        v_rows = torch.randint(0, C, (bs, NHK, T, M), device="cuda", dtype=torch.int16).view(torch.uint16)
        kprep, vprep = ops.prepare_cents(kc[:, :256].contiguous()), ops.prepare_cents(vc[:, :256].contiguous())
        kp8 = torch.randint(0, 256, (n_pool, PS, M), device="cuda", dtype=torch.uint8)
        vp8 = torch.randint(0, 256, (n_pool, M, PS), device="cuda", dtype=torch.uint8)
        for n_q in a.n_q:
            steps = max(a.steps // 4, 1) if n_q >= 2048 else a.steps
            q = torch.randn(bs, NH, n_q, D, device="cuda").half()
            kch, vch = torch.randn(bs, NHK, n_q, D, device="cuda").half(), torch.randn(bs, NHK, n_q, D, device="cuda").half()
            outs = {k: torch.empty_like(q) for k in "ac"}
            desc = ops.chunk_attn_desc(q, kres, nh_k=NHK, M=M, C=C, n_tokens=T, r=0, n_c=n_q, k_paged=True, v_paged=True, page_size=PS,
                                       n_pages_cap=npc)
            need = ops.chunk_attn_wide_workspace_bytes(desc)
            S = need // (bs * NHK * n_q * (NH // NHK) * (D + 2) * 4) if need else 1
            ws = torch.empty(max(need, 16), dtype=torch.uint8, device="cuda")
            ws8 = torch.empty(max(need, 16), dtype=torch.uint8, device="cuda")      # the same function of the descriptor

            def wide():
                ops.pq_chunk_attn_wide(q, kch, vch, kp, vp, kc, vc, kres, vres, 0, M=M, C=C, n_tokens=T, k_page_ids=ids, v_page_ids=ids,
                                       page_size=PS, out=outs["a"], workspace=ws)

            def dequant():
                K = torch.cat([ops.pq_decode(k_rows, kc), kch], dim=2)
                V = torch.cat([ops.pq_decode(v_rows, vc), vch], dim=2)
                return ops.prefill_attn(q, K, V, causal=True, q_pos0=T)

            def uint8():
                ops.pq_chunk_attn(q, kch, vch, kp8, vp8, kprep, vprep, kres, vres, 0, M=M, C=256, n_tokens=T, k_page_ids=ids, v_page_ids=ids,
                                  page_size=PS, out=outs["c"], workspace=ws8)

            graphs = {}
            for name, fn in (("a", wide), ("b", dequant), ("c", uint8)):
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
                    for _ in range(steps):
                        g.replay()
                    e1.record()
                    torch.cuda.synchronize()
                    if w:
                        times[name].append(e0.elapsed_time(e1) * 1e3 / steps)
            ta, tb, tc = times["a"], times["b"], times["c"]
            beats = min(tb) > max(ta)
            if n_q in GATED:
                verdicts[(M, C, n_q)] = beats
            lines += [f"\nM = {M}, C = {C} (d_m = {dm}), n_q = {n_q}: {S} splits, {-(-n_q * (NH // NHK) // 256)} query block(s) per kv head",
                      f"  (a) wide launch + merge              {fmt(ta)}",
                      f"  (b) pq_decode + cat + prefill_attn   {fmt(tb)}   (b) / (a) = {statistics.median(tb) / statistics.median(ta):.2f}",
                      f"  (c) uint8 launch + merge, C = 256    {fmt(tc)}   (a) / (c) = {statistics.median(ta) / statistics.median(tc):.2f}  (not gated)",
                      f"  (a)'s highest window below (b)'s lowest: {'yes' if beats else 'NO'}" + ("" if n_q in GATED else "  (reported, no condition at this size)")]
            del graphs
            torch.cuda.empty_cache()
        del k_rows, v_rows, kp, vp, kp8, vp8
        torch.cuda.empty_cache()
    failed = [k for k, v in verdicts.items() if not v]
    lines.append(f"\nthe condition - (a)'s highest window below (b)'s lowest at n_q in {GATED} for both shapes: "
                 f"{'met' if not failed else 'NOT met at (M, C, n_q) = ' + str(failed)}")
    text = "\n".join(lines) + "\n"
    print(text)
    if a.out:
        Path(a.out).parent.mkdir(parents=True, exist_ok=True)
        Path(a.out).write_text(text)


if __name__ == "__main__":
    main()
