#!/usr/bin/env python3
"""A block of n_q new tokens against 32K tokens of PQ codes in packed 10- / 12-bit pages, three routes; and the gather of one 32K
block from packed pages against the gather from uint16 pages -> profiles/chunk_attn_packed.txt.

At the Llama-3.1-8B shape (32 query heads on 8 kv heads, d = 128), one request, 32K coded tokens in pages of 64, an empty window,
the block attended causally, for the code configurations (M 64, C 1024: 10 bits) and (M 32, C 4096: 12 bits), n_q in {1, 16, 64}:
  (a) packed   ops.pq_chunk_attn_packed: the launch over the packed pages and its merge
  (b) uint16   ops.pq_chunk_attn_wide over uint16 pages holding the same codes (ops.pq_unpack_pages of the packed pools, once)
  (c) repack   what packed pages had before (a): ops.pq_unpack_pages of the request's live K and V pages into a uint16
               transient (one launch per side, the page-id gather of the live pages in front of it) + ops.pq_chunk_attn_wide
and, once per configuration,
  (g) ops.pq_gather_rows(packed=True) of tokens [0, 32K) against (h) ops.pq_gather_rows over the uint16 pages.
Every route is captured in a hipGraph of its own after an eager warm-up; the routes alternate window by window in one process, a
window is `--steps` replays between two device events, window 0 is dropped.  Reported: the median window, the lowest and the
highest (the run-to-run spread).  No ratio is a condition: for each shape the tool says whether (a) is slower than (b) beyond the
spread - (a)'s lowest window above (b)'s highest - and prints the bytes of the uint16 transient (c) needs.  No GPU: the tool fails.

    python tools/chunk_packed_bench.py --out profiles/chunk_attn_packed.txt
"""
import argparse
import statistics
import sys
from pathlib import Path

HERE = Path(__file__).resolve().parents[1]
sys.path.insert(0, str(HERE))
NH, NHK, D, PS, CAP = 32, 8, 128, 64, 128


def fmt(xs):
    return f"{statistics.median(xs):10.1f}  [{min(xs):9.1f} .. {max(xs):9.1f}]"


def measure(torch, fns, steps, windows):
    """{name: [us per call, one per window]}: each fn warmed up eagerly, captured, the graphs replayed alternately."""
    graphs = {}
    for name, fn in fns.items():
        fn()
        torch.cuda.synchronize()
        g = torch.cuda.CUDAGraph()
        with torch.cuda.graph(g):
            fn()
        graphs[name] = g
    times = {k: [] for k in graphs}
    for w in range(windows + 1):      # window 0 warms every graph up and is dropped
        for name, g in graphs.items():
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            for _ in range(steps):
                g.replay()
            e1.record()
            torch.cuda.synchronize()
            if w:
                times[name].append(e0.elapsed_time(e1) * 1e3 / steps)
    return times


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--out", default=None)
    ap.add_argument("--n-q", type=int, nargs="+", default=[1, 16, 64])
    ap.add_argument("--ctx", type=int, default=32768)
    ap.add_argument("--steps", type=int, default=20, help="replays per window")
    ap.add_argument("--windows", type=int, default=8)
    a = ap.parse_args()
    import torch
    from million_amd import ops
    assert torch.cuda.is_available(), "chunk_packed_bench measures on the GPU only"
    T, bs = a.ctx, 1
    npc = -(-T // PS)
    lines = [f"tools/chunk_packed_bench.py: us per layer-call, median [lowest .. highest window]; 1 request, nh {NH} / nh_k {NHK}, d {D}, "
             f"{T} coded tokens in pages of {PS}, empty window, the block attended causally; {a.steps} replays per window, "
             f"{a.windows} windows per route, routes alternating"]
    slower = []
    for M, C in ((64, 1024), (32, 4096)):
        dm, h = D // M, ops.packed_hi_bits(C)
        kres, vres = torch.zeros(bs, NHK, CAP, D, device="cuda").half(), torch.zeros(bs, NHK, CAP, D, device="cuda").half()
        kc, vc = torch.randn(M, C, dm, device="cuda").half(), torch.randn(M, C, dm, device="cuda").half()
        n_pool = bs * NHK * npc
        ids = torch.randperm(n_pool, device="cuda").to(torch.int32).view(bs, NHK, npc)
        kp = torch.randint(0, C, (n_pool, PS, M), device="cuda", dtype=torch.int16).view(torch.uint16)
        vp = torch.randint(0, C, (n_pool, M, PS), device="cuda", dtype=torch.int16).view(torch.uint16)
        kpk, vpk = ops.pq_pack_pages(kp, side="k", C=C), ops.pq_pack_pages(vp, side="v", C=C)      # the same codes, packed
        # route (c): the live pages gathered and unpacked into a transient, read through the identity table
        live = ids.view(-1).long()
        kt, vt = torch.empty_like(kp), torch.empty_like(vp)
        ident = torch.arange(n_pool, device="cuda", dtype=torch.int32).view(bs, NHK, npc)
        transient = kt.numel() * 2 + vt.numel() * 2
        lines.append(f"\nM = {M}, C = {C} (d_m = {dm}, {8 + h} bits per code): packed pools {2 * kpk.numel() / 2 ** 20:.1f} MiB, uint16 pools "
                     f"{transient / 2 ** 20:.1f} MiB - the transient of route (c), per layer and request")
        for n_q in a.n_q:
            q = torch.randn(bs, NH, n_q, D, device="cuda").half()
            kch, vch = torch.randn(bs, NHK, n_q, D, device="cuda").half(), torch.randn(bs, NHK, n_q, D, device="cuda").half()
            outs = {k: torch.empty_like(q) for k in "abc"}
            desc = ops.chunk_attn_desc(q, kres, nh_k=NHK, M=M, C=C, n_tokens=T, r=0, n_c=n_q, k_paged=True, v_paged=True, page_size=PS,
                                       n_pages_cap=npc)
            need = ops.chunk_attn_wide_workspace_bytes(desc)
            S = need // (bs * NHK * n_q * (NH // NHK) * (D + 2) * 4) if need else 1
            wss = {k: torch.empty(max(need, 16), dtype=torch.uint8, device="cuda") for k in "abc"}
            kw = dict(M=M, C=C, n_tokens=T, page_size=PS)

            def packed():
                ops.pq_chunk_attn_packed(q, kch, vch, kpk, vpk, kc, vc, kres, vres, 0, k_page_ids=ids, v_page_ids=ids, out=outs["a"],
                                         workspace=wss["a"], **kw)

            def uint16():
                ops.pq_chunk_attn_wide(q, kch, vch, kp, vp, kc, vc, kres, vres, 0, k_page_ids=ids, v_page_ids=ids, out=outs["b"],
                                       workspace=wss["b"], **kw)

            def repack():
                ops.pq_unpack_pages(kpk[live], side="k", page_size=PS, M=M, C=C, out=kt)
                ops.pq_unpack_pages(vpk[live], side="v", page_size=PS, M=M, C=C, out=vt)
                ops.pq_chunk_attn_wide(q, kch, vch, kt, vt, kc, vc, kres, vres, 0, k_page_ids=ident, v_page_ids=ident, out=outs["c"],
                                       workspace=wss["c"], **kw)

            t = measure(torch, {"a": packed, "b": uint16, "c": repack}, a.steps, a.windows)
            assert torch.equal(outs["a"].view(torch.int16), outs["b"].view(torch.int16)) and torch.equal(outs["a"].view(torch.int16), outs["c"].view(torch.int16))
            ta, tb, tc = t["a"], t["b"], t["c"]
            is_slower = min(ta) > max(tb)
            if is_slower:
                slower.append((M, C, n_q))
            lines += [f"  n_q = {n_q}: {S} splits",
                      f"    (a) packed launch + merge                   {fmt(ta)}",
                      f"    (b) uint16 launch + merge, same codes       {fmt(tb)}   (a) / (b) = {statistics.median(ta) / statistics.median(tb):.2f}"
                      f"   (a) slower than (b) beyond the spread: {'YES' if is_slower else 'no'}",
                      f"    (c) unpack live pages + uint16 launch       {fmt(tc)}   (c) / (a) = {statistics.median(tc) / statistics.median(ta):.2f}"]
            torch.cuda.empty_cache()
        # the gather of one block of T tokens: what the block route reads per block
        ko, vo = torch.empty(bs, NHK, T, D, device="cuda").half(), torch.empty(bs, NHK, T, D, device="cuda").half()
        ko2, vo2 = torch.empty_like(ko), torch.empty_like(vo)
        g = measure(torch, {"g": lambda: ops.pq_gather_rows(kpk, vpk, kc, vc, ko, vo, t0=0, t1=T, k_page_ids=ids, v_page_ids=ids, page_size=PS, packed=True),
                            "h": lambda: ops.pq_gather_rows(kp, vp, kc, vc, ko2, vo2, t0=0, t1=T, k_page_ids=ids, v_page_ids=ids, page_size=PS)},
                    a.steps, a.windows)
        assert torch.equal(ko.view(torch.int16), ko2.view(torch.int16)) and torch.equal(vo.view(torch.int16), vo2.view(torch.int16))
        is_slower = min(g["g"]) > max(g["h"])
        if is_slower:
            slower.append((M, C, "gather"))
        lines += [f"  gather of tokens [0, {T}), K and V in one launch",
                  f"    (g) from packed pages                       {fmt(g['g'])}",
                  f"    (h) from uint16 pages                       {fmt(g['h'])}   (g) / (h) = {statistics.median(g['g']) / statistics.median(g['h']):.2f}"
                  f"   (g) slower than (h) beyond the spread: {'YES' if is_slower else 'no'}"]
        del kp, vp, kpk, vpk, kt, vt, ko, vo, ko2, vo2
        torch.cuda.empty_cache()
    lines.append(f"\npacked slower than uint16 beyond the run-to-run spread at: {slower if slower else 'no shape'}")
    text = "\n".join(lines) + "\n"
    print(text)
    if a.out:
        Path(a.out).parent.mkdir(parents=True, exist_ok=True)
        Path(a.out).write_text(text)


if __name__ == "__main__":
    main()
