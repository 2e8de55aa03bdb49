"""The block route of chunk attention (ops.pq_chunk_attn_blocks) against the chunk route (ops.pq_chunk_attn / pq_chunk_attn_wide)
and against the route a user has without either: dequantise the past to fp16, concatenate window and chunk, ops.prefill_attn
(q_pos0 = T + r).  Llama-3.1-8B shape (nh 32, nh_k 8, d 128), M 64 with C 256 (uint8 codes) and C 1024 (uint16 codes), paged
stores of 64-token pages.  HIP events, medians, every shape warmed up.  One JSON line per shape, with the transient bytes of
each route (what it allocates besides its inputs and its output).

  python tools/chunk_blocks_bench.py [--reps 10] [--shapes all|quick] [--block-tokens N]
  python tools/chunk_blocks_bench.py --gather [--reps 20]     the gather kernel alone, one 32K block at bs 1, against torch page
                                                              indexing (PagedPQCache._codes_rowmajor) + ops.pq_decode

Kernel times: run under `rocprofv3 --kernel-trace --stats -- python tools/chunk_blocks_bench.py` (a run of its own)."""
from __future__ import annotations

import argparse
import json
import sys
from pathlib import Path

sys.path.insert(0, str(Path(__file__).resolve().parents[1]))

import torch  # noqa: E402

from million_amd import ops  # noqa: E402

NH, NHK, D, M, PS, CAP, R = 32, 8, 128, 64, 64, 128, 77
N_QS = (64, 256, 512, 1024, 2048, 8192)


def _median_us(fn, reps):
    for _ in range(3):
        fn()
    times = []
    for _ in range(reps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        b.synchronize()
        times.append(a.elapsed_time(b) * 1e3)
    times.sort()
    return times[len(times) // 2], times[0], times[-1]


def _state(bs, n_q, T, C, g):
    dev = torch.device("cuda")
    dt = torch.uint8 if C <= 256 else torch.uint16
    kcent = torch.randn(M, C, D // M, device=dev, generator=g).half()
    vcent = torch.randn(M, C, D // M, device=dev, generator=g).half()
    n_pg = (T + PS - 1) // PS
    rnd = lambda *s: (torch.randint(0, C, s, device=dev, dtype=torch.uint8, generator=g) if C <= 256 else
                      torch.randint(0, C, s, device=dev, dtype=torch.int16, generator=g).view(dt))
    kpool, vpool = rnd(bs * NHK * n_pg, PS, M), rnd(bs * NHK * n_pg, M, PS)
    ids = torch.arange(bs * NHK * n_pg, device=dev, dtype=torch.int32).reshape(bs, NHK, n_pg)
    h = lambda *s: torch.randn(*s, device=dev, generator=g).half()
    return dict(kcent=kcent, vcent=vcent, kpool=kpool, vpool=vpool, ids=ids, n_pg=n_pg, kres=h(bs, NHK, CAP, D), vres=h(bs, NHK, CAP, D),
                q=h(bs, NH, n_q, D), kc=h(bs, NHK, n_q, D), vc=h(bs, NHK, n_q, D))


def _rowmajor(s, bs, T):
    """The row-major codes a user dequantises (the torch page gather of PagedPQCache._codes_rowmajor)."""
    ids = s["ids"].long()
    dt = s["kpool"].dtype
    kpool, vpool = (t.view(torch.int16) if dt == torch.uint16 else t for t in (s["kpool"], s["vpool"]))      # (torch indexes signed types)
    kc = kpool[ids].reshape(bs, NHK, s["n_pg"] * PS, M)[:, :, :T]
    vc = vpool[ids].permute(0, 1, 2, 4, 3).reshape(bs, NHK, s["n_pg"] * PS, M)[:, :, :T]
    return kc.contiguous().view(dt), vc.contiguous().view(dt)


def run_shape(bs, n_q, T, C, reps, block_tokens):
    g = torch.Generator(device="cuda").manual_seed(0)
    s = _state(bs, n_q, T, C, g)
    wide = C > 256
    kp, vp = (s["kcent"], s["vcent"]) if wide else (ops.prepare_cents(s["kcent"], cache=False), ops.prepare_cents(s["vcent"], cache=False))
    kw = dict(M=M, C=C, n_tokens=T, k_page_ids=s["ids"], v_page_ids=s["ids"], page_size=PS)
    args = (s["q"], s["kc"], s["vc"], s["kpool"], s["vpool"], kp, vp, s["kres"], s["vres"], R)
    chunk_op = ops.pq_chunk_attn_wide if wide else ops.pq_chunk_attn
    kcodes, vcodes = _rowmajor(s, bs, T)
    ws_bytes = ops.chunk_blocks_workspace_bytes(bs, NH, NHK, n_q, D, CAP, block_tokens)
    ws = torch.empty(ws_bytes, dtype=torch.uint8, device="cuda")
    out_blocks = torch.empty(bs, n_q, NH, D, dtype=torch.float16, device="cuda").transpose(1, 2)

    def chunk():
        return chunk_op(*args, **kw)

    def blocks():
        return ops.pq_chunk_attn_blocks(*args, block_tokens=block_tokens, out=out_blocks, workspace=ws, **kw)

    def baseline():
        K = torch.cat([ops.pq_decode(kcodes, s["kcent"]), s["kres"][:, :, :R], s["kc"]], dim=2)
        V = torch.cat([ops.pq_decode(vcodes, s["vcent"]), s["vres"][:, :, :R], s["vc"]], dim=2)
        return ops.prefill_attn(s["q"], K, V, causal=True, q_pos0=T + R)

    o_c, o_k, o_b = chunk().float(), blocks().float().clone(), baseline().float()
    torch.cuda.synchronize()
    rel = lambda a, b: float(f"{((a - b).norm() / b.norm()).item():.2e}")
    t_c, t_k, t_b, t_c2 = _median_us(chunk, reps), _median_us(blocks, reps), _median_us(baseline, reps), _median_us(chunk, reps)
    desc = ops.chunk_attn_desc(s["q"], s["kres"], nh_k=NHK, M=M, C=C, n_tokens=T, r=R, n_c=n_q, resid_start=0, k_paged=True, v_paged=True,
                               page_size=PS, n_pages_cap=s["n_pg"], page_ids_i64=False, k_codes=s["kpool"], v_codes=s["vpool"],
                               k_chunk=s["kc"], v_chunk=s["vc"])
    chunk_ws = (ops.chunk_attn_wide_workspace_bytes if wide else ops.chunk_attn_workspace_bytes)(desc)
    n_parts = len(ops.chunk_blocks_plan(T, R, True, block_tokens)["parts"])
    return dict(bs=bs, n_q=n_q, T=T, M=M, C=C, parts=n_parts, block_tokens=block_tokens or ops.CHUNK_BLOCK_TOKENS,
                chunk_us=round(t_c[0], 1), chunk_again_us=round(t_c2[0], 1), blocks_us=round(t_k[0], 1), baseline_us=round(t_b[0], 1),
                chunk_min_max_us=[round(t_c[1], 1), round(t_c[2], 1)], blocks_min_max_us=[round(t_k[1], 1), round(t_k[2], 1)],
                baseline_min_max_us=[round(t_b[1], 1), round(t_b[2], 1)],
                blocks_over_chunk=round(t_k[0] / t_c[0], 3), blocks_over_baseline=round(t_k[0] / t_b[0], 3),
                rel_blocks_vs_chunk=rel(o_k, o_c), rel_blocks_vs_baseline=rel(o_k, o_b),
                transient_bytes=dict(chunk=int(chunk_ws), blocks=int(ws_bytes),
                                     # the row-major copy of the codes, both dequantised pasts and both concatenations
                                     baseline=2 * bs * NHK * T * M * kcodes.element_size() + 2 * bs * NHK * T * D * 2 + 2 * bs * NHK * (T + R + n_q) * D * 2))


def run_gather(reps, C):
    """One block of 32K tokens at bs 1: million_pq_gather_rows from the pages against torch page indexing + pq_decode."""
    bs, T = 1, 32768
    g = torch.Generator(device="cuda").manual_seed(0)
    s = _state(bs, 16, T, C, g)
    k_out = torch.empty(bs, NHK, T + CAP, D, dtype=torch.float16, device="cuda")
    v_out = torch.empty_like(k_out)

    def gather():
        return ops.pq_gather_rows(s["kpool"], s["vpool"], s["kcent"], s["vcent"], k_out, v_out, t0=0, t1=T, k_res=s["kres"], v_res=s["vres"],
                                  r=R, k_page_ids=s["ids"], v_page_ids=s["ids"], page_size=PS)

    def torch_route():
        kc, vc = _rowmajor(s, bs, T)
        return ops.pq_decode(kc, s["kcent"]), ops.pq_decode(vc, s["vcent"])

    n = gather()
    kd, vd = torch_route()
    torch.cuda.synchronize()
    same = torch.equal(k_out[:, :, :T].view(torch.int16), kd.view(torch.int16)) and torch.equal(v_out[:, :, :T].view(torch.int16), vd.view(torch.int16))
    t_g, t_t = _median_us(gather, reps), _median_us(torch_route, reps)
    nbytes = 2 * bs * NHK * T * M * s["kpool"].element_size() + 2 * bs * NHK * n * D * 2 + 2 * bs * NHK * R * D * 2
    return dict(gather=True, bs=bs, T=T, r=R, M=M, C=C, rows=n, gather_us=round(t_g[0], 1), gather_min_max_us=[round(t_g[1], 1), round(t_g[2], 1)],
                torch_index_plus_decode_us=round(t_t[0], 1), bytes=nbytes, gather_GBps=round(nbytes / (t_g[0] * 1e-6) / 1e9, 1),
                bitwise_equal_to_pq_decode=same)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--shapes", default="all", choices=["all", "quick"])
    ap.add_argument("--block-tokens", type=int, default=None)
    ap.add_argument("--gather", action="store_true", help="the gather kernel alone")
    a = ap.parse_args()
    assert torch.cuda.is_available(), "chunk_blocks_bench needs the GPU (no CPU timing)"
    if a.gather:
        for C in (256, 1024):
            print(json.dumps(run_gather(a.reps, C)), flush=True)
        return
    shapes = [(1, n_q, T, C) for C in (256, 1024) for T in (32768, 131072) for n_q in N_QS] + [(4, 2048, T, C) for C in (256, 1024) for T in (32768, 131072)]
    if a.shapes == "quick":
        shapes = [(1, 512, 32768, 256), (1, 2048, 32768, 256), (1, 2048, 32768, 1024)]
    for bs, n_q, T, C in shapes:
        print(json.dumps(run_shape(bs, n_q, T, C, a.reps, a.block_tokens)), flush=True)
        torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
