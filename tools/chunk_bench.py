"""Chunk attention (million_pq_chunk_attn) against the route a user has without it: dequantise the past to fp16, concatenate
window and chunk, ops.prefill_attn(q_pos0 = T + r).  HIP events, medians, every shape warmed up.  One JSON line per shape.

  python tools/chunk_bench.py [--reps 20] [--shapes all|quick]
  python tools/chunk_bench.py --ragged [--reps 20]      four requests at 32K / 24K / 8K / 1K tokens: one ragged launch (A)
      against four batch-1 calls with host lengths (B), and the lockstep call at 4 x 32K without / with device lengths (C)

Kernel times: run under `rocprofv3 --kernel-trace --stats -- python tools/chunk_bench.py` (a run of its own)."""
from __future__ import annotations

import argparse
import json
import sys
from pathlib import Path

sys.path.insert(0, str(Path(__file__).resolve().parents[1]))

import torch  # noqa: E402

from million_amd import ops  # noqa: E402

NH, NHK, D, C, PS, CAP, R = 32, 8, 128, 256, 64, 128, 77
PEAK_BW, PEAK_FLOPS = 8.0e12, 2.5e15


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
    return times[len(times) // 2]


def run_shape(bs, n_q, T, M, reps):
    dev = torch.device("cuda")
    g = torch.Generator(device=dev).manual_seed(0)
    dm = D // M
    kcent = torch.randn(M, C, dm, device=dev, generator=g).half()
    vcent = torch.randn(M, C, dm, device=dev, generator=g).half()
    kp, vp = ops.prepare_cents(kcent, cache=False), ops.prepare_cents(vcent, cache=False)
    n_pg = (T + PS - 1) // PS
    kpool = torch.randint(0, C, (bs * NHK * n_pg, PS, M), device=dev, dtype=torch.uint8, generator=g)
    vpool = torch.randint(0, C, (bs * NHK * n_pg, M, PS), device=dev, dtype=torch.uint8, generator=g)
    ids = torch.arange(bs * NHK * n_pg, device=dev, dtype=torch.int32).reshape(bs, NHK, n_pg)
    kres = torch.randn(bs, NHK, CAP, D, device=dev, generator=g).half()
    vres = torch.randn(bs, NHK, CAP, D, device=dev, generator=g).half()
    q = torch.randn(bs, NH, n_q, D, device=dev, generator=g).half()
    kc = torch.randn(bs, NHK, n_q, D, device=dev, generator=g).half()
    vc = torch.randn(bs, NHK, n_q, D, device=dev, generator=g).half()
    # the baseline's row-major codes (what a user dequantises)
    kcodes = kpool.reshape(bs, NHK, n_pg * PS, M)[:, :, :T].contiguous()
    vcodes = vpool.reshape(bs, NHK, n_pg, M, PS).permute(0, 1, 2, 4, 3).reshape(bs, NHK, n_pg * PS, M)[:, :, :T].contiguous()

    def chunk():
        return ops.pq_chunk_attn(q, kc, vc, kpool, vpool, kp, vp, kres, vres, R, M=M, C=C, n_tokens=T, k_page_ids=ids,
                                 v_page_ids=ids, page_size=PS)

    def baseline():
        K = torch.cat([ops.pq_decode(kcodes, kcent), kres[:, :, :R], kc], dim=2)
        V = torch.cat([ops.pq_decode(vcodes, vcent), vres[:, :, :R], vc], dim=2)
        return ops.prefill_attn(q, K, V, causal=True, q_pos0=T + R)

    out_c, out_b = chunk(), baseline()
    torch.cuda.synchronize()
    rel = ((out_c.float() - out_b.float()).norm() / out_b.float().norm()).item()
    t_c = _median_us(chunk, reps)
    t_b = _median_us(baseline, reps)
    rec = dict(bs=bs, n_q=n_q, T=T, M=M, G=NH // NHK, chunk_us=round(t_c, 2), baseline_us=round(t_b, 2),
               speedup=round(t_b / t_c, 2), rel_vs_baseline=float(f"{rel:.2e}"))
    if n_q == 1:      # the decode launch over the same state (its own append of the one new row)
        kr2, vr2 = kres.clone(), vres.clone()
        q1 = q.contiguous()
        t_d = _median_us(lambda: ops.pq_decode_attn(q1, kpool, vpool, kp, vp, kr2, vr2, R, M=M, C=C, n_tokens=T, k_page_ids=ids,
                                                    v_page_ids=ids, page_size=PS), reps)
        rec["decode_us"] = round(t_d, 2)
    pairs = bs * NH * n_q * (T + R) + bs * NH * n_q * (n_q + 1) // 2
    flops = 4 * D * pairs
    nbytes = 2 * bs * NHK * T * M + 2 * bs * NHK * (R + n_q) * D * 2 + 2 * bs * NH * n_q * D * 2
    t_bw, t_fl = nbytes / PEAK_BW, flops / PEAK_FLOPS
    rec.update(bytes=nbytes, flops=flops, bound="bandwidth" if t_bw >= t_fl else "mfma",
               share_of_peak=round(max(t_bw, t_fl) / (t_c * 1e-6), 3),
               baseline_transient_fp16_bytes=2 * bs * NHK * (T + R + n_q) * D * 2)
    return rec


RAGGED_T = (32768, 24576, 8192, 1024)
RAGGED_RS = 100      # a wrapped window: R rows from ring row 100 of CAP


def run_ragged(n_q, reps, M=64):
    """A: one launch, per-request lengths read on the device.  B: the same work as four batch-1 calls with host lengths (what
    PagedPQCache.extend_request does), each call's median and the four calls timed as one span.  C: the lockstep call at
    4 x 32K, host lengths against the same values in dev_lengths (the cost of the device read)."""
    dev = torch.device("cuda")
    g = torch.Generator(device=dev).manual_seed(0)
    bs, T_max = len(RAGGED_T), max(RAGGED_T)
    kcent = torch.randn(M, C, D // M, device=dev, generator=g).half()
    vcent = torch.randn(M, C, D // M, device=dev, generator=g).half()
    kp, vp = ops.prepare_cents(kcent, cache=False), ops.prepare_cents(vcent, cache=False)
    n_pg = (T_max + PS - 1) // PS
    kpool = torch.randint(0, C, (bs * NHK * n_pg, PS, M), device=dev, dtype=torch.uint8, generator=g)
    vpool = torch.randint(0, C, (bs * NHK * n_pg, M, PS), device=dev, dtype=torch.uint8, generator=g)
    ids = torch.arange(bs * NHK * n_pg, device=dev, dtype=torch.int32).reshape(bs, NHK, n_pg)
    kres = torch.randn(bs, NHK, CAP, D, device=dev, generator=g).half()
    vres = torch.randn(bs, NHK, CAP, D, device=dev, generator=g).half()
    q = torch.randn(bs, NH, n_q, D, device=dev, generator=g).half()
    kc = torch.randn(bs, NHK, n_q, D, device=dev, generator=g).half()
    vc = torch.randn(bs, NHK, n_q, D, device=dev, generator=g).half()
    rows = lambda Ts: torch.tensor([[T, R, RAGGED_RS, 0] for T in Ts], dtype=torch.int32, device=dev)
    dl, dl_lock = rows(RAGGED_T), rows((T_max,) * bs)
    nq = torch.full((bs,), n_q, dtype=torch.int32, device=dev)
    kw = dict(M=M, C=C, page_size=PS)
    one = [tuple(t[b:b + 1] for t in (q, kc, vc, kres, vres, ids)) for b in range(bs)]

    def A():
        return ops.pq_chunk_attn(q, kc, vc, kpool, vpool, kp, vp, kres, vres, 0, n_tokens=T_max, k_page_ids=ids, v_page_ids=ids,
                                 dev_lengths=dl, dev_n_q=nq, **kw)

    def B1(b):
        q1, kc1, vc1, kr1, vr1, id1 = one[b]
        return ops.pq_chunk_attn(q1, kc1, vc1, kpool, vpool, kp, vp, kr1, vr1, R, n_tokens=RAGGED_T[b], resid_start=RAGGED_RS,
                                 k_page_ids=id1, v_page_ids=id1, **kw)

    def B():
        return [B1(b) for b in range(bs)]

    def C_host():
        return ops.pq_chunk_attn(q, kc, vc, kpool, vpool, kp, vp, kres, vres, R, n_tokens=T_max, resid_start=RAGGED_RS,
                                 k_page_ids=ids, v_page_ids=ids, **kw)

    def C_dev():
        return ops.pq_chunk_attn(q, kc, vc, kpool, vpool, kp, vp, kres, vres, 0, n_tokens=T_max, k_page_ids=ids, v_page_ids=ids,
                                 dev_lengths=dl_lock, **kw)

    out_a, out_b = A(), torch.cat(B())
    same_lock = torch.equal(C_host(), C_dev())
    torch.cuda.synchronize()
    rel = ((out_a.float() - out_b.float()).norm() / out_b.float().norm()).item()
    t_a = _median_us(A, reps)
    t_b_each = [_median_us(lambda b=b: B1(b), reps) for b in range(bs)]
    t_b_span = _median_us(B, reps)
    t_ch, t_cd = _median_us(C_host, reps), _median_us(C_dev, reps)
    t_ch2 = _median_us(C_host, reps)      # the host-length call again: this run's own scatter
    return dict(ragged=True, n_q=n_q, T=list(RAGGED_T), r=R, resid_start=RAGGED_RS, M=M, A_one_launch_us=round(t_a, 2),
                B_each_us=[round(t, 2) for t in t_b_each], B_sum_us=round(sum(t_b_each), 2), B_span_us=round(t_b_span, 2),
                A_over_B_sum=round(t_a / sum(t_b_each), 3), A_over_B_max=round(t_a / max(t_b_each), 3),
                C_lockstep_host_us=round(t_ch, 2), C_lockstep_dev_lengths_us=round(t_cd, 2), C_lockstep_host_again_us=round(t_ch2, 2),
                C_bitwise_equal=same_lock, rel_A_vs_B=float(f"{rel:.2e}"))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--ragged", action="store_true", help="the ragged batch against per-request calls (rows A / B / C)")
    ap.add_argument("--shapes", default="all", choices=["all", "quick"])
    a = ap.parse_args()
    assert torch.cuda.is_available(), "chunk_bench needs the GPU (no CPU timing)"
    if a.ragged:
        for n_q in (8, 64):
            print(json.dumps(run_ragged(n_q, a.reps)), flush=True)
        return
    shapes = [(bs, n_q, 32768, 64) for bs in (1, 4) for n_q in (1, 4, 16, 64, 512, 2048)] + [(1, 16, 131072, 32)]
    if a.shapes == "quick":
        shapes = [(1, 16, 32768, 64), (1, 2048, 32768, 64)]
    for s in shapes:
        print(json.dumps(run_shape(*s, a.reps)), flush=True)


if __name__ == "__main__":
    main()
