"""The store step of a ragged batch: ONE ops.pq_store_ragged call (A) against the host-driven per-slot store of
PagedPQCache._store (B: per participating slot K and V of the window in ring order, K and V of the new rows through
ops.pq_encode_into with host values, then the host-to-device copy of the slot's lengths row), in the same process.

Four requests at the Llama-3.1-8B shape (nh_k 8, d 128, M 64, C 256, pages of 64 tokens, a window of 128 rows), (T, r, n):
a long chunk (8192, 77, 2048), a short chunk (4096, 128, 64), an empty slot (0, 0, 512) and a non-participant (1024, 50, 0);
the new rows are padded to 2048.  For each side: the host time to issue the calls (perf_counter around the calls on an idle
device, no synchronisation inside) and the device time to finish (HIP events around them).  `--rounds` repetitions per side,
interleaved A B A B ..., each the median of `--reps` calls; one JSON line with every repetition, the medians and the spread.

  python tools/store_bench.py [--reps 20] [--rounds 3]"""
from __future__ import annotations

import argparse
import json
import sys
import time
from pathlib import Path

sys.path.insert(0, str(Path(__file__).resolve().parents[1]))

import numpy as np  # noqa: E402
import torch  # noqa: E402

from million_amd import _lib as L  # noqa: E402
from million_amd import ops  # noqa: E402

NHK, D, M, C, PS, CAP = 8, 128, 64, 256, 64, 128
REQUESTS = [(8192, 77, 100, 2048), (4096, 128, 64, 64), (0, 0, 0, 512), (1024, 50, 7, 0)]      # (T, r, resid_start, n)
N_PAGES_CAP = 192


def _median(xs):
    xs = sorted(xs)
    return xs[len(xs) // 2]


def _time(fn, reset, reps):
    """(median host microseconds to issue, median device microseconds to finish) of fn(); reset() runs before each call,
    outside both measurements."""
    for _ in range(3):
        reset()
        fn()
    host, dev = [], []
    for _ in range(reps):
        reset()
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        fn()
        host.append((time.perf_counter() - t0) * 1e6)
        torch.cuda.synchronize()
        reset()
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        b.synchronize()
        dev.append(a.elapsed_time(b) * 1e3)
    return _median(host), _median(dev)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--rounds", type=int, default=3)
    a = ap.parse_args()
    assert torch.cuda.is_available(), "store_bench needs the GPU (no CPU timing)"
    dev = torch.device("cuda")
    g = torch.Generator(device=dev).manual_seed(0)
    bs, n_bound = len(REQUESTS), max(r[3] for r in REQUESTS)
    kcent = torch.randn(M, C, D // M, device=dev, generator=g).half()
    vcent = torch.randn(M, C, D // M, device=dev, generator=g).half()
    kp, vp = ops.prepare_cents(kcent, cache=False), ops.prepare_cents(vcent, cache=False)
    n_pool = bs * NHK * N_PAGES_CAP
    pools = {s: (torch.zeros(n_pool, PS, M, device=dev, dtype=torch.uint8), torch.zeros(n_pool, M, PS, device=dev, dtype=torch.uint8)) for s in "AB"}
    ids = torch.randperm(n_pool, device=dev, generator=g).to(torch.int32).reshape(bs, NHK, N_PAGES_CAP)
    kres = torch.randn(bs, NHK, CAP, D, device=dev, generator=g).half()
    vres = torch.randn(bs, NHK, CAP, D, device=dev, generator=g).half()
    k_new = torch.randn(bs, NHK, n_bound, D, device=dev, generator=g).half()
    v_new = torch.randn(bs, NHK, n_bound, D, device=dev, generator=g).half()
    rows0 = torch.tensor([[T, r, s, 0] for T, r, s, _ in REQUESTS], dtype=torch.int32, device=dev)
    lengths = {s: rows0.clone() for s in "AB"}
    dev_n = torch.tensor([r[3] for r in REQUESTS], dtype=torch.int32, device=dev)
    after = [np.array([[T + r + n, 0, 0, 0]], np.int32) for T, r, _, n in REQUESTS]      # B's host rows, as _sync_lengths builds them

    def A():
        ops.pq_store_ragged(k_new, v_new, kres, vres, kp, vp, *pools["A"], ids, lengths["A"], dev_n, M=M, C=C, page_size=PS)

    def B():
        kpool, vpool = pools["B"]
        for b, (T, r, s, n) in enumerate(REQUESTS):
            if n == 0:
                continue
            sl = slice(b, b + 1)
            kw = dict(page_ids=ids[sl], page_size=PS)
            if r:
                ops.pq_encode_into(kres[sl], kcent, kpool, layout=L.MILLION_CODES_KPAGES, prepared=kp, token_start=T, n=r, x_row_start=s, x_row_mod=CAP, **kw)
                ops.pq_encode_into(vres[sl], vcent, vpool, layout=L.MILLION_CODES_VPAGES, prepared=vp, token_start=T, n=r, x_row_start=s, x_row_mod=CAP, **kw)
            ops.pq_encode_into(k_new[sl, :, :n], kcent, kpool, layout=L.MILLION_CODES_KPAGES, prepared=kp, token_start=T + r, n=n, **kw)
            ops.pq_encode_into(v_new[sl, :, :n], vcent, vpool, layout=L.MILLION_CODES_VPAGES, prepared=vp, token_start=T + r, n=n, **kw)
            lengths["B"][sl].copy_(torch.from_numpy(after[b]))

    reset = {s: (lambda s=s: lengths[s].copy_(rows0)) for s in "AB"}
    reset["A"](), A(), reset["B"](), B()
    torch.cuda.synchronize()
    same = bool(torch.equal(pools["A"][0], pools["B"][0]) and torch.equal(pools["A"][1], pools["B"][1]) and torch.equal(lengths["A"], lengths["B"]))
    res = {s: [] for s in "AB"}
    for _ in range(a.rounds):
        for s, fn in (("A", A), ("B", B)):
            res[s].append(_time(fn, reset[s], a.reps))
    out = dict(requests=REQUESTS, n_bound=n_bound, nh_k=NHK, d=D, M=M, C=C, page_size=PS, resid_cap=CAP, reps=a.reps, bitwise_equal=same)
    for s, name in (("A", "A_one_call"), ("B", "B_per_slot")):
        for i, what in enumerate(("host_issue_us", "device_us")):
            xs = [round(r[i], 2) for r in res[s]]
            out[f"{name}_{what}"] = dict(rounds=xs, median=_median(xs), spread=round(max(xs) - min(xs), 2))
    out["A_over_B_device"] = round(out["A_one_call_device_us"]["median"] / out["B_per_slot_device_us"]["median"], 3)
    out["A_over_B_host_issue"] = round(out["A_one_call_host_issue_us"]["median"] / out["B_per_slot_host_issue_us"]["median"], 3)
    print(json.dumps(out), flush=True)


if __name__ == "__main__":
    main()
