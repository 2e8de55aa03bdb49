#!/usr/bin/env python3
"""Development helper: prompt attention (million_prefill_attn, default policy) of TWO builds of the library in one process, same
tensors, alternating rounds (A B A B ...), HIP events, median of the repeats of a round; and the largest difference of their outputs.
    python tools/prefill_ab_libs.py build/ab/libmillion_parent.so million_amd/libmillion_hip.so [--rounds 5] [--n 32768] [--out FILE]
        [--policy 64]   both builds run the plain tile loop at d = 128 (million_set_force_generic(64)) instead of the pipelined one
        [--lse]         a third column: build B's million_prefill_attn_lse on the same tensors, in the same rounds (A B L A B L ...)
A build from before a trailing field of million_prefill_desc (dev_spans) is recognised by the struct_size it accepts; both builds
get the lockstep call (dev_spans = NULL).  Each line ends with the band of the rounds' medians, lowest .. highest, of both builds."""
import argparse
import ctypes
import sys
from pathlib import Path

import torch

sys.path.insert(0, str(Path(__file__).resolve().parents[1]))
from million_amd import _lib as L  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("lib_a")
ap.add_argument("lib_b")
ap.add_argument("--rounds", type=int, default=5)
ap.add_argument("--n", type=int, default=None, help="only the shapes with this many tokens")
ap.add_argument("--out", default=None)
ap.add_argument("--policy", type=int, default=0, choices=[0, 64])
ap.add_argument("--lse", action="store_true")
args = ap.parse_args()
dev = torch.device("cuda", 0)
libs = [ctypes.CDLL(str(Path(p).resolve())) for p in (args.lib_a, args.lib_b)]
for lib in libs:
    lib.million_prefill_attn.restype = ctypes.c_int32
    lib.million_prefill_attn.argtypes = [ctypes.POINTER(L.PrefillDesc)] + [ctypes.c_void_p] * 5
    lib.million_set_force_generic.restype, lib.million_set_force_generic.argtypes = None, [ctypes.c_int32]
    lib.million_set_force_generic(args.policy)
if args.lse:
    libs[1].million_prefill_attn_lse.restype = ctypes.c_int32
    libs[1].million_prefill_attn_lse.argtypes = [ctypes.POINTER(L.PrefillDesc)] + [ctypes.c_void_p] * 6


def desc_bytes(lib):
    """The struct_size this build accepts: today's, or the one without the trailing pointer (n_q = 0 returns before any launch)."""
    for size in (ctypes.sizeof(L.PrefillDesc), ctypes.sizeof(L.PrefillDesc) - 8):
        desc = L.PrefillDesc()
        desc.struct_size, desc.bs, desc.nh, desc.nh_k, desc.d = size, 1, 1, 1, 128
        if lib.million_prefill_attn(ctypes.byref(desc), 16, 16, 16, 16, None) == 0:
            return size
    raise RuntimeError("neither descriptor size is accepted")


sizes = {id(lib): desc_bytes(lib) for lib in libs}


def call(lib, q, k, v, out, lse=None):
    desc = L.PrefillDesc()
    desc.struct_size = sizes[id(lib)]
    desc.bs, desc.nh, desc.n_q, desc.d = q.shape
    desc.nh_k, desc.n_kv, desc.q_pos0, desc.causal = k.shape[1], k.shape[2], 0, 1
    for name, t in (("q", q), ("k", k), ("v", v), ("o", out)):
        for i, ax in enumerate("bhn"):
            setattr(desc, f"{name}_stride_{ax}", t.stride(i))
    if lse is not None:
        rc = lib.million_prefill_attn_lse(ctypes.byref(desc), q.data_ptr(), k.data_ptr(), v.data_ptr(), out.data_ptr(), lse.data_ptr(), None)
    else:
        rc = lib.million_prefill_attn(ctypes.byref(desc), q.data_ptr(), k.data_ptr(), v.data_ptr(), out.data_ptr(), None)
    assert rc == 0, rc


def timed(fn, reps):
    fn()
    torch.cuda.synchronize()
    ts = []
    for _ in range(reps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        torch.cuda.synchronize()
        ts.append(a.elapsed_time(b))
    return sorted(ts)[len(ts) // 2]


lines = [f"A = {args.lib_a}   B = {args.lib_b}   policy {args.policy}   (TFLOP/s = 2 d nh n (n + 1) / time; rounds alternate A, B"
         + (", L = B's million_prefill_attn_lse)" if args.lse else ")")]
# n = 512: short prompts, where what a workgroup does once (prologue, barriers outside the tile loop) weighs most
for (bs, nh, nhk, n) in ((1, 32, 8, 512), (16, 32, 8, 512), (1, 32, 8, 4096), (1, 32, 8, 32768), (1, 32, 32, 32768), (1, 32, 8, 131072)):
    if args.n is not None and n != args.n:
        continue
    d = 128
    q, k, v = (torch.randn(bs, h, n, d, device=dev).half() for h in (nh, nhk, nhk))
    outs = [torch.empty_like(q), torch.empty_like(q)]
    flops = 2.0 * d * nh * bs * n * (n + 1)
    ms = [[], []]
    reps = 100 if n <= 512 else 20 if n <= 4096 else 5 if n <= 32768 else 3
    ms_l, out_l, lse_l = [], torch.empty_like(q) if args.lse else None, torch.empty(bs, nh, n, device=dev) if args.lse else None
    for _ in range(args.rounds):
        for i, lib in enumerate(libs):
            ms[i].append(timed(lambda: call(lib, q, k, v, outs[i]), reps))
        if args.lse:
            ms_l.append(timed(lambda: call(libs[1], q, k, v, out_l, lse_l), reps))
    diff = (outs[0].float() - outs[1].float()).abs().max().item()
    tf = [[flops / t / 1e9 for t in m] for m in ms]
    best = [max(t) for t in tf]
    lines.append(f"n={n:6d} bs={bs:2d} nh_k={nhk:2d}:  A best {best[0]:7.1f} ({' '.join('%.0f' % x for x in tf[0])})   B best {best[1]:7.1f} "
                 f"({' '.join('%.0f' % x for x in tf[1])})   B / A {best[1] / best[0] - 1:+.1%}   max |A - B| {diff:.2e}   "
                 f"bands A {min(tf[0]):.1f} .. {max(tf[0]):.1f}  B {min(tf[1]):.1f} .. {max(tf[1]):.1f}")
    if args.lse:
        tl = [flops / t / 1e9 for t in ms_l]
        lines[-1] += (f"   L best {max(tl):7.1f} ({' '.join('%.0f' % x for x in tl)})   L / B {max(tl) / best[1] - 1:+.1%}   "
                      f"out of L bitwise B's: {torch.equal(out_l.view(torch.int16), outs[1].view(torch.int16))}")
    print(lines[-1], flush=True)
    del q, k, v, outs
    torch.cuda.empty_cache()
if args.out:
    Path(args.out).write_text("\n".join(lines) + "\n")
