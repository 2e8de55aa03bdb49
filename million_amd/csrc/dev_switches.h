// dev_switches.h - every development-only switch of the kernels, in one place, compiled out of the product build by
// construction.
//
// The product library (million_amd/build.py, `make bindings`) defines NONE of these: MILLION_EXP is then the constant 0, every
// `#if MILLION_EXP & n` branch is dead text, and no environment variable changes which kernel form runs.  The A/B builds of
// tools/ab_build.py define MILLION_DEV_BUILD together with the switch they measure; a switch without MILLION_DEV_BUILD is a
// build error, so a product object can never carry a path the parity suite has not built.
//
//   MILLION_EXP (bit mask)
//     attn_mfma.hip   2  the last-arriving workgroup merges alone (no helpers)                    profiles/r04_ab_merge.txt
//     attn_tail.h    64  a fused append with device-resident lengths does not advance r: no second-level ticket, no bump
//                        (timing only - what the step form pays for the advance; tools/advance_probe.py)  profiles/ab_decode_advance.txt
//     attn_lean.h   128  a wave's last block is a requesting BLOCK again: it re-requests the wave's last unit (the clamp of
//                        LAUNCH_FRONT_ROUND), as every build did before BLOCK_LAST                  profiles/ab_decode_loadpath.txt
//                  4096  every wave loads its own query operand (Q[], qb) from global memory instead of reading the
//                        workgroup's image in LDS (kQOff)                                           profiles/ab_decode_loadpath.txt
//                  8192  the read-once instances keep the lane = token code requests (partial lines, merged by the L1)
//                 65536  the read-once instances request without the non-temporal hint
//                        (8192: the hint on the old requests - the L1 -> L2 request blow-up, for counters only; 65536: the
//                        whole-line requests alone; 8192 | 65536: the parent's requests in the new instances)  profiles/ab_decode_code_stream.txt
//     attn_stream.h  32"the launch without arithmetic": every request, wait, barrier and the tail stay, a unit's bytes are
//                        xor-ed into a sink instead of gathered, multiplied and soft-maxed         profiles/r04_launch_floor.txt
//     prefill.hip   (the pipelined kernel only; the plain loop's round 3-4 bits are in profiles/r03_prefill.txt, r04_prefill.txt)
//                     4  no value products, 8 no score products
//                   256  no exponentials, 512 no tile DMA behind the prologue, 1024 no tile wait/barrier  profiles/r05_prefill.txt
//                  2048  per-phase shader-clock sums of workgroup 0's waves, written into their own query rows (tools/prefill_prof.py)
//                 16384  only waves 0 - 3 compute (one computing wave per SIMD; its partner issues DMA and joins barriers)
//                 32768  a computing wave sleeps about 17 us (five s_sleep 127; no loop, no memory) between the prologue barrier and
//                        its first read of K half 0: a request into quarter 0 that no barrier holds back lands first, every
//                        time                                                                      profiles/prefill_prologue_race.txt
//   MILLION_TILE_PROF      attn_tile.hip: per-tile shader-clock stamps (tools/tile_prof.py)
//   MILLION_DEV_M32_PACKED() run-time A/B (environment MILLION_M32_PACKED=1, dev builds only): M = 32 keeps the packed value form
//                          at up to 4 query heads per kv head too (the product build takes the d_m = 4 form there and the
//                          packed form above; both are parity-tested through those two ranges)
//
// MILLION_DEBUG_CHECK_IDS is NOT a development switch: it builds the shipped diagnostic variant libmillion_hip_dbgids.so
// (`make debug-ids`, include/million_hip.h), which the parity suite runs (tests/dbgids_child.py, tests/lds_poison_child.py).
// Besides checking page ids, its decode-attention kernels (lean, streaming, tile, scalar) and the chunk kernel fill their
// whole dynamic LDS allocation with 0xFFFF (fp16 NaN) at entry and join a barrier before their first LDS write
// (common.h: debug_fill_lds; the launchers pass the byte count in AttnParams / ChunkParams::lds_fill, fields that only this
// build has): a gather from LDS the kernel never wrote then reads NaN every time instead of an earlier workgroup's data.
#pragma once

#ifndef MILLION_DEV_BUILD
#if defined(MILLION_EXP) || defined(MILLION_TILE_PROF)
#error "MILLION_EXP / MILLION_TILE_PROF are development switches: add -DMILLION_DEV_BUILD (tools/ab_build.py does); the product build defines neither"
#endif
#define MILLION_EXP 0
#define MILLION_DEV_M32_PACKED() 0
#else
#ifndef MILLION_EXP
#define MILLION_EXP 0
#endif
#include <stdlib.h>
#define MILLION_DEV_M32_PACKED() ([] { const char *e = getenv("MILLION_M32_PACKED"); return e && *e == '1' ? 1 : 0; }())
#endif
