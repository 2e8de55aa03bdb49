// attn_mfma.hip — fused decode attention over PQ code pages on the matrix cores: d = 128 with M = 64 / 32 / 16 and (lean
// kernel) d = 64, C = 256 / 128, transposed V pages, hand-written for gfx950 / CDNA4.
//
// Replaces (one launch): the LUT matmul + flash_decoding_split_kernel + flash_decoding_residual_kernel
// + torch::zeros + flash_decoding_reduce_kernel of the reference (Interface.template.cu:26-120,
// Kernel.cuh:11-166, 1038-1270), and the intended paged-V kernel (MILLION_技术分析文档.md:1292-1345).
//
// Design (DESIGN.md "decode attention kernel"):
//   * one 512-thread workgroup per CU; both codebooks live in LDS for the whole kernel:
//       K table, row image [m][c] (4-byte entries): bank = code  -> random gather
//       V table, col image [c][m] (4-byte entries): bank = m     -> conflict-free gather (lane = m)
//   * all G = nh/nh_k query heads of a kv head are served by the same workgroup, so every code byte is
//     read from HBM once per kv head (the reference re-reads it G times);
//   * a wave walks 32-token units.  K side: lane = (token, 16-byte quarter of the code row); each code
//     byte fetches its 2-dim centroid from LDS straight into the A operand of
//     v_mfma_f32_16x16x32_f16 (rows = 16 tokens, K = 32 dims), B = the query heads -> fp32 scores with
//     exact fp16 centroids (no fp16 LUT rounding).  V side: lane = subspace m; 16 consecutive token
//     bytes of a transposed page row are one 16-byte load; the looked-up centroids are the B operand of
//     v_mfma_f32_32x32x16_f16 (K = 16 tokens, cols = 32 subspaces) - as gathered at M = 64 ("parity-V"), packed by v_perm
//     at M = 32 - and A = the probabilities of the G heads, moved from the score layout with v_permlane16_swap;
//   * online softmax per wave in the exp2 domain, fp32; wave partials are merged through LDS, split
//     partials through the workspace by the last-arriving workgroup (attn_tail.h: merge_and_publish);
//   * the residual window (r <= 128 fp16 rows) is dealt round-robin to the splits and, inside a split, to its
//     waves: each wave's rows are ONE 16-row MFMA tile (scores: A = the fp16 K rows; values: B = the fp16 V rows)
//     that the wave runs before its code units - no separate partial, no scalar FMA loop.
//   * round 4: M = 16 (d_m = 8) and M = 32 at G <= 4 run the streaming kernel in the "d_m = 8 / 4 forms" (see there): the query
//     heads are replicated over the four column groups of the score tile, a gathered codebook entry is a lane's reduction slots of
//     a 16x16x32 operand as it stands (K: A operand, V: B operand), 8 accumulator registers, no pack and no lane movement;
//   * two kernels share everything above and the merge tail: attn_stream_kernel (value steps of unit u interleaved with the
//     score stages of unit u + 1, online softmax per unit, up to 64 rounds per wave) and attn_lean_kernel (attn_lean.h:
//     64-token units, lane = token, up to 4 query heads per kv head).  plan_attn_mfma leaves what neither takes - T = 0,
//     more than 64 rounds per wave - to the tile kernel (attn_tile.hip).
//
// This file is the translation unit: the LDS layout, the split policy, the instance table and the planner.  The device code is in
// the headers it includes below, in this order: decode_wave.h (what every wave uses: LDS reads, reductions, online softmax, the
// residual-window tile), attn_tail.h (the split merge), attn_front.h (the launch front: workgroup placement, page walk, lengths,
// fused append - the contract with plan_attn_mfma), attn_stream.h and attn_lean.h (the two kernels).
#include <type_traits>

#include "common.h"
#include "dev_switches.h"      // MILLION_EXP (0 in the product build) and the other development A/B switches

namespace million {

constexpr int kNW = 8;                       // waves per workgroup
constexpr int kRing = 4;                     // 32-token units in flight per wave (16 VGPRs each)
constexpr int kTabBytes = 64 * 1024;         // one codebook image (M*C*dm*2)
constexpr int kVBase = kTabBytes;            // V col image behind the K row image
constexpr int kPartOff = 2 * kTabBytes;      // [128K,136K): final partial, flag
constexpr int kStampOff = kPartOff + 8192;   // [136K,138K): diagnostic stamps (only touched when a stamp buffer is set)
constexpr int kQOff = kStampOff + kStampWaves * kStampSlots * 8;      // [138K,139K): the (b, kv head)'s query rows (lean kernel: G x d fp16, <= 1 KiB)
constexpr int kLdsBytes = kQOff + 1024;      // 139 KiB
constexpr int kResRows = 16;                 // residual-window rows per wave (one MFMA tile): 8 waves x 16 = 128 rows per split

#include "decode_wave.h"     // wave helpers, online softmax, the residual-window tile: both kernels and the tail
#include "attn_tail.h"       // merge_and_publish: wave partials -> the split's partial -> the merge over the splits
#include "attn_front.h"      // the launch front: workgroup placement, page walk, lengths, fused append - the contract with the planner below
#include "attn_stream.h"     // attn_stream_kernel
#include "attn_lean.h"       // attn_lean_kernel (round 5): the MFMA-lean core on the same launch skeleton and tail

// Self-check of the row-swap reductions (tests/test_gpu_parity.py): one wave, in[64] -> max / sum over the
// four 16-lane rows per column.
__global__ void rows_reduce_check_kernel(const float *in, float *out_max, float *out_sum) {
    const float x = in[threadIdx.x];
    out_max[threadIdx.x] = rows_max(x);
    out_sum[threadIdx.x] = rows_sum(x);
}
int launch_rows_reduce_check(const float *in, float *out_max, float *out_sum, hipStream_t s) {
    hipLaunchKernelGGL(rows_reduce_check_kernel, dim3(1), dim3(64), 0, s, in, out_max, out_sum);
    return hipGetLastError() == hipSuccess ? MILLION_OK : MILLION_ERR_LAUNCH;
}

// A split takes every nsplit-th window row and has kNW * kResRows = 128 slots for them in its waves' residual tiles:
// windows of up to 128 rows work with any split count, longer ones (extended_residual_size 256, the reference's
// flash_decoding_paged_v_*_Lt256 names) get at least ceil(rcap / 128) splits (mfma_splits).
// d = 64 with M = 32 / 16 (d_m = 2 / 4) and M = 64 (d_m = 1: run as d_m = 2 with every odd dim zero, attn_lean.h): the lean kernel
// only (round 5; before: the tile kernel) - 256 centroids, up to 4 query heads per kv head
static int g_tail_test = 0, g_lean_off = 0;      // test and A/B knobs: see set_mfma_policy below
// 5 .. 16 query heads per kv head: the launch runs ceil(G / 4) VIRTUAL kv heads of ceil(G / parts) heads per real one (AttnParams::nhk_real;
// the parts re-read the codes - from the XCD's L2 when they run together: the parts of a real head sit on one XCD).  The workspace
// head is laid out for max(2048, bs * nh_k) pairs (million_api.hip): the virtual pairs must fit it.
static int mfma_hparts(const AttnParams &p) {      // (the lean kernel's d = 64 forms and the streaming kernel's d = 128 / M = 16 form)
    if (!(p.d == 64 || (p.d == 128 && p.M == 16)) || p.nhk_mul || g_lean_off) return 1;      // (policy 16: no parts either - the tile kernel)
    const int P = p.G > 4 && p.G <= 16 ? (p.G + 3) / 4 : 1;      // 5 .. 8 heads: 2 parts, 9 .. 12: 3, 13 .. 16: 4
    return (P > 1 && (long long)p.bs * p.nh_k * P <= 2048) ? P : 1;
}
static AttnParams mfma_virtual(const AttnParams &p_in) {      // the call as the lean kernel sees it
    AttnParams p = p_in;
    const int P = mfma_hparts(p);
    if (P > 1) {
        p.nhk_real = p.nhk_mul = p.nh_k;
        p.hparts_m1 = P - 1;
        p.nh_k *= P;
        p.G_all = p.G;
        p.G = (p.G + P - 1) / P;      // 3 or 4 heads per part; the last part: G_all - (P - 1) G >= 1
        p.slot_floats = (p.G * p.d + 2 * p.G + 31) / 32 * 32;      // = slot_floats_for (million_api.hip)
    }
    return p;
}
static bool lean_d64_shape(const AttnParams &p) {
    return p.d == 64 && (p.M == 64 || p.M == 32 || p.M == 16) && (p.C == 256 || p.C == 128) && (p.G <= 4 || mfma_hparts(p) > 1) && p.rcap <= 4 * kNW * kResRows;
}
static bool mfma_shape_ok(const AttnParams &p) {
    if (lean_d64_shape(p)) return true;
    if (p.d == 128 && p.M == 16)      // d_m = 8 form of the streaming kernel (round 4): up to 4 query heads per kv head (5 .. 16: as parts)
        return (p.C == 256 || p.C == 128) && (p.G <= 4 || mfma_hparts(p) > 1) && p.rcap <= 4 * kNW * kResRows;
    return p.d == 128 && (p.M == 64 || p.M == 32) && (p.C == 256 || p.C == 128) && p.G <= kMaxGMfma && p.rcap <= 4 * kNW * kResRows;
}

// host side of g_tail_faults: waits for the device, returns and clears the count (-1: the runtime refused)
int read_tail_faults() {
    unsigned n = 0, zero = 0;
    if (hipDeviceSynchronize() != hipSuccess) return -1;
    if (hipMemcpyFromSymbol(&n, HIP_SYMBOL(g_tail_faults), sizeof(n)) != hipSuccess) return -1;
    if (n && hipMemcpyToSymbol(HIP_SYMBOL(g_tail_faults), &zero, sizeof(zero)) != hipSuccess) return -1;
    return (int)n;
}

// g_tail_test (million_set_force_generic 4 / 8): the merge helpers give up at once - the last arriver's take-over path, for
// tests: 1 = every give-up bit is set in the prologue, 2 = the helpers give up through the real path (no polls, then the atomic)
// g_lean_off (million_set_force_generic 16): the lean kernel's shapes stay on the streaming kernel (A/B, tests of the parity-V form)
// development A/B (dev_switches.h; environment MILLION_M32_PACKED=1 in a MILLION_DEV_BUILD): M = 32 keeps the packed form at G <= 4
// too.  The constant 0 in the product build.
static const int g_mfma_form = MILLION_DEV_M32_PACKED();
void set_mfma_policy(int policy) { g_tail_test = policy & 3; g_lean_off = (policy >> 2) & 1; }

// split policy: about one workgroup per CU; a split is at least 512 tokens long
// (tests/test_decode_advance.py: _mfma_grid restates this rule - without the 64-round extension - to assert that its bs = 5 shape
//  exceeds the chip, i.e. runs with nmerge = 1; the plan cannot be queried through the C ABI.  Change both together.)
static int mfma_splits(const AttnParams &p, int cus) {
    const int bh = p.bs * p.nh_k;
    int ns = (cus + bh - 1) / bh;
    if (ns > kMaxSplits) ns = kMaxSplits;
    const int by_len = p.T > 0 ? (p.T + 511) / 512 : 1;
    if (ns > by_len) ns = by_len;
    if (ns < 1) ns = 1;
    // the kernels deal whole 32-token units to the splits (first units % ns splits carry one more): len = the longest
    const int units = p.T > 0 ? (p.T + 31) / 32 : 1;
    if (ns > units) ns = units;
    const int ns_window = (p.rcap + kNW * kResRows - 1) / (kNW * kResRows);      // splits the residual window needs
    if (ns < ns_window) ns = ns_window;      // (a split beyond the last unit just has no code units)
    // The streaming kernel preloads the page ids of a wave's first 64 rounds (one vector load, lane = round): a call with more
    // rounds per wave - many (b, kv head) pairs AND a long context, e.g. 16 requests x 8 kv heads at 40K tokens - gets more
    // splits (round 4; rounds 2-3 dropped such calls to a slower fallback).  The grid then holds more workgroups than CUs; the
    // tail's single merger waits only for workgroups that have started, so any dispatch order is fine.  64 splits x 64 rounds
    // x 256 tokens = 1M tokens per (b, kv head); longer calls go to the tile kernel (plan_attn_mfma).
    if (p.T > 0 && (p.T + ns * 256 - 1) / (ns * 256) > 64) {
        while (ns < kMaxSplits && (p.T + ns * 256 - 1) / (ns * 256) > 64) ++ns;
        // more workgroups than CUs now: prefer a grid that is a whole number of chip-fulls (128 pairs: 4 splits = 2 x 256
        // workgroups of 40 rounds instead of 3 splits = 256 + 128 of 53), if that costs at most twice the splits
        for (int n2 = ns; n2 <= 2 * ns && n2 <= kMaxSplits; ++n2)
            if ((long long)bh * n2 % cus == 0) { ns = n2; break; }
    }
    return ns;
}
// streaming kernel: rounds per wave = ceil(T / (ns * 256 tokens)) must fit the 64 page ids a wave preloads
static bool mfma_stream_ok(const AttnParams &p, int ns) { return p.T > 0 && (p.T + ns * 256 - 1) / (ns * 256) <= 64; }

// The instances this file launches, by form and layout mode (0: paged K with int32 ids and V through its id table, 1: row-major
// K with dense V pages, 2: anything else, 3: mode 0 as a read-once launch - 64-token pages, one part per kv head: the lean kernel's
// whole-line code requests with the non-temporal hint, attn_lean.h; the streaming kernel has no such form: its mode 0 instance).
// The C = 128 forms have one instance for every mode.  The rows
// keep the order in which the instances were first named before this table: it is their order in the code object.
enum MfmaForm {
    kStream64, kStream32, kStream32D4, kStream16,                       // streaming kernel (D4: the d_m = 4 form of M = 32; M = 16: d_m = 8)
    kStream16C128, kStream64C128, kStream32C128,
    kLean64, kLean64C128, kLean32, kLean32C128,                         // lean kernel, d = 128
    kLeanD64M32, kLeanD64M16, kLeanD64M64,                              // lean kernel, d = 64
    kMfmaForms
};
#define MFMA_ONE(...) {(const void *)__VA_ARGS__, (const void *)__VA_ARGS__, (const void *)__VA_ARGS__, (const void *)__VA_ARGS__}
static const void *const kMfmaKernels[kMfmaForms][4] = {
    {(const void *)attn_stream_kernel<64, 0>, (const void *)attn_stream_kernel<64, 1>, (const void *)attn_stream_kernel<64, 2>, (const void *)attn_stream_kernel<64, 0>},
    {(const void *)attn_stream_kernel<32, 0>, (const void *)attn_stream_kernel<32, 1>, (const void *)attn_stream_kernel<32, 2>, (const void *)attn_stream_kernel<32, 0>},
    {(const void *)attn_stream_kernel<320, 0>, (const void *)attn_stream_kernel<320, 1>, (const void *)attn_stream_kernel<320, 2>, (const void *)attn_stream_kernel<320, 0>},
    {(const void *)attn_stream_kernel<16, 0>, (const void *)attn_stream_kernel<16, 1>, (const void *)attn_stream_kernel<16, 2>, (const void *)attn_stream_kernel<16, 0>},
    MFMA_ONE(attn_stream_kernel<16, 2, 7>),
    MFMA_ONE(attn_stream_kernel<64, 2, 7>),
    MFMA_ONE(attn_stream_kernel<32, 2, 7>),
    {(const void *)attn_lean_kernel<0>, (const void *)attn_lean_kernel<1>, (const void *)attn_lean_kernel<2>, (const void *)attn_lean_kernel<3>},
    MFMA_ONE(attn_lean_kernel<2, 64, 128, 128, 1>),
    {(const void *)attn_lean_kernel<0, 32>, (const void *)attn_lean_kernel<1, 32>, (const void *)attn_lean_kernel<2, 32>, (const void *)attn_lean_kernel<3, 32>},
    MFMA_ONE(attn_lean_kernel<2, 32, 128, 128, 1>),
    {(const void *)attn_lean_kernel<0, 32, 64, 64, 3>, (const void *)attn_lean_kernel<1, 32, 64, 64, 3>, (const void *)attn_lean_kernel<2, 32, 64, 64, 3>, (const void *)attn_lean_kernel<3, 32, 64, 64, 3>},
    {(const void *)attn_lean_kernel<0, 16, 64, 64, 3>, (const void *)attn_lean_kernel<1, 16, 64, 64, 3>, (const void *)attn_lean_kernel<2, 16, 64, 64, 3>, (const void *)attn_lean_kernel<3, 16, 64, 64, 3>},
    {(const void *)attn_lean_kernel<0, 64, 128, 64, 3>, (const void *)attn_lean_kernel<1, 64, 128, 64, 3>, (const void *)attn_lean_kernel<2, 64, 128, 64, 3>, (const void *)attn_lean_kernel<3, 64, 128, 64, 3>},
};
// the same instances with LSE = true (common.h, "Log-sum-exp"): behind the others in the code object
static const void *const kMfmaKernelsLse[kMfmaForms][4] = {
    {(const void *)attn_stream_kernel<64, 0, 8, true>, (const void *)attn_stream_kernel<64, 1, 8, true>, (const void *)attn_stream_kernel<64, 2, 8, true>, (const void *)attn_stream_kernel<64, 0, 8, true>},
    {(const void *)attn_stream_kernel<32, 0, 8, true>, (const void *)attn_stream_kernel<32, 1, 8, true>, (const void *)attn_stream_kernel<32, 2, 8, true>, (const void *)attn_stream_kernel<32, 0, 8, true>},
    {(const void *)attn_stream_kernel<320, 0, 8, true>, (const void *)attn_stream_kernel<320, 1, 8, true>, (const void *)attn_stream_kernel<320, 2, 8, true>, (const void *)attn_stream_kernel<320, 0, 8, true>},
    {(const void *)attn_stream_kernel<16, 0, 8, true>, (const void *)attn_stream_kernel<16, 1, 8, true>, (const void *)attn_stream_kernel<16, 2, 8, true>, (const void *)attn_stream_kernel<16, 0, 8, true>},
    MFMA_ONE(attn_stream_kernel<16, 2, 7, true>),
    MFMA_ONE(attn_stream_kernel<64, 2, 7, true>),
    MFMA_ONE(attn_stream_kernel<32, 2, 7, true>),
    {(const void *)attn_lean_kernel<0, 64, 128, 128, 0, true>, (const void *)attn_lean_kernel<1, 64, 128, 128, 0, true>, (const void *)attn_lean_kernel<2, 64, 128, 128, 0, true>, (const void *)attn_lean_kernel<3, 64, 128, 128, 0, true>},
    MFMA_ONE(attn_lean_kernel<2, 64, 128, 128, 1, true>),
    {(const void *)attn_lean_kernel<0, 32, 128, 128, 0, true>, (const void *)attn_lean_kernel<1, 32, 128, 128, 0, true>, (const void *)attn_lean_kernel<2, 32, 128, 128, 0, true>, (const void *)attn_lean_kernel<3, 32, 128, 128, 0, true>},
    MFMA_ONE(attn_lean_kernel<2, 32, 128, 128, 1, true>),
    {(const void *)attn_lean_kernel<0, 32, 64, 64, 3, true>, (const void *)attn_lean_kernel<1, 32, 64, 64, 3, true>, (const void *)attn_lean_kernel<2, 32, 64, 64, 3, true>, (const void *)attn_lean_kernel<3, 32, 64, 64, 3, true>},
    {(const void *)attn_lean_kernel<0, 16, 64, 64, 3, true>, (const void *)attn_lean_kernel<1, 16, 64, 64, 3, true>, (const void *)attn_lean_kernel<2, 16, 64, 64, 3, true>, (const void *)attn_lean_kernel<3, 16, 64, 64, 3, true>},
    {(const void *)attn_lean_kernel<0, 64, 128, 64, 3, true>, (const void *)attn_lean_kernel<1, 64, 128, 64, 3, true>, (const void *)attn_lean_kernel<2, 64, 128, 64, 3, true>, (const void *)attn_lean_kernel<3, 64, 128, 64, 3, true>},
};
#undef MFMA_ONE
static void mfma_setup() {
    if (device_once(1))
        for (const auto *tab : {kMfmaKernels, kMfmaKernelsLse})
            for (int f = 0; f < kMfmaForms; ++f)
                for (const void *k : tab[f]) (void)hipFuncSetAttribute(k, hipFuncAttributeMaxDynamicSharedMemorySize, kLdsBytes);
}

bool plan_attn_mfma(const AttnParams &p_in, AttnPlan &plan) {
    if (!p_in.v_paged || !mfma_shape_ok(p_in)) return false;
    AttnParams p = mfma_virtual(p_in);      // (the identity unless the shape runs as head parts)
    const int cus = device_cus();
    const int ns = mfma_splits(p, cus);
    if (!mfma_stream_ok(p, ns)) return false;      // T = 0 or more than 64 rounds per wave: the caller's next choice, the tile kernel
    // lean kernel (round 5): 64-token units, lane = token; C = 256 and (its table copy spreads the K rows) C = 128
    const bool lean = p.G <= 4 && p.page_size >= 64 && !g_lean_off;
    int form;
    if (p.d == 64) {              // the lean kernel or none of this file's
        if (!lean) return false;
        form = p.M == 64 ? kLeanD64M64 : p.M == 32 ? kLeanD64M32 : kLeanD64M16;
    } else if (p.M == 16) {       // d_m = 8 form of the streaming kernel
        form = p.C == 128 ? kStream16C128 : kStream16;
    } else if (lean && (p.M == 64 || !(g_mfma_form & 1))) {
        form = p.M == 64 ? (p.C == 128 ? kLean64C128 : kLean64) : (p.C == 128 ? kLean32C128 : kLean32);
    } else if (p.C == 128) {      // 128 centroids per subspace (reference setup.py:15): streaming kernel by run-time layout flags only
        form = p.M == 64 ? kStream64C128 : kStream32C128;
    } else {
        // d_m = 4 form at M = 32 and up to 4 query heads: query heads replicated over the column groups of the score tile
        form = p.M == 64 ? kStream64 : (p.G <= 4 && !(g_mfma_form & 1)) ? kStream32D4 : kStream32;
    }
    int mode = (p.k_paged && !p.v_identity && !p.ids64) ? 0 : (!p.k_paged && p.v_identity) ? 1 : 2;
    // read-once: a unit is a whole page that one wave reads once per step (128-token pages: a line belongs to two waves' units;
    // query-head parts: the second part re-reads the page from L2 - both keep the default policy)
    if (mode == 0 && form >= kLean64 && p.page_size == 64 && !p.nhk_mul) mode = 3;
    const int bh = p.bs * p.nh_k;
    const int units = (p.T + 31) / 32;
    p.nsplit = ns;
    p.nslots = ns;
    p.split_len = 32 * ((units + ns - 1) / ns);
    // mergers per (b, kv head): helpers only when every workgroup of the launch is resident at once (one per CU); a helper
    // that still cannot see its flags gives up and the last arriver takes over (merge_and_publish)
    int nm = p.G < ns ? p.G : ns;
    if (nm > 8) nm = 8;
    p.nmerge = (long long)bh * ns <= cus ? (nm > 0 ? nm : 1) : 1;
    p.tail_test = g_tail_test;
#if MILLION_EXP & 2
    p.nmerge = 1;      // A/B: the primary alone
#endif
    plan = {(p.lse ? kMfmaKernelsLse : kMfmaKernels)[form][mode], dim3(ns, bh), dim3(kNW * 64), kLdsBytes, p, 1, mfma_setup};
    return true;
}

}  // namespace million
