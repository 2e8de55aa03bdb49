// attn_block.hip — the causal block of a draft verification merged into its past part in one launch (million_attn_block_merge,
// include/million_hip.h), gfx950.
//
// n <= 16 draft rows per request have attended to the cache (out_a, lse_a: a decode launch over the rows as query heads, or chunk
// attention without a chunk).  What is left is their attention among themselves - row i sees block keys j <= i - and the merge of
// the two parts (million_attn_merge's formula with the second part computed here, never stored).
//
// The work is at most 16 x 16 scores per head: the launch is shaped for latency.  One wave per (b, query head); lane = (row i,
// quarter of d).  Every global load of the wave - its quarter of q_i and of out_a_i, lse_a_i, and the wave's share of the K and V
// block, which goes through LDS - is issued before the first use, so the launch pays one memory round trip.  The score of (i, j) is
// four partial dot products summed across the row's four lanes; the scores of a row stay in registers (the j loop is unrolled over
// the 16 possible keys under a wave-uniform bound).  No atomics, no workspace, no private memory; the first query head of every kv
// head also copies the block rows to k_stage / v_stage from the registers that feed LDS.
//
// million_attn_tree_merge is the same kernel body for a draft that is a tree in topological order (TREE = true): row i sees the
// block rows its ancestor-mask word names instead of the rows j <= i.  The word is one more load among the wave's first loads and
// is sanitised before use, m = (mask & ((2u << i) - 1)) | (1u << i); j is a compile-time constant under the unrolled loop, so the
// test is a bit test per score and the scores stay in registers.  million_attn_block_merge launches the TREE = false instances.
#include <math.h>
#include <string.h>

#include <type_traits>

#include "common.h"

namespace million {

namespace {

constexpr int kBlkRows = 16;      // draft rows per request, at most

typedef f16 h8 __attribute__((ext_vector_type(8)));

struct BlockMergeParams {
    const f16 *q, *k, *v, *out_a;
    const float *lse_a;
    const int *dev_n;
    f16 *out;
    float *lse_out;
    f16 *k_stage, *v_stage;
    long long qs[3], ks[3], vs[3], as[3], os[3];      // element strides (b, h, n)
    long long ss[2];                                  // staging strides (b, h); rows of d
    int nh, G, n;
    float scale;
};

// million_attn_tree_merge: the same block under an ancestor mask, bit j of word (b, i) = row i sees block row j
struct TreeMergeParams : BlockMergeParams {
    const int *dev_mask;      // (bs, n)
};

// TREE = false is the chain (row i sees j <= i), the kernel of million_attn_block_merge; TREE = true takes the row's visibility
// from its mask word, loaded with the wave's other loads and sanitised before use: the row itself always, no later row, no bit
// at or above 16.
template <int D, bool TREE = false>
__global__ __launch_bounds__(64) void attn_block_merge_kernel(std::conditional_t<TREE, TreeMergeParams, BlockMergeParams> p) {
    constexpr int DP = D / 4;       // dims per lane
    constexpr int NV = DP / 8;      // 16-byte vectors per lane and row part; also the wave's loads per side of the block
    constexpr int VPR = D / 8;      // vectors per row
    __shared__ h8 sK[kBlkRows * VPR], sV[kBlkRows * VPR];
    const int lane = threadIdx.x;
    const int h = blockIdx.x % p.nh;
    const int b = blockIdx.x / p.nh;
    const int hk = h / p.G;
    const int i = lane >> 2, part = lane & 3;
    const int n = p.n;
    int nb = n;
    if (p.dev_n) nb = clamp_count(p.dev_n[b], n);
    nb = __builtin_amdgcn_readfirstlane(nb);
    const int ic = i < n ? i : n - 1;      // lanes past the block read its last row and store nothing

    // ---- every load of the wave, before any use
    h8 kv[NV], vv[NV], qv[NV], av[NV];
#pragma unroll
    for (int u = 0; u < NV; ++u) {
        const int t = lane + 64 * u;
        const int row = t / VPR, col = t % VPR;
        const int rc = row < n ? row : n - 1;
        kv[u] = *(const h8 *)(p.k + b * p.ks[0] + hk * p.ks[1] + rc * p.ks[2] + 8 * col);
        vv[u] = *(const h8 *)(p.v + b * p.vs[0] + hk * p.vs[1] + rc * p.vs[2] + 8 * col);
    }
#pragma unroll
    for (int u = 0; u < NV; ++u) {
        qv[u] = *(const h8 *)(p.q + b * p.qs[0] + h * p.qs[1] + ic * p.qs[2] + part * DP + 8 * u);
        av[u] = *(const h8 *)(p.out_a + b * p.as[0] + h * p.as[1] + ic * p.as[2] + part * DP + 8 * u);
    }
    const float la = p.lse_a[((long long)b * p.nh + h) * n + ic];
    unsigned vis = 0;
    if constexpr (TREE) vis = (unsigned)p.dev_mask[(long long)b * n + ic];

#pragma unroll
    for (int u = 0; u < NV; ++u) {
        const int t = lane + 64 * u;
        sK[t] = kv[u];
        sV[t] = vv[u];
    }
    if (p.k_stage && h == hk * p.G) {
#pragma unroll
        for (int u = 0; u < NV; ++u) {
            const int t = lane + 64 * u;
            const int row = t / VPR, col = t % VPR;
            if (row < n) {
                const long long o = b * p.ss[0] + hk * p.ss[1] + (long long)row * D + 8 * col;
                *(h8 *)(p.k_stage + o) = kv[u];
                *(h8 *)(p.v_stage + o) = vv[u];
            }
        }
    }
    __syncthreads();

    // ---- scores of row i against the keys j < nb (wave-uniform bound: rows at or past nb are never read from LDS)
    float qf[DP];
#pragma unroll
    for (int u = 0; u < NV; ++u)
#pragma unroll
        for (int e = 0; e < 8; ++e) qf[8 * u + e] = (float)qv[u][e];
    if constexpr (TREE) vis = (vis & ((2u << i) - 1u)) | (1u << i);      // i <= 15
    float s[kBlkRows];
    float m = -INFINITY;
#pragma unroll
    for (int j = 0; j < kBlkRows; ++j) {
        s[j] = -INFINITY;
        if (j < nb) {
            float acc = 0.f;
#pragma unroll
            for (int u = 0; u < NV; ++u) {
                const h8 kk = sK[j * VPR + part * NV + u];
#pragma unroll
                for (int e = 0; e < 8; ++e) acc = fmaf(qf[8 * u + e], (float)kk[e], acc);
            }
            acc += __shfl_xor(acc, 1);
            acc += __shfl_xor(acc, 2);
            bool sees = j <= i;
            if constexpr (TREE) sees = (vis >> j) & 1u;
            s[j] = sees ? acc * p.scale : -INFINITY;
            m = fmaxf(m, s[j]);
        }
    }
    // ---- merge with the past part: L = max(lse_a, m), the past's weight w = exp(lse_a - L)
    const bool live = i < nb;                  // then key j = i is visible: m is finite
    const bool nan = la != la;
    const float L = fmaxf(la, m);              // (fmaxf drops a NaN: looked for on its own)
    const float Ls = L > -INFINITY ? L : 0.f;
    const float w = la > -INFINITY ? expf(la - Ls) : 0.f;
    float den = w, acc[DP];
#pragma unroll
    for (int u = 0; u < NV; ++u)
#pragma unroll
        for (int e = 0; e < 8; ++e) acc[8 * u + e] = w > 0.f ? w * (float)av[u][e] : 0.f;      // w = 0: out_a is not used
#pragma unroll
    for (int j = 0; j < kBlkRows; ++j) {
        if (j < nb) {
            const float pj = s[j] > -INFINITY ? expf(s[j] - Ls) : 0.f;
            den += pj;
#pragma unroll
            for (int u = 0; u < NV; ++u) {
                const h8 x = sV[j * VPR + part * NV + u];
#pragma unroll
                for (int e = 0; e < 8; ++e) acc[8 * u + e] = fmaf(pj, (float)x[e], acc[8 * u + e]);
            }
        }
    }
    const float qnan = __builtin_nanf("");
    const float inv = !live ? 0.f : nan ? qnan : 1.0f / den;
    if (i < n) {
        f16 *op = p.out + b * p.os[0] + h * p.os[1] + i * p.os[2] + part * DP;
#pragma unroll
        for (int u = 0; u < NV; ++u) {
            h8 o;
#pragma unroll
            for (int e = 0; e < 8; ++e) o[e] = live ? (f16)(acc[8 * u + e] * inv) : (f16)0.f;
            *(h8 *)(op + 8 * u) = o;
        }
        if (p.lse_out && part == 0)
            p.lse_out[((long long)b * p.nh + h) * n + i] = !live ? -INFINITY : nan ? qnan : Ls + logf(den);
    }
}

}  // namespace

}  // namespace million

using namespace million;

// Validation and parameter fill shared by the two entries; `who` names the entry in the messages.  No HIP call.
static int block_merge_fill(const char *who, const million_block_merge_desc *desc, const void *q, const void *k_blk, const void *v_blk,
                            const void *out_a, const float *lse_a, const int32_t *dev_n, void *out, float *lse_out, void *k_stage,
                            void *v_stage, BlockMergeParams &p) {
    if (!desc || desc->struct_size != sizeof(million_block_merge_desc)) { set_error("%s: bad desc / struct_size", who); return MILLION_ERR_ARG; }
    const million_block_merge_desc &d = *desc;
    if (d.n < 1 || d.n > kBlkRows) { set_error("%s: n=%d (1 .. %d draft rows)", who, d.n, kBlkRows); return MILLION_ERR_SHAPE; }
    if (d.d != 64 && d.d != 128) { set_error("%s: d=%d (64 / 128)", who, d.d); return MILLION_ERR_SHAPE; }
    if (d.bs <= 0 || d.nh <= 0 || d.nh_k <= 0 || d.nh % d.nh_k || (long long)d.bs * d.nh > 0x7fffffffLL) {
        set_error("%s: bs=%d nh=%d nh_k=%d (nh a multiple of nh_k)", who, d.bs, d.nh, d.nh_k);
        return MILLION_ERR_SHAPE;
    }
    if (!q || !k_blk || !v_blk || !out_a || !lse_a || !out) { set_error("%s: null q / k_blk / v_blk / out_a / lse_a / out", who); return MILLION_ERR_ARG; }
    if ((k_stage == nullptr) != (v_stage == nullptr)) { set_error("%s: k_stage and v_stage go together", who); return MILLION_ERR_ARG; }
    if (((uintptr_t)q | (uintptr_t)k_blk | (uintptr_t)v_blk | (uintptr_t)out_a | (uintptr_t)out | (uintptr_t)k_stage | (uintptr_t)v_stage) & 15) {
        set_error("%s: q, block rows, outs and staging must be 16-byte aligned", who);
        return MILLION_ERR_ALIGN;
    }
    if (((uintptr_t)lse_a | (uintptr_t)lse_out | (uintptr_t)dev_n) & 3) { set_error("%s: lse_a / lse_out / dev_n must be 4-byte aligned", who); return MILLION_ERR_ALIGN; }
    long long strides = d.stage_stride_b | d.stage_stride_h;
    for (int k = 0; k < 3; ++k) strides |= d.q_stride[k] | d.k_stride[k] | d.v_stride[k] | d.a_stride[k] | d.o_stride[k];
    if (strides & 7) { set_error("%s: fp16 strides must be multiples of 8 elements (16-byte rows)", who); return MILLION_ERR_ALIGN; }
    memset(&p, 0, sizeof(p));
    p.q = (const f16 *)q; p.k = (const f16 *)k_blk; p.v = (const f16 *)v_blk; p.out_a = (const f16 *)out_a;
    p.lse_a = lse_a; p.dev_n = dev_n; p.out = (f16 *)out; p.lse_out = lse_out;
    p.k_stage = (f16 *)k_stage; p.v_stage = (f16 *)v_stage;
    for (int k = 0; k < 3; ++k) {
        p.qs[k] = d.q_stride[k]; p.ks[k] = d.k_stride[k]; p.vs[k] = d.v_stride[k]; p.as[k] = d.a_stride[k]; p.os[k] = d.o_stride[k];
    }
    p.ss[0] = d.stage_stride_b; p.ss[1] = d.stage_stride_h;
    p.nh = d.nh; p.G = d.nh / d.nh_k; p.n = d.n;
    p.scale = 1.0f / sqrtf((float)d.d);
    return MILLION_OK;
}

extern "C" int million_attn_block_merge(const million_block_merge_desc *desc, const void *q, const void *k_blk, const void *v_blk,
                                        const void *out_a, const float *lse_a, const int32_t *dev_n, void *out, float *lse_out,
                                        void *k_stage, void *v_stage, million_stream_t stream) {
    BlockMergeParams p;
    const int rc = block_merge_fill("attn_block_merge", desc, q, k_blk, v_blk, out_a, lse_a, dev_n, out, lse_out, k_stage, v_stage, p);
    if (rc != MILLION_OK) return rc;
    const dim3 grid((unsigned)(desc->bs * desc->nh));
    hipStream_t s = (hipStream_t)stream;
    if (desc->d == 128) hipLaunchKernelGGL(attn_block_merge_kernel<128>, grid, dim3(64), 0, s, p);
    else hipLaunchKernelGGL(attn_block_merge_kernel<64>, grid, dim3(64), 0, s, p);
    const hipError_t e = hipGetLastError();
    if (e != hipSuccess) { set_error("attn_block_merge launch: %s", hipGetErrorString(e)); return MILLION_ERR_LAUNCH; }
    return MILLION_OK;
}

extern "C" int million_attn_tree_merge(const million_block_merge_desc *desc, const void *q, const void *k_blk, const void *v_blk,
                                       const void *out_a, const float *lse_a, const int32_t *dev_n, const int32_t *dev_mask, void *out,
                                       float *lse_out, void *k_stage, void *v_stage, million_stream_t stream) {
    TreeMergeParams p;
    const int rc = block_merge_fill("attn_tree_merge", desc, q, k_blk, v_blk, out_a, lse_a, dev_n, out, lse_out, k_stage, v_stage, p);
    if (rc != MILLION_OK) return rc;
    if (!dev_mask) { set_error("attn_tree_merge: null dev_mask (million_attn_block_merge is the entry without a mask)"); return MILLION_ERR_ARG; }
    if ((uintptr_t)dev_mask & 3) { set_error("attn_tree_merge: dev_mask must be 4-byte aligned"); return MILLION_ERR_ALIGN; }
    p.dev_mask = dev_mask;
    const dim3 grid((unsigned)(desc->bs * desc->nh));
    hipStream_t s = (hipStream_t)stream;
    if (desc->d == 128) hipLaunchKernelGGL((attn_block_merge_kernel<128, true>), grid, dim3(64), 0, s, p);
    else hipLaunchKernelGGL((attn_block_merge_kernel<64, true>), grid, dim3(64), 0, s, p);
    const hipError_t e = hipGetLastError();
    if (e != hipSuccess) { set_error("attn_tree_merge launch: %s", hipGetErrorString(e)); return MILLION_ERR_LAUNCH; }
    return MILLION_OK;
}
