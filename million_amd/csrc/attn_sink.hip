// attn_sink.hip — the exact fp16 sink rows of a request attended to and merged into the past part in one launch
// (million_attn_sink_merge, include/million_hip.h), gfx950.
//
// n query rows per (b, query head) have attended to the cache (out_a, lse_a: a decode, chunk or verify call with its lse).  What is
// left is their attention over the s_b <= s_cap <= 64 sink rows kept in full precision beside the pages - every sink row is visible
// to every query row - and the merge of the two parts (million_attn_merge's formula with the second part computed here, never stored).
//
// The work is at most 64 keys per row: the launch is shaped for latency, as attn_block.hip.  One wave per workgroup; every global load
// of the wave - q, out_a, lse_a, the two counts and the wave's share of the K and V sink rows, which go through LDS - is issued before
// the first use, so the launch pays one memory round trip.  Two instances, chosen on the host:
//   rows (n > 4):  one wave per (block of 16 rows, b, head); lane = (row, quarter of d), attn_block.hip's mapping.  The keys run
//                  under a wave-uniform bound s_b; the scores of a row wait in LDS (16 x s_b floats) between the maximum and the sum.
//                  Every lane of a quarter reads the same 16 bytes of a sink row: a broadcast, no bank conflict.
//   keys (n <= 4): one wave per (b, head); lane = sink row for the scores - the lane holds its K row in registers (read from LDS
//                  rows padded by one 16-byte slot: lane j starts at slot 17 j, so the 16 lanes of a ds_read_b128 group hit 16
//                  different slots), q_i is an LDS broadcast, maximum and sum are wave reductions - and lane = 2 dims for the value
//                  sum, p_j taken from lane j with v_readlane under the uniform key counter.  A decode step (n = 1) with 64 sinks
//                  then has 64 lanes at work where the rows mapping would have four; it has a build of its own (NQ = 1), the
//                  rows 2 .. 4 share the build unrolled for four.
// No atomics, no workspace, no private memory.  s_b = 0 is the identity: w = 1, out = out_a through fp32 and back, lse_out = lse_a.
#include <math.h>
#include <string.h>

#include "common.h"

namespace million {

namespace {

constexpr int kSinkCap = 64;       // sink rows per request, at most
constexpr int kSinkRows = 16;      // query rows per workgroup of the rows instance
constexpr int kSinkSmall = 4;      // query rows up to which the keys instance serves the call

typedef f16 h8 __attribute__((ext_vector_type(8)));
typedef f16 h2 __attribute__((ext_vector_type(2)));

struct SinkMergeParams {
    const f16 *q, *k, *v, *out_a;
    const float *lse_a;
    const int *dev_s, *dev_n;
    f16 *out;
    float *lse_out;
    long long qs[3], as[3], os[3];      // element strides (b, h, n)
    long long ks[2];                    // sink strides (b, h); rows of d
    int nh, G, n, s_cap, n_sink, n_blk;
    float scale;
};

__device__ __forceinline__ float wave_max(float x) {
#pragma unroll
    for (int o = 32; o >= 1; o >>= 1) x = fmaxf(x, __shfl_xor(x, o));
    return x;
}
__device__ __forceinline__ float wave_sum(float x) {
#pragma unroll
    for (int o = 32; o >= 1; o >>= 1) x += __shfl_xor(x, o);
    return x;
}

// The two counts of request b, clamped and wave-uniform: sb live sink rows, nb live query rows
__device__ __forceinline__ void sink_counts(const SinkMergeParams &p, int b, int &sb, int &nb) {
    sb = p.n_sink;
    nb = p.n;
    if (p.dev_s) sb = p.dev_s[b];
    if (p.dev_n) nb = p.dev_n[b];
    sb = __builtin_amdgcn_readfirstlane(clamp_count(sb, p.s_cap));
    nb = __builtin_amdgcn_readfirstlane(clamp_count(nb, p.n));
}

// ---- rows instance: lane = (row, quarter of d) ------------------------------------------------------------------------------
template <int D>
__global__ __launch_bounds__(64) void attn_sink_rows_kernel(SinkMergeParams p) {
    constexpr int DP = D / 4;       // dims per lane
    constexpr int NV = DP / 8;      // 16-byte vectors per lane and row part
    constexpr int VPR = D / 8;      // vectors per row
    constexpr int NL = kSinkCap * VPR / 64;      // the wave's loads per side at s_cap = 64
    extern __shared__ h8 smem[];
    h8 *sK = smem, *sV = smem + p.s_cap * VPR;
    float *sS = (float *)(smem + 2 * p.s_cap * VPR);      // [key][row of the block]
    const int lane = threadIdx.x;
    const int blk = blockIdx.x % p.n_blk;
    const int bh = blockIdx.x / p.n_blk;
    const int h = bh % p.nh, b = bh / p.nh;
    const int hk = h / p.G;
    const int row = lane >> 2, part = lane & 3;
    const int i = blk * kSinkRows + row;
    const int n = p.n;
    const int ic = i < n ? i : n - 1;      // lanes past the rows read the last row and store nothing
    const int nvec = (p.dev_s ? p.s_cap : p.n_sink) * VPR;      // the sink rows a count on the device may name: all of them

    // ---- every load of the wave, before any use
    int sb, nb;
    h8 kv[NL], vv[NL], qv[NV], av[NV];
    const f16 *kp = p.k + b * p.ks[0] + hk * p.ks[1], *vp = p.v + b * p.ks[0] + hk * p.ks[1];
#pragma unroll
    for (int u = 0; u < NL; ++u) {
        const int t = lane + 64 * u;
        if (t < nvec) {
            kv[u] = *(const h8 *)(kp + 8 * t);
            vv[u] = *(const h8 *)(vp + 8 * t);
        }
    }
#pragma unroll
    for (int u = 0; u < NV; ++u) {
        qv[u] = *(const h8 *)(p.q + b * p.qs[0] + h * p.qs[1] + ic * p.qs[2] + part * DP + 8 * u);
        av[u] = *(const h8 *)(p.out_a + b * p.as[0] + h * p.as[1] + ic * p.as[2] + part * DP + 8 * u);
    }
    const float la = p.lse_a[((long long)b * p.nh + h) * n + ic];
    sink_counts(p, b, sb, nb);

#pragma unroll
    for (int u = 0; u < NL; ++u) {
        const int t = lane + 64 * u;
        if (t < nvec) {
            sK[t] = kv[u];
            sV[t] = vv[u];
        }
    }
    __syncthreads();

    // ---- scores of the row against the keys j < sb (wave-uniform bound: rows at or past sb are never read from LDS)
    float qf[DP];
#pragma unroll
    for (int u = 0; u < NV; ++u)
#pragma unroll
        for (int e = 0; e < 8; ++e) qf[8 * u + e] = (float)qv[u][e];
    float m = -INFINITY;
    for (int j = 0; j < sb; ++j) {
        float acc = 0.f;
#pragma unroll
        for (int u = 0; u < NV; ++u) {
            const h8 kk = sK[j * VPR + part * NV + u];
#pragma unroll
            for (int e = 0; e < 8; ++e) acc = fmaf(qf[8 * u + e], (float)kk[e], acc);
        }
        acc += __shfl_xor(acc, 1);
        acc += __shfl_xor(acc, 2);
        const float s = acc * p.scale;
        m = fmaxf(m, s);
        if (part == 0) sS[j * kSinkRows + row] = s;
    }
    __syncthreads();

    // ---- merge with the past part: L = max(lse_a, m), the past's weight w = exp(lse_a - L)
    const bool live = i < nb;
    const bool nan = la != la;
    const float L = fmaxf(la, m);              // (fmaxf drops a NaN: looked for on its own)
    const float Ls = L > -INFINITY ? L : 0.f;
    const float w = la > -INFINITY ? expf(la - Ls) : 0.f;
    float den = w, acc[DP];
#pragma unroll
    for (int u = 0; u < NV; ++u)
#pragma unroll
        for (int e = 0; e < 8; ++e) acc[8 * u + e] = w > 0.f ? w * (float)av[u][e] : 0.f;      // w = 0: out_a is not used
    for (int j = 0; j < sb; ++j) {
        const float pj = expf(sS[j * kSinkRows + row] - Ls);
        den += pj;
#pragma unroll
        for (int u = 0; u < NV; ++u) {
            const h8 x = sV[j * VPR + part * NV + u];
#pragma unroll
            for (int e = 0; e < 8; ++e) acc[8 * u + e] = fmaf(pj, (float)x[e], acc[8 * u + e]);
        }
    }
    const float qnan = __builtin_nanf("");
    const float inv = !live ? 0.f : nan ? qnan : den > 0.f ? 1.0f / den : 0.f;      // den = 0: no past and no sink
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
            p.lse_out[((long long)b * p.nh + h) * n + i] = !live ? -INFINITY : nan ? qnan : den > 0.f ? Ls + logf(den) : -INFINITY;
    }
}

// ---- keys instance (n <= 4): lane = sink row for the scores, lane = 2 dims for the value sum --------------------------------
// NQ: the query rows the instance is unrolled for, 1 (a decode step) or kSinkSmall
template <int D, int NQ>
__global__ __launch_bounds__(64) void attn_sink_keys_kernel(SinkMergeParams p) {
    constexpr int VPR = D / 8;       // vectors per row
    constexpr int KPR = VPR + 1;     // ... of a padded K row in LDS
    constexpr int HD = D / 2;        // lanes that own 2 dims of a row
    constexpr int NL = kSinkCap * VPR / 64;
    extern __shared__ h8 smem[];
    h8 *sK = smem, *sV = smem + p.s_cap * KPR, *sQ = sV + p.s_cap * VPR;
    const int lane = threadIdx.x;
    const int h = blockIdx.x % p.nh, b = blockIdx.x / p.nh;
    const int hk = h / p.G;
    const int n = p.n;      // 1 .. NQ
    const int td = lane % HD;
    const int nvec = (p.dev_s ? p.s_cap : p.n_sink) * VPR;

    // ---- every load of the wave, before any use
    int sb, nb;
    h8 kv[NL], vv[NL], qv = {};
    h2 av[NQ];
    float la[NQ];
    const f16 *kp = p.k + b * p.ks[0] + hk * p.ks[1], *vp = p.v + b * p.ks[0] + hk * p.ks[1];
#pragma unroll
    for (int u = 0; u < NL; ++u) {
        const int t = lane + 64 * u;
        if (t < nvec) {
            kv[u] = *(const h8 *)(kp + 8 * t);
            vv[u] = *(const h8 *)(vp + 8 * t);
        }
    }
    if (lane < n * VPR) qv = *(const h8 *)(p.q + b * p.qs[0] + h * p.qs[1] + (lane / VPR) * p.qs[2] + 8 * (lane % VPR));
#pragma unroll
    for (int i = 0; i < NQ; ++i) {
        const int ic = i < n ? i : n - 1;
        av[i] = *(const h2 *)(p.out_a + b * p.as[0] + h * p.as[1] + ic * p.as[2] + 2 * td);
        la[i] = p.lse_a[((long long)b * p.nh + h) * n + ic];
    }
    sink_counts(p, b, sb, nb);

#pragma unroll
    for (int u = 0; u < NL; ++u) {
        const int t = lane + 64 * u;
        if (t < nvec) {
            sK[(t / VPR) * KPR + t % VPR] = kv[u];
            sV[t] = vv[u];
        }
    }
    if (lane < NQ * VPR) sQ[lane] = qv;
    __syncthreads();

    // ---- the lane's K row (zeros past sb: those rows are never read from LDS), then one score per query row
    const bool has = lane < sb;
    h8 kr[VPR];
#pragma unroll
    for (int c = 0; c < VPR; ++c) kr[c] = has ? sK[lane * KPR + c] : (h8){};
    float pr[NQ], w[NQ], den[NQ], Ls[NQ];
#pragma unroll
    for (int i = 0; i < NQ; ++i) {
        pr[i] = 0.f; w[i] = 0.f; den[i] = 0.f; Ls[i] = 0.f;
        if (i < nb) {      // wave-uniform: the q rows at or past nb reach no product
            float a = 0.f;
#pragma unroll
            for (int c = 0; c < VPR; ++c) {
                const h8 qq = sQ[i * VPR + c];
#pragma unroll
                for (int e = 0; e < 8; ++e) a = fmaf((float)qq[e], (float)kr[c][e], a);
            }
            const float s = has ? a * p.scale : -INFINITY;
            const float L = fmaxf(la[i], wave_max(s));      // (fmaxf drops a NaN lse_a: looked for at the store)
            Ls[i] = L > -INFINITY ? L : 0.f;
            w[i] = la[i] > -INFINITY ? expf(la[i] - Ls[i]) : 0.f;
            pr[i] = has ? expf(s - Ls[i]) : 0.f;
            den[i] = w[i] + wave_sum(pr[i]);
        }
    }

    // ---- value sum: the lane's 2 dims of every query row, p_j from lane j under the uniform key counter
    float acc[NQ][2];
#pragma unroll
    for (int i = 0; i < NQ; ++i) {
        acc[i][0] = w[i] > 0.f ? w[i] * (float)av[i][0] : 0.f;      // w = 0: out_a is not used
        acc[i][1] = w[i] > 0.f ? w[i] * (float)av[i][1] : 0.f;
    }
    const h2 *sV2 = (const h2 *)sV;
    for (int j = 0; j < sb; ++j) {
        const h2 x = sV2[j * HD + td];
        const float x0 = (float)x[0], x1 = (float)x[1];
#pragma unroll
        for (int i = 0; i < NQ; ++i) {
            const float pj = __int_as_float(__builtin_amdgcn_readlane(__float_as_int(pr[i]), j));
            acc[i][0] = fmaf(pj, x0, acc[i][0]);
            acc[i][1] = fmaf(pj, x1, acc[i][1]);
        }
    }
    const float qnan = __builtin_nanf("");
#pragma unroll
    for (int i = 0; i < NQ; ++i) {
        if (i < n) {
            const bool live = i < nb;
            const bool nan = la[i] != la[i];
            const float inv = !live ? 0.f : nan ? qnan : den[i] > 0.f ? 1.0f / den[i] : 0.f;
            if (lane < HD) {
                h2 o;
                o[0] = live ? (f16)(acc[i][0] * inv) : (f16)0.f;
                o[1] = live ? (f16)(acc[i][1] * inv) : (f16)0.f;
                *(h2 *)(p.out + b * p.os[0] + h * p.os[1] + i * p.os[2] + 2 * td) = o;
            }
            if (p.lse_out && lane == 0)
                p.lse_out[((long long)b * p.nh + h) * n + i] =
                    !live ? -INFINITY : nan ? qnan : den[i] > 0.f ? Ls[i] + logf(den[i]) : -INFINITY;
        }
    }
}

}  // namespace

}  // namespace million

using namespace million;

extern "C" int million_attn_sink_merge(const million_sink_merge_desc *desc, const void *q, const void *k_sink, const void *v_sink,
                                       const void *out_a, const float *lse_a, const int32_t *dev_s, const int32_t *dev_n, void *out,
                                       float *lse_out, million_stream_t stream) {
    const char *who = "attn_sink_merge";
    if (!desc || desc->struct_size != sizeof(million_sink_merge_desc)) { set_error("%s: bad desc / struct_size", who); return MILLION_ERR_ARG; }
    const million_sink_merge_desc &d = *desc;
    if (d.n < 1) { set_error("%s: n=%d (>= 1 query rows)", who, d.n); return MILLION_ERR_SHAPE; }
    if (d.d != 64 && d.d != 128) { set_error("%s: d=%d (64 / 128)", who, d.d); return MILLION_ERR_SHAPE; }
    if (d.s_cap < 1 || d.s_cap > kSinkCap) { set_error("%s: s_cap=%d (1 .. %d sink rows)", who, d.s_cap, kSinkCap); return MILLION_ERR_SHAPE; }
    if (d.n_sink < 0 || d.n_sink > d.s_cap) { set_error("%s: n_sink=%d (0 .. s_cap = %d)", who, d.n_sink, d.s_cap); return MILLION_ERR_SHAPE; }
    if (d.bs <= 0 || d.nh <= 0 || d.nh_k <= 0 || d.nh % d.nh_k) {
        set_error("%s: bs=%d nh=%d nh_k=%d (nh a multiple of nh_k)", who, d.bs, d.nh, d.nh_k);
        return MILLION_ERR_SHAPE;
    }
    if (!q || !k_sink || !v_sink || !out_a || !lse_a || !out) { set_error("%s: null q / k_sink / v_sink / out_a / lse_a / out", who); return MILLION_ERR_ARG; }
    if (((uintptr_t)q | (uintptr_t)k_sink | (uintptr_t)v_sink | (uintptr_t)out_a | (uintptr_t)out) & 15) {
        set_error("%s: q, sink rows and outs must be 16-byte aligned", who);
        return MILLION_ERR_ALIGN;
    }
    if (((uintptr_t)lse_a | (uintptr_t)lse_out | (uintptr_t)dev_s | (uintptr_t)dev_n) & 3) {
        set_error("%s: lse_a / lse_out / dev_s / dev_n must be 4-byte aligned", who);
        return MILLION_ERR_ALIGN;
    }
    long long strides = d.sink_stride_b | d.sink_stride_h;
    for (int k = 0; k < 3; ++k) strides |= d.q_stride[k] | d.a_stride[k] | d.o_stride[k];
    if (strides & 7) { set_error("%s: fp16 strides must be multiples of 8 elements (16-byte rows)", who); return MILLION_ERR_ALIGN; }
    const bool small = d.n <= kSinkSmall;
    const long long n_blk = small ? 1 : ((long long)d.n + kSinkRows - 1) / kSinkRows;
    const long long groups = (long long)d.bs * d.nh * n_blk;
    if (groups > 0x7fffffffLL) { set_error("%s: %lld workgroups", who, groups); return MILLION_ERR_SHAPE; }
    SinkMergeParams p;
    memset(&p, 0, sizeof(p));
    p.q = (const f16 *)q; p.k = (const f16 *)k_sink; p.v = (const f16 *)v_sink; p.out_a = (const f16 *)out_a;
    p.lse_a = lse_a; p.dev_s = dev_s; p.dev_n = dev_n; p.out = (f16 *)out; p.lse_out = lse_out;
    for (int k = 0; k < 3; ++k) { p.qs[k] = d.q_stride[k]; p.as[k] = d.a_stride[k]; p.os[k] = d.o_stride[k]; }
    p.ks[0] = d.sink_stride_b; p.ks[1] = d.sink_stride_h;
    p.nh = d.nh; p.G = d.nh / d.nh_k; p.n = d.n; p.s_cap = d.s_cap; p.n_sink = d.n_sink; p.n_blk = (int)n_blk;
    p.scale = 1.0f / sqrtf((float)d.d);
    const int vpr = d.d / 8;
    // LDS: K and V sink rows, then the scores of 16 rows (rows instance) or the padded K rows' extra slot and 4 q rows (keys instance)
    const size_t lds = small ? 16u * ((size_t)d.s_cap * (2 * vpr + 1) + kSinkSmall * vpr)
                             : 16u * (size_t)d.s_cap * 2 * vpr + sizeof(float) * kSinkRows * d.s_cap;
    const dim3 grid((unsigned)groups);
    hipStream_t s = (hipStream_t)stream;
    if (small) {
        if (d.d == 128 && d.n == 1) hipLaunchKernelGGL((attn_sink_keys_kernel<128, 1>), grid, dim3(64), lds, s, p);
        else if (d.d == 128) hipLaunchKernelGGL((attn_sink_keys_kernel<128, kSinkSmall>), grid, dim3(64), lds, s, p);
        else if (d.n == 1) hipLaunchKernelGGL((attn_sink_keys_kernel<64, 1>), grid, dim3(64), lds, s, p);
        else hipLaunchKernelGGL((attn_sink_keys_kernel<64, kSinkSmall>), grid, dim3(64), lds, s, p);
    } else {
        if (d.d == 128) hipLaunchKernelGGL(attn_sink_rows_kernel<128>, grid, dim3(64), lds, s, p);
        else hipLaunchKernelGGL(attn_sink_rows_kernel<64>, grid, dim3(64), lds, s, p);
    }
    const hipError_t e = hipGetLastError();
    if (e != hipSuccess) { set_error("%s launch: %s", who, hipGetErrorString(e)); return MILLION_ERR_LAUNCH; }
    return MILLION_OK;
}
