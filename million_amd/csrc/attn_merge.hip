// attn_merge.hip — merge of partial attentions (million_attn_merge, include/million_hip.h): n_parts results (out_i, lse_i) of one
// query over disjoint key sets -> the result over their union.  One launch, one thread per (row, 8 dims), 16-byte loads and
// stores, as chunk_merge_kernel; every part's 8 dims are in registers before the thread stores, so `out` may be one of the parts.
#include <math.h>
#include <string.h>

#include "common.h"

namespace million {

namespace {

constexpr int kMaxParts = MILLION_MERGE_MAX_PARTS;

struct MergeParams {
    const f16 *po[kMaxParts];
    const float *pl[kMaxParts];
    f16 *out;
    float *lse_out;
    long long os[kMaxParts][3], ls[kMaxParts][3], ros[3], rls[3];      // element strides (b, h, n)
    int nh, n_q;
    long long rows;      // bs * nh * n_q
};

template <int D, int P>
__global__ __launch_bounds__(256) void attn_merge_kernel(MergeParams p) {
    constexpr int TPR = D / 8;
    const long long gid = (long long)blockIdx.x * 256 + threadIdx.x;
    const long long row = gid / TPR;
    const int part = (int)(gid - row * TPR);
    if (row >= p.rows) return;
    const int n = (int)(row % p.n_q);
    const long long bh = row / p.n_q;
    const int h = (int)(bh % p.nh);
    const long long b = bh / p.nh;
    typedef f16 h8 __attribute__((ext_vector_type(8)));
    float ls[P];
    h8 v[P];
#pragma unroll
    for (int i = 0; i < P; ++i) {
        ls[i] = p.pl[i][b * p.ls[i][0] + h * p.ls[i][1] + n * p.ls[i][2]];
        v[i] = *(const h8 *)(p.po[i] + b * p.os[i][0] + h * p.os[i][1] + n * p.os[i][2] + 8 * part);
    }
    float L = ls[0];
    bool nan = ls[0] != ls[0];
#pragma unroll
    for (int i = 1; i < P; ++i) {
        L = fmaxf(L, ls[i]);      // fmaxf drops a NaN: looked for on its own
        nan = nan || ls[i] != ls[i];
    }
    const float Ls = L > -INFINITY ? L : 0.f;
    float W = 0.f, acc[8];
#pragma unroll
    for (int e = 0; e < 8; ++e) acc[e] = 0.f;
#pragma unroll
    for (int i = 0; i < P; ++i) {
        const float w = ls[i] > -INFINITY ? expf(ls[i] - Ls) : 0.f;      // -inf (and NaN, handled below): the part's out is not used
        W += w;
        if (w > 0.f) {
#pragma unroll
            for (int e = 0; e < 8; ++e) acc[e] = fmaf(w, (float)v[i][e], acc[e]);
        }
    }
    const float inv = nan ? __builtin_nanf("") : W > 0.f ? 1.0f / W : 0.f;
    h8 o;
#pragma unroll
    for (int e = 0; e < 8; ++e) o[e] = (f16)(acc[e] * inv);
    *(h8 *)(p.out + b * p.ros[0] + h * p.ros[1] + n * p.ros[2] + 8 * part) = o;
    if (p.lse_out && part == 0)
        p.lse_out[b * p.rls[0] + h * p.rls[1] + n * p.rls[2]] = nan ? __builtin_nanf("") : W > 0.f ? Ls + logf(W) : -INFINITY;
}

template <int D>
const void *merge_instance(int P) {
    switch (P) {
        case 1: return (const void *)attn_merge_kernel<D, 1>;
        case 2: return (const void *)attn_merge_kernel<D, 2>;
        case 3: return (const void *)attn_merge_kernel<D, 3>;
        case 4: return (const void *)attn_merge_kernel<D, 4>;
        case 5: return (const void *)attn_merge_kernel<D, 5>;
        case 6: return (const void *)attn_merge_kernel<D, 6>;
        case 7: return (const void *)attn_merge_kernel<D, 7>;
        default: return (const void *)attn_merge_kernel<D, 8>;
    }
}

}  // namespace

}  // namespace million

using namespace million;

extern "C" int million_attn_merge(const million_attn_merge_desc *desc, const void *const *part_outs, const float *const *part_lses,
                                  void *out, float *lse_out, million_stream_t stream) {
    if (!desc || desc->struct_size != sizeof(million_attn_merge_desc)) { set_error("attn_merge: bad desc / struct_size"); return MILLION_ERR_ARG; }
    const million_attn_merge_desc &d = *desc;
    if (d.n_parts < 1 || d.n_parts > kMaxParts) { set_error("attn_merge: n_parts=%d (1 .. %d)", d.n_parts, kMaxParts); return MILLION_ERR_ARG; }
    if (d.bs <= 0 || d.nh <= 0 || d.n_q < 0 || (d.d != 64 && d.d != 128)) {
        set_error("attn_merge: bs=%d nh=%d n_q=%d d=%d (d 64 / 128)", d.bs, d.nh, d.n_q, d.d);
        return MILLION_ERR_SHAPE;
    }
    if (!part_outs || !part_lses || !out) { set_error("attn_merge: null pointer"); return MILLION_ERR_ARG; }
    uintptr_t ptrs = (uintptr_t)out, lptrs = (uintptr_t)lse_out;
    long long strides = d.res_out_stride[0] | d.res_out_stride[1] | d.res_out_stride[2];
    for (int i = 0; i < d.n_parts; ++i) {
        if (!part_outs[i] || !part_lses[i]) { set_error("attn_merge: part %d is null", i); return MILLION_ERR_ARG; }
        ptrs |= (uintptr_t)part_outs[i];
        lptrs |= (uintptr_t)part_lses[i];
        strides |= d.out_stride[i][0] | d.out_stride[i][1] | d.out_stride[i][2];
    }
    if ((ptrs & 15) || (lptrs & 3)) { set_error("attn_merge: out pointers must be 16-byte aligned (lse: 4-byte)"); return MILLION_ERR_ALIGN; }
    if (strides & 7) { set_error("attn_merge: out strides must be multiples of 8 elements (16-byte rows)"); return MILLION_ERR_ALIGN; }
    const long long rows = (long long)d.bs * d.nh * d.n_q;
    if (rows == 0) return MILLION_OK;
    const long long blocks = (rows * (d.d / 8) + 255) / 256;
    if (blocks > 0x7fffffffLL) { set_error("attn_merge: %lld workgroups", blocks); return MILLION_ERR_SHAPE; }
    MergeParams p;
    memset(&p, 0, sizeof(p));
    for (int i = 0; i < d.n_parts; ++i) {
        p.po[i] = (const f16 *)part_outs[i];
        p.pl[i] = part_lses[i];
        for (int k = 0; k < 3; ++k) { p.os[i][k] = d.out_stride[i][k]; p.ls[i][k] = d.lse_stride[i][k]; }
    }
    for (int k = 0; k < 3; ++k) { p.ros[k] = d.res_out_stride[k]; p.rls[k] = d.res_lse_stride[k]; }
    p.out = (f16 *)out; p.lse_out = lse_out;
    p.nh = d.nh; p.n_q = d.n_q; p.rows = rows;
    void *args[] = {(void *)&p};
    (void)hipLaunchKernel(d.d == 128 ? merge_instance<128>(d.n_parts) : merge_instance<64>(d.n_parts), dim3((unsigned)blocks), dim3(256),
                          args, 0, (hipStream_t)stream);
    const hipError_t e = hipGetLastError();
    if (e != hipSuccess) { set_error("attn_merge launch: %s", hipGetErrorString(e)); return MILLION_ERR_LAUNCH; }
    return MILLION_OK;
}
