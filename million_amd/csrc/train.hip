// train.hip — PQ codebook training: per-subspace Lloyd k-means, gfx950.
//
// Replaces train_pq (reference scripts/utils/pq_utils.py:586-609: faiss IndexPQ.train, i.e. ProductQuantizer's default
// training: one independent k-means per subspace).  The arithmetic contract is stated in include/million_hip.h
// ("PQ codebook training"); tests/kmeans_ref.py restates it in numpy and tests/test_train_gpu.py compares bit for bit.
//
// One iteration is three launches on the caller's stream:
//   kmeans_assign_kernel   pq_encode_kernel's scheme (encode.hip): lane = point, a wave owns 4 consecutive subspaces of 64
//                          points, the centroid rows are wave-uniform fp32 scalar operands; the distance loop is
//                          pq_scan_sgpr (pq_scan.h).  Codes leave TRANSPOSED, (M, N), so that the update reads one
//                          subspace contiguously; each workgroup leaves one fp64 partial of the objective.
//   kmeans_update_kernel   one wave = (chunk of kTrainChunk rows, subspace, 64 centroids), lane = centroid.  The wave loads
//                          64 rows at a time (lane = row: one code and one sub-vector each), then walks them in row order
//                          with v_readlane: acc += (code == c ? x : +0.0f).  Adding +0.0f never changes a sum that started
//                          from +0.0f (such a sum is never -0.0f), so the select-then-add is bit-identical to the
//                          conditional add of the contract.  Chunk partials (S, M, C, d_m + 1) go to the workspace.
//   kmeans_finish_kernel   one workgroup per subspace: chunk partials added in chunk order, the division, the serial
//                          empty-cluster split (the donor search is a workgroup-wide argmax, largest count, lowest index),
//                          the fp32 table and the counts.  One more workgroup adds the objective partials in a fixed order.
// No atomics anywhere: every bit of the result is fixed by the contract, not by the schedule.  Every workspace byte that is
// read has been written earlier in the same call, so the workspace needs no initialisation.
//
// Roofline: pure vector ALU, as encode.hip.  N = 65536 points x 64 subspaces x 256 centroids = 1.07e9 tests at 6 vector
// instructions each (d_m = 2) = 1.0e8 wave instructions; 1024 SIMDs x one instruction per 4 cycles x ~2.4 GHz: ~0.16 ms per
// iteration (measured 0.21).  The update walks N x M rows once per 64 centroids at 11.5 instructions per row (3 v_readlane,
// compare, 2 selects, 2 adds, count): 65536 x 64 x 4 x 11.5 = 1.9e8 wave instructions, a floor of ~0.31 ms (measured 0.40): it
// is the larger half of an iteration (profiles/train_pq.txt).
#include <string.h>

#include "common.h"
#include "pq_scan.h"

#pragma clang fp contract(off)

namespace million {

constexpr int kTrainChunk = 4096;     // rows per partial sum of the update: depends on N only, never on the grid
constexpr int kAssignBlock = 256;
constexpr int kAssignSub = 4;         // subspaces per wave
constexpr int kFinishBlock = 256;

struct TrainParams {
    const void *x;               // (N, d) fp32 or fp16, row stride xsn elements
    const float *cents;          // table the assign step reads: (M, C, dm)
    float *cents_out;            // table the finish step writes
    int *counts_out;             // (M, C) or null
    double *objective_out;       // this iteration's slot, or null
    const int *init_rows;        // gather only
    void *codes;                 // workspace: (M, N) u8 / u16
    float *partials;             // workspace: (S, M, C, dm + 1), the last word of a row is the int32 count
    double *obj_partials;        // workspace: one per assign workgroup
    long long xsn;
    int n, M, C, dm, S, n_obj;
    float eps_hi, eps_lo;        // 1 + eps, 1 - eps (fp32)
};

template <bool XF32, int DM>
__device__ __forceinline__ void load_sub(const void *x, long long elem, float (&out)[DM]) {
    if constexpr (DM == 1) {
        out[0] = XF32 ? ((const float *)x)[elem] : (float)((const f16 *)x)[elem];
    } else if constexpr (XF32) {
        typedef float fvec __attribute__((ext_vector_type(DM)));
        const fvec v = *(const fvec *)((const float *)x + elem);
#pragma unroll
        for (int k = 0; k < DM; ++k) out[k] = v[k];
    } else {
        typedef f16 hvec __attribute__((ext_vector_type(DM)));
        const hvec v = *(const hvec *)((const f16 *)x + elem);
#pragma unroll
        for (int k = 0; k < DM; ++k) out[k] = (float)v[k];      // exact widening
    }
}

// ---- init: centroid c of every subspace = the sub-vector of row init_rows[c] (row indices are not trusted: clamped) ----
template <bool XF32>
__global__ __launch_bounds__(256) void kmeans_gather_kernel(TrainParams p) {
    const long long total = (long long)p.M * p.C * p.dm;
    for (long long i = (long long)blockIdx.x * 256 + threadIdx.x; i < total; i += (long long)gridDim.x * 256) {
        const int e = (int)(i % p.dm), c = (int)((i / p.dm) % p.C), m = (int)(i / ((long long)p.dm * p.C));
        int row = p.init_rows[c];
        row = row < 0 ? 0 : (row >= p.n ? p.n - 1 : row);
        const long long src = (long long)row * p.xsn + m * p.dm + e;
        p.cents_out[i] = XF32 ? ((const float *)p.x)[src] : (float)((const f16 *)p.x)[src];
    }
}

// ---- assign ----
template <int DM, bool XF32, typename CodeT>
__global__ __launch_bounds__(kAssignBlock) void kmeans_assign_kernel(TrainParams p) {
    __shared__ double wave_obj[kAssignBlock / 64];
    const int lane = threadIdx.x & 63;
    const int w = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
    const int m0 = (int)(blockIdx.y * (kAssignBlock / 64) + w) * kAssignSub;
    const int t = blockIdx.x * 64 + lane;
    const bool valid = t < p.n;
    const int tc = valid ? t : p.n - 1;
    int nsub = p.M - m0;                                          // wave-uniform; <= 0: a wave past the last subspace
    nsub = nsub < 0 ? 0 : (nsub < kAssignSub ? nsub : kAssignSub);
    float x[kAssignSub][DM];
#pragma unroll
    for (int j = 0; j < kAssignSub; ++j) {
        if (j < nsub) load_sub<XF32, DM>(p.x, (long long)tc * p.xsn + (m0 + j) * DM, x[j]);
        else {
#pragma unroll
            for (int k = 0; k < DM; ++k) x[j][k] = 0.f;
        }
    }
    double obj = 0.0;
    CodeT *codes = (CodeT *)p.codes;
#pragma unroll
    for (int j = 0; j < kAssignSub; ++j) {
        if (j >= nsub) break;
        const int m = m0 + j;
        float best = INFINITY;
        int best_c = 0;
        pq_scan_sgpr<DM>(x[j], p.cents + (long long)m * p.C * DM, p.C, best, best_c);      // wave-uniform rows: scalar operands
        if (valid) {
            codes[(long long)m * p.n + t] = (CodeT)best_c;
            obj += (double)best;
        }
    }
    // objective partial of the workgroup: lanes by butterfly, waves in order (a fixed order: two runs give the same bits)
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) obj += __shfl_xor(obj, o, 64);
    if (lane == 0) wave_obj[w] = obj;
    __syncthreads();
    if (threadIdx.x == 0) {
        double s = wave_obj[0];
#pragma unroll
        for (int i = 1; i < kAssignBlock / 64; ++i) s += wave_obj[i];
        p.obj_partials[(long long)blockIdx.y * gridDim.x + blockIdx.x] = s;
    }
}

// ---- update ----
template <int DM, bool XF32, typename CodeT>
__global__ __launch_bounds__(64) void kmeans_update_kernel(TrainParams p) {
    const int lane = threadIdx.x;
    const int c = blockIdx.x * 64 + lane;                        // this lane's centroid
    const int m = blockIdx.y, s = blockIdx.z;
    const int row0 = s * kTrainChunk;
    const int row1 = min(row0 + kTrainChunk, p.n);
    const CodeT *codes = (const CodeT *)p.codes + (long long)m * p.n;
    float acc[DM];
#pragma unroll
    for (int k = 0; k < DM; ++k) acc[k] = 0.f;
    int cnt = 0;
    for (int base = row0; base < row1; base += 64) {
        // lane = row: one code and one sub-vector each (rows past the chunk's end: a code no lane owns, clamped address)
        const int row = base + lane;
        const int rc = row < row1 ? row : row1 - 1;
        const int code = row < row1 ? (int)codes[rc] : -1;
        float xv[DM];
        load_sub<XF32, DM>(p.x, (long long)rc * p.xsn + m * DM, xv);
#pragma unroll
        for (int i = 0; i < 64; ++i) {
            const int ci = __builtin_amdgcn_readlane(code, i);
            const bool mine = ci == c;
#pragma unroll
            for (int k = 0; k < DM; ++k) {
                const float xi = __int_as_float(__builtin_amdgcn_readlane(__float_as_int(xv[k]), i));
                acc[k] = acc[k] + (mine ? xi : 0.f);
            }
            cnt += mine ? 1 : 0;
        }
    }
    if (c < p.C) {
        float *dst = p.partials + (((long long)s * p.M + m) * p.C + c) * (DM + 1);
#pragma unroll
        for (int k = 0; k < DM; ++k) dst[k] = acc[k];
        ((int *)dst)[DM] = cnt;
    }
}

// ---- finish ----
// larger count wins, lowest index on equal counts
__device__ __forceinline__ void donor_pick(int &cnt, int &idx, int ocnt, int oidx) {
    if (ocnt > cnt || (ocnt == cnt && oidx < idx)) { cnt = ocnt; idx = oidx; }
}

__global__ __launch_bounds__(kFinishBlock) void kmeans_finish_kernel(TrainParams p) {
    extern __shared__ int fin_counts[];                          // C ints
    __shared__ int red_cnt[kFinishBlock / 64], red_idx[kFinishBlock / 64];
    __shared__ double red_obj[kFinishBlock];
    const int tid = threadIdx.x;
    const int C = p.C, dm = p.dm, M = p.M;
    if ((int)blockIdx.x == M) {
        // the objective of this iteration's assignment: partials in a fixed order
        if (!p.objective_out) return;
        double s = 0.0;
        for (int i = tid; i < p.n_obj; i += kFinishBlock) s += p.obj_partials[i];
        red_obj[tid] = s;
        __syncthreads();
        if (tid == 0) {
            double tot = red_obj[0];
            for (int i = 1; i < kFinishBlock; ++i) tot += red_obj[i];
            *p.objective_out = tot;
        }
        return;
    }
    const int m = blockIdx.x;
    float *tab = p.cents_out + (long long)m * C * dm;
    const int stride = dm + 1;
    for (int c = tid; c < C; c += kFinishBlock) {
        const float *src = p.partials + ((long long)m * C + c) * stride;
        const long long chunk = (long long)M * C * stride;
        int cnt = ((const int *)src)[dm];
        for (int s = 1; s < p.S; ++s) cnt += ((const int *)src)[s * chunk + dm];
        fin_counts[c] = cnt;
        if (cnt > 0) {
            const float fc = (float)cnt;
            for (int k = 0; k < dm; ++k) {
                float sum = src[k];
                for (int s = 1; s < p.S; ++s) sum = sum + src[s * chunk + k];
                tab[c * dm + k] = sum / fc;
            }
        }
    }
    __syncthreads();
    // empty clusters in ascending order; each takes half of the largest cluster (lowest index on ties)
    for (int c = 0; c < C; ++c) {
        if (fin_counts[c] != 0) continue;                        // workgroup-uniform (LDS, behind a barrier)
        int bc = -1, bi = 0x7fffffff;
        for (int i = tid; i < C; i += kFinishBlock) donor_pick(bc, bi, fin_counts[i], i);
#pragma unroll
        for (int o = 32; o > 0; o >>= 1) donor_pick(bc, bi, __shfl_xor(bc, o, 64), __shfl_xor(bi, o, 64));
        if ((tid & 63) == 0) { red_cnt[tid >> 6] = bc; red_idx[tid >> 6] = bi; }
        __syncthreads();
        bc = red_cnt[0]; bi = red_idx[0];
#pragma unroll
        for (int i = 1; i < kFinishBlock / 64; ++i) donor_pick(bc, bi, red_cnt[i], red_idx[i]);
        if (tid < dm) {
            const float v = tab[bi * dm + tid];
            const bool even = (tid & 1) == 0;
            tab[c * dm + tid] = v * (even ? p.eps_hi : p.eps_lo);
            tab[bi * dm + tid] = v * (even ? p.eps_lo : p.eps_hi);
        }
        __syncthreads();                                         // every thread has read red_* and fin_counts
        if (tid == 0) {
            const int half = bc / 2;
            fin_counts[c] = half;
            fin_counts[bi] = bc - half;
        }
        __syncthreads();
    }
    if (p.counts_out)
        for (int c = tid; c < C; c += kFinishBlock) p.counts_out[(long long)m * C + c] = fin_counts[c];
}

// ---- host side ----
static size_t align_up(size_t v, size_t a) { return (v + a - 1) / a * a; }

// Fills the layout of the workspace; returns its size.
static size_t train_layout(int n, int M, int C, int dm, size_t *off_partials, size_t *off_obj) {
    const size_t code_bytes = C <= 256 ? 1 : 2;
    const size_t S = ((size_t)n + kTrainChunk - 1) / kTrainChunk;
    const size_t groups = ((size_t)M + kAssignSub - 1) / kAssignSub;
    const size_t gy = (groups + kAssignBlock / 64 - 1) / (kAssignBlock / 64);
    const size_t n_obj = (((size_t)n + 63) / 64) * gy;
    const size_t codes = align_up((size_t)M * n * code_bytes, 256);
    const size_t partials = align_up(S * M * C * (dm + 1) * sizeof(float), 256);
    if (off_partials) *off_partials = codes;
    if (off_obj) *off_obj = codes + partials;
    return codes + partials + align_up(n_obj * sizeof(double), 256);
}

static int train_check(const million_train_desc *desc) {
    if (!desc || desc->struct_size != sizeof(million_train_desc)) { set_error("train: bad desc / struct_size"); return MILLION_ERR_ARG; }
    const int n = desc->n, d = desc->d, M = desc->M, C = desc->C;
    if (M <= 0 || d <= 0 || d % M) { set_error("train: d=%d is not a multiple of M=%d", d, M); return MILLION_ERR_SHAPE; }
    const int dm = d / M;
    if (dm != 1 && dm != 2 && dm != 4 && dm != 8) { set_error("train: d/M=%d unsupported (1,2,4,8)", dm); return MILLION_ERR_SHAPE; }
    if (C < 2 || C > 4096) { set_error("train: C=%d outside [2, 4096]", C); return MILLION_ERR_SHAPE; }
    if (n < C) { set_error("train: n=%d points for C=%d centroids (n >= C)", n, C); return MILLION_ERR_SHAPE; }
    if (n >= (1 << 24)) { set_error("train: n=%d (n < 2^24: counts must be exact in fp32)", n); return MILLION_ERR_SHAPE; }
    if (M > 65535) { set_error("train: M=%d exceeds the grid", M); return MILLION_ERR_SHAPE; }
    if (desc->niter < 1) { set_error("train: niter=%d (>= 1)", desc->niter); return MILLION_ERR_ARG; }
    if (desc->x_stride_n < d) { set_error("train: x_stride_n=%lld < d=%d", (long long)desc->x_stride_n, d); return MILLION_ERR_ARG; }
    if (!(desc->eps >= 0.f && desc->eps < 1.f)) { set_error("train: eps=%g outside [0, 1)", (double)desc->eps); return MILLION_ERR_ARG; }
    return MILLION_OK;
}

template <int DM, bool XF32, typename CodeT>
static void launch_iter_kernels(const TrainParams &p, dim3 ga, dim3 gu, hipStream_t s) {
    hipLaunchKernelGGL((kmeans_assign_kernel<DM, XF32, CodeT>), ga, dim3(kAssignBlock), 0, s, p);
    hipLaunchKernelGGL((kmeans_update_kernel<DM, XF32, CodeT>), gu, dim3(64), 0, s, p);
}
template <int DM>
static void launch_iter_dm(const TrainParams &p, bool xf32, dim3 ga, dim3 gu, hipStream_t s) {
    if (p.C <= 256) {
        if (xf32) launch_iter_kernels<DM, true, uint8_t>(p, ga, gu, s); else launch_iter_kernels<DM, false, uint8_t>(p, ga, gu, s);
    } else {
        if (xf32) launch_iter_kernels<DM, true, uint16_t>(p, ga, gu, s); else launch_iter_kernels<DM, false, uint16_t>(p, ga, gu, s);
    }
}

}  // namespace million

using namespace million;

extern "C" {

size_t million_pq_train_workspace_bytes(const million_train_desc *desc) {
    if (train_check(desc) != MILLION_OK) return 0;
    return train_layout(desc->n, desc->M, desc->C, desc->d / desc->M, nullptr, nullptr);
}

int million_pq_train(const million_train_desc *desc, const void *x, const int32_t *init_rows, const float *cents_init,
                     float *cents_out, int32_t *counts_out, double *objective_out, void *workspace, size_t workspace_bytes,
                     million_stream_t stream) {
    const int rc = train_check(desc);
    if (rc != MILLION_OK) return rc;
    if ((init_rows != nullptr) == (cents_init != nullptr)) { set_error("train: exactly one of init_rows and cents_init must be given"); return MILLION_ERR_ARG; }
    if (!x || !cents_out || !workspace) { set_error("train: null pointer"); return MILLION_ERR_ARG; }
    const int dm = desc->d / desc->M;
    const bool xf32 = desc->x_is_f32 != 0;
    const size_t sub_bytes = (size_t)dm * (xf32 ? 4 : 2);       // a sub-vector is one vector load
    if (((uintptr_t)x % sub_bytes) || (desc->x_stride_n % dm)) { set_error("train: x and x_stride_n must be aligned to a sub-vector (%zu bytes)", sub_bytes); return MILLION_ERR_ALIGN; }
    if (((uintptr_t)workspace & 255) || ((uintptr_t)cents_out & 3) || ((uintptr_t)cents_init & 3)) { set_error("train: workspace must be 256-byte aligned, tables 4-byte aligned"); return MILLION_ERR_ALIGN; }
    size_t off_partials = 0, off_obj = 0;
    const size_t need = train_layout(desc->n, desc->M, desc->C, dm, &off_partials, &off_obj);
    if (workspace_bytes < need) { set_error("train: workspace %zu < %zu bytes", workspace_bytes, need); return MILLION_ERR_WORKSPACE; }

    TrainParams p;
    memset(&p, 0, sizeof(p));
    p.x = x; p.cents_out = cents_out; p.counts_out = counts_out; p.init_rows = init_rows;
    p.codes = workspace;
    p.partials = (float *)((char *)workspace + off_partials);
    p.obj_partials = (double *)((char *)workspace + off_obj);
    p.xsn = desc->x_stride_n;
    p.n = desc->n; p.M = desc->M; p.C = desc->C; p.dm = dm;
    p.S = (desc->n + kTrainChunk - 1) / kTrainChunk;
    const float eps = desc->eps > 0.f ? desc->eps : 1.0f / 1024.0f;
    p.eps_hi = 1.0f + eps; p.eps_lo = 1.0f - eps;
    const int groups = (p.M + kAssignSub - 1) / kAssignSub;
    const dim3 ga((p.n + 63) / 64, (groups + kAssignBlock / 64 - 1) / (kAssignBlock / 64));
    const dim3 gu((p.C + 63) / 64, p.M, p.S);
    p.n_obj = (int)(ga.x * ga.y);
    hipStream_t s = (hipStream_t)stream;

    if (init_rows) {
        const long long total = (long long)p.M * p.C * dm;
        const dim3 gg((unsigned)((total + 255) / 256 < 1024 ? (total + 255) / 256 : 1024));
        if (xf32) hipLaunchKernelGGL(kmeans_gather_kernel<true>, gg, dim3(256), 0, s, p);
        else hipLaunchKernelGGL(kmeans_gather_kernel<false>, gg, dim3(256), 0, s, p);
        p.cents = cents_out;
    } else {
        p.cents = cents_init;
    }
    for (int it = 0; it < desc->niter; ++it) {
        p.objective_out = objective_out ? objective_out + it : nullptr;
        dispatch_dm(dm, [&](auto w) { launch_iter_dm<w()>(p, xf32, ga, gu, s); });      // train_check: dm is 1, 2, 4 or 8
        hipLaunchKernelGGL(kmeans_finish_kernel, dim3(p.M + 1), dim3(kFinishBlock), (size_t)p.C * sizeof(int), s, p);
        p.cents = cents_out;
        const hipError_t e = hipGetLastError();
        if (e != hipSuccess) { set_error("train launch (iteration %d): %s", it, hipGetErrorString(e)); return MILLION_ERR_LAUNCH; }
    }
    return MILLION_OK;
}

}  // extern "C"
