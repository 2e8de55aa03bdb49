// pq_scan.h — the nearest-centroid scan of the PQ encoder kernels: pq_encode_kernel and pq_encode_small_kernel (encode.hip),
// kmeans_assign_kernel (train.hip), paged_store_kernel (paged_store.h: the ragged store and the window commit), store_ragged_wide_kernel
// (store_ragged.hip), pq_flush_wide_kernel (flush_wide.hip: pq_scan_lds_chunk).  The scan is written here and nowhere else,
// with one exception: pq_flush_kernel (encode.hip) carries pq_scan_lds's loop in its own body (see there).
//
// Arithmetic contract (bit-exact with oracle/pq_oracle.c:pq_encode_direct): e = x - c, sq = e * e,
// acc = sq_0 + sq_1 + ... sequentially, every operation one IEEE fp32 round-to-nearest, no FMA
// contraction; strict '<' scan over increasing c, so the lowest index wins exact ties.
//
// Both forms update a running (best, best_c) that the caller holds and initialises (best = +inf, best_c = its first
// centroid), so a caller may scan a part of the centroid range and combine the parts in centroid order.  x is the
// sub-vector's DM floats as a plain pointer, not a reference to an array: a `const float (&)[DM]` parameter makes hipcc
// (ROCm 7.2) lay out the callers' prologues differently at DM >= 2 (the record is profiles/pq_scan_refactor.txt, A.3).
#pragma once
#include "common.h"

#pragma clang fp contract(off)

namespace million {

typedef float v2f __attribute__((ext_vector_type(2)));

// Scalar-cache form: `tab` is the wave-uniform row [c][DM] of one subspace (fp32, or fp16: the widening is exact), read
// through the scalar cache as SGPR operands; all C centroids.
template <int DM, typename TabT>
__device__ __forceinline__ void pq_scan_sgpr(const float *x, const TabT *__restrict__ tab, int C, float &best, int &best_c) {
#pragma unroll 16
    for (int c = 0; c < C; ++c) {
        float cv[DM];
#pragma unroll
        for (int k = 0; k < DM; ++k) cv[k] = (float)tab[c * DM + k];
        float acc = 0.f;
        if (DM % 2 == 0) {
            // pairs of dims as packed fp32: every lane-half is one IEEE round-to-nearest operation
#pragma unroll
            for (int k = 0; k < DM; k += 2) {
                const v2f xv = {x[k], x[k + 1]}, cc = {cv[k], cv[k + 1]};
                const v2f e = xv - cc;
                const v2f sq = e * e;
                acc = (k == 0) ? sq[0] : acc + sq[0];
                acc = acc + sq[1];
            }
        } else {
#pragma unroll
            for (int k = 0; k < DM; ++k) {
                const float e = x[k] - cv[k];
                const float sq = e * e;
                acc = (k == 0) ? sq : acc + sq;
            }
        }
        // strict '<', increasing c: the lowest index wins exact ties.  Written as "keep unless smaller" so that the
        // select is (condition ? register : constant): v_cndmask takes the constant c as a literal, no v_mov
        best_c = !(acc < best) ? best_c : c;
        best = fminf(best, acc);
    }
}

// LDS form: `rows` is the fp32 row [c][DM] of one subspace in LDS, read with wave-uniform (broadcast) ds_reads; centroids
// [c0, c1), unrolled UNROLL times (the caller's register budget).
template <int DM, int UNROLL>
__device__ __forceinline__ void pq_scan_lds(const float *x, const float *rows, int c0, int c1, float &best, int &best_c) {
#pragma unroll UNROLL
    for (int c = c0; c < c1; ++c) {
        float acc = 0.f;
#pragma unroll
        for (int k = 0; k < DM; ++k) {
            const float e = x[k] - rows[c * DM + k];
            const float sq = e * e;
            acc = (k == 0) ? sq : acc + sq;
        }
        best_c = acc < best ? c : best_c;
        best = fminf(best, acc);
    }
}

// LDS form over a staged chunk: `rows` holds the n centroids [c_base, c_base + n) of one subspace as fp32 [i][DM] (a part of the
// row that a wave widened from fp16 into LDS: pq_flush_wide_kernel, flush_wide.hip), read with wave-uniform ds_reads; centroid
// i of the chunk is index c_base + i.  Same operations and the same strict '<' as the forms above, so chunks scanned in centroid
// order over one running (best, best_c) give the codes of a scan of the whole range.
template <int DM, int UNROLL>
__device__ __forceinline__ void pq_scan_lds_chunk(const float *x, const float *rows, int n, int c_base, float &best, int &best_c) {
#pragma unroll UNROLL
    for (int i = 0; i < n; ++i) {
        float acc = 0.f;
#pragma unroll
        for (int k = 0; k < DM; ++k) {
            const float e = x[k] - rows[i * DM + k];
            const float sq = e * e;
            acc = (k == 0) ? sq : acc + sq;
        }
        best_c = acc < best ? c_base + i : best_c;
        best = fminf(best, acc);
    }
}

}  // namespace million
