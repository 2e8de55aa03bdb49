// flash_tile.h — the flash-attention tile step shared by the prompt-attention kernels (prefill.hip: prefill_attn_kernel, and in
// part prefill_attn_pipe_kernel) and the chunk-attention kernels (chunk_attn.h: chunk_attn.hip, chunk_attn_wide.hip), gfx950.
//
// Everything is computed TRANSPOSED so that a query row lives on a lane: S^T = K Q^T (A = K rows from LDS, B = Q^T from
// registers, v_mfma_f32_32x32x16_f16): lane (q, h) = lane 32 h + q holds 16 of a 32-key block's scores of query row q; the
// softmax is in-lane plus ONE half-wave exchange; P^T, converted pairwise to fp16, IS the B operand of O^T += V^T P^T (the
// accumulator's row index is the next product's reduction index: no lane movement, no LDS), and the running rescale of O^T is
// lane-local.  fp32 online softmax in the exp2 domain, fp32 accumulation.
//
// A tile is 64 keys of K and of V, each a [64][D] fp16 image in LDS (tile_off) at a compile-time byte base: the kernels address
// LDS absolutely (their dynamic LDS starts at 0), so the base rides in the immediate offset of every ds_read.
// Score layout: sc[16 jt + j] is key 32 jt + 8 (j >> 2) + 4 h + (j & 3) of the tile.  The masks are the callers': they differ.
#pragma once

#include "common.h"

namespace million {

typedef _Float16 v8h __attribute__((ext_vector_type(8)));
typedef float v16f __attribute__((ext_vector_type(16)));
typedef unsigned pv4u __attribute__((ext_vector_type(4)));
typedef short pv4s __attribute__((__vector_size__(4 * sizeof(short))));
typedef __attribute__((address_space(3))) pv4u *lds_v4u_p;
typedef __attribute__((address_space(3))) pv4s *lds_v4s_p;

// LDS image of a [64 keys][D] fp16 tile; tile_off(row, ch) = byte offset of 16-byte chunk ch of a row.  D = 128 (256-byte rows):
// image (b) of cdna_hip_programming.md T10.  D = 64 (128-byte rows, two to a bank row): slot = ((row & 1) << 3 | ch) ^
// (((rp & 1) << 2) | ((rp >> 2) & 3)) with rp = row >> 1 - found by exhaustive search over the linear maps rp -> 4 bits for
// the one that leaves BOTH the ds_read_b128 row reads of the 32x32x16 A operand and the ds_read_b64_tr_b16 reads
// conflict-free (checked lane group by lane group against the bank rules of MI355X_MICROARCH.md, LDS).
template <int D>
constexpr __host__ __device__ __forceinline__ unsigned tile_off(int row, int ch) {
    if (D == 128) return 256u * row + 16u * (ch ^ (((row & 3) << 2) | ((row >> 2) & 3)));
    const int rp = row >> 1;
    return 256u * rp + 16u * ((((row & 1) << 3) | ch) ^ (((rp & 1) << 2) | ((rp >> 2) & 3)));
}

// The inverse: the (row, chunk) that tile_off puts into 16-byte slot `slot` of the image (the kernels that fill a tile with
// global_load_lds_dwordx4 write consecutive slots and apply the swizzle on the global side).
struct TileRC { int row, ch; };
template <int D>
constexpr __host__ __device__ __forceinline__ TileRC tile_rc(int slot) {
    if (D == 128) {
        const int row = slot >> 4;
        return {row, (slot & 15) ^ (((row & 3) << 2) | ((row >> 2) & 3))};
    }
    const int rp = slot >> 4, x = (slot & 15) ^ (((rp & 1) << 2) | ((rp >> 2) & 3));
    return {2 * rp + (x >> 3), x & 7};
}

template <int D>
constexpr bool tile_off_is_bijection() {
    for (int slot = 0; slot < 64 * (D / 8); ++slot) {
        const TileRC rc = tile_rc<D>(slot);
        if (rc.row < 0 || rc.row >= 64 || rc.ch < 0 || rc.ch >= D / 8 || tile_off<D>(rc.row, rc.ch) != 16u * slot) return false;
    }
    return true;
}
static_assert(tile_off_is_bijection<128>() && tile_off_is_bijection<64>(), "tile_rc must invert tile_off over the whole image");

// Q^T fragments, the B operand of the score product: lane (q, h) holds Q[q][16 s + 8 h .. + 8]; `row` = the lane's query row
template <int D>
__device__ __forceinline__ void flash_load_q(v8h (&qf)[D / 16], const f16 *row, int hh) {
    const f16 *qp = row + 8 * hh;
#pragma unroll
    for (int s = 0; s < D / 16; ++s) qf[s] = *(const v8h *)(qp + 16 * s);
}

// S^T = K Q^T over the 64 keys of the K tile at LDS byte KB: two 32-key x 32-query products, unscaled
template <int D, unsigned KB>
__device__ __forceinline__ void flash_scores(float (&sc)[32], const v8h (&qf)[D / 16], int r32, int hh) {
    v16f S0, S1;
#pragma unroll
    for (int j = 0; j < 16; ++j) { S0[j] = 0.f; S1[j] = 0.f; }
#pragma unroll
    for (int s = 0; s < D / 16; ++s) {
        const v8h a0 = __builtin_bit_cast(v8h, ((lds_v4u_p)(size_t)tile_off<D>(r32, 2 * s + hh))[KB / 16]);
        const v8h a1 = __builtin_bit_cast(v8h, ((lds_v4u_p)(size_t)tile_off<D>(32 + r32, 2 * s + hh))[KB / 16]);
        S0 = __builtin_amdgcn_mfma_f32_32x32x16_f16(a0, qf[s], S0, 0, 0, 0);
        S1 = __builtin_amdgcn_mfma_f32_32x32x16_f16(a1, qf[s], S1, 0, 0, 0);
    }
#pragma unroll
    for (int j = 0; j < 16; ++j) { sc[j] = S0[j]; sc[16 + j] = S1[j]; }
}

// Online softmax over the tile's 32 (masked) scores of the lane's row, c = scale log2 e, m_run in the scaled exp2 domain: the row
// maximum of both half-waves (the same query rows), the rescale of O and l (lane-local) when some row's maximum moved, then
// sc <- exp2(c sc - m) and l += their sum.  A row without a visible key so far keeps m = -inf and adds zeros.
template <int NB>
__device__ __forceinline__ void flash_softmax(float (&sc)[32], v16f (&O)[NB], float &m_run, float &l_run, float c) {
    float mx = sc[0];
#pragma unroll
    for (int j = 1; j < 32; ++j) mx = fmaxf(mx, sc[j]);
    {
        const v2u ex = swap32_self(__float_as_uint(mx));
        const unsigned e0 = ex[0], e1 = ex[1];
        mx = fmaxf(__uint_as_float(e0), __uint_as_float(e1));
    }
    const float m_new = fmaxf(m_run, mx * c);
    const float m_safe = m_new > -INFINITY ? m_new : 0.f;
    if (__any(m_new > m_run && m_run > -INFINITY)) {
        const float alpha = __builtin_amdgcn_exp2f(m_run - m_safe);
#pragma unroll
        for (int i = 0; i < NB; ++i)
#pragma unroll
            for (int j = 0; j < 16; ++j) O[i][j] *= alpha;
        l_run *= alpha;
    }
    m_run = m_new;
    float ls = 0.f;
#pragma unroll
    for (int j = 0; j < 32; ++j) {
        sc[j] = __builtin_amdgcn_exp2f(fmaf(sc[j], c, -m_safe));
        ls += sc[j];
    }
    l_run += ls;
}

// O^T += V^T P^T with the V tile at LDS byte VB: P^T registers 8 ks .. 8 ks + 7 of a 32-key block are k-step ks of the B operand;
// the A operand V^T comes from ds_read_b64_tr_b16: element e of lane half h is key 32 jt + 16 ks + 8 (e >> 2) + 4 h + (e & 3),
// its row the value dimension
template <int D, unsigned VB>
__device__ __forceinline__ void flash_pv(v16f (&O)[D / 32], const float (&sc)[32], int lane) {
    const int hh = lane >> 5;
#pragma unroll
    for (int jt = 0; jt < 2; ++jt)
#pragma unroll
        for (int ks = 0; ks < 2; ++ks) {
            typedef _Float16 h2v __attribute__((ext_vector_type(2)));
            unsigned pw[4];
#pragma unroll
            for (int e = 0; e < 4; ++e) {
                const h2v t2 = {(f16)sc[16 * jt + 8 * ks + 2 * e], (f16)sc[16 * jt + 8 * ks + 2 * e + 1]};
                pw[e] = __builtin_bit_cast(unsigned, t2);
            }
            const pv4u pwv = {pw[0], pw[1], pw[2], pw[3]};
            const v8h pb = __builtin_bit_cast(v8h, pwv);
            const int kvr0 = 32 * jt + 16 * ks + 4 * hh;
            const int qd = (lane >> 2) & 3, pp = lane & 3, g16 = (lane >> 4) & 1;      // lane 4 qd + pp of its 16-lane group
#pragma unroll
            for (int blk = 0; blk < D / 32; ++blk) {
                const int chn = 4 * blk + 2 * g16 + (pp >> 1);
                const pv4s lo = __builtin_amdgcn_ds_read_tr16_b64_v4i16((lds_v4s_p)(size_t)(tile_off<D>(kvr0 + qd, chn) + 8 * (pp & 1)) + VB / 8);
                const pv4s hi = __builtin_amdgcn_ds_read_tr16_b64_v4i16((lds_v4s_p)(size_t)(tile_off<D>(kvr0 + 8 + qd, chn) + 8 * (pp & 1)) + VB / 8);
                typedef short v8s __attribute__((ext_vector_type(8)));
                const v8s av = {lo[0], lo[1], lo[2], lo[3], hi[0], hi[1], hi[2], hi[3]};
                O[blk] = __builtin_amdgcn_mfma_f32_32x32x16_f16(__builtin_bit_cast(v8h, av), pb, O[blk], 0, 0, 0);
            }
        }
}

// the row sum l over both half-waves (each holds half of the row's keys)
__device__ __forceinline__ float flash_l_total(float l) {
    const v2u ex = swap32_self(__float_as_uint(l));
    const unsigned e0 = ex[0], e1 = ex[1];
    return __uint_as_float(e0) + __uint_as_float(e1);
}

// O / l as fp16 into the lane's output row `row`: lane (q, h) holds dims 32 blk + 8 i + 4 h + (0..3); l = 0 (no visible key) writes 0
template <int NB>
__device__ __forceinline__ void flash_store_row(const v16f (&O)[NB], float l, f16 *row, int hh) {
    const float inv = l > 0.f ? 1.0f / l : 0.f;
    f16 *op = row + 4 * hh;
#pragma unroll
    for (int blk = 0; blk < NB; ++blk)
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            typedef f16 h4 __attribute__((ext_vector_type(4)));
            const h4 o = {(f16)(O[blk][4 * i] * inv), (f16)(O[blk][4 * i + 1] * inv), (f16)(O[blk][4 * i + 2] * inv),
                          (f16)(O[blk][4 * i + 3] * inv)};
            *(h4 *)(op + 32 * blk + 8 * i) = o;
        }
}

// the lane's part of an output row as zeros (the layout of flash_store_row): rows past a request's own length in a ragged batch
template <int NB>
__device__ __forceinline__ void flash_store_zero_row(f16 *row, int hh) {
    typedef f16 h4 __attribute__((ext_vector_type(4)));
    const h4 z = {(f16)0.f, (f16)0.f, (f16)0.f, (f16)0.f};
#pragma unroll
    for (int blk = 0; blk < NB; ++blk)
#pragma unroll
        for (int i = 0; i < 4; ++i) *(h4 *)(row + 4 * hh + 32 * blk + 8 * i) = z;
}

}  // namespace million
