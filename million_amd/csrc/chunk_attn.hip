// chunk_attn.hip — a block of new query tokens attended to the PQ-coded cache (chunked prefill, multi-turn, draft
// verification), gfx950.
//
//   out[b,h,i,:] = softmax_j( q[b,h,i,:] . Kall[b,hk,j,:] / sqrt(d) ) Vall[b,hk,j,:],   hk = h / G
//   Kall = [ dequant(K codes, T tokens) ; window rows (r rows of the ring, from resid_start) ; chunk rows 0 .. n_c - 1 ]
//   every row sees the T + r past keys; chunk key j is visible to row i iff j <= i (n_c = n_q) - n_c = 0: past only.
//
// Design
//   * the flash-attention tile step of prefill_attn_kernel, shared through flash_tile.h: S^T = K Q^T with
//     v_mfma_f32_32x32x16_f16, a query row on a lane, in-lane online softmax in the exp2 domain, O^T += V^T P^T with V^T read by
//     ds_read_b64_tr_b16 from the same tile_off LDS image; only the mask is this kernel's own.  The G query heads of a kv head are flattened, rho = i G + g, so a
//     workgroup of 8 waves holds 256 consecutive rows of one (b, kv head) and a wave's 32 rows have a monotone causal limit.
//   * three producers fill ONE [64 keys][D] K and V tile image: (a) 64 tokens of codes, dequantised through both codebooks held
//     in LDS (the row image [m][c][d_m] of million_prepare_cents: the gather of pq_decode, bit for bit); (b) window rows read
//     through the ring; (c) chunk rows.  A tile holds one source; its rows past the source's end are written as zeros and
//     masked, and a code byte is clamped to C - 1 before it indexes the codebook: nothing outside the valid data reaches an
//     MFMA, whatever the pages hold past T (the kernel is total).  Dequantised once per workgroup, the tile serves all 8 waves.
//   * LDS: K + V tile (single-buffered, 2 x 64 x D x 2 B) + the two codebook images (2 x C x D x 2 B): 160 KiB at C = 256,
//     d = 128 - the whole gfx950 CU.  The next tile's code bytes / fp16 rows are loaded into registers while the current tile
//     is computed; two barriers per tile.
//   * the visible tiles of a query block ([codes | window | chunk up to the block's last row]) are cut into S contiguous
//     ranges, one per split (chunk_splits: host logic).  S = 1 writes fp16 out directly; otherwise each split writes
//     unnormalised fp32 O and (m, l) per row to the workspace and chunk_merge_kernel combines them: two plain launches, no
//     atomics, nothing in the workspace has to be initialised.
//   * ragged batches (desc->dev_lengths / dev_n_q): the RAGGED instances read T, r, resid_start and the valid query rows of
//     their request on the device and clamp them; grid, S and workspace are those of the bounds, every request's own tiles
//     are cut into the S ranges (empty ranges write m = -inf, l = 0), rows past a request's n_q are stored as zeros.  The
//     lockstep instances (RAGGED = false) are the kernel without any of it.
//   * linear block id: kv head fastest (a kv head's codes stay on one XCD's L2), then split, then query block, then batch.
#include <math.h>
#include <string.h>

#include "flash_tile.h"

namespace million {

namespace {

constexpr int kKeys = 64;            // keys per tile
constexpr int kRowsWG = 256;         // flattened query rows per workgroup (8 waves x 32)
constexpr int kThreads = 512;

struct ChunkParams {
    const f16 *q, *kc, *vc;                   // queries, chunk K / V
    const uint8_t *kcodes, *vcodes;           // row-major codes or page pools
    const void *kids, *vids;                  // page ids (PAGED sides)
    const f16 *ktab, *vtab;                   // prepared row images [m][c][d_m]
    const f16 *kres, *vres;                   // window rings (bs, nh_k, resid_cap, d)
    f16 *out;
    float *ws_o, *ws_ml;                      // split partials (S > 1)
    int bs, nh, nh_k, G, M, C;
    int n_q, n_c, T, r, rs, rcap;
    long long res_sb, res_sh;
    int k_paged, v_paged, ps, n_pages_cap, ids64;
    long long k_sb, k_sh, v_sb, v_sh;         // row-major code strides, bytes
    long long q_sb, q_sh, q_sn, kc_sb, kc_sh, kc_sn, vc_sb, vc_sh, vc_sn, o_sb, o_sh, o_sn;      // fp16 elements
    int nrows;                                // n_q * G
    int n_qb;                                 // query blocks per (b, kv head)
    int S;                                    // splits
    int ntT, ntR;                             // code tiles, window tiles
    int cb_bytes;                             // one codebook image in LDS (0: no code tiles)
    float scale_log2e;
    const int *dev_lengths;                   // RAGGED: (bs, 4) {T, r, resid_start, ticket} per request, or null (host T / r / rs)
    const int *dev_n_q;                       // RAGGED: (bs,) valid query rows per request, or null (n_q)
    float *lse;                               // LSE instances: (bs, nh, n_q) fp32 log-sum-exp of each row's visible scores (million_hip.h); last, so
                                              // that no other argument moves: the instances without it are the code they were
#ifdef MILLION_DEBUG_CHECK_IDS
    int lds_fill;                             // dynamic LDS bytes of the launch: debug_fill_lds (common.h)
#endif
};

__device__ __forceinline__ long long ca_page(const ChunkParams &p, const void *ids, int b, int hk, int pg) {
    const long long i = ((long long)b * p.nh_k + hk) * p.n_pages_cap + pg;
    return p.ids64 ? ((const long long *)ids)[i] : (long long)((const int *)ids)[i];
}

// NM = 8 / d_m code bytes of token `tok`, subspaces m0 .. m0 + NM - 1, packed little-endian
template <int NM>
__device__ __forceinline__ unsigned long long ca_load_codes(const ChunkParams &p, bool is_v, int b, int hk, int tok, int m0) {
    const bool paged = is_v ? p.v_paged : p.k_paged;
    const uint8_t *base = is_v ? p.vcodes : p.kcodes;
    const uint8_t *src;
    if (!paged) {
        src = base + b * (is_v ? p.v_sb : p.k_sb) + hk * (is_v ? p.v_sh : p.k_sh) + (long long)tok * p.M + m0;
    } else {
        const long long pg = ca_page(p, is_v ? p.vids : p.kids, b, hk, tok / p.ps);
        const int o = tok - (tok / p.ps) * p.ps;
        if (is_v) {      // transposed page (M, ps): one byte per subspace, ps apart
            src = base + pg * p.M * p.ps + (long long)m0 * p.ps + o;
            unsigned long long w = 0;
#pragma unroll
            for (int e = 0; e < NM; ++e) w |= (unsigned long long)src[(long long)e * p.ps] << (8 * e);
            return w;
        }
        src = base + pg * p.ps * p.M + (long long)o * p.M + m0;
    }
    if (NM == 8) return *(const unsigned long long *)src;
    if (NM == 4) return *(const unsigned *)src;
    if (NM == 2) return *(const unsigned short *)src;
    return *src;
}

// 8 fp16 of one 16-byte chunk from NM codes through a codebook row image at LDS byte offset `tab`: NM reads of d_m fp16
template <int DM>
__device__ __forceinline__ pv4u ca_dequant(unsigned long long w, unsigned tab, int m0, int C) {
    constexpr int NM = 8 / DM;
    unsigned u[4];
#pragma unroll
    for (int e = 0; e < NM; ++e) {
        int c = (int)((w >> (8 * e)) & 0xffu);
        c = c < C ? c : C - 1;      // totality: a byte past the valid codes still reads a centroid
        const unsigned a = tab + 2u * (unsigned)(((m0 + e) * C + c) * DM);
        if (DM == 8) {
            const pv4u x = *(const __attribute__((address_space(3))) pv4u *)(size_t)a;
            u[0] = x[0]; u[1] = x[1]; u[2] = x[2]; u[3] = x[3];
        } else if (DM == 4) {
            typedef unsigned u2 __attribute__((ext_vector_type(2)));
            const u2 x = *(const __attribute__((address_space(3))) u2 *)(size_t)a;
            u[2 * e] = x[0]; u[2 * e + 1] = x[1];
        } else if (DM == 2) {
            u[e] = *(const __attribute__((address_space(3))) unsigned *)(size_t)a;
        } else {
            const unsigned x = *(const __attribute__((address_space(3))) unsigned short *)(size_t)a;
            u[e >> 1] = (e & 1) ? (u[e >> 1] | (x << 16)) : x;
        }
    }
    const pv4u v = {u[0], u[1], u[2], u[3]};
    return v;
}

// RAGGED: a request's valid query rows, never trusted (its lengths row: load_len_row of common.h, T into [0, the bound p.T])
__device__ __forceinline__ int ca_load_n_q(const ChunkParams &p, int b) { return clamp_count(p.dev_n_q[b], p.n_q); }
// the log-sum-exp slot of query row qi of head `head`: indexed like out without the d axis, contiguous
__device__ __forceinline__ float *ca_lse_at(const ChunkParams &p, int b, int head, int qi) {
    return p.lse + ((long long)b * p.nh + head) * p.n_q + qi;
}

// RAGGED: T, r, resid_start (dev_lengths) and the valid query rows (dev_n_q) are per request, read on the device; the grid,
// the split count S and the workspace rows are those of the bounds p.T / p.n_q.  A request's tiles are cut into the same S
// ranges, so a range may be empty: such a split writes m = -inf, l = 0, which the merge skips.
// LSE: the instances that also store every row's log-sum-exp (common.h, "Log-sum-exp"); the others are the kernel without it
template <int D, int DM, bool RAGGED, bool LSE>
__global__ __launch_bounds__(kThreads, 1) void chunk_attn_kernel(ChunkParams p) {
    constexpr int DS = D / 16;                    // k-steps of the score product
    constexpr int NB = D / 32;                    // 32-row blocks of O^T
    constexpr int CH = D / 8;                     // 16-byte chunks per row
    constexpr int CPT = kKeys * CH / kThreads;    // chunks per thread and tile side (2 / 1)
    constexpr int NM = 8 / DM;                    // subspaces per chunk
    constexpr unsigned kTileBytes = kKeys * 2 * D;
    extern __shared__ __attribute__((aligned(16))) char ca_smem[];      // [K tile | V tile | K codebook | V codebook]
    MILLION_DEBUG_FILL_LDS(ca_smem, p.lds_fill);
    if ((unsigned)(size_t)(__attribute__((address_space(3))) char *)ca_smem != 0u) __builtin_trap();      // absolute LDS addressing
    const int tid = threadIdx.x, lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int r32 = lane & 31, hh = lane >> 5;
    int id = blockIdx.x;
    const int hk = id % p.nh_k;
    id /= p.nh_k;
    const int s = id % p.S;
    id /= p.S;
    const int qb = p.n_qb - 1 - id % p.n_qb;      // heaviest (most chunk tiles) first
    const int b = id / p.n_qb;
    const int rho_lo = qb * kRowsWG + wave * 32;   // this wave's first flattened row
    const int rho = rho_lo + r32;
    // ---- this request's lengths: the launch's own, or (RAGGED) its device row ----
    int T = p.T, r = p.r, rs = p.rs, ntT = p.ntT, ntR = p.ntR, n_c = p.n_c, nrows = p.nrows;
    if (RAGGED) {
        if (p.dev_lengths) {
            load_len_row(p.dev_lengths + 4 * b, p.T, p.rcap, p.rcap, T, r, rs);
            ntT = (T + kKeys - 1) / kKeys;
            ntR = (r + kKeys - 1) / kKeys;
        }
        if (p.dev_n_q) {
            const int nq = ca_load_n_q(p, b);
            nrows = nq * p.G;
            n_c = p.n_c > 0 ? nq : 0;
        }
    }
    const bool wg_live = !RAGGED || qb * kRowsWG < nrows;      // RAGGED: a block past the request's rows has no tile, its out rows are zeros
    const bool wave_live = rho_lo < nrows;         // wave-uniform
    const int rho_c = rho < nrows ? rho : (wg_live ? nrows - 1 : 0);
    const int qi = rho_c / p.G, head = hk * p.G + (rho_c - qi * p.G);
    const int w_last = (rho_lo + 31 < nrows ? rho_lo + 31 : nrows - 1);
    const int wave_i_hi = (w_last > 0 ? w_last : 0) / p.G;                     // last query index of the wave
    const int wg_last = qb * kRowsWG + kRowsWG - 1 < nrows ? qb * kRowsWG + kRowsWG - 1 : nrows - 1;
    const int wg_i_hi = wg_last / p.G;
    // ---- the visible tiles of this query block and this split's range of them ----
    const int ntC_all = (n_c + kKeys - 1) / kKeys;
    const int ntC = n_c > 0 ? (wg_i_hi / kKeys + 1 < ntC_all ? wg_i_hi / kKeys + 1 : ntC_all) : 0;
    const int nt = wg_live ? ntT + ntR + ntC : 0;
    const int t_beg = (int)((long long)s * nt / p.S), t_end = (int)((long long)(s + 1) * nt / p.S);

    v8h qf[DS];
    flash_load_q<D>(qf, p.q + b * p.q_sb + head * p.q_sh + (long long)qi * p.q_sn, hh);
    const unsigned cbK = 2u * kTileBytes, cbV = cbK + (unsigned)p.cb_bytes;
    if ((!RAGGED || t_beg < t_end) && t_beg < ntT) {      // this split dequantises: both codebooks into LDS (made visible by the loop's first barrier)
        const pv4u *sk = (const pv4u *)p.ktab, *sv = (const pv4u *)p.vtab;
        for (int o = tid; o < p.cb_bytes / 16; o += kThreads) {
            *(pv4u *)(ca_smem + cbK + 16 * o) = sk[o];
            *(pv4u *)(ca_smem + cbV + 16 * o) = sv[o];
        }
    }

    // ---- producers: a tile's raw bytes (codes, or fp16 rows) into registers, then dequantised / copied into LDS ----
    pv4u rk[CPT], rv[CPT];
    auto tile_src = [&](int t, int &kind, int &j0, int &nv) {      // kind 0 codes, 1 window, 2 chunk
        if (t < ntT) { kind = 0; j0 = t * kKeys; nv = T - j0; }
        else if (t < ntT + ntR) { kind = 1; j0 = (t - ntT) * kKeys; nv = r - j0; }
        else { kind = 2; j0 = (t - ntT - ntR) * kKeys; nv = n_c - j0; }
        nv = nv < kKeys ? nv : kKeys;
    };
    auto load_raw = [&](int t) {
        int kind, j0, nv;
        tile_src(t, kind, j0, nv);
#pragma unroll
        for (int k = 0; k < CPT; ++k) {
            const int c = tid + kThreads * k, row = c / CH, ch = c % CH;
            const pv4u z = {0u, 0u, 0u, 0u};
            rk[k] = z;
            rv[k] = z;
            if (row < nv) {
                const int j = j0 + row;
                if (kind == 0) {
                    const unsigned long long wk = ca_load_codes<NM>(p, false, b, hk, j, ch * NM);
                    const unsigned long long wv = ca_load_codes<NM>(p, true, b, hk, j, ch * NM);
                    rk[k][0] = (unsigned)wk; rk[k][1] = (unsigned)(wk >> 32);
                    rv[k][0] = (unsigned)wv; rv[k][1] = (unsigned)(wv >> 32);
                } else if (kind == 1) {
                    int rr = rs + j;
                    rr = rr < p.rcap ? rr : rr - p.rcap;
                    const long long o = b * p.res_sb + hk * p.res_sh + (long long)rr * (CH * 8) + 8 * ch;
                    rk[k] = *(const pv4u *)(p.kres + o);
                    rv[k] = *(const pv4u *)(p.vres + o);
                } else {
                    rk[k] = *(const pv4u *)(p.kc + b * p.kc_sb + hk * p.kc_sh + (long long)j * p.kc_sn + 8 * ch);
                    rv[k] = *(const pv4u *)(p.vc + b * p.vc_sb + hk * p.vc_sh + (long long)j * p.vc_sn + 8 * ch);
                }
            }
        }
    };
    auto produce = [&](int t) {
        int kind, j0, nv;
        tile_src(t, kind, j0, nv);
#pragma unroll
        for (int k = 0; k < CPT; ++k) {
            const int c = tid + kThreads * k, row = c / CH, ch = c % CH;
            pv4u kx = rk[k], vx = rv[k];
            if (kind == 0 && row < nv) {
                kx = ca_dequant<DM>((unsigned long long)rk[k][0] | ((unsigned long long)rk[k][1] << 32), cbK, ch * NM, p.C);
                vx = ca_dequant<DM>((unsigned long long)rv[k][0] | ((unsigned long long)rv[k][1] << 32), cbV, ch * NM, p.C);
            }
            *(pv4u *)(ca_smem + tile_off<D>(row, ch)) = kx;
            *(pv4u *)(ca_smem + kTileBytes + tile_off<D>(row, ch)) = vx;
        }
    };

    v16f O[NB];
#pragma unroll
    for (int i = 0; i < NB; ++i)
#pragma unroll
        for (int j = 0; j < 16; ++j) O[i][j] = 0.f;
    float m_run = -INFINITY, l_run = 0.f;      // m in the scaled exp2 domain
    const float cs = p.scale_log2e;

    if (t_beg < t_end) load_raw(t_beg);
    for (int t = t_beg; t < t_end; ++t) {
        __syncthreads();      // the previous tile's reads are done (first tile: the codebooks are in LDS)
        produce(t);
        __syncthreads();
        if (t + 1 < t_end) load_raw(t + 1);      // in flight during this tile's products
        int kind, j0, nv;
        tile_src(t, kind, j0, nv);
        const bool live = wave_live && (kind != 2 || j0 <= wave_i_hi);      // wave-uniform
        if (!live) continue;
        float sc[32];
        flash_scores<D, 0>(sc, qf, r32, hh);
        // ---- mask (rows past the source's end; chunk keys after the row's own position), online softmax ----
        if (nv < kKeys || kind == 2) {
            int lim = nv - 1;                                     // last key of the tile this row sees
            if (kind == 2) lim = qi - j0 < lim ? qi - j0 : lim;
            const int rel = lim - 4 * hh;                         // key 32 (j >> 4) + 8 ((j & 15) >> 2) + (j & 3) + 4 hh: compares against immediates
#pragma unroll
            for (int j = 0; j < 32; ++j) sc[j] = 32 * (j >> 4) + (j & 3) + 8 * ((j & 15) >> 2) <= rel ? sc[j] : -INFINITY;
        }
        flash_softmax(sc, O, m_run, l_run, cs);
        flash_pv<D, kTileBytes>(O, sc, lane);
    }
    // ---- epilogue: lane (q, h) holds dims 32 blk + 8 i + 4 h + (0..3) of its row ----
    l_run = flash_l_total(l_run);
    if (RAGGED && rho >= nrows) {      // a row past the request's n_q: zeros (S > 1: by the merge, which does not read the workspace for it)
        if (p.S == 1 && rho < p.nrows) {
            const int qz = rho / p.G;
            flash_store_zero_row<NB>(p.out + b * p.o_sb + (hk * p.G + (rho - qz * p.G)) * p.o_sh + (long long)qz * p.o_sn, hh);
            if constexpr (LSE) if (hh == 0) *ca_lse_at(p, b, hk * p.G + (rho - qz * p.G), qz) = -INFINITY;
        }
        return;
    }
    if (!wave_live || rho >= p.nrows) return;
    if (p.S == 1) {
        flash_store_row(O, l_run, p.out + b * p.o_sb + head * p.o_sh + (long long)qi * p.o_sn, hh);
        // both half-waves hold the row's m and total l; a row without a visible key: m = -inf, l = 0
        if constexpr (LSE) if (hh == 0) *ca_lse_at(p, b, head, qi) = lse_of(m_run > -INFINITY ? m_run : 0.f, l_run);
        return;
    }
    const long long wrow = (((long long)b * p.nh_k + hk) * p.S + s) * p.nrows + rho;
    float *wo = p.ws_o + wrow * D + 4 * hh;
#pragma unroll
    for (int blk = 0; blk < NB; ++blk)
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            typedef float f4 __attribute__((ext_vector_type(4)));
            const f4 o = {O[blk][4 * i], O[blk][4 * i + 1], O[blk][4 * i + 2], O[blk][4 * i + 3]};
            *(f4 *)(wo + 32 * blk + 8 * i) = o;
        }
    if (hh == 0) {
        typedef float f2 __attribute__((ext_vector_type(2)));
        const f2 ml = {m_run, l_run};
        *(f2 *)(p.ws_ml + 2 * wrow) = ml;
    }
}

// ---- merge of the splits: one thread per (row, 8 dims) ----
template <int D, bool RAGGED, bool LSE>
__global__ __launch_bounds__(256) void chunk_merge_kernel(ChunkParams p) {
    constexpr int TPR = D / 8;
    const long long gid = (long long)blockIdx.x * 256 + threadIdx.x;
    const long long row = gid / TPR;
    const int part = (int)(gid - row * TPR);
    if (row >= (long long)p.bs * p.nh_k * p.nrows) return;
    const int rho = (int)(row % p.nrows);
    const long long bh = row / p.nrows;
    const int hk = (int)(bh % p.nh_k), b = (int)(bh / p.nh_k);
    typedef f16 h8 __attribute__((ext_vector_type(8)));
    if (RAGGED && p.dev_n_q && rho >= ca_load_n_q(p, b) * p.G) {      // past the request's n_q: no split wrote this row
        const int qz = rho / p.G;
        const h8 z = {(f16)0.f, (f16)0.f, (f16)0.f, (f16)0.f, (f16)0.f, (f16)0.f, (f16)0.f, (f16)0.f};
        *(h8 *)(p.out + b * p.o_sb + (hk * p.G + (rho - qz * p.G)) * p.o_sh + (long long)qz * p.o_sn + 8 * part) = z;
        if constexpr (LSE) if (part == 0) *ca_lse_at(p, b, hk * p.G + (rho - qz * p.G), qz) = -INFINITY;
        return;
    }
    float mx = -INFINITY;
    for (int s = 0; s < p.S; ++s) mx = fmaxf(mx, p.ws_ml[2 * ((bh * p.S + s) * p.nrows + rho)]);
    float L = 0.f, acc[8];
#pragma unroll
    for (int e = 0; e < 8; ++e) acc[e] = 0.f;
    if (mx > -INFINITY) {
        for (int s = 0; s < p.S; ++s) {
            const long long wrow = (bh * p.S + s) * p.nrows + rho;
            const float m = p.ws_ml[2 * wrow], l = p.ws_ml[2 * wrow + 1];
            if (!(m > -INFINITY)) continue;      // a split without a visible key for this row
            const float w = exp2f(m - mx);
            L += w * l;
            const float *o = p.ws_o + wrow * D + 8 * part;
#pragma unroll
            for (int e = 0; e < 8; ++e) acc[e] += w * o[e];
        }
    }
    const float inv = L > 0.f ? 1.0f / L : 0.f;
    const int qi = rho / p.G, head = hk * p.G + (rho - qi * p.G);
    h8 v;
#pragma unroll
    for (int e = 0; e < 8; ++e) v[e] = (f16)(acc[e] * inv);
    *(h8 *)(p.out + b * p.o_sb + head * p.o_sh + (long long)qi * p.o_sn + 8 * part) = v;
    if constexpr (LSE) if (part == 0) *ca_lse_at(p, b, head, qi) = lse_of(mx > -INFINITY ? mx : 0.f, L);
}

constexpr int kChunkTargetWGs = 256;     // one workgroup per MI355X CU (the LDS budget at C = 256 admits one)
constexpr int kChunkMaxSplits = 64;

template <int D, int DM, bool RAGGED, bool LSE>
void launch_chunk_r(const ChunkParams &p, long long blocks, int lds, hipStream_t s) {
#ifdef MILLION_DEBUG_CHECK_IDS
    ChunkParams pf = p;
    pf.lds_fill = lds;      // debug_fill_lds (common.h)
    hipLaunchKernelGGL((chunk_attn_kernel<D, DM, RAGGED, LSE>), dim3((unsigned)blocks), dim3(kThreads), lds, s, pf);
#else
    hipLaunchKernelGGL((chunk_attn_kernel<D, DM, RAGGED, LSE>), dim3((unsigned)blocks), dim3(kThreads), lds, s, p);
#endif
}
template <int D, int DM>
void launch_chunk_t(const ChunkParams &p, long long blocks, int lds, hipStream_t s) {
    const bool ragged = p.dev_lengths || p.dev_n_q;
    if (p.lse) { if (ragged) launch_chunk_r<D, DM, true, true>(p, blocks, lds, s); else launch_chunk_r<D, DM, false, true>(p, blocks, lds, s); }
    else if (ragged) launch_chunk_r<D, DM, true, false>(p, blocks, lds, s);
    else launch_chunk_r<D, DM, false, false>(p, blocks, lds, s);
}
template <int D, bool RAGGED>
void launch_chunk_merge(const ChunkParams &p, long long mblocks, hipStream_t s) {
    if (p.lse) hipLaunchKernelGGL((chunk_merge_kernel<D, RAGGED, true>), dim3((unsigned)mblocks), dim3(256), 0, s, p);
    else hipLaunchKernelGGL((chunk_merge_kernel<D, RAGGED, false>), dim3((unsigned)mblocks), dim3(256), 0, s, p);
}

void chunk_attrs_once() {
    if (!device_once(4)) return;
    const int mx = 160 * 1024;
#define CA_ATTR(D, DM)                                                                                                          \
    (void)hipFuncSetAttribute((const void *)chunk_attn_kernel<D, DM, false, false>, hipFuncAttributeMaxDynamicSharedMemorySize, mx); \
    (void)hipFuncSetAttribute((const void *)chunk_attn_kernel<D, DM, true, false>, hipFuncAttributeMaxDynamicSharedMemorySize, mx);  \
    (void)hipFuncSetAttribute((const void *)chunk_attn_kernel<D, DM, false, true>, hipFuncAttributeMaxDynamicSharedMemorySize, mx);  \
    (void)hipFuncSetAttribute((const void *)chunk_attn_kernel<D, DM, true, true>, hipFuncAttributeMaxDynamicSharedMemorySize, mx)
    CA_ATTR(128, 2); CA_ATTR(128, 4); CA_ATTR(128, 8); CA_ATTR(64, 1); CA_ATTR(64, 2); CA_ATTR(64, 4);
#undef CA_ATTR
}

}  // namespace

// Splits of the past: enough workgroups for every CU where the context allows, never more splits than code tiles (every
// split owns >= 1 tile), at most 64.  A pure function of (bs, nh_k, query blocks, T).
int chunk_splits(int bs, int nh_k, int n_qb, int T) {
    const long long blocks = (long long)bs * nh_k * n_qb;
    const long long ntT = ((long long)T + kKeys - 1) / kKeys;
    if (blocks <= 0) return 1;
    long long S = (kChunkTargetWGs + blocks - 1) / blocks;
    if (S > ntT) S = ntT;
    if (S > kChunkMaxSplits) S = kChunkMaxSplits;
    return S < 1 ? 1 : (int)S;
}

static bool chunk_geometry(const million_chunk_attn_desc *d, int &n_qb, int &S, size_t &ws) {
    if (!d || d->struct_size != sizeof(million_chunk_attn_desc) || d->bs <= 0 || d->nh_k <= 0 || d->nh <= 0 || d->nh % d->nh_k ||
        d->n_q < 0 || d->n_tokens < 0 || (d->d != 64 && d->d != 128))
        return false;
    const long long rows = (long long)d->n_q * (d->nh / d->nh_k);
    if (rows > 0x7fffffffLL) return false;
    n_qb = (int)((rows + kRowsWG - 1) / kRowsWG);
    S = chunk_splits(d->bs, d->nh_k, n_qb, d->n_tokens);
    ws = S > 1 ? (size_t)d->bs * d->nh_k * S * rows * (d->d + 2) * sizeof(float) : 0;
    return true;
}

}  // namespace million

using namespace million;

extern "C" size_t million_chunk_attn_workspace_bytes(const million_chunk_attn_desc *desc) {
    int n_qb, S;
    size_t ws;
    return chunk_geometry(desc, n_qb, S, ws) ? ws : 0;
}

static int chunk_attn_impl(const million_chunk_attn_desc *desc, const void *q, const void *k_chunk, const void *v_chunk,
                           const void *k_codes, const void *v_codes, const void *k_page_ids, const void *v_page_ids,
                           const void *k_cents_prepared, const void *v_cents_prepared, const void *k_resid,
                           const void *v_resid, void *out, float *lse, void *workspace, size_t workspace_bytes,
                           million_stream_t stream) {
    if (!desc || desc->struct_size != sizeof(million_chunk_attn_desc)) { set_error("chunk_attn: bad desc / struct_size"); return MILLION_ERR_ARG; }
    const million_chunk_attn_desc &d = *desc;
    if (d.bs <= 0 || d.nh <= 0 || d.nh_k <= 0 || d.nh % d.nh_k) { set_error("chunk_attn: bs=%d nh=%d nh_k=%d", d.bs, d.nh, d.nh_k); return MILLION_ERR_SHAPE; }
    if (!u8_geometry("chunk_attn", d.d, d.M, d.C)) return MILLION_ERR_SHAPE;
    if (d.n_q < 0 || (d.n_c != 0 && d.n_c != d.n_q)) { set_error("chunk_attn: n_q=%d n_c=%d (n_c must be 0 or n_q)", d.n_q, d.n_c); return MILLION_ERR_SHAPE; }
    const bool dev_len = d.dev_lengths != nullptr;      // n_tokens is then the bound; r and resid_start are not read
    if (d.n_tokens < 0 || d.resid_cap < 0 ||
        (!dev_len && (d.r < 0 || d.r > d.resid_cap || (d.r > 0 && (d.resid_start < 0 || d.resid_start >= d.resid_cap))))) {
        set_error("chunk_attn: n_tokens=%d r=%d resid_start=%d resid_cap=%d", d.n_tokens, d.r, d.resid_start, d.resid_cap);
        return MILLION_ERR_ARG;
    }
    if ((d.k_layout != MILLION_KV_ROWMAJOR && d.k_layout != MILLION_KV_PAGED) || (d.v_layout != MILLION_KV_ROWMAJOR && d.v_layout != MILLION_KV_PAGED)) {
        set_error("chunk_attn: k_layout=%d v_layout=%d", d.k_layout, d.v_layout);
        return MILLION_ERR_ARG;
    }
    const bool any_paged = d.k_layout == MILLION_KV_PAGED || d.v_layout == MILLION_KV_PAGED;
    if (any_paged && d.n_tokens > 0) {
        int ps_shift;      // the kernel divides by p.ps
        if (!page_shift("chunk_attn", d.page_size, ps_shift)) return MILLION_ERR_SHAPE;
        if ((long long)d.n_pages_cap * d.page_size < d.n_tokens) { set_error("chunk_attn: %d pages of %d tokens hold fewer than n_tokens=%d", d.n_pages_cap, d.page_size, d.n_tokens); return MILLION_ERR_SHAPE; }
    }
    if (d.n_q == 0) return MILLION_OK;
    if (!q || !out) { set_error("chunk_attn: null q / out"); return MILLION_ERR_ARG; }
    if (d.n_c > 0 && (!k_chunk || !v_chunk)) { set_error("chunk_attn: null chunk K / V with n_c=%d", d.n_c); return MILLION_ERR_ARG; }
    if ((dev_len ? d.resid_cap > 0 : d.r > 0) && (!k_resid || !v_resid)) {
        set_error("chunk_attn: null window with r=%d resid_cap=%d", dev_len ? -1 : d.r, d.resid_cap);
        return MILLION_ERR_ARG;
    }
    if (d.n_tokens > 0 && (!k_codes || !v_codes || !k_cents_prepared || !v_cents_prepared ||
                           (d.k_layout == MILLION_KV_PAGED && !k_page_ids) || (d.v_layout == MILLION_KV_PAGED && !v_page_ids))) {
        set_error("chunk_attn: null codes / prepared codebooks / page ids with n_tokens=%d", d.n_tokens);
        return MILLION_ERR_ARG;
    }
    int n_qb, S;
    size_t need;
    if (!chunk_geometry(desc, n_qb, S, need)) { set_error("chunk_attn: %d query rows per kv head", d.n_q); return MILLION_ERR_SHAPE; }
    if (need > 0 && (!workspace || workspace_bytes < need)) { set_error("chunk_attn: workspace %zu < %zu bytes", workspace_bytes, need); return MILLION_ERR_WORKSPACE; }
    if (((uintptr_t)q | (uintptr_t)k_chunk | (uintptr_t)v_chunk | (uintptr_t)k_codes | (uintptr_t)v_codes | (uintptr_t)k_resid |
         (uintptr_t)v_resid | (uintptr_t)out | (uintptr_t)workspace | (uintptr_t)k_cents_prepared | (uintptr_t)v_cents_prepared) & 15) {
        set_error("chunk_attn: every pointer must be 16-byte aligned");
        return MILLION_ERR_ALIGN;
    }
    if ((d.q_stride_b | d.q_stride_h | d.q_stride_n | d.kc_stride_b | d.kc_stride_h | d.kc_stride_n | d.vc_stride_b | d.vc_stride_h |
         d.vc_stride_n | d.o_stride_b | d.o_stride_h | d.o_stride_n | d.resid_stride_b | d.resid_stride_h) & 7) {
        set_error("chunk_attn: fp16 strides must be multiples of 8 elements (16-byte rows)");
        return MILLION_ERR_ALIGN;
    }
    if ((d.k_layout == MILLION_KV_ROWMAJOR && ((d.k_stride_b | d.k_stride_h) & 15)) ||
        (d.v_layout == MILLION_KV_ROWMAJOR && ((d.v_stride_b | d.v_stride_h) & 15))) {
        set_error("chunk_attn: code strides must be multiples of 16 bytes");
        return MILLION_ERR_ALIGN;
    }
    ChunkParams p;
    memset(&p, 0, sizeof(p));
    p.q = (const f16 *)q; p.kc = (const f16 *)k_chunk; p.vc = (const f16 *)v_chunk;
    p.kcodes = (const uint8_t *)k_codes; p.vcodes = (const uint8_t *)v_codes;
    p.kids = k_page_ids; p.vids = v_page_ids;
    p.ktab = (const f16 *)k_cents_prepared; p.vtab = (const f16 *)v_cents_prepared;
    p.kres = (const f16 *)k_resid; p.vres = (const f16 *)v_resid;
    p.out = (f16 *)out;
    p.lse = lse;
    p.bs = d.bs; p.nh = d.nh; p.nh_k = d.nh_k; p.G = d.nh / d.nh_k; p.M = d.M; p.C = d.C;
    p.n_q = d.n_q; p.n_c = d.n_c; p.T = d.n_tokens; p.rcap = d.resid_cap;
    p.r = dev_len ? 0 : d.r;
    p.rs = p.r > 0 ? d.resid_start : 0;
    p.dev_lengths = d.dev_lengths; p.dev_n_q = d.dev_n_q;
    p.res_sb = d.resid_stride_b; p.res_sh = d.resid_stride_h;
    p.k_paged = d.k_layout == MILLION_KV_PAGED; p.v_paged = d.v_layout == MILLION_KV_PAGED;
    p.ps = d.page_size > 0 ? d.page_size : 64; p.n_pages_cap = d.n_pages_cap; p.ids64 = d.page_ids_i64 != 0;
    p.k_sb = d.k_stride_b; p.k_sh = d.k_stride_h; p.v_sb = d.v_stride_b; p.v_sh = d.v_stride_h;
    p.q_sb = d.q_stride_b; p.q_sh = d.q_stride_h; p.q_sn = d.q_stride_n;
    p.kc_sb = d.kc_stride_b; p.kc_sh = d.kc_stride_h; p.kc_sn = d.kc_stride_n;
    p.vc_sb = d.vc_stride_b; p.vc_sh = d.vc_stride_h; p.vc_sn = d.vc_stride_n;
    p.o_sb = d.o_stride_b; p.o_sh = d.o_stride_h; p.o_sn = d.o_stride_n;
    p.nrows = d.n_q * p.G;
    p.n_qb = n_qb;
    p.S = S;
    p.ntT = (d.n_tokens + kKeys - 1) / kKeys;
    p.ntR = (p.r + kKeys - 1) / kKeys;
    p.cb_bytes = d.n_tokens > 0 ? d.C * d.d * 2 : 0;
    p.scale_log2e = 1.4426950408889634f / sqrtf((float)d.d);
    if (S > 1) {
        p.ws_o = (float *)workspace;
        p.ws_ml = p.ws_o + (size_t)d.bs * d.nh_k * S * p.nrows * d.d;
    }
    const long long blocks = (long long)d.bs * d.nh_k * n_qb * S;
    if (blocks > 0x7fffffffLL) { set_error("chunk_attn: %lld workgroups", blocks); return MILLION_ERR_SHAPE; }
    const int lds = 2 * kKeys * 2 * d.d + 2 * p.cb_bytes;
    chunk_attrs_once();
    const hipStream_t s = (hipStream_t)stream;
    const int dm = d.d / d.M;
    if (d.d == 128) {
        if (dm == 2) launch_chunk_t<128, 2>(p, blocks, lds, s);
        else if (dm == 4) launch_chunk_t<128, 4>(p, blocks, lds, s);
        else launch_chunk_t<128, 8>(p, blocks, lds, s);
    } else {
        if (dm == 1) launch_chunk_t<64, 1>(p, blocks, lds, s);
        else if (dm == 2) launch_chunk_t<64, 2>(p, blocks, lds, s);
        else launch_chunk_t<64, 4>(p, blocks, lds, s);
    }
    if (S > 1) {
        const long long threads = (long long)d.bs * d.nh_k * p.nrows * (d.d / 8);
        const long long mblocks = (threads + 255) / 256;
        const bool ragged = p.dev_lengths || p.dev_n_q;
        if (d.d == 128 && ragged) launch_chunk_merge<128, true>(p, mblocks, s);
        else if (d.d == 128) launch_chunk_merge<128, false>(p, mblocks, s);
        else if (ragged) launch_chunk_merge<64, true>(p, mblocks, s);
        else launch_chunk_merge<64, false>(p, mblocks, s);
    }
    const hipError_t e = hipGetLastError();
    if (e != hipSuccess) { set_error("chunk_attn launch: %s", hipGetErrorString(e)); return MILLION_ERR_LAUNCH; }
    return MILLION_OK;
}

extern "C" int million_pq_chunk_attn(const million_chunk_attn_desc *desc, const void *q, const void *k_chunk, const void *v_chunk,
                                     const void *k_codes, const void *v_codes, const void *k_page_ids, const void *v_page_ids,
                                     const void *k_cents_prepared, const void *v_cents_prepared, const void *k_resid,
                                     const void *v_resid, void *out, void *workspace, size_t workspace_bytes,
                                     million_stream_t stream) {
    return chunk_attn_impl(desc, q, k_chunk, v_chunk, k_codes, v_codes, k_page_ids, v_page_ids, k_cents_prepared, v_cents_prepared,
                           k_resid, v_resid, out, nullptr, workspace, workspace_bytes, stream);
}

extern "C" int million_pq_chunk_attn_lse(const million_chunk_attn_desc *desc, const void *q, const void *k_chunk, const void *v_chunk,
                                         const void *k_codes, const void *v_codes, const void *k_page_ids, const void *v_page_ids,
                                         const void *k_cents_prepared, const void *v_cents_prepared, const void *k_resid,
                                         const void *v_resid, void *out, float *lse, void *workspace, size_t workspace_bytes,
                                         million_stream_t stream) {
    if (!lse) { set_error("chunk_attn_lse: lse null"); return MILLION_ERR_ARG; }
    if ((uintptr_t)lse & 3) { set_error("chunk_attn_lse: lse must be 4-byte aligned"); return MILLION_ERR_ALIGN; }
    return chunk_attn_impl(desc, q, k_chunk, v_chunk, k_codes, v_codes, k_page_ids, v_page_ids, k_cents_prepared, v_cents_prepared,
                           k_resid, v_resid, out, lse, workspace, workspace_bytes, stream);
}
