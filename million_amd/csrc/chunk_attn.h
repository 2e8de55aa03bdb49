// chunk_attn.h — what the chunk-attention kernels share: chunk_attn.hip (uint8 codes, both codebooks in LDS) and
// chunk_attn_wide.hip (uint16 codes or packed 10- / 12-bit pages, the codebooks gathered from global memory), gfx950.
//
// ONE body, chunk_attn_body<D, DM, RAGGED, LSE, WIDE, PACKED>: the tile loop over flash_tile.h's step, the mask, the cut of a query
// block's visible tiles into the S split ranges, the ragged clamps and the epilogue are the same text for every code format;
// WIDE / PACKED select the code producer and nothing else (the design notes are at the top of the two .hip files).  The host half -
// validation, chunk_splits, the workspace, chunk_merge_kernel - is chunk_attn.hip's for both.
#pragma once

#include "flash_tile.h"

namespace million {

constexpr int kKeys = 64;            // keys per tile
constexpr int kRowsWG = 256;         // flattened query rows per workgroup (8 waves x 32)
constexpr int kThreads = 512;

struct ChunkParams {
    const f16 *q, *kc, *vc;                   // queries, chunk K / V
    const uint8_t *kcodes, *vcodes;           // row-major codes or page pools (WIDE: uint16 codes behind the same byte pointers)
    const void *kids, *vids;                  // page ids (PAGED sides)
    const f16 *ktab, *vtab;                   // prepared row images [m][c][d_m] (WIDE: the plain (M, C, d_m) codebooks, read where they are)
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
    int cb_bytes;                             // one codebook image in LDS (0: no code tiles; WIDE: always 0)
    float scale_log2e;
    const int *dev_lengths;                   // RAGGED: (bs, 4) {T, r, resid_start, ticket} per request, or null (host T / r / rs)
    const int *dev_n_q;                       // RAGGED: (bs,) valid query rows per request, or null (n_q)
    float *lse;                               // LSE instances: (bs, nh, n_q) fp32 log-sum-exp of each row's visible scores (million_hip.h); last, so
                                              // that no other argument moves: the instances without it are the code they were
    int hb;                                   // PACKED instances: high bits of a code beside its low byte (2 / 4; packed_hi_bits(C)), else 0
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

// WIDE: the NM = 8 / d_m uint16 codes of token `tok`, subspaces m0 .. m0 + NM - 1, packed little-endian (8 or 4 bytes: one
// load from a row-major row or a K page, NM two-byte loads page_size apart from a transposed V page)
template <int NM>
__device__ __forceinline__ unsigned long long ca_load_codes16(const ChunkParams &p, bool is_v, int b, int hk, int tok, int m0) {
    const bool paged = is_v ? p.v_paged : p.k_paged;
    const uint8_t *base = is_v ? p.vcodes : p.kcodes;
    const unsigned short *src;
    if (!paged) {
        src = (const unsigned short *)(base + b * (is_v ? p.v_sb : p.k_sb) + hk * (is_v ? p.v_sh : p.k_sh)) + (long long)tok * p.M + m0;
    } else {
        const long long pg = ca_page(p, is_v ? p.vids : p.kids, b, hk, tok / p.ps);
        const int o = tok - (tok / p.ps) * p.ps;
        if (is_v) {      // transposed page (M, ps): one code per subspace, ps apart
            src = (const unsigned short *)base + pg * p.M * p.ps + (long long)m0 * p.ps + o;
            unsigned long long w = 0;
#pragma unroll
            for (int e = 0; e < NM; ++e) w |= (unsigned long long)src[(long long)e * p.ps] << (16 * e);
            return w;
        }
        src = (const unsigned short *)base + pg * p.ps * p.M + (long long)o * p.M + m0;
    }
    if (NM == 4) return *(const unsigned long long *)src;
    return *(const unsigned *)src;
}

// PACKED: ca_load_codes16's word from packed pages (million_hip.h, "Packed code pages"; both sides paged): the NM low bytes
// - one load of NM bytes from a K page, NM byte loads page_size apart from a transposed V page - and the token's high-plane
// byte(s) of the same subspaces.  m0 is a multiple of NM, so the NM fields of h = p.hb bits start at bit (m0 h) mod 8 of high
// byte m0 h / 8: a whole byte (h 2, NM 4; h 4, NM 2), a nibble (h 2, NM 2) or two bytes (h 4, NM 4).  Exactly those bytes are
// loaded.  A page is page_size M (8 + h) / 8 bytes, no power of two: its offset is a 64-bit multiply.
template <int NM>
__device__ __forceinline__ unsigned long long ca_load_codes_packed(const ChunkParams &p, bool is_v, int b, int hk, int tok, int m0) {
    static_assert(NM == 2 || NM == 4, "d / M 4 or 2");
    const int h = p.hb;                                 // wave-uniform: 2 or 4
    const bool two = NM == 4 && h == 4;                 // 16 high bits
    const long long pg = ca_page(p, is_v ? p.vids : p.kids, b, hk, tok / p.ps);
    const int o = tok - (tok / p.ps) * p.ps;
    const uint8_t *page = (is_v ? p.vcodes : p.kcodes) + pg * ((long long)p.ps * ((p.M * (8 + h)) >> 3));
    const uint8_t *hi_plane = page + p.ps * p.M;
    const int hb0 = (m0 * h) >> 3;
    unsigned lo, hi;
    if (is_v) {      // transposed planes: low (M, ps), high (M h / 8, ps)
        const uint8_t *src = page + m0 * p.ps + o;
        lo = 0;
#pragma unroll
        for (int e = 0; e < NM; ++e) lo |= (unsigned)src[e * p.ps] << (8 * e);
        const uint8_t *hs = hi_plane + hb0 * p.ps + o;
        hi = hs[0];
        if (two) hi |= (unsigned)hs[p.ps] << 8;
    } else {         // low (ps, M), high (ps, M h / 8)
        const uint8_t *src = page + o * p.M + m0;
        lo = NM == 4 ? *(const unsigned *)src : (unsigned)*(const unsigned short *)src;
        const uint8_t *hs = hi_plane + o * ((p.M * h) >> 3) + hb0;
        hi = two ? (unsigned)*(const unsigned short *)hs : (unsigned)*hs;
    }
    hi >>= (m0 * h) & 7;
    const unsigned fmask = (1u << h) - 1u;
    unsigned long long w = 0;
#pragma unroll
    for (int e = 0; e < NM; ++e)
        w |= (unsigned long long)(((lo >> (8 * e)) & 0xffu) | (((hi >> (h * e)) & fmask) << 8)) << (16 * e);
    return w;
}

// WIDE: 8 fp16 of one 16-byte chunk from NM codes through the plain (M, C, d_m) codebook in global memory: NM loads of one whole
// entry (4 bytes at d_m = 2, 8 at d_m = 4).  EVERY index is code & (C - 1) (C is a power of two): whatever 16 bits a code word
// holds, the load stays inside its subspace's C entries.
template <int DM>
__device__ __forceinline__ pv4u ca_gather16(unsigned long long w, const f16 *tab, int m0, int C) {
    constexpr int NM = 8 / DM;
    static_assert(DM == 2 || DM == 4, "entries of 4 or 8 bytes");
    const unsigned cmask = (unsigned)C - 1u;
    unsigned u[4];
#pragma unroll
    for (int e = 0; e < NM; ++e) {
        const unsigned c = (unsigned)(w >> (16 * e)) & cmask;
        const char *ep = (const char *)tab + ((unsigned)(m0 + e) * (unsigned)C + c) * (unsigned)(2 * DM);      // < d C 2 <= 1 MiB
        if (DM == 4) {
            typedef unsigned u2 __attribute__((ext_vector_type(2)));
            const u2 x = *(const u2 *)ep;
            u[2 * e] = x[0]; u[2 * e + 1] = x[1];
        } else {
            u[e] = *(const unsigned *)ep;
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
// WIDE: the code producer.  false: uint8 codes through the two codebook images this workgroup copied to LDS.  true: uint16
// codes through the codebooks in global memory - a code tile's entries are gathered straight into the registers that hold a
// window or chunk tile's rows (an entry group IS a 16-byte chunk of the dequantised row), one tile ahead of the products, and
// its code words one tile ahead of that; LDS holds the K + V tile only.
// PACKED (with WIDE): the code words come from packed 10- / 12-bit pages (ca_load_codes_packed) instead of uint16 pages; the
// word is the same, so nothing behind cwk / cwv differs and the result is the uint16 instance's bit for bit.
template <int D, int DM, bool RAGGED, bool LSE, bool WIDE, bool PACKED = false>
__device__ __forceinline__ void chunk_attn_body(const ChunkParams &p) {
    constexpr int DS = D / 16;                    // k-steps of the score product
    constexpr int NB = D / 32;                    // 32-row blocks of O^T
    constexpr int CH = D / 8;                     // 16-byte chunks per row
    constexpr int CPT = kKeys * CH / kThreads;    // chunks per thread and tile side (2 / 1)
    constexpr int NM = 8 / DM;                    // subspaces per chunk
    constexpr unsigned kTileBytes = kKeys * 2 * D;
    extern __shared__ __attribute__((aligned(16))) char ca_smem[];      // [K tile | V tile | K codebook | V codebook] (WIDE: the tiles only)
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
    [[maybe_unused]] const unsigned cbK = 2u * kTileBytes, cbV = cbK + (unsigned)p.cb_bytes;
    if constexpr (!WIDE) if ((!RAGGED || t_beg < t_end) && t_beg < ntT) {      // this split dequantises: both codebooks into LDS (made visible by the loop's first barrier)
        const pv4u *sk = (const pv4u *)p.ktab, *sv = (const pv4u *)p.vtab;
        for (int o = tid; o < p.cb_bytes / 16; o += kThreads) {
            *(pv4u *)(ca_smem + cbK + 16 * o) = sk[o];
            *(pv4u *)(ca_smem + cbV + 16 * o) = sv[o];
        }
    }

    // ---- producers: a tile's raw bytes (codes, or fp16 rows) into registers, then dequantised / copied into LDS ----
    pv4u rk[CPT], rv[CPT];
    unsigned long long cwk[CPT], cwv[CPT];      // WIDE: the code words of the next tile to gather
    auto tile_src = [&](int t, int &kind, int &j0, int &nv) {      // kind 0 codes, 1 window, 2 chunk
        if (t < ntT) { kind = 0; j0 = t * kKeys; nv = T - j0; }
        else if (t < ntT + ntR) { kind = 1; j0 = (t - ntT) * kKeys; nv = r - j0; }
        else { kind = 2; j0 = (t - ntT - ntR) * kKeys; nv = n_c - j0; }
        nv = nv < kKeys ? nv : kKeys;
    };
    [[maybe_unused]] auto load_codes = [&](int t) {      // WIDE: a code tile's words (another tile: nothing, its rows are loaded by load_raw)
        int kind, j0, nv;
        tile_src(t, kind, j0, nv);
#pragma unroll
        for (int k = 0; k < CPT; ++k) {
            const int c = tid + kThreads * k, row = c / CH, ch = c % CH;
            cwk[k] = 0;
            cwv[k] = 0;
            if (kind == 0 && row < nv) {
                if constexpr (PACKED) {
                    cwk[k] = ca_load_codes_packed<NM>(p, false, b, hk, j0 + row, ch * NM);
                    cwv[k] = ca_load_codes_packed<NM>(p, true, b, hk, j0 + row, ch * NM);
                } else {
                    cwk[k] = ca_load_codes16<NM>(p, false, b, hk, j0 + row, ch * NM);
                    cwv[k] = ca_load_codes16<NM>(p, true, b, hk, j0 + row, ch * NM);
                }
            }
        }
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
                    if constexpr (WIDE) {      // the entries of the code words load_codes(t) brought
                        rk[k] = ca_gather16<DM>(cwk[k], p.ktab, ch * NM, p.C);
                        rv[k] = ca_gather16<DM>(cwv[k], p.vtab, ch * NM, p.C);
                    } else {
                        const unsigned long long wk = ca_load_codes<NM>(p, false, b, hk, j, ch * NM);
                        const unsigned long long wv = ca_load_codes<NM>(p, true, b, hk, j, ch * NM);
                        rk[k][0] = (unsigned)wk; rk[k][1] = (unsigned)(wk >> 32);
                        rv[k][0] = (unsigned)wv; rv[k][1] = (unsigned)(wv >> 32);
                    }
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
            if constexpr (!WIDE) if (kind == 0 && row < nv) {
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

    if constexpr (WIDE) if (t_beg < t_end) load_codes(t_beg);
    if (t_beg < t_end) load_raw(t_beg);
    if constexpr (WIDE) if (t_beg + 1 < t_end) load_codes(t_beg + 1);
    for (int t = t_beg; t < t_end; ++t) {
        __syncthreads();      // the previous tile's reads are done (first tile: the codebooks are in LDS)
        produce(t);
        __syncthreads();
        if (t + 1 < t_end) load_raw(t + 1);      // in flight during this tile's products
        if constexpr (WIDE) if (t + 2 < t_end) load_codes(t + 2);      // behind the gathers that consumed the words of tile t + 1
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

// Launches one instance of either kernel (the diagnostic build passes the LDS byte count along: debug_fill_lds, common.h)
template <typename Kernel>
inline void launch_chunk_kernel(Kernel kernel, const ChunkParams &p, long long blocks, int lds, hipStream_t s) {
#ifdef MILLION_DEBUG_CHECK_IDS
    ChunkParams pf = p;
    pf.lds_fill = lds;
    hipLaunchKernelGGL(kernel, dim3((unsigned)blocks), dim3(kThreads), lds, s, pf);
#else
    hipLaunchKernelGGL(kernel, dim3((unsigned)blocks), dim3(kThreads), lds, s, p);
#endif
}

// chunk_attn_wide.hip: launches chunk_attn_wide_kernel<d, d / p.M, ragged, lse> (ragged and lse as the fields of p say) or, with
// p.hb != 0, chunk_attn_packed_kernel of the same four; the descriptor was validated and p filled by chunk_attn.hip, which also
// launches the merge
void launch_chunk_wide(const ChunkParams &p, int d, long long blocks, int lds, hipStream_t s);

}  // namespace million
