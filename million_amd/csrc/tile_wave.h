// tile_wave.h — what the two wave-tile decode kernels share: attn_tile.hip (8-bit codes, codebooks in LDS) and attn_wide.hip
// (16-bit codes, codebooks in global memory).  gfx950, wave64.
//
// Both kernels have the same skeleton.  A wave walks 16-token tiles on its own (no workgroup barrier inside its loop), lane =
// 16 q4 + c16.  Scores: v_mfma_f32_16x16x32_f16, A = 8 dims of the lane's quarter q4 of a K^ row (token c16), B = the query
// heads (up to 16: the 16 columns), so acc[v] = S[token 4 q4 + v][head c16].  Online softmax in the exp2 domain, fp32, head =
// lane column: the probabilities come out laid out as the B operand of the value step, v_mfma_f32_16x16x16_f16 (A = 16 rows x
// 16 tokens of V^T), which adds to D/16 accumulator tiles O^T[row][head c16]; the running rescale is lane-local.  The residual
// window is one more workgroup per (b, kv head) that fills an LDS tile per wave from the fp16 rows (K rows -> K^ tile -> scores,
// V rows -> transposed V^T tile -> values), the fused append included.  The waves' partials merge through LDS into `part`, the
// workgroups' through the workspace by the last arriver (common.h: publish_and_merge).
// A kernel keeps what is its own: where a code tile's K^ and V^ operands come from (its loads, prefetch ring and gathers), its
// LDS region and its instances.  Everything here is written once and takes no word about which kernel calls it.
#pragma once
#include "common.h"

namespace million {

typedef _Float16 t8f16 __attribute__((ext_vector_type(8)));
typedef _Float16 t4f16 __attribute__((ext_vector_type(4)));
typedef float t4f32 __attribute__((ext_vector_type(4)));
typedef unsigned t4u __attribute__((ext_vector_type(4)));

constexpr int kTT = 16;    // tokens per wave tile

// LDS wave tile of the residual-window workgroup: the K^ tile, then (same bytes) the V^T tile
template <int D>
struct TileGeom {
    static constexpr int kKRow = D * 2 + 16;                    // K^ row stride (bytes): 16 tokens x (d halves + pad)
    static constexpr int kVRow = kTT * 2 + 16;                  // V^T row stride (bytes): d rows x (16 halves + pad)
    static constexpr int kTile = (kTT * kKRow > D * kVRow) ? kTT * kKRow : D * kVRow;
};

// LDS of both kernels: [region][partial of the workgroup][flag].  Every workgroup's region holds the window workgroup's K^ / V^T
// wave tiles and, after the loop, the waves' merge scratch (merge_waves: G d + 2 G floats per wave): wave_scratch_bytes.
__host__ __device__ inline int wave_scratch_bytes(int d, int G, int waves) {
    const int tiles = waves * (d == 128 ? TileGeom<128>::kTile : TileGeom<64>::kTile);
    const int wf = waves * (G * d + 2 * G) * 4;
    return wf > tiles ? wf : tiles;
}
// attn_tile.hip: the region is first the two codebooks (code workgroups; the window workgroup loads none)
__host__ __device__ inline int tile_region_bytes(int d, int C, int G, int waves) {
    int r = 2 * d * C * 2;
    if (wave_scratch_bytes(d, G, waves) > r) r = wave_scratch_bytes(d, G, waves);
    return (r + 15) / 16 * 16;
}
// attn_wide.hip: no codebook in LDS; at least the last arriver's merge scratch (common.h merge_vec4: 512 weights + 2048 floats)
__host__ __device__ inline int wide_region_bytes(int d, int G, int waves) {
    int r = wave_scratch_bytes(d, G, waves);
    if (r < 16 * 1024) r = 16 * 1024;
    return (r + 15) / 16 * 16;
}

__device__ __forceinline__ float fast_exp2_tile(float x) { return __builtin_amdgcn_exp2f(x); }   // v_exp_f32: exp2(-inf) = 0

__device__ __forceinline__ void lds_phase() {      // LDS writes of this wave before, LDS reads of this wave after
    asm volatile("" ::: "memory");
    __builtin_amdgcn_wave_barrier();
    asm volatile("" ::: "memory");
}

// A wave's running softmax: the reference maximum of head c16, this lane's share of the denominator, this lane's O^T tiles
template <int D>
struct WaveAcc {
    float m_run = -INFINITY, l_run = 0.f;
    t4f32 O[D / 16] = {};
};

struct Pids { long long k, v; };      // page ids of one tile, K side and V side

// first token of a wave's j-th code tile (clamped: a re-request, never past the split)
template <int WAVES>
__device__ __forceinline__ int wave_tile_t0(int j, int wave, int n_tiles, int t_begin) {
    int ti = wave + WAVES * j;
    if (ti > n_tiles - 1) ti = n_tiles - 1;
    return t_begin + kTT * ti;
}

// The query operand of the score MFMAs.  row0: row of q of the launch's first query head of this kv head, (long long)b * p.nh +
// head0(p, hk), formed by the kernel (with head0 called in here hipcc stops hoisting the head arithmetic of publish_and_merge out
// of its unrolled loops: profiles/tile_wave_refactor.txt).  Columns >= G are zeros.
template <int D>
__device__ __forceinline__ void load_query(t8f16 (&qb)[D / 32], const f16 *q, long long row0, int G, int q4, int c16) {
#pragma unroll
    for (int s = 0; s < D / 32; ++s) {
        t4u z = {0u, 0u, 0u, 0u};
        // stage s of lane quarter q4 = dims q4 * D/4 + 8 s .. + 8: the dims of the lane's own code bytes (direct gathers)
        if (c16 < G) z = *(const t4u *)(q + (row0 + c16) * D + q4 * (D / 4) + 8 * s);
        qb[s] = __builtin_bit_cast(t8f16, z);
    }
}

// Online-softmax step of one tile: scores acc (tokens >= n_valid masked) -> probabilities, a updated
template <int D>
__device__ __forceinline__ t4f16 softmax_tile(WaveAcc<D> &a, t4f32 acc, int n_valid, float scale_log2e, int q4) {
    float sc[4], mx = -INFINITY;
#pragma unroll
    for (int v = 0; v < 4; ++v) {          // acc[v] = S[token 4*q4 + v][head c16]
        sc[v] = (4 * q4 + v < n_valid) ? acc[v] * scale_log2e : -INFINITY;
        mx = fmaxf(mx, sc[v]);
    }
    // m_run is the softmax reference of head c16, moved (with the cross-lane maximum and the rescale of O, l) only
    // when a score exceeds it by more than 2^8: the common tile needs no reduction (decode_wave.h: softmax_online_raw)
    if (__builtin_amdgcn_ballot_w64(mx > a.m_run + 8.0f)) {      // also the first tile: m_run = -inf, mx finite
        const float m_new = fmaxf(a.m_run, rows_max(mx));          // over the four lane rows: all 16 tokens of head c16
        const float alpha = fast_exp2_tile(a.m_run - m_new);
        a.l_run *= alpha;
        a.m_run = m_new;
        if (__builtin_amdgcn_ballot_w64(alpha != 1.0f)) {
#pragma unroll
            for (int n = 0; n < D / 16; ++n) a.O[n] *= alpha;      // O^T[dim][head c16]: this lane's own head
        }
    }
    float pe[4], ls = 0.f;
#pragma unroll
    for (int v = 0; v < 4; ++v) { pe[v] = fast_exp2_tile(sc[v] - a.m_run); ls += pe[v]; }
    a.l_run += ls;                         // per-lane partial sum; the four lane rows are added once, at the end
    return t4f16{(_Float16)pe[0], (_Float16)pe[1], (_Float16)pe[2], (_Float16)pe[3]};
}

// Fused append: thread tid < D parks element tid of the new K and V rows in window row r_old (window_pass reads them back
// from k_new / v_new)
template <int D>
__device__ __forceinline__ void park_new_row(const AttnParams &p, int b, int hk, int bh, int rstart, int r_old, int tid) {
    const long long o = b * p.res_sb + hk * p.res_sh + (long long)((rstart + r_old) % p.rcap) * D + tid;
    p.k_res_w[o] = p.k_new[(long long)bh * D + tid];
    p.v_res_w[o] = p.v_new[(long long)bh * D + tid];
}

// The residual window of (b, kv head hk), r rows (the fused append's new row, r_old, included): the same steps as a code tile,
// the wave's LDS tile filled from the fp16 rows.  A row index past the window is clamped to a valid row; its probability is an
// exact zero (softmax_tile's n_valid).
template <int D, int WAVES>
__device__ __forceinline__ void window_pass(WaveAcc<D> &a, const t8f16 (&qb)[D / 32], const AttnParams &p, char *tile, int b, int hk,
                                            int bh, int r, int r_old, int rstart, int wave, int lane) {
    constexpr int NTASK = D / 64;              // V tasks per lane and tile: (d/2 dim pairs) x (2 token octets) / 64
    constexpr int kKRow = TileGeom<D>::kKRow, kVRow = TileGeom<D>::kVRow;
    const int q4 = lane >> 4, c16 = lane & 15;
    const int n_tiles = (r + kTT - 1) / kTT;
    const f16 *kres = p.k_res + b * p.res_sb + hk * p.res_sh;
    const f16 *vres = p.v_res + b * p.res_sb + hk * p.res_sh;
    auto row_of = [&](int i, const f16 *base, const f16 *fresh) -> const f16 * {      // window row i (clamped to a valid one)
        if (i > r - 1) i = r - 1;
        if (fresh && i == r_old) return fresh + (long long)bh * D;
        return base + (long long)((rstart + i) % p.rcap) * D;
    };
    for (int ti = wave; ti < n_tiles; ti += WAVES) {
        const int t0 = kTT * ti;
        {
            const f16 *src = row_of(t0 + c16, kres, p.k_new) + q4 * (D / 4);
            char *dst = tile + c16 * kKRow + q4 * (D / 2);
#pragma unroll
            for (int i = 0; i < D / 32; ++i) *(t4u *)(dst + 16 * i) = *(const t4u *)((const char *)src + 16 * i);
        }
        lds_phase();
        t4f32 acc = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
        for (int s = 0; s < D / 32; ++s) {
            const t4u ka = *(const t4u *)(tile + c16 * kKRow + (q4 * (D / 4) + 8 * s) * 2);
            acc = __builtin_amdgcn_mfma_f32_16x16x32_f16(__builtin_bit_cast(t8f16, ka), qb[s], acc, 0, 0, 0);
        }
        const t4f16 P = softmax_tile(a, acc, min(kTT, r - t0), p.scale_log2e, q4);
        lds_phase();
#pragma unroll
        for (int j = 0; j < NTASK; ++j) {      // eight (d0, d1) pairs of consecutive tokens -> the two V^T rows of that dim pair
            const int task = j * 64 + lane, dp = task >> 1, oct = task & 1;
            unsigned e[8];
#pragma unroll
            for (int t = 0; t < 8; ++t) e[t] = *(const unsigned *)(row_of(t0 + 8 * oct + t, vres, p.v_new) + 2 * dp);
            t4u lo, hi;
#pragma unroll
            for (int i = 0; i < 4; ++i) {
                lo[i] = __builtin_amdgcn_perm(e[2 * i + 1], e[2 * i], 0x05040100u);
                hi[i] = __builtin_amdgcn_perm(e[2 * i + 1], e[2 * i], 0x07060302u);
            }
            *(t4u *)(tile + (2 * dp) * kVRow + oct * 16) = lo;
            *(t4u *)(tile + (2 * dp + 1) * kVRow + oct * 16) = hi;
        }
        lds_phase();
#pragma unroll
        for (int n = 0; n < D / 16; ++n) {     // O^T += V^T P
            const v2u va = *(const v2u *)(tile + (16 * n + c16) * kVRow + (4 * q4) * 2);
            a.O[n] = __builtin_amdgcn_mfma_f32_16x16x16f16(__builtin_bit_cast(t4f16, va), P, a.O[n], 0, 0, 0);
        }
        lds_phase();
    }
}

// Merge the waves' partials through LDS into `part` (O[g][dim], then m[g], then l[g]: what publish_and_merge hands over).
// smem: the start of the region; whatever the waves kept there (codebooks, wave tiles) is dead behind the first barrier, and
// the waves' partials are dead once `part` is complete (the last barrier): the region is then the last arriver's merge scratch.
template <int D, int DM, int WAVES>
__device__ __forceinline__ void merge_waves(const WaveAcc<D> &a, float *smem, float *part, int G, bool is_resid, int tid) {
    const int lane = tid & 63, wave = tid >> 6, q4 = lane >> 4, c16 = lane & 15;
    __syncthreads();
    const int wf = G * D + 2 * G;                         // floats per wave
    const float l_sum = rows_sum(a.l_run);
    float *ws = smem + wave * wf;
    if (c16 < G) {
#pragma unroll
        for (int n = 0; n < D / 16; ++n)
#pragma unroll
            for (int v = 0; v < 4; ++v) {
                // code workgroups: tile n = (column group n / d_m, dim e = n % d_m), row = subspace 16 cg + 4 q4 + v;
                // residual workgroup: tile n = dims 16 n .. 16 n + 15
                const int dim = is_resid ? 16 * n + 4 * q4 + v : (16 * (n / DM) + 4 * q4 + v) * DM + n % DM;
                ws[c16 * D + dim] = a.O[n][v];
            }
        if (q4 == 0) { ws[G * D + c16] = a.m_run; ws[G * D + G + c16] = l_sum; }
    }
    __syncthreads();
    for (int e = tid; e < wf; e += WAVES * 64) {          // e: O[g][dim], then m[g], then l[g]
        const int g = e < G * D ? e / D : (e - G * D) % G;
        float mm = -INFINITY;
#pragma unroll
        for (int w = 0; w < WAVES; ++w) mm = fmaxf(mm, smem[w * wf + G * D + g]);
        const float ms = mm > -INFINITY ? mm : 0.f;
        float o = mm;
        if (e < G * D || e >= G * D + G) {
            o = 0.f;
#pragma unroll
            for (int w = 0; w < WAVES; ++w) o += smem[w * wf + e] * exp2f(smem[w * wf + G * D + g] - ms);
        }
        part[e] = o;
    }
    __syncthreads();
}

// Split policy of both planners: the splits of all (b, kv head) pairs and their window workgroups fill `room` workgroups once
// (room: how many workgroups the chip holds at a time - each planner says why its room is what it is); a split is a multiple of
// 64 tokens and at least 256 tokens long.
inline void split_by_room(AttnParams &p, int room) {
    const int bh = p.bs * p.nh_k;
    int ns = room > 2 * bh ? (room - bh) / bh : (room + bh - 1) / bh;
    if (ns > kMaxSplits) ns = kMaxSplits;
    int by_len = (p.T + 255) / 256;
    if (by_len < 1) by_len = 1;
    if (ns > by_len) ns = by_len;
    int len = (p.T + ns - 1) / ns;
    len = (len + 63) / 64 * 64;
    if (len < 64) len = 64;
    ns = p.T > 0 ? (p.T + len - 1) / len : 1;
    p.nsplit = ns;
    p.split_len = len;
    p.nslots = ns + 1;
}

}  // namespace million
