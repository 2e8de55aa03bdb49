// attn_wide.hip — fused decode attention over 16-bit PQ codes (512 .. 4096 centroids per subspace) in page pools, gfx950 / CDNA4.
//
// Same job and same single launch as attn_tile.hip, whose structure this kernel keeps: a wave walks 16-token tiles on its own,
// a lane's gathered codebook entries ARE the MFMA operands (scores: v_mfma_f32_16x16x32_f16, A = 8 dims of the lane's quarter
// of the K^ row; values: v_mfma_f32_16x16x16_f16, A = one dim of 16 subspaces x 16 tokens, B = the probabilities), up to 16
// query heads are the 16 columns, the residual window runs as one more workgroup per (b, kv head) through an LDS tile, the
// waves' partials merge through LDS and the workgroups' through the workspace (common.h: publish_and_merge, unchanged).
//
// The one structural difference: a table is C * d * 2 bytes = 128 KiB .. 1 MiB, so no codebook is in LDS.  Both tables are the
// plain (M, C, d_m) fp16 tensors in global memory (resident in L2 / the Infinity Cache: every workgroup gathers from the same
// two) and every entry is one global load of the whole sub-vector: 4 bytes at d_m = 2, 8 bytes at d_m = 4.  The gathers of
// tile j + 1 are issued before tile j is computed (its entries were requested one iteration earlier), the code words kPF
// tiles ahead, the page ids 2 kPF tiles ahead.
//
// EVERY gathered index is code & (C - 1).  An LDS gather forgives a stray index; a global one would read outside the table.
// Codes past T in the last page, in pages nobody names and in poisoned memory may hold any 16 bits: their entries are read
// (inside the table) and meet probabilities that are exact zeros.  Page ids are trusted, as in every other kernel.
//
// Lane roles (lane = 16 q4 + c16), d_m in {2, 4}, M = d / d_m:
//   K  lane (token c16, quarter q4): the M/4 codes [q4 M/4, (q4 + 1) M/4) of its token's row = dims [q4 d/4, (q4 + 1) d/4)
//   V  lane (tokens 4 q4 .. 4 q4 + 3, subspace 16 cg + c16): 4 codes (8 bytes of a transposed page row) per column group cg
//   O  tile n = (cg = n / d_m, e = n % d_m): O^T[(16 cg + 4 q4 + v) d_m + e][head c16]
#include "common.h"

namespace million {

typedef _Float16 w8f16 __attribute__((ext_vector_type(8)));
typedef _Float16 w4f16 __attribute__((ext_vector_type(4)));
typedef float w4f32 __attribute__((ext_vector_type(4)));
typedef unsigned w4u __attribute__((ext_vector_type(4)));

constexpr int kWT = 16;     // tokens per wave tile
constexpr int kWW = 8;      // waves per workgroup
constexpr int kWidePF = 2;  // code tiles in flight per wave

template <int D>
struct WideGeom {
    static constexpr int kKRow = D * 2 + 16;                    // window K^ row stride (bytes)
    static constexpr int kVRow = kWT * 2 + 16;                  // window V^T row stride (bytes)
    static constexpr int kTile = (kWT * kKRow > D * kVRow) ? kWT * kKRow : D * kVRow;
};

// LDS: [region][partial of the workgroup][flag].  region = the window workgroup's K^ / V^T wave tiles, then the waves' merge
// scratch, then the last arriver's (common.h merge_vec4: 512 weights + 2048 floats)
__host__ __device__ inline int wide_region_bytes(int d, int G) {
    int r = kWW * (d == 128 ? WideGeom<128>::kTile : WideGeom<64>::kTile);
    const int wf = kWW * (G * d + 2 * G) * 4;
    if (wf > r) r = wf;
    if (r < 16 * 1024) r = 16 * 1024;
    return (r + 15) / 16 * 16;
}

__device__ __forceinline__ float wide_exp2(float x) { return __builtin_amdgcn_exp2f(x); }      // exp2(-inf) = 0
__device__ __forceinline__ void wide_lds_phase() {
    asm volatile("" ::: "memory");
    __builtin_amdgcn_wave_barrier();
    asm volatile("" ::: "memory");
}

template <int D, int DM, bool LSE = false>
__global__ __launch_bounds__(kWW * 64, 2) void attn_wide_kernel(AttnParams p) {
    constexpr int M = D / DM;
    constexpr int NS = D / 32;                 // score stages (32 dims each)
    constexpr int NC = D / 16;                 // output tiles of 16 dims
    constexpr int KD = M / 8;                  // K code dwords per lane and tile (M/4 codes of 16 bits)
    constexpr int CG = M / 16;                 // column groups of 16 subspaces
    constexpr int EW = DM / 2;                 // dwords per codebook entry
    constexpr int NTASK = D / 64;
    constexpr int kKRow = WideGeom<D>::kKRow, kVRow = WideGeom<D>::kVRow, kTile = WideGeom<D>::kTile;
    static_assert(DM == 2 || DM == 4, "entries of 4 or 8 bytes");
    extern __shared__ __attribute__((aligned(16))) char smem[];
    MILLION_DEBUG_FILL_LDS(smem, p.lds_fill);

    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int q4 = lane >> 4, c16 = lane & 15;
    const int slot = blockIdx.x, bh = blockIdx.y;
    const int b = bh / p.nh_k, hk = bh % p.nh_k;
    const int G = p.G;
    const unsigned cmask = (unsigned)p.C - 1u;     // C is a power of two: the mask that keeps every gather inside its table row
    int T, r, rstart;
    load_lengths(p, b, T, r, rstart);              // a device row is clamped to the host bounds (common.h: load_len_row)
    const int r_old = r;
    if (p.k_new) r += 1;                           // fused append: the new token is window row r_old

    char *tile = smem + wave * kTile;              // window workgroup only
    float *part = (float *)(smem + wide_region_bytes(D, G));
    int *flag = (int *)(part + p.slot_floats);

    const bool is_resid = slot == p.nsplit;
    const int t_begin = is_resid ? 0 : min(slot * p.split_len, T);
    const int t_end = is_resid ? r : min(t_begin + p.split_len, T);
    const int n_tiles = (t_end - t_begin + kWT - 1) / kWT;

    if (p.k_new && is_resid && tid < D) {          // fused append: park the new row in the window (read back from k_new below)
        const long long o = b * p.res_sb + hk * p.res_sh + (long long)((rstart + r_old) % p.rcap) * D + tid;
        p.k_res_w[o] = p.k_new[(long long)bh * D + tid];
        p.v_res_w[o] = p.v_new[(long long)bh * D + tid];
    }
    w8f16 qb[NS];
#pragma unroll
    for (int s = 0; s < NS; ++s) {
        w4u z = {0u, 0u, 0u, 0u};
        if (c16 < G) z = *(const w4u *)(p.q + ((long long)b * p.nh + head0(p, hk) + c16) * D + q4 * (D / 4) + 8 * s);
        qb[s] = __builtin_bit_cast(w8f16, z);
    }

    float m_run = -INFINITY, l_run = 0.f;
    w4f32 O[NC];
#pragma unroll
    for (int n = 0; n < NC; ++n) O[n] = w4f32{0.f, 0.f, 0.f, 0.f};

    auto softmax_tile = [&](w4f32 acc, int n_valid) -> w4f16 {
        float sc[4], mx = -INFINITY;
#pragma unroll
        for (int v = 0; v < 4; ++v) {              // acc[v] = S[token 4 q4 + v][head c16]
            sc[v] = (4 * q4 + v < n_valid) ? acc[v] * p.scale_log2e : -INFINITY;
            mx = fmaxf(mx, sc[v]);
        }
        // the reference maximum of head c16 moves only when a score exceeds it by more than 2^8 (attn_tile.hip)
        if (__builtin_amdgcn_ballot_w64(mx > m_run + 8.0f)) {
            const float m_new = fmaxf(m_run, rows_max(mx));
            const float alpha = wide_exp2(m_run - m_new);
            l_run *= alpha;
            m_run = m_new;
            if (__builtin_amdgcn_ballot_w64(alpha != 1.0f)) {
#pragma unroll
                for (int n = 0; n < NC; ++n) O[n] *= alpha;
            }
        }
        float pe[4], ls = 0.f;
#pragma unroll
        for (int v = 0; v < 4; ++v) { pe[v] = wide_exp2(sc[v] - m_run); ls += pe[v]; }
        l_run += ls;
        return w4f16{(_Float16)pe[0], (_Float16)pe[1], (_Float16)pe[2], (_Float16)pe[3]};
    };

    if (!is_resid) {
        // ================= code tiles =================
        const int ps_mask = p.page_size - 1;
        struct Codes { unsigned k[KD]; unsigned v[CG][2]; };
        struct Pids { long long k, v; };
        struct Ent { unsigned k[D / 8]; unsigned v[CG][4][EW]; };      // the lane's d/4 dims of K^; 4 tokens x CG sub-vectors of V^
        const unsigned short *kc = (const unsigned short *)p.k_codes, *vc = (const unsigned short *)p.v_codes;
        auto tile_t0 = [&](int j) {                // first token of this wave's j-th tile (clamped: re-request, never past the split)
            int ti = wave + kWW * j;
            if (ti > n_tiles - 1) ti = n_tiles - 1;
            return t_begin + kWT * ti;
        };
        const int *kid_base = p.ids64 ? (const int *)p.k_ids64 : p.k_ids32;      // low dword of an id (ids are < 2^31)
        const int *vid_base = p.ids64 ? (const int *)p.v_ids64 : p.v_ids32;
        const int id_stride = p.ids64 ? 2 : 1;
        auto load_pids = [&](int t0) -> Pids {
            const int idx = bh * p.n_pages_cap + (t0 >> p.ps_shift);             // < 2^31 (the host checks the page table size)
            Pids o;
            o.k = MILLION_CHECK_KID(p, (long long)kid_base[idx * id_stride]);
            o.v = MILLION_CHECK_VID(p, (long long)vid_base[idx * id_stride]);
            return o;
        };
        auto load_codes = [&](int t0, Pids id) -> Codes {
            Codes c;
            const int tk_ = min(t0 + c16, t_end - 1);
            const unsigned short *krow = kc + ((id.k << p.ps_shift) + (tk_ & ps_mask)) * M + q4 * (M / 4);
            if constexpr (KD == 2) { const v2u w = *(const v2u *)krow; c.k[0] = w[0]; c.k[1] = w[1]; }
            else {
#pragma unroll
                for (int i = 0; i < KD / 4; ++i) {
                    const w4u w = *(const w4u *)(krow + 8 * i);
                    c.k[4 * i] = w[0]; c.k[4 * i + 1] = w[1]; c.k[4 * i + 2] = w[2]; c.k[4 * i + 3] = w[3];
                }
            }
            // V: a tile never straddles a page (16 | page_size); codes of tokens >= T inside the page are whatever the page holds
#pragma unroll
            for (int cg = 0; cg < CG; ++cg) {
                const v2u w = *(const v2u *)(vc + ((id.v * M + 16 * cg + c16) << p.ps_shift) + (t0 & ps_mask) + 4 * q4);
                c.v[cg][0] = w[0]; c.v[cg][1] = w[1];
            }
            return c;
        };
        auto code_of = [&](unsigned w, int i) -> unsigned { return (w >> (16 * (i & 1))) & cmask; };
        const char *ktab = (const char *)p.k_tab, *vtab = (const char *)p.v_tab;
        const unsigned esz = DM * 2;
        const unsigned kbase = (unsigned)(q4 * (M / 4)) * (unsigned)p.C;          // entry index of the lane's first K subspace
        // every entry of a tile, requested in one burst: D/8 + 4 CG EW dwords per lane
        auto gather = [&](const Codes &c) -> Ent {
            Ent e;
#pragma unroll
            for (int j = 0; j < M / 4; ++j) {
                const char *ep = ktab + (kbase + (unsigned)j * (unsigned)p.C + code_of(c.k[j >> 1], j)) * esz;
                if constexpr (DM == 4) { const v2u x = *(const v2u *)ep; e.k[2 * j] = x[0]; e.k[2 * j + 1] = x[1]; }
                else e.k[j] = *(const unsigned *)ep;
            }
#pragma unroll
            for (int cg = 0; cg < CG; ++cg)
#pragma unroll
                for (int t = 0; t < 4; ++t) {
                    const char *ep = vtab + ((unsigned)(16 * cg + c16) * (unsigned)p.C + code_of(c.v[cg][t >> 1], t)) * esz;
                    if constexpr (DM == 4) { const v2u x = *(const v2u *)ep; e.v[cg][t][0] = x[0]; e.v[cg][t][1] = x[1]; }
                    else e.v[cg][t][0] = *(const unsigned *)ep;
                }
            return e;
        };
        auto scores_direct = [&](const Ent &e) -> w4f32 {
            w4f32 acc = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
            for (int st = 0; st < NS; ++st) {      // stage st = dims q4 d/4 + 8 st .. + 8 = dwords 4 st .. 4 st + 3 of the lane's K^ quarter
                const w4u a = {e.k[4 * st], e.k[4 * st + 1], e.k[4 * st + 2], e.k[4 * st + 3]};
                acc = __builtin_amdgcn_mfma_f32_16x16x32_f16(__builtin_bit_cast(w8f16, a), qb[st], acc, 0, 0, 0);
            }
            return acc;
        };
        auto values_direct = [&](const Ent &e, w4f16 P) {
#pragma unroll
            for (int cg = 0; cg < CG; ++cg)
#pragma unroll
                for (int x = 0; x < DM; ++x) {
                    const unsigned sel = (x & 1) ? 0x07060302u : 0x05040100u;
                    const v2u a = {__builtin_amdgcn_perm(e.v[cg][1][x >> 1], e.v[cg][0][x >> 1], sel),
                                   __builtin_amdgcn_perm(e.v[cg][3][x >> 1], e.v[cg][2][x >> 1], sel)};
                    O[cg * DM + x] = __builtin_amdgcn_mfma_f32_16x16x16f16(__builtin_bit_cast(w4f16, a), P, O[cg * DM + x], 0, 0, 0);
                }
        };

        if (n_tiles > 0) {
            const int my_tiles = wave < n_tiles ? (n_tiles - wave + kWW - 1) / kWW : 0;
            constexpr int kPF = kWidePF;
            Codes ring[kPF];
            Pids idr[kPF];
#pragma unroll
            for (int k = 0; k < kPF; ++k) idr[k] = load_pids(tile_t0(k));
#pragma unroll
            for (int k = 0; k < kPF; ++k) {
                ring[k] = load_codes(tile_t0(k), idr[k]);
                idr[k] = load_pids(tile_t0(k + kPF));
            }
            Ent ent = gather(ring[0]);
            for (int j0 = 0; j0 < my_tiles; j0 += kPF) {
#pragma unroll
                for (int k = 0; k < kPF; ++k) {
                    const int j = j0 + k;
                    const Ent cur = ent;
                    ring[k] = load_codes(tile_t0(j + kPF), idr[k]);
                    idr[k] = load_pids(tile_t0(j + 2 * kPF));
                    ent = gather(ring[(k + 1) % kPF]);                    // tile j + 1 (a clamped re-request past the last one)
                    if (j < my_tiles) {                                   // wave-uniform; no global load inside
                        const int t0 = tile_t0(j);
                        const w4f32 acc = scores_direct(cur);
                        const w4f16 P = softmax_tile(acc, min(kWT, t_end - t0));
                        values_direct(cur, P);
                    }
                }
            }
        }
    } else {
        // ================= residual window: the LDS tile of attn_tile.hip, filled from the fp16 rows =================
        const f16 *kres = p.k_res + b * p.res_sb + hk * p.res_sh;
        const f16 *vres = p.v_res + b * p.res_sb + hk * p.res_sh;
        auto row_of = [&](int i, const f16 *base, const f16 *fresh) -> const f16 * {      // window row i (clamped to a valid one)
            if (i > r - 1) i = r - 1;
            if (fresh && i == r_old) return fresh + (long long)bh * D;
            return base + (long long)((rstart + i) % p.rcap) * D;
        };
        for (int ti = wave; ti < n_tiles; ti += kWW) {
            const int t0 = kWT * ti;
            {
                const f16 *src = row_of(t0 + c16, kres, p.k_new) + q4 * (D / 4);
                char *dst = tile + c16 * kKRow + q4 * (D / 2);
#pragma unroll
                for (int i = 0; i < D / 32; ++i) *(w4u *)(dst + 16 * i) = *(const w4u *)((const char *)src + 16 * i);
            }
            wide_lds_phase();
            w4f32 acc = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
            for (int s = 0; s < NS; ++s) {
                const w4u a = *(const w4u *)(tile + c16 * kKRow + (q4 * (D / 4) + 8 * s) * 2);
                acc = __builtin_amdgcn_mfma_f32_16x16x32_f16(__builtin_bit_cast(w8f16, a), qb[s], acc, 0, 0, 0);
            }
            const w4f16 P = softmax_tile(acc, min(kWT, t_end - t0));
            wide_lds_phase();
#pragma unroll
            for (int j = 0; j < NTASK; ++j) {      // eight (d0, d1) pairs of consecutive tokens -> the two V^T rows of that dim pair
                const int task = j * 64 + lane, dp = task >> 1, oct = task & 1;
                unsigned e[8];
#pragma unroll
                for (int t = 0; t < 8; ++t) e[t] = *(const unsigned *)(row_of(t0 + 8 * oct + t, vres, p.v_new) + 2 * dp);
                w4u lo, hi;
#pragma unroll
                for (int i = 0; i < 4; ++i) {
                    lo[i] = __builtin_amdgcn_perm(e[2 * i + 1], e[2 * i], 0x05040100u);
                    hi[i] = __builtin_amdgcn_perm(e[2 * i + 1], e[2 * i], 0x07060302u);
                }
                *(w4u *)(tile + (2 * dp) * kVRow + oct * 16) = lo;
                *(w4u *)(tile + (2 * dp + 1) * kVRow + oct * 16) = hi;
            }
            wide_lds_phase();
#pragma unroll
            for (int n = 0; n < NC; ++n) {
                const v2u a = *(const v2u *)(tile + (16 * n + c16) * kVRow + (4 * q4) * 2);
                O[n] = __builtin_amdgcn_mfma_f32_16x16x16f16(__builtin_bit_cast(w4f16, a), P, O[n], 0, 0, 0);
            }
            wide_lds_phase();
        }
    }

    // ---- merge the waves' partials through LDS, then hand the workgroup's partial over ----
    __syncthreads();
    {
        const int wf = G * D + 2 * G;                         // floats per wave
        const float l_sum = rows_sum(l_run);
        float *ws = (float *)smem + wave * wf;                 // the wave tiles are dead (barrier above)
        if (c16 < G) {
#pragma unroll
            for (int n = 0; n < NC; ++n)
#pragma unroll
                for (int v = 0; v < 4; ++v) {
                    const int dim = is_resid ? 16 * n + 4 * q4 + v : (16 * (n / DM) + 4 * q4 + v) * DM + n % DM;
                    ws[c16 * D + dim] = O[n][v];
                }
            if (q4 == 0) { ws[G * D + c16] = m_run; ws[G * D + G + c16] = l_sum; }
        }
        __syncthreads();
        const float *w0 = (const float *)smem;
        for (int e = tid; e < wf; e += kWW * 64) {            // e: O[g][dim], then m[g], then l[g]
            const int g = e < G * D ? e / D : (e - G * D) % G;
            float mm = -INFINITY;
#pragma unroll
            for (int w = 0; w < kWW; ++w) mm = fmaxf(mm, w0[w * wf + G * D + g]);
            const float ms = mm > -INFINITY ? mm : 0.f;
            float o = mm;
            if (e < G * D || e >= G * D + G) {
                o = 0.f;
#pragma unroll
                for (int w = 0; w < kWW; ++w) o += w0[w * wf + e] * exp2f(w0[w * wf + G * D + g] - ms);
            }
            part[e] = o;
        }
        __syncthreads();
    }
    publish_and_merge<LSE>(p, b, hk, slot, part, (float *)smem, flag);
}

// The instances, by d (128, 64) and d_m (2, 4)
static const void *const kWideKernels[2][2][2] = {
    {{(const void *)attn_wide_kernel<128, 2>, (const void *)attn_wide_kernel<128, 2, true>},
     {(const void *)attn_wide_kernel<128, 4>, (const void *)attn_wide_kernel<128, 4, true>}},
    {{(const void *)attn_wide_kernel<64, 2>, (const void *)attn_wide_kernel<64, 2, true>},
     {(const void *)attn_wide_kernel<64, 4>, (const void *)attn_wide_kernel<64, 4, true>}},
};
static void wide_setup() {
    if (device_once(5))
        for (const auto &by_d : kWideKernels)
            for (const auto &by_dm : by_d)
                for (const void *k : by_dm) (void)hipFuncSetAttribute(k, hipFuncAttributeMaxDynamicSharedMemorySize, 160 * 1024);
}

bool wide_geometry(int d, int M, int C, int G) {
    const bool c_ok = C == 512 || C == 1024 || C == 2048 || C == 4096;
    return (d == 128 || d == 64) && M > 0 && d % M == 0 && (d / M == 2 || d / M == 4) && c_ok && G >= 1 && G <= kMaxGMfma;
}

bool plan_attn_wide(const AttnParams &p_in, AttnPlan &plan) {
    AttnParams p = p_in;
    if (!wide_geometry(p.d, p.M, p.C, p.Gt) || !p.k_paged || !p.v_paged || p.v_identity) return false;
    // split policy: the registers decide how many workgroups of 8 waves a CU holds (no codebook is in LDS): one at d = 128
    // (two tiles of entries in flight: ~200 VGPRs), two at d = 64; the splits of all (b, kv head) pairs and their window
    // workgroups fill that once.  A split is a multiple of 64 tokens and at least 256 tokens long.
    const int bh = p.bs * p.nh_k;
    const int room = (p.d == 64 ? 2 : 1) * device_cus();
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
    const size_t lds = (size_t)wide_region_bytes(p.d, p.G) + (size_t)p.slot_floats * 4 + 16;
    plan = {kWideKernels[p.d == 64][p.dm == 4][p.lse ? 1 : 0], dim3(p.nslots, bh), dim3(kWW * 64), lds, p, 6, wide_setup};
    return true;
}

}  // namespace million
