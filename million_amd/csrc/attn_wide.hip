// attn_wide.hip — fused decode attention over 16-bit PQ codes (512 .. 4096 centroids per subspace) in page pools, gfx950 / CDNA4.
//
// Same job and same single launch as attn_tile.hip, and the same wave-tile skeleton (tile_wave.h: lane roles, softmax step,
// residual-window pass, wave merge, split rule): a lane's gathered codebook entries ARE the MFMA operands (scores: A = 8 dims of
// the lane's quarter of the K^ row; values: A = one dim of 16 subspaces x 16 tokens, B = the probabilities).
//
// What is this kernel's own: a table is C * d * 2 bytes = 128 KiB .. 1 MiB, so no codebook is in LDS.  Both tables are the
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
//
// Packed pages (million_hip.h, "Packed code pages"; million_pq_decode_attn_packed): the same kernel, HB = 2 / 4 high bits per
// code beside a low byte.  The K lane loads M/4 low bytes and M HB / 32 high bytes of its token, the V lane the low dword of its 4
// tokens and the dword of their high bytes (shared by 8 / HB lanes); a code is two shifts and an or in front of the same mask.
#include "tile_wave.h"

namespace million {

constexpr int kWW = 8;      // waves per workgroup
constexpr int kWidePF = 2;  // code tiles in flight per wave

// HB = 0: one uint16 per code.  HB = 2 / 4: packed pages (million_hip.h, "Packed code pages": a low-byte plane and a plane of HB
// high bits per code) - other load_codes / kcode / vcode and a smaller Codes ring; every other line is shared.
template <int D, int DM, bool LSE = false, int HB = 0>
__global__ __launch_bounds__(kWW * 64, 2) void attn_wide_kernel(AttnParams p) {
    constexpr int M = D / DM;
    constexpr int NS = D / 32;                 // score stages (32 dims each)
    constexpr int KD = M / 8;                  // K code dwords per lane and tile (M/4 codes of 16 bits)
    constexpr int CG = M / 16;                 // column groups of 16 subspaces
    constexpr int EW = DM / 2;                 // dwords per codebook entry
    constexpr int KLO = M / 16;                // packed: dwords of low bytes per K lane and tile (M/4 codes)
    constexpr int KHB = M * HB / 32;           // packed: bytes of high bits per K lane and tile (1, 2, 4 or 8)
    static_assert(DM == 2 || DM == 4, "entries of 4 or 8 bytes");
    static_assert(HB == 0 || HB == 2 || HB == 4, "uint16 codes, or 2 / 4 high bits beside a low byte");
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

    float *part = (float *)(smem + wide_region_bytes(D, G, kWW));
    int *flag = (int *)(part + p.slot_floats);

    const bool is_resid = slot == p.nsplit;
    const int t_begin = is_resid ? 0 : min(slot * p.split_len, T);
    const int t_end = is_resid ? r : min(t_begin + p.split_len, T);
    const int n_tiles = (t_end - t_begin + kTT - 1) / kTT;

    if (p.k_new && is_resid && tid < D) park_new_row<D>(p, b, hk, bh, rstart, r_old, tid);
    t8f16 qb[NS];
    load_query<D>(qb, p.q, (long long)b * p.nh + head0(p, hk), G, q4, c16);
    WaveAcc<D> run;

    if (!is_resid) {
        // ================= code tiles =================
        const int ps_mask = p.page_size - 1;
        // uint16: k = the lane's M/4 codes, v[cg] = 4 tokens' codes.  Packed: k = KLO dwords of low bytes then the high bits
        // (<= 2 dwords), v[cg] = {4 tokens' low bytes, the 4 bytes of their high fields}
        struct Codes { unsigned k[HB ? KLO + (KHB + 3) / 4 : KD]; unsigned v[CG][2]; };
        struct Ent { unsigned k[D / 8]; unsigned v[CG][4][EW]; };      // the lane's d/4 dims of K^; 4 tokens x CG sub-vectors of V^
        const unsigned short *kc = (const unsigned short *)p.k_codes, *vc = (const unsigned short *)p.v_codes;
        auto tile_t0 = [&](int j) { return wave_tile_t0<kWW>(j, wave, n_tiles, t_begin); };
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
        // packed pages: a page is page_size * M * (8 + HB) / 8 bytes - no power of two, so a page's offset is a 64-bit multiply
        const long long page_bytes = (long long)p.page_size * (M * (8 + HB) / 8);
        auto load_codes = [&](int t0, Pids id) -> Codes {
            Codes c;
            const int tk_ = min(t0 + c16, t_end - 1);
            if constexpr (HB != 0) {
                const uint8_t *kpage = p.k_codes + id.k * page_bytes, *vpage = p.v_codes + id.v * page_bytes;
                const uint8_t *klo = kpage + (tk_ & ps_mask) * M + q4 * (M / 4);
                const uint8_t *khi = kpage + (p.page_size * M + (tk_ & ps_mask) * (M * HB / 8) + q4 * KHB);
                if constexpr (KLO == 4) { const t4u w = *(const t4u *)klo; c.k[0] = w[0]; c.k[1] = w[1]; c.k[2] = w[2]; c.k[3] = w[3]; }
                else if constexpr (KLO == 2) { const v2u w = *(const v2u *)klo; c.k[0] = w[0]; c.k[1] = w[1]; }
                else c.k[0] = *(const unsigned *)klo;
                if constexpr (KHB == 8) { const v2u w = *(const v2u *)khi; c.k[KLO] = w[0]; c.k[KLO + 1] = w[1]; }
                else if constexpr (KHB == 4) c.k[KLO] = *(const unsigned *)khi;
                else if constexpr (KHB == 2) c.k[KLO] = *(const unsigned short *)khi;
                else c.k[KLO] = *khi;
                // V: the low dword of 4 tokens of the lane's subspace, and the dword of their high bytes, which 8 / HB
                // neighbouring lanes share
                const int tv = (t0 & ps_mask) + 4 * q4;
#pragma unroll
                for (int cg = 0; cg < CG; ++cg) {
                    const int m = 16 * cg + c16;
                    c.v[cg][0] = *(const unsigned *)(vpage + ((m << p.ps_shift) + tv));
                    c.v[cg][1] = *(const unsigned *)(vpage + (((M + m / (8 / HB)) << p.ps_shift) + tv));
                }
                return c;
            } else {
                const unsigned short *krow = kc + ((id.k << p.ps_shift) + (tk_ & ps_mask)) * M + q4 * (M / 4);
                if constexpr (KD == 2) { const v2u w = *(const v2u *)krow; c.k[0] = w[0]; c.k[1] = w[1]; }
                else {
#pragma unroll
                    for (int i = 0; i < KD / 4; ++i) {
                        const t4u w = *(const t4u *)(krow + 8 * i);
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
            }
        };
        auto code_of = [&](unsigned w, int i) -> unsigned { return (w >> (16 * (i & 1))) & cmask; };
        // code j of the lane's M/4 K codes; code of token t (0 .. 3) of column group cg.  Packed: the high field of the lane's
        // j-th subspace sits at bit HB j of its high bytes (the lane's first subspace is a multiple of 8 / HB), a V field at
        // the lane-constant bit HB (c16 mod 8 / HB) of its token's byte; `& cmask` drops the unused top bit at C = 512 / 2048
        const unsigned vsh = HB ? (unsigned)(HB * (c16 % (HB ? 8 / HB : 1))) : 0u;
        auto kcode = [&](const Codes &c, int j) -> unsigned {
            if constexpr (HB != 0) {
                const unsigned lo = (c.k[j >> 2] >> (8 * (j & 3))) & 0xffu;
                const unsigned hi = c.k[KLO + ((HB * j) >> 5)] >> ((HB * j) & 31);      // (what lies above the field: masked with the code)
                return ((hi << 8) | lo) & cmask;
            } else return code_of(c.k[j >> 1], j);
        };
        auto vcode = [&](const Codes &c, int cg, int t) -> unsigned {
            if constexpr (HB != 0) {
                const unsigned lo = (c.v[cg][0] >> (8 * t)) & 0xffu;
                const unsigned hi = c.v[cg][1] >> (8 * t + vsh);
                return ((hi << 8) | lo) & cmask;
            } else return code_of(c.v[cg][t >> 1], t);
        };
        const char *ktab = (const char *)p.k_tab, *vtab = (const char *)p.v_tab;
        const unsigned esz = DM * 2;
        const unsigned kbase = (unsigned)(q4 * (M / 4)) * (unsigned)p.C;          // entry index of the lane's first K subspace
        // every entry of a tile, requested in one burst: D/8 + 4 CG EW dwords per lane
        auto gather = [&](const Codes &c) -> Ent {
            Ent e;
#pragma unroll
            for (int j = 0; j < M / 4; ++j) {
                const char *ep = ktab + (kbase + (unsigned)j * (unsigned)p.C + kcode(c, j)) * esz;
                if constexpr (DM == 4) { const v2u x = *(const v2u *)ep; e.k[2 * j] = x[0]; e.k[2 * j + 1] = x[1]; }
                else e.k[j] = *(const unsigned *)ep;
            }
#pragma unroll
            for (int cg = 0; cg < CG; ++cg)
#pragma unroll
                for (int t = 0; t < 4; ++t) {
                    const char *ep = vtab + ((unsigned)(16 * cg + c16) * (unsigned)p.C + vcode(c, cg, t)) * esz;
                    if constexpr (DM == 4) { const v2u x = *(const v2u *)ep; e.v[cg][t][0] = x[0]; e.v[cg][t][1] = x[1]; }
                    else e.v[cg][t][0] = *(const unsigned *)ep;
                }
            return e;
        };
        auto scores_direct = [&](const Ent &e) -> t4f32 {
            t4f32 acc = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
            for (int st = 0; st < NS; ++st) {      // stage st = dims q4 d/4 + 8 st .. + 8 = dwords 4 st .. 4 st + 3 of the lane's K^ quarter
                const t4u a = {e.k[4 * st], e.k[4 * st + 1], e.k[4 * st + 2], e.k[4 * st + 3]};
                acc = __builtin_amdgcn_mfma_f32_16x16x32_f16(__builtin_bit_cast(t8f16, a), qb[st], acc, 0, 0, 0);
            }
            return acc;
        };
        auto values_direct = [&](const Ent &e, t4f16 P) {
#pragma unroll
            for (int cg = 0; cg < CG; ++cg)
#pragma unroll
                for (int x = 0; x < DM; ++x) {
                    const unsigned sel = (x & 1) ? 0x07060302u : 0x05040100u;
                    const v2u a = {__builtin_amdgcn_perm(e.v[cg][1][x >> 1], e.v[cg][0][x >> 1], sel),
                                   __builtin_amdgcn_perm(e.v[cg][3][x >> 1], e.v[cg][2][x >> 1], sel)};
                    run.O[cg * DM + x] = __builtin_amdgcn_mfma_f32_16x16x16f16(__builtin_bit_cast(t4f16, a), P, run.O[cg * DM + x], 0, 0, 0);
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
                        const t4f32 acc = scores_direct(cur);
                        const t4f16 P = softmax_tile(run, acc, min(kTT, t_end - t0), p.scale_log2e, q4);
                        values_direct(cur, P);
                    }
                }
            }
        }
    } else {
        window_pass<D, kWW>(run, qb, p, smem + wave * TileGeom<D>::kTile, b, hk, bh, r, r_old, rstart, wave, lane);
    }
    merge_waves<D, DM, kWW>(run, (float *)smem, part, G, is_resid, tid);
    publish_and_merge<LSE>(p, b, hk, slot, part, (float *)smem, flag);
}

// The instances, by d (128, 64) and d_m (2, 4)
static const void *const kWideKernels[2][2][2] = {
    {{(const void *)attn_wide_kernel<128, 2>, (const void *)attn_wide_kernel<128, 2, true>},
     {(const void *)attn_wide_kernel<128, 4>, (const void *)attn_wide_kernel<128, 4, true>}},
    {{(const void *)attn_wide_kernel<64, 2>, (const void *)attn_wide_kernel<64, 2, true>},
     {(const void *)attn_wide_kernel<64, 4>, (const void *)attn_wide_kernel<64, 4, true>}},
};
// ... and over packed pages, by the high bits of a code too (2: C = 512 / 1024, 4: C = 2048 / 4096)
#define MILLION_PACKED_PAIR(D, DM, HB) {(const void *)attn_wide_kernel<D, DM, false, HB>, (const void *)attn_wide_kernel<D, DM, true, HB>}
static const void *const kPackedKernels[2][2][2][2] = {
    {{MILLION_PACKED_PAIR(128, 2, 2), MILLION_PACKED_PAIR(128, 4, 2)}, {MILLION_PACKED_PAIR(64, 2, 2), MILLION_PACKED_PAIR(64, 4, 2)}},
    {{MILLION_PACKED_PAIR(128, 2, 4), MILLION_PACKED_PAIR(128, 4, 4)}, {MILLION_PACKED_PAIR(64, 2, 4), MILLION_PACKED_PAIR(64, 4, 4)}},
};
#undef MILLION_PACKED_PAIR
static void wide_setup() {
    if (device_once(5)) {
        for (const auto &by_d : kWideKernels)
            for (const auto &by_dm : by_d)
                for (const void *k : by_dm) (void)hipFuncSetAttribute(k, hipFuncAttributeMaxDynamicSharedMemorySize, 160 * 1024);
        for (const auto &by_hb : kPackedKernels)
            for (const auto &by_d : by_hb)
                for (const auto &by_dm : by_d)
                    for (const void *k : by_dm) (void)hipFuncSetAttribute(k, hipFuncAttributeMaxDynamicSharedMemorySize, 160 * 1024);
    }
}

bool wide_geometry(int d, int M, int C, int G) {
    const bool c_ok = C == 512 || C == 1024 || C == 2048 || C == 4096;
    return (d == 128 || d == 64) && M > 0 && d % M == 0 && (d / M == 2 || d / M == 4) && c_ok && G >= 1 && G <= kMaxGMfma;
}

bool plan_attn_wide(const AttnParams &p_in, AttnPlan &plan, bool packed) {
    AttnParams p = p_in;
    if (!wide_geometry(p.d, p.M, p.C, p.Gt) || !p.k_paged || !p.v_paged || p.v_identity) return false;
    // split policy: the registers decide how many workgroups of 8 waves a CU holds (no codebook is in LDS): one at d = 128
    // (two tiles of entries in flight: ~200 VGPRs), two at d = 64; the splits of all (b, kv head) pairs and their window
    // workgroups fill that once.  A split is a multiple of 64 tokens and at least 256 tokens long.
    split_by_room(p, (p.d == 64 ? 2 : 1) * device_cus());
    const size_t lds = (size_t)wide_region_bytes(p.d, p.G, kWW) + (size_t)p.slot_floats * 4 + 16;
    const void *kernel = packed ? kPackedKernels[packed_hi_bits(p.C) == 4][p.d == 64][p.dm == 4][p.lse ? 1 : 0]
                                : kWideKernels[p.d == 64][p.dm == 4][p.lse ? 1 : 0];
    plan = {kernel, dim3(p.nslots, p.bs * p.nh_k), dim3(kWW * 64), lds, p, 6, wide_setup};
    return true;
}

}  // namespace million
