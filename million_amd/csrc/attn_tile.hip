// attn_tile.hip — fused decode attention over PQ codes for the shapes the streaming kernel does not take:
// d = 64 with M in {16, 32, 64}, d = 128 with M = 16, and whatever plan_attn_mfma declines (plan_attn_tile),
// gfx950 / CDNA4.
//
// Same job and same single launch as attn_mfma.hip (reference: LUT matmul + flash_decoding_split_kernel +
// flash_decoding_residual_kernel + flash_decoding_reduce_kernel, Interface.template.cu:26-120, Kernel.cuh:11-166,
// 1038-1270), written once for every sub-vector width d_m in {1, 2, 4, 8}:
//   * both codebooks (row image [m][c][d_m], fp16) sit in LDS for the whole kernel;
//   * a wave walks 16-token tiles on its own (no workgroup barrier inside the loop).  Round 4: a code tile no longer goes
//     through LDS (rounds 1-3 dequantised K^ and V^T into an LDS tile and read them back: four dependent LDS round trips per
//     tile, 3-15 % of the HBM peak) - the centroids go from the LDS-resident codebooks STRAIGHT into MFMA operands, as in
//     attn_mfma.hip:
//       1. scores: lane (quarter q4 of the dims, token): the lane's M/4 code bytes are its quarter of the code row; stage s
//          (8 dims of the quarter) gathers 8/d_m entries of the K row image - one ds_read_b128 / two b64 / four b32 / eight
//          u16 - which ARE the A operand of v_mfma_f32_16x16x32_f16 (B = the query heads, same dim order);
//       2. online softmax in the exp2 domain, fp32 (head = lane column; the probabilities are already laid out as the B
//          operand of step 4);
//       3. values: lane (4 tokens q4, subspace m = 16 cg + c16): 4 gathers of the V col image per column group cg (bank =
//          subspace); for every dim e of the sub-vector the four tokens' halves are packed (2 v_perm) into the A operand of
//          v_mfma_f32_16x16x16_f16 (rows = 16 subspaces, k = 16 tokens), B = P -> tile (cg, e) of O^T[(16 cg + row) d_m + e][head]:
//          d/16 accumulator tiles as before, the running rescale is lane-local;
//     M/4 + M/4 gathers, d/8 packs and d/32 + d/16 MFMAs per tile and wave; up to 16 query heads per launch (the 16 columns);
//   * the residual window keeps the LDS tile (one extra workgroup per (b, kv head), as in attn_generic.hip: K rows -> K^ tile ->
//     scores, V rows -> transposed V^T tile -> values), the fused append included (tile_wave.h: window_pass, park_new_row);
//   * the waves' partials are merged through LDS (tile_wave.h: merge_waves), the workgroups' through the workspace by the last
//     arriver (common.h: publish_and_merge), exactly as in the other two kernels.
// Code bytes are read once per kv head (all G = nh / nh_k query heads share a workgroup) straight into registers,
// kPF tiles ahead; page ids 2 kPF tiles ahead.  V must be in transposed pages (the reference's 10-argument row-major call
// is transposed first, million_api.hip).
#include "tile_wave.h"         // the wave-tile skeleton shared with attn_wide.hip: softmax step, window pass, wave merge, split rule
#include "dev_switches.h"      // MILLION_TILE_PROF (per-tile stamps) is a development switch: never in the product build

namespace million {

// Waves per workgroup (template parameter TW): see plan_attn_tile.  LDS: tile_wave.h, tile_region_bytes.
static size_t tile_lds_bytes(int d, int C, int slot_floats, int waves, int G) {
    return (size_t)tile_region_bytes(d, C, G, waves) + (size_t)slot_floats * 4 + 16;
}

template <int D, int DM, int TW, bool LSE = false>      // LSE: common.h, "Log-sum-exp"
__global__ __launch_bounds__(TW * 64, TW / 4) void attn_tile_kernel(AttnParams p) {
    constexpr int kTW = TW;
    constexpr int M = D / DM;
    constexpr int NS = D / 32;                 // score stages (32 dims each)
    constexpr int KD = M / 16;                 // K code dwords per lane and tile: lane (token, quarter) owns M/4 bytes
    constexpr int CG = M / 16;                 // column groups of 16 subspaces: V code dwords per lane and tile (4 tokens each)
    constexpr int EW = DM >= 2 ? DM / 2 : 1;   // dwords per gathered codebook entry
    extern __shared__ __attribute__((aligned(16))) char smem[];
    MILLION_DEBUG_FILL_LDS(smem, p.lds_fill);

    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int q4 = lane >> 4, c16 = lane & 15;
    const int slot = blockIdx.x, bh = blockIdx.y;
    const int b = bh / p.nh_k, hk = bh % p.nh_k;
    const int G = p.G, C = p.C;
    const unsigned cmask = (unsigned)C - 1u;   // C is 128 or 256: a stray byte past T still indexes inside its table row
    int T, r, rstart;
    load_lengths(p, b, T, r, rstart);
    const int r_old = r;
    if (p.k_new) r += 1;                       // fused append: the new token is window row r_old

    const int tab_bytes = D * C * 2;
    char *tk = smem, *tv = smem + tab_bytes;
    float *part = (float *)(smem + tile_region_bytes(D, C, G, kTW));
    int *flag = (int *)(part + p.slot_floats);

    const bool is_resid = slot == p.nsplit;
    const int t_begin = is_resid ? 0 : min(slot * p.split_len, T);
    const int t_end = is_resid ? r : min(t_begin + p.split_len, T);
    const int n_tiles = (t_end - t_begin + kTT - 1) / kTT;

    if (p.k_new && is_resid && tid < D) park_new_row<D>(p, b, hk, bh, rstart, r_old, tid);
    if (!is_resid && n_tiles > 0) {
        for (int i = tid * 16; i < tab_bytes; i += kTW * 64 * 16) {
            *(t4u *)(tk + i) = *(const t4u *)((const char *)p.k_tab + i);
            *(t4u *)(tv + i) = *(const t4u *)((const char *)p.v_tab_col + i);      // col image [c][m][d_m]: bank = subspace
        }
    }
    t8f16 qb[NS];
    load_query<D>(qb, p.q, (long long)b * p.nh + head0(p, hk), G, q4, c16);
    __syncthreads();

    WaveAcc<D> run;

#ifdef MILLION_TILE_PROF
    unsigned long long prof_t[5] = {0, 0, 0, 0, 0}, prof_acc[5] = {0, 0, 0, 0, 0};
    const unsigned long long prof_start = __builtin_amdgcn_s_memtime();
#define TILE_PROF_T(i) do { unsigned long long t_; asm volatile("s_waitcnt lgkmcnt(0)\n\ts_memtime %0\n\ts_waitcnt lgkmcnt(0)" : "=s"(t_) :: "memory"); prof_t[i] = t_; } while (0)
#define TILE_PROF_ACC() do { for (int i_ = 0; i_ < 4; ++i_) prof_acc[i_] += prof_t[i_ + 1] - prof_t[i_]; prof_acc[4] += 1; } while (0)
#else
#define TILE_PROF_T(i) do { } while (0)
#define TILE_PROF_ACC() do { } while (0)
#endif
    if (!is_resid) {
        // ================= code tiles =================
        const int tl = c16, mq = q4;           // step 1 lane roles: token, quarter of the code row
        const int ps_mask = p.page_size - 1;
        struct Codes { unsigned k[KD]; unsigned v[CG]; };      // K: the lane's quarter of its token's code row; V: 4 tokens of subspace 16 cg + c16
        auto tile_t0 = [&](int j) { return wave_tile_t0<kTW>(j, wave, n_tiles, t_begin); };
        // Page ids without a branch around the load (hipcc answers a load in a conditional with s_waitcnt vmcnt(0),
        // which would drain the code prefetch every tile): one 4-byte load of the low dword of the id (ids are < 2^31)
        // from a table chosen before the loop; a side without a table reads a dummy word and ignores it.
        const int *kid_base = p.k_paged ? (p.ids64 ? (const int *)p.k_ids64 : p.k_ids32) : (const int *)p.q;
        const int *vid_base = !p.v_identity ? (p.ids64 ? (const int *)p.v_ids64 : p.v_ids32) : (const int *)p.q;
        const int kid_stride = p.k_paged ? (p.ids64 ? 2 : 1) : 0;
        const int vid_stride = !p.v_identity ? (p.ids64 ? 2 : 1) : 0;
        auto load_pids = [&](int t0) -> Pids {
            const int idx = bh * p.n_pages_cap + (t0 >> p.ps_shift);      // < 2^31 (the host checks the page table size)
            Pids o;
            o.k = kid_base[idx * kid_stride];                               // 32-bit index arithmetic: a 64-bit multiply
            const int v = vid_base[idx * vid_stride];                       // here made hipcc tie a wait to an in-flight load
            o.v = p.v_identity ? idx : v;
#ifdef MILLION_DEBUG_CHECK_IDS
            if (p.k_paged) o.k = MILLION_CHECK_KID(p, o.k);
            if (!p.v_identity) o.v = MILLION_CHECK_VID(p, o.v);
#endif
            return o;
        };
        auto load_codes = [&](int t0, Pids id) -> Codes {
            Codes c;
            const int tk_ = min(t0 + tl, t_end - 1);
            const long long koff = p.k_paged ? ((id.k << p.ps_shift) + (tk_ & ps_mask)) * M
                                             : b * p.k_sb + hk * p.k_sh + (long long)tk_ * M;
            const uint8_t *krow = p.k_codes + koff + mq * (M / 4);
            if constexpr (KD == 1) c.k[0] = *(const unsigned *)krow;
            else if constexpr (KD == 2) { const v2u w = *(const v2u *)krow; c.k[0] = w[0]; c.k[1] = w[1]; }
            else { const t4u w = *(const t4u *)krow; c.k[0] = w[0]; c.k[1] = w[1]; c.k[2] = w[2]; c.k[3] = w[3]; }
            // V: a tile never straddles a page (16 | page_size); bytes of tokens >= T inside the page are whatever the page
            // holds: "& (C - 1)" keeps them inside the table and their probabilities are exact zeros
#pragma unroll
            for (int cg = 0; cg < CG; ++cg)
                c.v[cg] = *(const unsigned *)(p.v_codes + ((id.v * M + 16 * cg + c16) << p.ps_shift) + (t0 & ps_mask) + 4 * q4);
            return c;
        };
        // Lookup addresses: one v_bfe_u32 + one v_lshl_add_u32 per code byte.  The per-subspace table bases are lane
        // constants kept in registers, and the "& (C - 1)" that keeps a stray byte inside its table row is applied to four
        // bytes at once.
        constexpr unsigned kEsh = DM == 8 ? 4 : DM == 4 ? 3 : DM == 2 ? 2 : 1;      // log2(bytes per codebook entry)
        constexpr unsigned kVsh = D == 128 ? 8 : 7;                                  // log2(bytes per code of the V col image = 2 d)
        const unsigned cm4 = cmask * 0x01010101u;
        const char *kb[M / 4];
#pragma unroll
        for (int j = 0; j < M / 4; ++j) kb[j] = tk + (mq * (M / 4) + j) * C * (DM * 2);
        const char *vb[CG];
#pragma unroll
        for (int cg = 0; cg < CG; ++cg) vb[cg] = tv + (16 * cg + c16) * (DM * 2);
        auto code_of = [&](unsigned w, int i) -> unsigned { return ((w & cm4) >> (8 * (i & 3))) & 0xffu; };
        // ---- step 1: scores straight from the K row image ----
        auto scores_direct = [&](const Codes &c) -> t4f32 {
            t4f32 acc = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
            for (int st = 0; st < NS; ++st) {
                t4u a;
                if constexpr (DM == 8) {
                    a = *(const t4u *)(kb[st] + (code_of(c.k[st >> 2], st) << kEsh));
                } else if constexpr (DM == 4) {
                    const v2u x = *(const v2u *)(kb[2 * st] + (code_of(c.k[(2 * st) >> 2], 2 * st) << kEsh));
                    const v2u y = *(const v2u *)(kb[2 * st + 1] + (code_of(c.k[(2 * st + 1) >> 2], 2 * st + 1) << kEsh));
                    a = t4u{x[0], x[1], y[0], y[1]};
                } else if constexpr (DM == 2) {
#pragma unroll
                    for (int i = 0; i < 4; ++i) a[i] = *(const unsigned *)(kb[4 * st + i] + (code_of(c.k[(4 * st + i) >> 2], 4 * st + i) << kEsh));
                } else {
#pragma unroll
                    for (int i = 0; i < 4; ++i) {
                        const unsigned lo = *(const unsigned short *)(kb[8 * st + 2 * i] + (code_of(c.k[(8 * st + 2 * i) >> 2], 8 * st + 2 * i) << kEsh));
                        const unsigned hi = *(const unsigned short *)(kb[8 * st + 2 * i + 1] + (code_of(c.k[(8 * st + 2 * i + 1) >> 2], 8 * st + 2 * i + 1) << kEsh));
                        a[i] = __builtin_amdgcn_perm(hi, lo, 0x05040100u);
                    }
                }
                acc = __builtin_amdgcn_mfma_f32_16x16x32_f16(__builtin_bit_cast(t8f16, a), qb[st], acc, 0, 0, 0);
            }
            return acc;
        };
        // ---- step 3: the V entries of this lane's 4 tokens x CG subspaces (independent of the softmax: issued with the K gathers) ----
        struct VEnt { unsigned e[CG][4][EW]; };
        auto gather_v = [&](const Codes &c) -> VEnt {
            VEnt v;
#pragma unroll
            for (int cg = 0; cg < CG; ++cg)
#pragma unroll
                for (int t = 0; t < 4; ++t) {
                    const char *ep = vb[cg] + (code_of(c.v[cg], t) << kVsh);
                    if constexpr (DM == 8) { const t4u x = *(const t4u *)ep; v.e[cg][t][0] = x[0]; v.e[cg][t][1] = x[1]; v.e[cg][t][2] = x[2]; v.e[cg][t][3] = x[3]; }
                    else if constexpr (DM == 4) { const v2u x = *(const v2u *)ep; v.e[cg][t][0] = x[0]; v.e[cg][t][1] = x[1]; }
                    else if constexpr (DM == 2) v.e[cg][t][0] = *(const unsigned *)ep;
                    else v.e[cg][t][0] = *(const unsigned short *)ep;
                }
            return v;
        };
        // ---- step 4: O^T tile (cg, e) += V^T_e (rows = subspaces 16 cg + .., k = 16 tokens) P ----
        auto values_direct = [&](const VEnt &v, t4f16 P) {
#pragma unroll
            for (int cg = 0; cg < CG; ++cg)
#pragma unroll
                for (int e = 0; e < DM; ++e) {
                    const unsigned sel = (e & 1) ? 0x07060302u : 0x05040100u;
                    const v2u a = {__builtin_amdgcn_perm(v.e[cg][1][e >> 1], v.e[cg][0][e >> 1], sel),
                                   __builtin_amdgcn_perm(v.e[cg][3][e >> 1], v.e[cg][2][e >> 1], sel)};
                    run.O[cg * DM + e] = __builtin_amdgcn_mfma_f32_16x16x16f16(__builtin_bit_cast(t4f16, a), P, run.O[cg * DM + e], 0, 0, 0);
                }
        };

        if (n_tiles > 0) {
            const int my_tiles = wave < n_tiles ? (n_tiles - wave + kTW - 1) / kTW : 0;
            // Code bytes kPF tiles ahead, page ids 2 kPF tiles ahead, in a register ring with compile-time slots (the loop
            // is unrolled by the ring size; a tile is 5-9 registers).  One tile ahead is not enough: an iteration is
            // ~0.6 us of work and a load under traffic takes 1-2 us, so the loop ran at the load latency.
            constexpr int kPF = TW <= 8 ? 4 : 2;       // (sixteen waves per CU hide latency by themselves; <= 128 VGPRs)
            Codes ring[kPF];
            Pids idr[kPF];
#pragma unroll
            for (int k = 0; k < kPF; ++k) idr[k] = load_pids(tile_t0(k));
#pragma unroll
            for (int k = 0; k < kPF; ++k) {
                ring[k] = load_codes(tile_t0(k), idr[k]);
                idr[k] = load_pids(tile_t0(k + kPF));
            }
            for (int j0 = 0; j0 < my_tiles; j0 += kPF) {
#pragma unroll
                for (int k = 0; k < kPF; ++k) {
                    const int j = j0 + k;
                    const Codes cur = ring[k];
                    ring[k] = load_codes(tile_t0(j + kPF), idr[k]);
                    idr[k] = load_pids(tile_t0(j + 2 * kPF));
                    if (j < my_tiles) {                                   // wave-uniform; no global load inside
                        const int t0 = tile_t0(j);
                        TILE_PROF_T(0);
                        const t4f32 acc = scores_direct(cur);
                        const VEnt ve = gather_v(cur);
                        TILE_PROF_T(1);
                        const t4f16 P = softmax_tile(run, acc, min(kTT, t_end - t0), p.scale_log2e, q4);
                        TILE_PROF_T(2);
                        values_direct(ve, P);
                        TILE_PROF_T(3);
                        TILE_PROF_T(4);
                        TILE_PROF_ACC();
                    }
                }
            }
        }
    } else {
        window_pass<D, kTW>(run, qb, p, smem + wave * TileGeom<D>::kTile, b, hk, bh, r, r_old, rstart, wave, lane);
    }

#ifdef MILLION_TILE_PROF
    if (p.dbg && lane == 0) {
        unsigned long long *o = p.dbg + (((long long)blockIdx.y * gridDim.x + blockIdx.x) * kTW + wave) * 8;
        for (int i = 0; i < 5; ++i) o[i] = prof_acc[i];
        o[5] = __builtin_amdgcn_s_memtime() - prof_start;
    }
#endif
    merge_waves<D, DM, kTW>(run, (float *)smem, part, G, is_resid, tid);
    publish_and_merge<LSE>(p, b, hk, slot, part, (float *)smem, flag);
}

// The instances, by d (128, 64) and M (16, 32, 64)
static const void *const kTileKernels[2][3] = {
    {(const void *)attn_tile_kernel<128, 8, 16>, (const void *)attn_tile_kernel<128, 4, 8>, (const void *)attn_tile_kernel<128, 2, 8>},
    {(const void *)attn_tile_kernel<64, 4, 16>, (const void *)attn_tile_kernel<64, 2, 16>, (const void *)attn_tile_kernel<64, 1, 16>},
};
static const void *const kTileKernelsLse[2][3] = {      // LSE = true (common.h, "Log-sum-exp")
    {(const void *)attn_tile_kernel<128, 8, 16, true>, (const void *)attn_tile_kernel<128, 4, 8, true>, (const void *)attn_tile_kernel<128, 2, 8, true>},
    {(const void *)attn_tile_kernel<64, 4, 16, true>, (const void *)attn_tile_kernel<64, 2, 16, true>, (const void *)attn_tile_kernel<64, 1, 16, true>},
};
static void tile_setup() {
    if (device_once(2))
        for (const auto *tab : {kTileKernels, kTileKernelsLse})
            for (int i = 0; i < 2; ++i)
                for (const void *k : tab[i]) (void)hipFuncSetAttribute(k, hipFuncAttributeMaxDynamicSharedMemorySize, 160 * 1024);
}

bool plan_attn_tile(const AttnParams &p_in, AttnPlan &plan) {
    AttnParams p = p_in;
    const bool shape = (p.d == 128 || p.d == 64) && (p.M == 16 || p.M == 32 || p.M == 64) && (p.C == 128 || p.C == 256) &&
                       p.G <= kMaxGMfma;      // the 16 columns of the score tile: up to 16 query heads per kv head and launch (round 4)
    if (!shape || !p.v_paged || tile_lds_bytes(p.d, p.C, p.slot_floats, 16, p.G) > 160 * 1024) return false;
    // Waves per workgroup (round 4: a code tile needs no LDS of its own any more, so the codebooks alone decide how many
    // workgroups fit - one per CU at d = 128 - and the registers how many waves: 16 where the kernel stays within 128
    // registers (d = 64; d = 128 with 16-byte entries), 8 otherwise).  More waves = fewer 16-token tiles per wave and more
    // LDS round trips in flight.
    const int waves = (p.d == 64 || p.dm == 8) ? 16 : 8;
    // split policy: one workgroup per CU - the residual-window workgroup of every (b, kv head) included (rounds 2-3 sized the
    // splits for all CUs and launched bh more workgroups than the chip holds at d = 128: the last ones started when the first
    // finished)
    split_by_room(p, device_cus());
    const size_t lds = tile_lds_bytes(p.d, p.C, p.slot_floats, waves, p.G);
    plan = {(p.lse ? kTileKernelsLse : kTileKernels)[p.d == 64][p.M == 16 ? 0 : p.M == 32 ? 1 : 2], dim3(p.nslots, p.bs * p.nh_k), dim3(waves * 64), lds, p, 3, tile_setup};
    return true;
}

}  // namespace million
