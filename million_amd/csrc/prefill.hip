// prefill.hip — causal prompt attention on fp16 K/V (flash-style, MFMA), gfx950.
//
// Replaces: the scaled_dot_product_attention(q, repeat_kv(k), repeat_kv(v), is_causal=True) of the reference's prompt
// pass (scripts/utils/pq_utils.py:249-260 DynamicPQCache.prefill; scripts/utils/paged_pq_utils.py:216-320
// PagedPQCache.prefill) - without materialising repeat_kv: the G = nh / nh_k query heads of a kv head are served by the
// SAME workgroup, so a K/V tile is fetched once per kv head and q block, not once per query head.
//
//   out[b, h, i, :] = softmax_j<=q_pos0+i( q[b,h,i,:] . k[b,hk,j,:] / sqrt(d) ) v[b,hk,j,:],   hk = h / G
//
// Design
//   * workgroup = 8 waves = HPW query heads of one kv head x (256 / HPW) query rows; a wave owns 32 query rows of one head.
//     HPW = the largest of {8, 4, 2, 1} dividing G.  Linear block id -> kv head fastest (8 kv heads = 8 XCDs: every
//     workgroup that reads a kv head's K/V runs on one XCD, next to its L2), heaviest (last) query blocks first.
//   * K/V tiles of 64 keys go global -> LDS directly, issued one tile ahead (one barrier per tile); ONE LDS image serves the row
//     reads (ds_read_b128, K as the A operand) and the transposed reads (ds_read_b64_tr_b16, V^T as the A operand), both
//     conflict-free (tile_off, flash_tile.h).
//   * the tile step (flash_tile.h, shared with chunk_attn.hip): S^T = K Q^T with a query row on a lane, in-lane online softmax
//     in the exp2 domain plus one half-wave exchange, O^T += V^T P^T with P^T as the B operand straight from the score registers.
//   * causal: a workgroup walks the key tiles up to its last query row's diagonal; a wave skips tiles wholly above its own
//     rows and masks only the tiles its diagonal crosses.
//   * ragged batches (desc->dev_spans): the RAGGED instances read n_q, n_kv and q_pos0 of their request on the device and clamp
//     them (prefill_rows); the grid and the block order are those of the bounds, a query block at or past a request's rows
//     stores zeros and leaves before its first DMA, rows between a request's n_q and the bound are stored as zeros.  The
//     lockstep instances (RAGGED = false) are the kernels without any of it.
//
// Roofline: MFMA (2.5 PFLOP/s dense fp16).  FLOPs = 4 d nh (number of unmasked (i, j) pairs).  Per 64-key tile a wave
// issues 32 MFMAs (32 cycles each) and reads 32 KiB of LDS (K and V^T fragments are re-read by each of the 8 waves: 256
// B/clk/CU at the MFMA rate, i.e. the LDS ceiling equals the MFMA ceiling in this 8 x 32-row decomposition).
#include <type_traits>

#include "flash_tile.h"

#include "dev_switches.h"  // MILLION_EXP: development ablation switches of the pipelined kernel (tools/ab_build.py, tools/pf_ab.sh);
                           // 0 in the product build: 4 no value products, 8 no score products, 256 no exponentials, 512 no tile
                           // DMA, 1024 no tile wait / barrier, 2048 phase clock, 16384 one computing wave per SIMD, 32768 computing
                           // waves sleep behind the prologue barrier

namespace million {

struct PrefillParams {
    const f16 *q, *k, *v;
    f16 *out;
    int bs, nh, nh_k, G, d;
    int n_q, n_kv, q_pos0, causal;
    long long q_sb, q_sh, q_sn, k_sb, k_sh, k_sn, v_sb, v_sh, v_sn, o_sb, o_sh, o_sn;      // strides in elements; d contiguous
    int hpw;            // query heads per workgroup (1, 2, 4, 8)
    int n_qb;           // query blocks per head (of 256 / hpw rows)
    float scale_log2e;
    const int *dev_spans;      // RAGGED: (bs, 4) {n_q, n_kv, q_pos0, reserved} per request, or null (the host values above)
};

constexpr int kWaves = 8;         // waves per workgroup
constexpr int kKV = 64;           // keys per tile

// The rows of a wave and the key tiles of its workgroup (both kernels)
struct PrefillRows {
    int b, hk, head;
    int n_q, n_kv;               // the request's query rows and key rows: p.n_q / p.n_kv, or (RAGGED) its clamped device row
    int q_lo, q_row, q_pos;      // first query row of the wave, the lane's query row, its position among the keys (causal: keys <= q_pos)
    int nt;                      // key tiles of the workgroup: up to its last row's diagonal
    int w_pos_lo, w_pos_hi;      // positions of the wave's rows
    bool wg_live;                // RAGGED: false for a query block at or past the request's rows, or a request without keys
};
// RAGGED: n_q, n_kv and q_pos0 are per request, read once from its device row (scalar loads: b is workgroup-uniform) and never
// trusted - n_q into [0, p.n_q], n_kv and q_pos0 into [0, p.n_kv]; word 3 is not touched.  The grid, n_qb and the order of the
// query blocks are those of the bounds p.n_q / p.n_kv; everything below this function takes the request's own lengths from
// PrefillRows, so every tile boundary, clamp and mask is a function of them alone: a request's live rows are, bit for bit,
// those of the lockstep call on that request with the same three values.
template <bool RAGGED>
__device__ __forceinline__ PrefillRows prefill_rows(const PrefillParams &p, int wave, int r32) {
    PrefillRows w;
    int id = blockIdx.x;
    w.hk = id % p.nh_k;
    id /= p.nh_k;
    const int n_hg = p.G / p.hpw;
    const int hg = id % n_hg;
    id /= n_hg;
    const int qb = p.n_qb - 1 - id % p.n_qb;      // heaviest query blocks first
    w.b = id / p.n_qb;
    int n_q = p.n_q, n_kv = p.n_kv, q_pos0 = p.q_pos0;
    if (RAGGED) {
        // through the constant address space: the array is not written while the kernel runs, and only so does hipcc read it with
        // scalar loads (a plain global pointer might alias out: one vector load and three v_readfirstlane instead)
        typedef const __attribute__((address_space(4))) int *spans_p;
        const spans_p row = (spans_p)(p.dev_spans + 4 * (long long)w.b);
        n_q = clamp_count(row[0], p.n_q);
        n_kv = clamp_count(row[1], p.n_kv);
        q_pos0 = clamp_count(row[2], p.n_kv);
    }
    w.n_q = n_q;
    w.n_kv = n_kv;
    const int wph = kWaves / p.hpw;               // waves per head
    const int QB = wph * 32;                      // query rows per head in this workgroup
    const int g = hg * p.hpw + wave / wph;        // query head within the kv head's group
    w.head = w.hk * p.G + g;
    w.q_lo = qb * QB + (wave % wph) * 32;
    w.q_row = w.q_lo + r32;
    w.q_pos = q_pos0 + w.q_row;
    const int wg_q_hi = qb * QB + QB - 1 < n_q - 1 ? qb * QB + QB - 1 : n_q - 1;      // last query row of the workgroup
    int kv_end_wg = p.causal ? q_pos0 + wg_q_hi + 1 : n_kv;
    kv_end_wg = kv_end_wg < n_kv ? kv_end_wg : n_kv;
    w.nt = kv_end_wg > 0 ? (kv_end_wg + kKV - 1) / kKV : 0;
    w.w_pos_lo = q_pos0 + w.q_lo;
    w.w_pos_hi = q_pos0 + w.q_lo + 31;
    w.wg_live = !RAGGED || (qb * QB < n_q && n_kv > 0);
    return w;
}

// RAGGED: zeros into the lane's output row if it lies below the bound p.n_q - for a row at or past its request's n_q, and for
// every row of a workgroup without work (wg_live = false), which leaves through this before the first load of q, the first DMA
// and the first barrier (workgroup-uniform).
// LSE: such a row has no key - its log-sum-exp is -inf (prefill_store_lse).
template <int NB, bool LSE = false>
__device__ __forceinline__ void prefill_store_dead(const PrefillParams &p, const PrefillRows &w, int hh, float *lse = nullptr) {
    if (w.q_row < p.n_q) {
        flash_store_zero_row<NB>(p.out + w.b * p.o_sb + w.head * p.o_sh + (long long)w.q_row * p.o_sn, hh);
        if (LSE && hh == 0) lse[((long long)w.b * p.nh + w.head) * p.n_q + w.q_row] = -INFINITY;
    }
}

// LSE instances: ln sum_j exp(q . k_j / sqrt(d)) of the lane's row from the softmax state the output was divided by: ref2 = the
// reference of the exponentials in exp2 units (scale log2 e x raw score), l = the row's total of exp2(score2 - ref2) over both
// half-waves (after flash_l_total).  No visible key (l = 0): -inf, whatever the reference.  One store per row (half-wave 0).
__device__ __forceinline__ void prefill_store_lse(const PrefillParams &p, const PrefillRows &w, int hh, float ref2, float l, float *lse) {
    if (hh == 0) lse[((long long)w.b * p.nh + w.head) * p.n_q + w.q_row] = l > 0.f ? 0.6931471805599453f * (ref2 + __builtin_amdgcn_logf(l)) : -INFINITY;
}

// the lane's query row of Q (rows past the end read the last one: their output is not stored)
__device__ __forceinline__ const f16 *prefill_q_row(const PrefillParams &p, const PrefillRows &w) {
    const int qr = w.q_row < w.n_q ? w.q_row : w.n_q - 1;
    return p.q + w.b * p.q_sb + w.head * p.q_sh + (long long)qr * p.q_sn;
}

// D = 128 (the Llama head size of every BASELINE config) and D = 64 (the other head size the reference builds, setup.py:12).
// RAGGED (both kernels): the instances behind desc->dev_spans; the lockstep instances (RAGGED = false) are the kernels without any of it.
// LSE (both kernels): the instances behind million_prefill_attn_lse - the same body plus one fp32 store per row at the end; they are
// kernels of their own names (prefill_lse_kernel, prefill_lse_pipe_kernel below) with lse (bs, nh, n_q) as a second argument, so the
// six prefill_attn_* instances and their arguments are what they were.
template <int D, bool RAGGED, bool LSE>
__device__ __forceinline__ void prefill_attn_body(const PrefillParams p, float *lse) {
    constexpr int DS = D / 16;                 // k-steps of the score product
    constexpr int NB = D / 32;                 // 32-row blocks of O^T
    constexpr int kTileBytes = kKV * 2 * D;    // one [64][D] fp16 tile
    extern __shared__ __attribute__((aligned(16))) char pf_smem[];      // [2 buffers][K tile | V tile]
    if ((unsigned)(size_t)(__attribute__((address_space(3))) char *)pf_smem != 0u) __builtin_trap();      // absolute LDS addressing below
    const int tid = threadIdx.x, lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int r32 = lane & 31, hh = lane >> 5;
    const PrefillRows w = prefill_rows<RAGGED>(p, wave, r32);
    if (RAGGED && !w.wg_live) { prefill_store_dead<NB, LSE>(p, w, hh, lse); return; }
    const int nt = w.nt, n_q = w.n_q, n_kv = w.n_kv;
    const bool wave_live = w.q_lo < n_q;                                                   // wave-uniform
    v8h qf[DS];
    flash_load_q<D>(qf, prefill_q_row(p, w), hh);

    // ---- staging: global -> LDS directly (global_load_lds_dwordx4: no registers, no ds_write).  A wave instruction moves
    //      64 x 16 bytes into 1 KiB of CONSECUTIVE LDS, so the swizzle of the image is applied on the global side: lane l of
    //      piece j fills 16-byte slot 64 j + l of a tile and fetches the (row, chunk) that tile_off puts there (tile_rc).  The
    //      ablation of the register-staged form priced staging at 1.3 of 9.2 ms (address arithmetic, 4 global loads + 4
    //      ds_write_b128 per thread and tile, the wait in front of the stores).  The instruction is issued from inline asm: hipcc
    //      answers the builtin with s_waitcnt vmcnt(0) in front of every later LDS read; the waits are explicit (dma_wait). ----
    const f16 *kbase = p.k + w.b * p.k_sb + w.hk * p.k_sh;
    const f16 *vbase = p.v + w.b * p.v_sb + w.hk * p.v_sh;
    constexpr int kPieces = kTileBytes / 1024;          // 1-KiB pieces per tile side (16 / 8)
    constexpr int NPW = 2 * kPieces / kWaves;           // pieces per wave and tile: K and V (4 / 2)
    TileRC prc[NPW];                                    // the (row, 16-byte chunk) this lane fetches for its piece i
#pragma unroll
    for (int i = 0; i < NPW; ++i) prc[i] = tile_rc<D>(64 * ((wave + kWaves * i) % kPieces) + lane);
    auto dma_tile = [&](int t, int buf) {
#pragma unroll
        for (int i = 0; i < NPW; ++i) {
            const int pcg = wave + kWaves * i;          // wave-uniform: pieces [0, kPieces) are K, the rest V
            const bool is_v = pcg >= kPieces;
            int kvr = t * kKV + prc[i].row;
            kvr = kvr < n_kv ? kvr : n_kv - 1;          // clamped: rows past the end are masked below
            const f16 *src = (is_v ? vbase + (long long)kvr * p.v_sn : kbase + (long long)kvr * p.k_sn) + 8 * prc[i].ch;
            const unsigned dst = 2u * kTileBytes * buf + (is_v ? kTileBytes : 0) + 1024u * (pcg % kPieces);
            asm volatile("s_mov_b32 m0, %1\n\tglobal_load_lds_dwordx4 %0, off" :: "v"(src), "s"(dst) : "memory", "m0");
        }
    };
    auto dma_wait = [&]() { asm volatile("s_waitcnt vmcnt(0)" ::: "memory"); };

    v16f O[NB];
#pragma unroll
    for (int i = 0; i < NB; ++i)
#pragma unroll
        for (int j = 0; j < 16; ++j) O[i][j] = 0.f;
    float m_run = -INFINITY, l_run = 0.f;      // m in the scaled exp2 domain

    if (nt > 0) dma_tile(0, 0);
    dma_wait();
    __syncthreads();
    // One key tile.  The buffer index is a compile-time constant (the tile loop below is unrolled by two): the buffer's base then
    // rides in the immediate offset of every ds_read instead of one v_or per read (48 per tile; written as integer arithmetic
    // hipcc hoisted a second set of 48 address registers instead and spilled).
    auto tile = [&](auto bufc, const int t) {
        constexpr int buf = decltype(bufc)::value;
        // the other buffer was last read in iteration t - 1 and every wave has passed that iteration's barrier: the next
        // tile's bytes fly into it during this tile's products
        if (t + 1 < nt) dma_tile(t + 1, buf ^ 1);
        const int kv0 = t * kKV;
        const bool tile_live = wave_live && (!p.causal || kv0 <= w.w_pos_hi);      // wave-uniform
        if (tile_live) {
            constexpr unsigned kb = 2u * kTileBytes * buf, vb = kb + kTileBytes;
            float sc[32];
            flash_scores<D, kb>(sc, qf, r32, hh);
            // ---- mask (only where the diagonal or the end of the keys crosses this tile) ----
            const bool need_mask = (p.causal && kv0 + kKV - 1 > w.w_pos_lo) || kv0 + kKV > n_kv;        // wave-uniform
            if (need_mask) {
                const int lim = p.causal ? (w.q_pos < n_kv - 1 ? w.q_pos : n_kv - 1) : n_kv - 1;           // last key this row attends to
#pragma unroll
                for (int j = 0; j < 32; ++j) {
                    const int kv = kv0 + 32 * (j >> 4) + (j & 3) + 8 * ((j & 15) >> 2) + 4 * hh;
                    sc[j] = kv <= lim ? sc[j] : -INFINITY;
                }
            }
            flash_softmax(sc, O, m_run, l_run, p.scale_log2e);
            flash_pv<D, vb>(O, sc, lane);
        }
        dma_wait();
        __syncthreads();
    };
    for (int t = 0; t < nt; t += 2) {
        tile(std::integral_constant<int, 0>{}, t);
        if (t + 1 < nt) tile(std::integral_constant<int, 1>{}, t + 1);
    }
    l_run = flash_l_total(l_run);
    if (wave_live && w.q_row < n_q) {
        flash_store_row(O, l_run, p.out + w.b * p.o_sb + w.head * p.o_sh + (long long)w.q_row * p.o_sn, hh);
        if (LSE) prefill_store_lse(p, w, hh, m_run, l_run, lse);      // m_run: already in exp2 units (-inf only with l = 0)
    } else if (RAGGED) prefill_store_dead<NB, LSE>(p, w, hh, lse);      // rows between the request's n_q and the bound
}

// =====================================================================================================
// Pipelined form (round 5; d = 128, 8 waves): the same tiles, layouts and numerics as prefill_attn_kernel above, but a wave's
// instruction stream is software-pipelined across 32-key HALF tiles and every matrix instruction is PINNED where it is written:
//   half-step h:   phase 1   the 8 score products of half h + 1 (K operands requested three steps ahead), each followed by the
//                            exponentials / row sums / fp16 pack of TWO scores of half h; its last three gaps request phase 2's
//                            first three V operands;
//                  phase 2   the 8 value products of half h (V operands three steps ahead), each followed by one v_max3 of the running maximum over half h + 1's
//                            raw scores; then the reference decision for half h + 1 (lazy reference as in the decode kernels: it
//                            moves - rescale of O and l, a wave-uniform branch - only when a probability would exceed 2^8: P <= 2^8 is an
//                            exact fp16 operand; the rescale sits behind ALL value products of half h, cdna_hip_programming.md T13).
// Whole-tile pipelining (16 + 16 products per phase) holds both score halves of two tiles, 16 probability pairs and their operands:
// 256 registers and 41-127 spilled dwords - qf and the fragment addresses reloaded in front of every product with vmcnt(0) waits
// that also wait for the tile DMA: 646 TFLOP/s against 979 for the plain kernel.  Half tiles keep 16 + 16 score registers.
// The K stream runs half a tile ahead of V: iteration t reads K halves 2 t + 1, 2 t + 2 and V tile t, and its DMA brings K halves
// 2 t + 3, 2 t + 4 and V tile t + 1 (K half h sits in quarter h & 3 of the K region = tile (h >> 1) & 1's buffer: nothing moves).
// Round 4 built a cross-tile pipeline at source level and measured no gain: hipcc kept 'ds_read, s_waitcnt, v_mfma' triples and runs
// of 30-100 vector instructions - an MFMA is register-only and has no chain to sched_barrier() in the selection DAG, so the compiler
// moves it at will (seen again in the lean decode kernel this round).  Here an empty asm volatile("" : "+v"(accumulator)) behind
// every product and behind every softmax slice fixes the order: M, 7 vector, M, 7 vector ... as written.
// =====================================================================================================
#define PF_PIN(x) asm volatile("" : "+v"(x))
template <bool RAGGED, bool LSE>
__device__ __forceinline__ void prefill_attn_pipe_body(const PrefillParams p, float *lse) {
    constexpr int D = 128, DS = D / 16, NB = D / 32, kTileBytes = kKV * 2 * D;
    extern __shared__ __attribute__((aligned(16))) char pf_smem[];
    if ((unsigned)(size_t)(__attribute__((address_space(3))) char *)pf_smem != 0u) __builtin_trap();
    const int tid = threadIdx.x, lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int r32 = lane & 31, hh = lane >> 5;
    const PrefillRows w = prefill_rows<RAGGED>(p, wave, r32);
    if (RAGGED && !w.wg_live) { prefill_store_dead<NB, LSE>(p, w, hh, lse); return; }
    const int q_pos = w.q_pos, nt = w.nt, w_pos_lo = w.w_pos_lo, w_pos_hi = w.w_pos_hi, n_q = w.n_q, n_kv = w.n_kv;
    v8h qf[DS];
    flash_load_q<D>(qf, prefill_q_row(p, w), hh);
    // Q stays as it is given and a half's score products start from -reference instead of 0: the accumulator is s - reference in
    // raw score units and p = exp2(cs * accumulator), one packed multiply per two scores.  (Until profiles/flash_numerics.txt Q
    // carried cs, rounded to fp16 again, and the accumulator was the exponent itself: +2 % throughput, but a score error
    // proportional to the score - worst output row 1.7e-3 / 3.4e-3 at logit standard deviation 4 / 8 against the bar of 1e-3,
    // hidden by the whole-tensor norm: tests/test_flash_numerics_host.py.)
    const float cs = p.scale_log2e, thr_raw = 8.0f / cs;      // P <= 2^8: the accumulator may rise to 8 / cs before the reference moves
    const int nh2 = 2 * nt;                                              // 32-key halves of this workgroup
#if MILLION_EXP & 16384
    const bool wave_live = w.q_lo < n_q && wave < 4;      // diagnostic: one computing wave per SIMD (its partner only issues DMA and joins barriers)
#else
    const bool wave_live = w.q_lo < n_q;
#endif
    const f16 *kbase = p.k + w.b * p.k_sb + w.hk * p.k_sh;
    const f16 *vbase = p.v + w.b * p.v_sb + w.hk * p.v_sh;
    // one-KiB pieces (4 rows of a tile): a K half = pieces 8 jt .. 8 jt + 7 of its tile: one per wave; a V tile = 16: two per wave
    TileRC prc[2];
#pragma unroll
    for (int i = 0; i < 2; ++i) prc[i] = tile_rc<D>(64 * (wave + kWaves * i) + lane);
    auto dma_piece = [&](int t, int i, bool is_v) {      // piece wave + 8 i of tile t's K or V side -> buffer t & 1
        int kvr = t * kKV + prc[i].row;
        kvr = kvr < n_kv ? kvr : n_kv - 1;      // the request's own last key row: a V row past it may hold NaN, and 0 x NaN is NaN
        const f16 *src = (is_v ? vbase + (long long)kvr * p.v_sn : kbase + (long long)kvr * p.k_sn) + 8 * prc[i].ch;
        const unsigned dst = 2u * kTileBytes * (t & 1) + (is_v ? kTileBytes : 0) + 1024u * (wave + kWaves * i);
        asm volatile("s_mov_b32 m0, %1\n\tglobal_load_lds_dwordx4 %0, off" :: "v"(src), "s"(dst) : "memory", "m0");
    };
    auto dma_k_half = [&](int h) { if (h < nh2) dma_piece(h >> 1, h & 1, false); };
    auto dma_v_tile = [&](int t) { if (t < nt) { dma_piece(t, 0, true); dma_piece(t, 1, true); } };
    auto dma_wait = [&]() { asm volatile("s_waitcnt vmcnt(0)" ::: "memory"); };

    v16f O[NB];
#pragma unroll
    for (int i = 0; i < NB; ++i)
#pragma unroll
        for (int j = 0; j < 16; ++j) O[i][j] = 0.f;
    float m_ref = -INFINITY, neg_ref = 0.f, thr_rel = -INFINITY, l_run = 0.f;      // raw score units; thr_rel: thr_raw once a reference exists (scores are relative to it)
    const int qd = (lane >> 2) & 3, pp = lane & 3, g16 = (lane >> 4) & 1;

    // wave-uniform predicates of half h (keys 32 h .. 32 h + 31) for this wave
    auto live = [&](int h) { return h < nh2 && wave_live && (!p.causal || 32 * h <= w_pos_hi); };
    auto masked = [&](int h) { return (p.causal && 32 * h + 31 > w_pos_lo) || 32 * h + 32 > n_kv; };
    // raw scores of half h -> -inf where the row does not attend; compares against immediates: key = 32 h + 4 hh + (j & 3) + 8 (j >> 2) <= lim
    auto mask_half = [&](int h, v16f &S) {
        const int lim = p.causal ? (q_pos < n_kv - 1 ? q_pos : n_kv - 1) : n_kv - 1;
        const int rel = lim - 32 * h - 4 * hh;
#pragma unroll
        for (int j = 0; j < 16; ++j) S[j] = (j & 3) + 8 * (j >> 2) <= rel ? S[j] : -INFINITY;
    };
    v16f NEG;      // -reference of the lane's query row in every register: the initial accumulator of a half's score products
#pragma unroll
    for (int j = 0; j < 16; ++j) NEG[j] = 0.f;
    // the reference decision for a half whose per-lane maximum (relative to the current reference) is mx (both half-waves hold the
    // same query rows); Nx = that half's scores, already computed against the old reference: they move with it
    auto decide = [&](float mx, v16f &Nx) {
        {
            const v2u ex = swap32_self(__float_as_uint(mx));
            const unsigned e0 = ex[0], e1 = ex[1];
            mx = fmaxf(__uint_as_float(e0), __uint_as_float(e1));
        }
        if (__any(mx > thr_rel)) {
            const float m_new = fmaxf(m_ref, mx - neg_ref);      // mx is relative to the old reference (neg_ref = -m_safe)
            const float m_safe = m_new > -INFINITY ? m_new : 0.f;
            const float alpha = __builtin_amdgcn_exp2f((m_ref - m_safe) * cs);
#pragma unroll
            for (int i = 0; i < NB; ++i)      // alpha = 0 on the first move (O = 0 then), 1 when only another row's maximum moved
#pragma unroll
                for (int j = 0; j < 16; ++j) O[i][j] *= alpha;
            l_run *= alpha;
            m_ref = m_new;
            const float shift = -m_safe - neg_ref;      // the scores already computed move to the new reference
#pragma unroll
            for (int j = 0; j < 16; ++j) { Nx[j] += shift; NEG[j] = -m_safe; }
            neg_ref = -m_safe;
            thr_rel = thr_raw;
        }
    };
    // Fragment addresses as 8 + 8 lane constants with everything else in the ds_read immediates (the plain kernel keeps 16 + 32
    // address registers live across its loop; the pipeline has no room for them).  tile_off<128>(row, ch) = 256 row + 16 (ch ^ X(row)) with
    // X = ((row & 3) << 2) | ((row >> 2) & 3):
    //   K rows 32 jt + r32, chunk 2 s + hh: X depends on r32 only, so  addr = ka[s] + 256 * 32 jt,  ka[s] = 256 r32 + 16 ((2 s + hh) ^ X(r32))
    //   V rows 32 jt + 16 ks + 8 hi + 4 hh + qd, chunk 4 blk + 2 g16 + (pp >> 1): row & 3 = qd, (row >> 2) & 3 = 2 hi + hh, so
    //   addr = va[hi][blk] + 256 (32 jt + 16 ks),  va[hi][blk] = 256 (8 hi + 4 hh + qd) + 16 (((blk ^ qd) << 2) | ((2 g16 + (pp >> 1)) ^ (2 hi + hh))) + 8 (pp & 1)
    unsigned ka[DS], va[2][NB];
    {
        const unsigned X = ((r32 & 3) << 2) | ((r32 >> 2) & 3);
#pragma unroll
        for (int s_ = 0; s_ < DS; ++s_) ka[s_] = 256u * r32 + 16u * ((2u * s_ + hh) ^ X);
#pragma unroll
        for (int hi_ = 0; hi_ < 2; ++hi_)
#pragma unroll
            for (int blk_ = 0; blk_ < NB; ++blk_)
                va[hi_][blk_] = 256u * (8 * hi_ + 4 * hh + qd) + 16u * ((((unsigned)blk_ ^ qd) << 2) | ((2u * g16 + (pp >> 1)) ^ (2u * hi_ + hh))) + 8u * (pp & 1);
    }
    // K half HQ (0..3: buffer HQ >> 1, rows 32 (HQ & 1) ..), k-step S;  V of buffer BUFV, half JT, key step KS, operand half HI, dim block BLK
#define PF_KFRAG(HQ, S) __builtin_bit_cast(v8h, ((lds_v4u_p)(size_t)ka[S])[(2u * kTileBytes * ((HQ) >> 1) + 256u * 32u * ((HQ) & 1)) / 16])
#define PF_VFRAG(BUFV, JT, KS, HI, BLK) __builtin_amdgcn_ds_read_tr16_b64_v4i16((lds_v4s_p)(size_t)va[HI][BLK] + (2u * kTileBytes * (BUFV) + kTileBytes + 256u * (32u * (JT) + 16u * (KS))) / 8)

#if MILLION_EXP & 2048
    // phase clock of this wave (tools/prefill_prof.py): cycles since the previous stamp are added to slot I.  s_memtime needs
    // lgkmcnt(0), so a stamp also drains the wave's LDS reads - the profile runs a few percent slow and over-states the slot behind
    // a stamp that cuts a read-ahead.  Slots: 0 DMA issue, 1 phase 1, 2 mask, 3 phase 2, 4 reference decision, 5 DMA wait + barrier
    unsigned long long pt_last = __builtin_readcyclecounter();
    unsigned pt_acc[8] = {0, 0, 0, 0, 0, 0, 0, 0};
#define PT(I) { const unsigned long long n_ = __builtin_readcyclecounter(); pt_acc[I] += (unsigned)(n_ - pt_last); pt_last = n_; }
#else
#define PT(I)
#endif
    // prologue: K halves 0, 1, 2 and V tile 0
    dma_k_half(0); dma_k_half(1); dma_k_half(2); dma_v_tile(0);
#pragma unroll
    for (int s = 0; s < DS; ++s) asm volatile("" : "+v"(qf[s]));      // hipcc's vmcnt model: Q has landed here, not 'somewhere in the loop'
    dma_wait();
    __syncthreads();
    v16f SA, SB;      // raw scores: of the current half / accumulating the next one (roles swap every half-step)
    bool cur_live = live(0);
#if MILLION_EXP & 32768
    // diagnostic: a computing wave reaches its first read of K half 0 some 17 us behind the prologue barrier (5 x 8128 clocks;
    // no loop, no memory) - whatever an idle wave may write into quarter 0 before that read has landed by then
    if (cur_live) asm volatile("s_sleep 127\n\ts_sleep 127\n\ts_sleep 127\n\ts_sleep 127\n\ts_sleep 127" ::: "memory");
#endif
    if (cur_live) {      // scores of half 0 (plain), mask, reference
#pragma unroll
        for (int s = 0; s < DS; ++s)
            SA = s == 0 ? __builtin_amdgcn_mfma_f32_32x32x16_f16(PF_KFRAG(0, s), qf[s], v16f{0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f}, 0, 0, 0)
                        : __builtin_amdgcn_mfma_f32_32x32x16_f16(PF_KFRAG(0, s), qf[s], SA, 0, 0, 0);
        if (masked(0)) mask_half(0, SA);
        float mx = SA[0];
#pragma unroll
        for (int j = 1; j < 16; ++j) mx = fmaxf(mx, SA[j]);
        decide(mx, SA);
    }
    // The prologue's read of quarter 0 (K half 0) and the first burst's write into it (K half 4) need a barrier of their own: a
    // wave without rows skips the scores above (and any wave may be through them first) and would otherwise request half 4 while
    // its neighbours still multiply against half 0 (profiles/prefill_prologue_race.txt).  Every wave joins: nothing above
    // leaves the kernel but the workgroup-uniform wg_live exit.
    __syncthreads();
    // One half-step: half h (scores in C, reference decided; its V rows: buffer HQ >> 1, half HQ & 1) and half h + 1 (scores into N;
    // its K rows: quarter (HQ + 1) & 3).  HQ = h & 3 is a compile-time constant: the tile loop is unrolled by two.
    // iteration t: half-steps 2 t and 2 t + 1; its DMA: K halves 2 t + 3, 2 t + 4 and V tile t + 1.  The rule: between the last read
    // of a region (a K quarter, a V buffer) and the next request into it stands a barrier that every wave joins.  Quarter (2 t + 3) & 3
    // was last read by half-step 2 t - 2 (half 2 t - 1), quarter (2 t + 4) & 3 by half-step 2 t - 1 (half 2 t) and V buffer (t + 1) & 1
    // by both (tile t - 1): all in iteration t - 1, in front of its PF_SYNC.  For t = 0 there is no such iteration: quarter 3 and V
    // buffer 1 have never been read, and quarter 0 was read by the prologue's scores of half 0 - in front of the barrier above.
    // (tests/test_prefill_schedule_host.py restates this schedule and checks the rule for every tile count.)
#if MILLION_EXP & 512
#define PF_DMA(T) (void)0
#else
#define PF_DMA(T) dma_k_half(2 * (T) + 3); dma_k_half(2 * (T) + 4); dma_v_tile((T) + 1)
#endif
#if MILLION_EXP & 1024
#define PF_SYNC() (void)0
#else
#define PF_SYNC() dma_wait(); __syncthreads()
#endif
    // (Tried, no change: an iteration's first half-step requesting its first three K operands BEFORE it issues the iteration's DMA
    // pieces, and the second half-step's in the first one's last gaps - the LDS round trip at a phase's start is not what the
    // loop waits for: 1060 vs 1062 TFLOP/s, profiles/r05_prefill.txt.)
    // (Tried, slower: a wave's four DMA pieces issued inside the MFMA gaps of the iteration's first half-step, two per phase, at
    // wave-dependent gaps - the issue stall moves into the phases and grows: phase 1 732 -> 982 cycles, phase 2 330 -> 488 per half-step
    // for 250 saved: 1024 vs 1055 TFLOP/s, profiles/r05_prefill.txt.  A burst outside the phases is the cheapest place.)
    auto half_step = [&](auto hqc, v16f &C, v16f &N, const int h) {
        constexpr int HQ = decltype(hqc)::value, HN = (HQ + 1) & 3, BUFV = HQ >> 1, JT = HQ & 1;
        const bool nxt_live = live(h + 1);

        if (cur_live) {      // a wave's last live half runs the same code: the scores of the half behind it are masked whole
            float ls = 0.f, mx = -INFINITY;
            unsigned pw8[8];
            // phase 1: score products of half h + 1 (operands three k-steps ahead) | exponentials of half h; its last three gaps
            // also request the first three value operands of phase 2
            v8h af[3] = {PF_KFRAG(HN, 0), PF_KFRAG(HN, 1), PF_KFRAG(HN, 2)};
            pv4s lo[3], hi[3];
#pragma unroll
            for (int s = 0; s < DS; ++s) {
#if MILLION_EXP & 8
                if (s == 0) N = NEG;      // ablation: no score products (the operand reads stay: kept alive below)
                N[s] += (float)af[s % 3][0];
#else
                if (s == 0) N = __builtin_amdgcn_mfma_f32_32x32x16_f16(af[s % 3], qf[s], NEG, 0, 0, 0);
                else N = __builtin_amdgcn_mfma_f32_32x32x16_f16(af[s % 3], qf[s], N, 0, 0, 0);
#endif
                PF_PIN(N);
                if (s + 3 < DS) af[s % 3] = PF_KFRAG(HN, (s + 3) & 7);
                else { lo[s - 5] = PF_VFRAG(BUFV, JT, 0, 0, (s - 5) & 3); hi[s - 5] = PF_VFRAG(BUFV, JT, 0, 1, (s - 5) & 3); }
#if MILLION_EXP & 256
                const float p0 = C[2 * s] + 1.0f, p1 = C[2 * s + 1] + 1.0f;
#else
                typedef float f2v __attribute__((ext_vector_type(2)));
                const f2v ex = f2v{C[2 * s], C[2 * s + 1]} * cs;      // v_pk_mul_f32; -inf (masked) stays -inf
                const float p0 = __builtin_amdgcn_exp2f(ex[0]), p1 = __builtin_amdgcn_exp2f(ex[1]);
#endif
                ls += p0;
                ls += p1;
                typedef _Float16 h2v __attribute__((ext_vector_type(2)));
                const h2v t2 = {(f16)p0, (f16)p1};
                pw8[s] = __builtin_bit_cast(unsigned, t2);
                asm volatile("" : "+v"(pw8[s]), "+v"(ls));
            }
            PT(1)
            if (!nxt_live || masked(h + 1)) mask_half(h + 1, N);
            PT(2)
            // phase 2: value products of half h (operands three steps ahead) | running maximum of half h + 1's raw scores
#pragma unroll
            for (int i = 0; i < 8; ++i) {
                const int ks = i >> 2, blk = i & 3;
                typedef short v8s __attribute__((ext_vector_type(8)));
                const v8s av = {lo[i % 3][0], lo[i % 3][1], lo[i % 3][2], lo[i % 3][3], hi[i % 3][0], hi[i % 3][1], hi[i % 3][2], hi[i % 3][3]};
                const pv4u pwv = {pw8[4 * ks], pw8[4 * ks + 1], pw8[4 * ks + 2], pw8[4 * ks + 3]};
#if MILLION_EXP & 4
                O[blk][i] += __builtin_bit_cast(float, ((unsigned)(unsigned short)av[0] | pwv[0]) & 1u);      // ablation: no value products
#else
                O[blk] = __builtin_amdgcn_mfma_f32_32x32x16_f16(__builtin_bit_cast(v8h, av), __builtin_bit_cast(v8h, pwv), O[blk], 0, 0, 0);
#endif
                PF_PIN(O[blk]);
                if (i + 3 < 8) { lo[i % 3] = PF_VFRAG(BUFV, JT, ((i + 3) >> 2) & 1, 0, (i + 3) & 3); hi[i % 3] = PF_VFRAG(BUFV, JT, ((i + 3) >> 2) & 1, 1, (i + 3) & 3); }
                asm("v_max3_f32 %0, %1, %2, %3" : "=v"(mx) : "v"(mx), "v"(N[2 * i]), "v"(N[2 * i + 1]));
                PF_PIN(mx);
            }
            PT(3)
            l_run += ls;
            decide(mx, N);
            PT(4)
        }
        cur_live = nxt_live;
    };
    PT(7)
    for (int t = 0; t < nt; t += 2) {
        PF_DMA(t);
        PT(0)
        half_step(std::integral_constant<int, 0>{}, SA, SB, 2 * t);
        half_step(std::integral_constant<int, 1>{}, SB, SA, 2 * t + 1);
        PF_SYNC();
        PT(5)
        if (t + 1 < nt) {
            PF_DMA(t + 1);
            PT(0)
            half_step(std::integral_constant<int, 2>{}, SA, SB, 2 * t + 2);
            half_step(std::integral_constant<int, 3>{}, SB, SA, 2 * t + 3);
            PF_SYNC();
            PT(5)
        }
    }
#if MILLION_EXP & 2048
    if (blockIdx.x == 0 && lane < 8) {      // into this wave's own first query row (read into registers long ago; nobody else reads it)
        unsigned *dst = (unsigned *)(p.q + w.b * p.q_sb + w.head * p.q_sh + (long long)w.q_lo * p.q_sn);
        unsigned v_ = pt_acc[0];
#pragma unroll
        for (int i = 1; i < 8; ++i) v_ = lane == i ? pt_acc[i] : v_;
        dst[lane] = v_;
    }
#endif
#undef PT
#undef PF_DMA
#undef PF_SYNC
#undef PF_KFRAG
#undef PF_VFRAG
    l_run = flash_l_total(l_run);
    if (wave_live && w.q_row < n_q) {
        flash_store_row(O, l_run, p.out + w.b * p.o_sb + w.head * p.o_sh + (long long)w.q_row * p.o_sn, hh);
        // the lazy reference: every probability of l_run is exp2(cs (s + neg_ref)) with the neg_ref in force now - decide() moved
        // l_run along with each earlier one - so the reference is -neg_ref raw (0 while the row has seen no key: l = 0 then),
        // not the row's maximum
        if (LSE) prefill_store_lse(p, w, hh, -neg_ref * cs, l_run, lse);
    } else if (RAGGED) prefill_store_dead<NB, LSE>(p, w, hh, lse);      // rows between the request's n_q and the bound
}
#undef PF_PIN

template <int D, bool RAGGED>
__global__ __launch_bounds__(kWaves * 64, 2) void prefill_attn_kernel(PrefillParams p) { prefill_attn_body<D, RAGGED, false>(p, nullptr); }
template <bool RAGGED>
__global__ __launch_bounds__(kWaves * 64, 2) void prefill_attn_pipe_kernel(PrefillParams p) { prefill_attn_pipe_body<RAGGED, false>(p, nullptr); }
template <int D, bool RAGGED>
__global__ __launch_bounds__(kWaves * 64, 2) void prefill_lse_kernel(PrefillParams p, float *lse) { prefill_attn_body<D, RAGGED, true>(p, lse); }
template <bool RAGGED>
__global__ __launch_bounds__(kWaves * 64, 2) void prefill_lse_pipe_kernel(PrefillParams p, float *lse) { prefill_attn_pipe_body<RAGGED, true>(p, lse); }

template <int D, bool LSE>
static void launch_prefill_t(const PrefillParams &p, float *lse, long long blocks, int lds, hipStream_t s) {
    if (LSE) {
        if (p.dev_spans) hipLaunchKernelGGL((prefill_lse_kernel<D, true>), dim3((unsigned)blocks), dim3(kWaves * 64), lds, s, p, lse);
        else hipLaunchKernelGGL((prefill_lse_kernel<D, false>), dim3((unsigned)blocks), dim3(kWaves * 64), lds, s, p, lse);
    } else if (p.dev_spans) hipLaunchKernelGGL((prefill_attn_kernel<D, true>), dim3((unsigned)blocks), dim3(kWaves * 64), lds, s, p);
    else hipLaunchKernelGGL((prefill_attn_kernel<D, false>), dim3((unsigned)blocks), dim3(kWaves * 64), lds, s, p);
}
template <bool LSE>
static void launch_prefill_pipe(const PrefillParams &p, float *lse, long long blocks, int lds, hipStream_t s) {
    if (LSE) {
        if (p.dev_spans) hipLaunchKernelGGL(prefill_lse_pipe_kernel<true>, dim3((unsigned)blocks), dim3(kWaves * 64), lds, s, p, lse);
        else hipLaunchKernelGGL(prefill_lse_pipe_kernel<false>, dim3((unsigned)blocks), dim3(kWaves * 64), lds, s, p, lse);
    } else if (p.dev_spans) hipLaunchKernelGGL(prefill_attn_pipe_kernel<true>, dim3((unsigned)blocks), dim3(kWaves * 64), lds, s, p);
    else hipLaunchKernelGGL(prefill_attn_pipe_kernel<false>, dim3((unsigned)blocks), dim3(kWaves * 64), lds, s, p);
}
// dynamic-LDS attribute of the three kernels (lockstep and ragged instances, each without and with LSE): once per device, under the library's per-device mutex (common.h: device_once)
static bool g_prefill_plain = false;      // A/B and tests (million_set_force_generic(64)): the plain form at d = 128 too
void set_prefill_policy(bool plain) { g_prefill_plain = plain; }
static void prefill_attrs_once() {
    if (!device_once(3)) return;
    const auto lds_attr = [](const void *kernel, int bytes) { (void)hipFuncSetAttribute(kernel, hipFuncAttributeMaxDynamicSharedMemorySize, bytes); };
    lds_attr((const void *)prefill_attn_pipe_kernel<false>, 4 * kKV * 2 * 128);
    lds_attr((const void *)prefill_attn_pipe_kernel<true>, 4 * kKV * 2 * 128);
    lds_attr((const void *)prefill_attn_kernel<128, false>, 4 * kKV * 2 * 128);
    lds_attr((const void *)prefill_attn_kernel<128, true>, 4 * kKV * 2 * 128);
    lds_attr((const void *)prefill_attn_kernel<64, false>, 4 * kKV * 2 * 64);
    lds_attr((const void *)prefill_attn_kernel<64, true>, 4 * kKV * 2 * 64);
    lds_attr((const void *)prefill_lse_pipe_kernel<false>, 4 * kKV * 2 * 128);
    lds_attr((const void *)prefill_lse_pipe_kernel<true>, 4 * kKV * 2 * 128);
    lds_attr((const void *)prefill_lse_kernel<128, false>, 4 * kKV * 2 * 128);
    lds_attr((const void *)prefill_lse_kernel<128, true>, 4 * kKV * 2 * 128);
    lds_attr((const void *)prefill_lse_kernel<64, false>, 4 * kKV * 2 * 64);
    lds_attr((const void *)prefill_lse_kernel<64, true>, 4 * kKV * 2 * 64);
}

int launch_prefill(const PrefillParams &p_in, float *lse, hipStream_t s) {
    PrefillParams p = p_in;
    int hpw = 1;
    for (int c = kWaves; c >= 1; c >>= 1)
        if (p.G % c == 0) { hpw = c; break; }
    p.hpw = hpw;
    const int QB = (kWaves / hpw) * 32;
    p.n_qb = (p.n_q + QB - 1) / QB;
    const long long blocks = (long long)p.bs * p.nh_k * (p.G / hpw) * p.n_qb;
    if (blocks <= 0) return MILLION_OK;
    if (blocks > 0x7fffffffLL) { set_error("prefill: %lld workgroups", blocks); return MILLION_ERR_SHAPE; }
    const int lds = 4 * kKV * 2 * p.d;      // two buffers of (K tile, V tile)
    prefill_attrs_once();
    if (lse) {
        if (p.d == 128 && !g_prefill_plain) launch_prefill_pipe<true>(p, lse, blocks, lds, s);
        else if (p.d == 128) launch_prefill_t<128, true>(p, lse, blocks, lds, s);
        else launch_prefill_t<64, true>(p, lse, blocks, lds, s);
    } else if (p.d == 128 && !g_prefill_plain) launch_prefill_pipe<false>(p, nullptr, blocks, lds, s);
    else if (p.d == 128) launch_prefill_t<128, false>(p, nullptr, blocks, lds, s);
    else launch_prefill_t<64, false>(p, nullptr, blocks, lds, s);
    const hipError_t e = hipGetLastError();
    if (e != hipSuccess) { set_error("prefill launch: %s", hipGetErrorString(e)); return MILLION_ERR_LAUNCH; }
    return MILLION_OK;
}

}  // namespace million

using namespace million;

// both entries: lse = null is million_prefill_attn (the instances without LSE), anything else million_prefill_attn_lse
static int prefill_entry(const million_prefill_desc *desc, const void *q, const void *k, const void *v, void *out, float *lse,
                         million_stream_t stream) {
    if (!desc || desc->struct_size != sizeof(million_prefill_desc)) { set_error("prefill: bad desc / struct_size"); return MILLION_ERR_ARG; }
    if (!q || !k || !v || !out) { set_error("prefill: null pointer"); return MILLION_ERR_ARG; }
    PrefillParams p;
    p.q = (const f16 *)q; p.k = (const f16 *)k; p.v = (const f16 *)v; p.out = (f16 *)out;
    p.bs = desc->bs; p.nh = desc->nh; p.nh_k = desc->nh_k; p.d = desc->d;
    p.n_q = desc->n_q; p.n_kv = desc->n_kv; p.q_pos0 = desc->q_pos0; p.causal = desc->causal != 0;
    if (p.bs <= 0 || p.nh <= 0 || p.nh_k <= 0 || p.nh % p.nh_k) { set_error("prefill: bs=%d nh=%d nh_k=%d", p.bs, p.nh, p.nh_k); return MILLION_ERR_SHAPE; }
    if (p.d != 128 && p.d != 64) { set_error("prefill: d=%d (64 or 128)", p.d); return MILLION_ERR_SHAPE; }
    if (p.n_q < 0 || p.n_kv < 0 || p.q_pos0 < 0) { set_error("prefill: n_q=%d n_kv=%d q_pos0=%d", p.n_q, p.n_kv, p.q_pos0); return MILLION_ERR_ARG; }
    if (p.n_q == 0) return MILLION_OK;
    if (p.n_kv == 0) { set_error("prefill: no keys (n_kv = 0) for %d query rows", p.n_q); return MILLION_ERR_ARG; }
    p.G = p.nh / p.nh_k;
    p.q_sb = desc->q_stride_b; p.q_sh = desc->q_stride_h; p.q_sn = desc->q_stride_n;
    p.k_sb = desc->k_stride_b; p.k_sh = desc->k_stride_h; p.k_sn = desc->k_stride_n;
    p.v_sb = desc->v_stride_b; p.v_sh = desc->v_stride_h; p.v_sn = desc->v_stride_n;
    p.o_sb = desc->o_stride_b; p.o_sh = desc->o_stride_h; p.o_sn = desc->o_stride_n;
    if (((uintptr_t)q | (uintptr_t)k | (uintptr_t)v | (uintptr_t)out) & 15) { set_error("prefill: every pointer must be 16-byte aligned"); return MILLION_ERR_ALIGN; }
    if ((p.q_sb | p.q_sh | p.q_sn | p.k_sb | p.k_sh | p.k_sn | p.v_sb | p.v_sh | p.v_sn | p.o_sb | p.o_sh | p.o_sn) & 7) {
        set_error("prefill: strides must be multiples of 8 elements (16-byte rows)");
        return MILLION_ERR_ALIGN;
    }
    p.scale_log2e = 1.4426950408889634f / sqrtf((float)p.d);
    p.dev_spans = desc->dev_spans;      // non-null: n_q and n_kv above are the bounds, q_pos0 is not read (validated all the same)
    return launch_prefill(p, lse, (hipStream_t)stream);
}

extern "C" int million_prefill_attn(const million_prefill_desc *desc, const void *q, const void *k, const void *v, void *out,
                                    million_stream_t stream) {
    return prefill_entry(desc, q, k, v, out, nullptr, stream);
}

extern "C" int million_prefill_attn_lse(const million_prefill_desc *desc, const void *q, const void *k, const void *v, void *out,
                                        float *lse, million_stream_t stream) {
    if (!lse) { set_error("prefill: null lse (million_prefill_attn is the entry without it)"); return MILLION_ERR_ARG; }
    if ((uintptr_t)lse & 3) { set_error("prefill: lse must be 4-byte aligned"); return MILLION_ERR_ALIGN; }
    return prefill_entry(desc, q, k, v, out, lse, stream);
}
