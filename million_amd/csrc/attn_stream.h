// attn_stream.h - the streaming decode kernel: 32-token units, 16 x 16 x 32 score tiles, up to 16 query heads per kv head.
// Included by attn_mfma.hip (inside namespace million, behind decode_wave.h and attn_tail.h, in front of attn_lean.h); the design
// notes are in attn_mfma.hip's header.

struct UnitCodes {
    v4u k[2];   // K code bytes: score tile g2, lane (q, c): tile row c, bytes [16q, 16q+16) of that token's code row
                // (row c = token stream_token_of_row(g2, c) of the unit)
    v4u v[2];   // V code bytes: half n (32 subspaces), lane (h, c): m = 32n + c, tokens [16h, 16h+16)
};

// M = 32 (d_m = 4): a token's code row is 32 bytes, a codebook entry 8 bytes (one ds_read_b64)
struct UnitCodes32 {
    v2u k[2];   // K code bytes: score tile g2, lane (q, c): tile row c (see UnitCodes), bytes [8q, 8q+8)
    v4u v[1];   // V code bytes: lane (h, c): subspace m = c, tokens [16h, 16h+16)
};

// M = 16 (d_m = 8, streaming kernel only, round 4): a token's code row is 16 bytes, a codebook entry 16 bytes (one ds_read_b128)
// - the whole A operand of a 16x16x32 k-step on the K side and the whole B operand of one on the V side (see "d_m = 8 form")
struct UnitCodes16 {
    unsigned k[2];   // K code bytes: score tile g2, lane (q, c): tile row c, bytes [4q, 4q+4) = subspaces 4q .. 4q+3 of that token
    unsigned v[2];   // V code bytes: tile g2, lane (t, n): subspace n, tile rows 4t .. 4t+3 (tokens 8t + 4 g2 + 0..3 of the unit)
};
// M = 32 in the d_m = 4 form (streaming kernel, G <= 4, round 4): K bytes as UnitCodes32; V bytes as in UnitCodes16, for the two
// column tiles (subspaces n and n + 16)
struct UnitCodes32D {
    v2u k[2];             // as UnitCodes32
    unsigned v[2][2];     // V code bytes: tile g2, column tile j, lane (t, n): subspace n + 16 j, tile rows 4t .. 4t+3
};

// ---- parity-V (round 4): the value product without the pack -------------------------------------------------------
// A gathered V word is (dim 2m, dim 2m + 1) of ONE token; the value MFMA's operand register wants two reduction indices of one
// column.  Rounds 1-3 re-packed: 8 gathers -> 8 v_perm -> B0 (even dims), B1 (odd dims), two MFMAs, 64 accumulator registers.
// Here the reduction index IS (token, parity of the dim): the gathered word is the B operand as it stands (4 gathers = one
// lane's 8 reduction slots = 4 tokens), and the zero pattern moves to the cheap side - tile row (parity p, head g) holds
// P[g][token] in half p of the register and 0 in the other half, so that
//   D[(p, g)][m] = sum over (token, e) of P[g][token] [e == p] * Vhat[token][2m + e] = O[g][2m + p].
// Per 32-token unit: 32 gathers, 32 address v_perm, 16 placement v_perm, 8 MFMA (one per 8 tokens x 32 subspaces), 32
// accumulator registers - against 32 + 32 + 32 pack + 8 and 64 (tools/micro/core_micro.hip: +12 % units per SIMD and us).
// Tile rows: r = 16 p + g (g < 16 heads); lane (h, r) of the A operand, step s (tokens 16h + 4s + t, t = 0..3): register t.
// The score tiles leave, in lane (q4 = 2h + p', g), the probabilities of tokens 16h + 8p' + x, x = 0..7: W[k] = cvt_pk(x = 2k,
// 2k + 1); swap16_self hands every lane pair (p' = 0, 1) both rows' W (E: tokens 16h + 0..7, F: 16h + 8..15); sel_lo / sel_hi
// (lane constants, by the lane's OWN row parity) move one half of a W into the lane's half of the register.
struct ParA { unsigned E[4], F[4]; };
__device__ __forceinline__ void value_prep_par(const float (&pr)[8], ParA &pa) {
#pragma unroll
    for (int k = 0; k < 4; ++k) {
        h2 t = {(f16)pr[2 * k], (f16)pr[2 * k + 1]};
        const v2u y = swap16_self(__builtin_bit_cast(unsigned, t));
        const unsigned y0 = y[0], y1 = y[1];
        pa.E[k] = y0;
        pa.F[k] = y1;
    }
}
// A operand of token step s (0..3)
__device__ __forceinline__ v8f16 value_A_par(const ParA &pa, int s, unsigned sel_lo, unsigned sel_hi) {
    const unsigned w0 = s < 2 ? pa.E[2 * (s & 1)] : pa.F[2 * (s & 1)], w1 = s < 2 ? pa.E[2 * (s & 1) + 1] : pa.F[2 * (s & 1) + 1];
    return as_v8f16(__builtin_amdgcn_perm(0u, w0, sel_lo), __builtin_amdgcn_perm(0u, w0, sel_hi),
                    __builtin_amdgcn_perm(0u, w1, sel_lo), __builtin_amdgcn_perm(0u, w1, sel_hi));
}
__device__ __forceinline__ void par_selectors(int lane, unsigned &sel_lo, unsigned &sel_hi) {
    const bool odd = (lane >> 4) & 1;      // v_perm selectors: bytes 0-3 = the W register, 0x0c = zero
    sel_lo = odd ? 0x01000c0cu : 0x0c0c0100u;
    sel_hi = odd ? 0x03020c0cu : 0x0c0c0302u;
}
// the 4 gathers of value step (token step s, subspace half n): tokens 16h + 4s + t of subspace 32n + c32
__device__ __forceinline__ void v_gather_par(const v4u (&vc)[2], int s, int n, unsigned vconst0, unsigned vconst1, unsigned (&e)[4]) {
    const unsigned vconst = n ? vconst1 : vconst0;
    const unsigned w = vc[n][s];
    e[0] = lds32(__builtin_amdgcn_perm(w, vconst, 0x03020400u));
    e[1] = lds32(__builtin_amdgcn_perm(w, vconst, 0x03020500u));
    e[2] = lds32(__builtin_amdgcn_perm(w, vconst, 0x03020600u));
    e[3] = lds32(__builtin_amdgcn_perm(w, vconst, 0x03020700u));
}

// d_m = 8 form (decode_wave.h): the value step of the d_m = 4 form (d4_vstep) on the two 8-byte HALVES of a 16-byte entry (row tile
// h = dims 4 h .. 4 h + 3 of the entry): vconst = V col image base | 16 n, the halves 8 bytes apart
__device__ __forceinline__ void d8_vgather(const unsigned (&vc)[2], int i, unsigned vconst, unsigned (&e)[8]) {
    const unsigned sel[4] = {0x03020400u, 0x03020500u, 0x03020600u, 0x03020700u};
    const int g2 = i >> 1, s = i & 1;
    const unsigned w = vc[g2];
#pragma unroll
    for (int h = 0; h < 2; ++h) {
        const v2u x0 = lds64(__builtin_amdgcn_perm(w, vconst + 8u * h, sel[2 * s]));
        const v2u x1 = lds64(__builtin_amdgcn_perm(w, vconst + 8u * h, sel[2 * s + 1]));
        e[4 * h + 0] = x0[0]; e[4 * h + 1] = x0[1]; e[4 * h + 2] = x1[0]; e[4 * h + 3] = x1[1];
    }
}
// the 4 gathers of value step i = (tile g2 = i >> 1, k-step s = i & 1): bytes 2 s, 2 s + 1 of the lane's code words of the tile;
// vconst_j = V col image base | 8 (n + 16 j) (entries of 8 bytes, 256 bytes per code)
__device__ __forceinline__ void d4_vgather(const unsigned (&vc)[2][2], int i, unsigned vconst0, unsigned vconst1, unsigned (&e)[8]) {
    const unsigned sel[4] = {0x03020400u, 0x03020500u, 0x03020600u, 0x03020700u};
    const int g2 = i >> 1, s = i & 1;
#pragma unroll
    for (int j = 0; j < 2; ++j) {
        const unsigned w = vc[g2][j], vconst = j ? vconst1 : vconst0;
        const v2u x0 = lds64(__builtin_amdgcn_perm(w, vconst, sel[2 * s]));
        const v2u x1 = lds64(__builtin_amdgcn_perm(w, vconst, sel[2 * s + 1]));
        e[4 * j + 0] = x0[0]; e[4 * j + 1] = x0[1]; e[4 * j + 2] = x1[0]; e[4 * j + 3] = x1[1];
    }
}

// ---- value side of a 32-token unit in pieces, for the pipelined kernel ---------------------------------
// The A operand of the value MFMA (rows = heads, K = 16 tokens) wants, in lane (h, head), the probabilities of tokens
// 16h + 8s + j (token step s, j = 0..7).  The score MFMAs leave pr[4*g2 + rho] = row 4q' + rho of score tile g2 in lane
// (q', head), and WHICH token a tile row is, is the K gather's choice.  With tile g2, row i = token 8*(i >> 2) + 4*g2 +
// (i & 3) (stream_token_of_row), lane rows 0 and 2 - the lanes the value MFMA reads for h = 0 / 1 - already hold the
// eight tokens of step s = 0 in operand order: value_prep is four cvt_pk and nothing else.  Step s = 1 wants what lane
// rows 1 and 3 hold; value_next_step brings it over IN PLACE with four v_permlane16_swap, once the s = 0 steps have
// issued.  (Round 1-2 form: tiles of 16 consecutive tokens, 2 permlane32_swap + 4 copies + 4 permlane16_swap per unit.)
__device__ __forceinline__ int stream_token_of_row(int g2, int i) { return 8 * (i >> 2) + 4 * g2 + (i & 3); }
__device__ __forceinline__ void value_prep(const float (&pr)[8], unsigned (&P)[4]) {
#pragma unroll
    for (int g2 = 0; g2 < 2; ++g2)
#pragma unroll
        for (int i = 0; i < 2; ++i) {
            h2 t = {(f16)pr[g2 * 4 + 2 * i], (f16)pr[g2 * 4 + 2 * i + 1]};
            P[2 * g2 + i] = __builtin_bit_cast(unsigned, t);
        }
}
// P (token step 0) -> P (token step 1): lane rows 0 / 2 receive what lane rows 1 / 3 held.  v_permlane16_swap(a, b)
// returns {a with its odd rows replaced by b's even rows, b with its even rows replaced by a's odd rows}.
__device__ __forceinline__ void value_next_step(unsigned (&P)[4]) {
#pragma unroll
    for (int g2 = 0; g2 < 2; ++g2) {
        const v2u t = __builtin_amdgcn_permlane16_swap(P[2 * g2], P[2 * g2 + 1], false, false);
        const unsigned v = t[0], s = t[1];      // s rows 0 / 2 = P[2 g2] rows 1 / 3;  s rows 1 / 3 = P[2 g2 + 1] rows 1 / 3
        const v2u u = __builtin_amdgcn_permlane16_swap(s, v, false, false);
        const unsigned u0 = u[0], u1 = u[1];
        P[2 * g2] = u0;                         // rows 0 / 2 = s rows 0 / 2 (kept)
        P[2 * g2 + 1] = u1;                     // rows 0 / 2 = s rows 1 / 3
    }
}
// the 8 centroid gathers of value step st = 2n + s (subspaces 32n.., tokens 16h + 8s + j)
__device__ __forceinline__ void v_gather(const v4u (&vc)[2], int st, unsigned vconst0, unsigned vconst1, unsigned (&e)[8]) {
    const unsigned vconst = (st >> 1) ? vconst1 : vconst0;
    const unsigned w0 = vc[st >> 1][2 * (st & 1)], w1 = vc[st >> 1][2 * (st & 1) + 1];
    e[0] = lds32(__builtin_amdgcn_perm(w0, vconst, 0x03020400u));
    e[1] = lds32(__builtin_amdgcn_perm(w0, vconst, 0x03020500u));
    e[2] = lds32(__builtin_amdgcn_perm(w0, vconst, 0x03020600u));
    e[3] = lds32(__builtin_amdgcn_perm(w0, vconst, 0x03020700u));
    e[4] = lds32(__builtin_amdgcn_perm(w1, vconst, 0x03020400u));
    e[5] = lds32(__builtin_amdgcn_perm(w1, vconst, 0x03020500u));
    e[6] = lds32(__builtin_amdgcn_perm(w1, vconst, 0x03020600u));
    e[7] = lds32(__builtin_amdgcn_perm(w1, vconst, 0x03020700u));
}
// pack the gathered centroids (even dims -> B0, odd dims -> B1) and accumulate
__device__ __forceinline__ void v_step(const unsigned (&e)[8], const unsigned (&Ps)[4], v16f32 (&On)[2]) {
    const v8f16 B0 = as_v8f16(__builtin_amdgcn_perm(e[1], e[0], 0x05040100u), __builtin_amdgcn_perm(e[3], e[2], 0x05040100u),
                              __builtin_amdgcn_perm(e[5], e[4], 0x05040100u), __builtin_amdgcn_perm(e[7], e[6], 0x05040100u));
    const v8f16 B1 = as_v8f16(__builtin_amdgcn_perm(e[1], e[0], 0x07060302u), __builtin_amdgcn_perm(e[3], e[2], 0x07060302u),
                              __builtin_amdgcn_perm(e[5], e[4], 0x07060302u), __builtin_amdgcn_perm(e[7], e[6], 0x07060302u));
    const v8f16 A = as_v8f16(Ps[0], Ps[1], Ps[2], Ps[3]);
    On[0] = __builtin_amdgcn_mfma_f32_32x32x16_f16(A, B0, On[0], 0, 0, 0);
    On[1] = __builtin_amdgcn_mfma_f32_32x32x16_f16(A, B1, On[1], 0, 0, 0);
}

// =====================================================================================================
// Streaming kernel: the pipelined schedule for ANY split length, M = 64, M = 32 and (up to 4 query heads per kv head) M = 16.
//
// A score pass is LDS-bound (~7 LDS cycles per random K gather), a value pass issue-bound (v_perm address + pack work and
// the 32x32x16 MFMAs); run one after the other, with one workgroup per CU, nothing else fills the idle pipe.  In the
// pipelined schedule both codebooks are in LDS before the loop, the softmax is online PER UNIT (decode_wave.h:
// softmax_online_raw), and the value steps of unit u are interleaved instruction by instruction with the score stages of
// unit u + 1, so the LDS pipe and the vector/matrix issue work at the same time.
//
// What changed against round 1's 4-unit pipelined kernel (which it replaced):
//   * units are dealt to (split, wave) by PAGE and the page ids of a wave's first 64 rounds are one vector load: the launch
//     front, attn_front.h (with the layout modes MODE 0 / 1 / 2);
//   * the block "values of unit j | scores of unit j + 1" repeats for as many units as the wave has: whole rounds of
//     four units run in a loop (ring slot = unit & 3, the slot of unit j refilled with unit j + 4 right behind it, never
//     in a conditional: rounds past the last unit re-read it), the up to three units beyond the whole rounds run one by
//     one from the ring slots the last round refilled.  (hipcc keeps the loop at ~235 VGPRs only as long as no branch
//     leaves it with the pipeline state live: early exits, a switch over the slot, or a remainder chain of blocks each
//     spilled hundreds of registers; a self-contained unit behind a branch does not.)
// =====================================================================================================
template <int MS> struct StreamTypes;
template <> struct StreamTypes<64> { typedef UnitCodes Unit; typedef unsigned E[8]; };
template <> struct StreamTypes<32> { typedef UnitCodes32 Unit; typedef unsigned E[2][8]; };
template <> struct StreamTypes<16> { typedef UnitCodes16 Unit; typedef unsigned E[8]; };
template <> struct StreamTypes<320> { typedef UnitCodes32D Unit; typedef unsigned E[8]; };      // M = 32, d_m = 4 form

// the K gathers of score stage st (0..7) of a unit; CL2 = log2 of the centroids per subspace (8: C = 256, 7: C = 128):
// a subspace's row of the K row image is (4 << CL2) bytes at M = 64 and (8 << CL2) at M = 32, a stage covers 16 << CL2
template <int CL2>
__device__ __forceinline__ void st_kgather(const UnitCodes &u, int st, unsigned kbase, unsigned (&a)[4]) {
    const unsigned w = u.k[st >> 2][st & 3], base = kbase + (st & 3) * (16u << CL2);
    a[0] = lds32(base + 0 * (4u << CL2) + ((w & 0xffu) << 2));
    a[1] = lds32(base + 1 * (4u << CL2) + (((w >> 8) & 0xffu) << 2));
    a[2] = lds32(base + 2 * (4u << CL2) + (((w >> 16) & 0xffu) << 2));
    a[3] = lds32(base + 3 * (4u << CL2) + ((w >> 24) << 2));
}
template <int CL2>
__device__ __forceinline__ void st_kgather(const UnitCodes32 &u, int st, unsigned kbase, unsigned (&a)[4]) {
    const unsigned w = u.k[st >> 2][(st & 3) >> 1], base = kbase + (st & 3) * (16u << CL2);
    const unsigned sh = 16 * (st & 1);
    const v2u lo = lds64(base + 0 * (8u << CL2) + (((w >> sh) & 0xffu) << 3));
    const v2u hi = lds64(base + 1 * (8u << CL2) + (((w >> (sh + 8)) & 0xffu) << 3));
    a[0] = lo[0]; a[1] = lo[1]; a[2] = hi[0]; a[3] = hi[1];
}
template <int CL2>
__device__ __forceinline__ void st_kgather(const UnitCodes32D &u, int st, unsigned kbase, unsigned (&a)[4]) {      // as UnitCodes32
    const unsigned w = u.k[st >> 2][(st & 3) >> 1], base = kbase + (st & 3) * (16u << CL2);
    const unsigned sh = 16 * (st & 1);
    const v2u lo = lds64(base + 0 * (8u << CL2) + (((w >> sh) & 0xffu) << 3));
    const v2u hi = lds64(base + 1 * (8u << CL2) + (((w >> (sh + 8)) & 0xffu) << 3));
    a[0] = lo[0]; a[1] = lo[1]; a[2] = hi[0]; a[3] = hi[1];
}
// M = 16: stage st = (tile st >> 2, k-step st & 3): lane quarter q4 covers subspace 4 q4 + (st & 3) - byte (st & 3) of its code
// word - whose 16-byte entry (8 dims) IS the lane's half-row of the A operand; kbase = 4 q4 subspace rows as for the others
template <int CL2>
__device__ __forceinline__ void st_kgather(const UnitCodes16 &u, int st, unsigned kbase, unsigned (&a)[4]) {
    const unsigned code = (u.k[st >> 2] >> (8 * (st & 3))) & 0xffu;
    const v4u x = lds128(kbase + (st & 3) * (16u << CL2) + (code << 4));
    a[0] = x[0]; a[1] = x[1]; a[2] = x[2]; a[3] = x[3];
}
// the V gathers of value step i (M = 64: 4 steps of 8 four-byte gathers; M = 32: 2 steps of 8 eight-byte gathers)
__device__ __forceinline__ void st_vgather(const UnitCodes &u, int i, unsigned vconst0, unsigned vconst1, unsigned (&e)[8]) {
    v_gather(u.v, i, vconst0, vconst1, e);
}
__device__ __forceinline__ void st_vgather(const UnitCodes32 &u, int i, unsigned vconst0, unsigned, unsigned (&e)[2][8]) {
    const unsigned w0 = u.v[0][2 * i], w1 = u.v[0][2 * i + 1];
    const unsigned sel[4] = {0x03020400u, 0x03020500u, 0x03020600u, 0x03020700u};
#pragma unroll
    for (int j = 0; j < 8; ++j) {
        const v2u t = lds64(__builtin_amdgcn_perm(j < 4 ? w0 : w1, vconst0, sel[j & 3]));
        e[0][j] = t[0];
        e[1][j] = t[1];
    }
}
// value step i: pack the gathered centroids and accumulate
__device__ __forceinline__ void st_vstep(const unsigned (&e)[8], const unsigned (&Ps)[4], int i, v16f32 (&O)[2][2]) {
    v_step(e, Ps, O[i >> 1]);
}
__device__ __forceinline__ void st_vstep(const unsigned (&e)[2][8], const unsigned (&Ps)[4], int, v16f32 (&O)[2][2]) {
    v_step(e[0], Ps, O[0]);      // dims 4m + 0, 1
    v_step(e[1], Ps, O[1]);      // dims 4m + 2, 3
}

template <int MSX, int MODE, int CL2 = 8, bool LSE = false>      // MSX = M, or 320 = M 32 in the d_m = 4 form; LSE: common.h, "Log-sum-exp"
__global__ __launch_bounds__(kNW * 64, 2) void attn_stream_kernel(AttnParams p) {
    constexpr int MS = MSX == 320 ? 32 : MSX;
    constexpr bool D4 = MSX == 320;            // M = 32, d_m = 4 form (see "d_m = 4 form", decode_wave.h): G <= 4, replicated query heads
    typedef typename StreamTypes<MSX>::Unit Unit;
    typedef typename StreamTypes<MSX>::E EBuf;
    constexpr int kLog2M = MS == 64 ? 6 : MS == 32 ? 5 : 4;
    constexpr bool PV = MS == 64;              // parity-V value product (see "parity-V" above); M = 32 keeps the packed form
    constexpr bool D8 = MS == 16;              // d_m = 8 form (see "d_m = 8 form", decode_wave.h): G <= 4, query heads replicated over the column groups
    constexpr int NV = PV ? 8 : (D8 || D4) ? 4 : 2;      // value steps per unit (PV: token step s = i >> 1, subspace half n = i & 1; D8 / D4: tile i >> 1,
                                               // k-step i & 1)
    constexpr int SPV = 8 / NV;                // score stages that ride along with one value step
    constexpr int VD = PV ? 2 : 1;     // value steps the V gathers run ahead of their MFMA (a parity-V step is 4 gathers +
                                               // 1 MFMA, ~100 cycles of issue: one step ahead does not cover an LDS round trip)
    constexpr int NT = 8 >> (8 - CL2);         // 16-byte pieces of a codebook image per thread (C = 256: 64 KiB, C = 128: 32)
    extern __shared__ __attribute__((aligned(16))) char smem[];
    MILLION_DEBUG_FILL_LDS(smem, p.lds_fill);
    const int tid = threadIdx.x;
    const int lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    // ---- the launch front (attn_front.h): units of 32 tokens, rows of 128; only the d_m = 8 form runs as query-head parts:
    //      the other instances do not carry the code ----
    LAUNCH_FRONT_PLACE(MODE, MSX == 16)
    if ((unsigned)(size_t)(__attribute__((address_space(3))) char *)smem != 0u) __builtin_trap();
    const bool dbg_on = p.dbg != nullptr;
#define STAMP(i) stamp_lds(dbg_on, lane, wave, i)
    stamp_lds_clear(dbg_on, lane, wave);
    STAMP(0);
    const int q4 = lane >> 4, c16 = lane & 15;
    LAUNCH_FRONT_PAGE_IDS(5)
    v8f16 qb[4];
    {
        const int hq = (D8 || D4) ? (c16 & 3) : c16;      // D8: column 4 dq + g holds head g (four copies of every head)
        const f16 *qv = p.q + ((long long)b * p.nh + head0(p, hk) + (hq < G ? hq : 0)) * 128 + 32 * q4;
#pragma unroll
        for (int s = 0; s < 4; ++s) {
            v4u t = *(const v4u *)(qv + 8 * s);
            if (hq >= G) t = v4u{0, 0, 0, 0};
            qb[s] = __builtin_bit_cast(v8f16, t);
        }
    }
    LAUNCH_FRONT_NEW_ROW_AND_TABLES(128, NT)
    LAUNCH_FRONT_LENGTHS()
    ResTile rt;
    if (has_res) load_res_tile<MSX>(p, bhr, kr, vr, wave, rcnt, split, rstart, r_old, lane, rt);

    // ---- one unit's 16-byte requests into ring slot SL; J is wave-uniform ----
    Unit ring[kRing];
    typedef const __attribute__((address_space(1))) unsigned *gptr_u32;
    typedef typename std::conditional<D8 || D4, gptr_u32, gptr_v4u>::type VPtr;
    typedef typename std::conditional<MS == 64, gptr_v4u, typename std::conditional<MS == 32, gptr_v2u, gptr_u32>::type>::type KPtr;      // global address space: no FLAT loads
    const int krow0 = stream_token_of_row(0, c16);                                      // token of tile row c16 (tile 1: + 4)
    const unsigned k_lane_off = ((unsigned)krow0 << kLog2M) + (unsigned)(MS / 4) * q4;  // that token's code row, quarter q4
    const unsigned v_lane_off = (D8 || D4) ? ((unsigned)(lane & 15) << p.ps_shift) + 8u * (lane >> 4)     // subspace row n, tile rows 4 t ..: tokens 8 t + 4 g2 + 0..3
                                   : ((unsigned)(lane & 31) << p.ps_shift) + 16u * (lane >> 5);   // subspace row, 16-token half
#define UNIT_REQ_K(SL, J)                                                                                          \
    {                                                                                                              \
        const int jc_ = LAUNCH_FRONT_ROUND(J);                                                                     \
        gptr_u8 kb_;                                                                                               \
        if (k_paged) {                                                                                             \
            const long long pk_ = (long long)__builtin_amdgcn_readlane(vpk, jc_);                                  \
            kb_ = uniform_ptr(p.k_codes + (((pk_ << p.ps_shift) + tin) << kLog2M));                                \
            _Pragma("unroll") for (int g2 = 0; g2 < 2; ++g2)                                                       \
                ring[SL].k[g2] = *(KPtr)(kb_ + k_lane_off + ((4u * g2) << kLog2M));                                \
        } else {      /* row-major K: absolute row per lane, rows past T - 1 re-read it (masked later) */          \
            const int tu_ = t0 + jc_ * t_step;                                                                     \
            kb_ = uniform_ptr(p.k_codes + b * p.k_sb + hkr * p.k_sh);                                              \
            _Pragma("unroll") for (int g2 = 0; g2 < 2; ++g2)                                                       \
                ring[SL].k[g2] = *(KPtr)(kb_ + (((unsigned)min(tu_ + krow0 + 4 * g2, T_ld - 1) << kLog2M) +        \
                                                (unsigned)(MS / 4) * q4));                                         \
        }                                                                                                          \
    }
#define UNIT_REQ_V(SL, J)                                                                                          \
    {                                                                                                              \
        const int jc_ = LAUNCH_FRONT_ROUND(J);                                                                     \
        const long long pv_ = (long long)__builtin_amdgcn_readlane(vpv, jc_);                                      \
        const gptr_u8 vb_ = uniform_ptr(p.v_codes + (pv_ << (kLog2M + p.ps_shift)) + tin);                         \
        if constexpr (D8) {      /* the two tiles' rows of a lane are 8 consecutive token bytes: one 8-byte load */  \
            const v2u w_ = *(gptr_v2u)(vb_ + v_lane_off);                                                          \
            ring[SL].v[0] = w_[0];                                                                                 \
            ring[SL].v[1] = w_[1];                                                                                 \
        } else if constexpr (D4) {                                                                                 \
            _Pragma("unroll") for (int j_ = 0; j_ < 2; ++j_) {                                                     \
                const v2u w_ = *(gptr_v2u)(vb_ + v_lane_off + ((16u * j_) << p.ps_shift));                         \
                ring[SL].v[0][j_] = w_[0];                                                                         \
                ring[SL].v[1][j_] = w_[1];                                                                         \
            }                                                                                                      \
        } else {                                                                                                   \
            ring[SL].v[0] = *(VPtr)(vb_ + v_lane_off);                                                             \
            if (MS == 64) ring[SL].v[MS == 64 ? 1 : 0] = *(VPtr)(vb_ + v_lane_off + (32u << p.ps_shift));          \
        }                                                                                                          \
    }
#define UNIT_REQ(SL, J) { UNIT_REQ_K(SL, J) UNIT_REQ_V(SL, J) }
    UNIT_REQ(0, 0)
    UNIT_REQ(1, 1)
    // (Round 3, tools/ab_build.py: units 2 and 3 requested here too - all four ring slots up front - 19.5 us instead of 16.8 at
    // one request, 25.2 vs 24.0 at two; right behind the codebook barrier: 18.1 / 23.9.  The CU's request queue is in order:
    // what is asked for before the codebooks are in LDS delays the barrier every wave waits at.  Also without effect (+-0.15 us
    // at 1 and 2 requests and at 128K): the query rows through LDS (one request instead of 32 per workgroup), the V bytes of
    // units 0-1 requested behind the barrier, s_setprio 1 for waves 4-7 over the last one, two or three blocks.)
    STAMP(7);
    {
        v4u *ld = (v4u *)smem;
        v4u *ldv = (v4u *)(smem + kVBase);
#pragma unroll
        for (int i = 0; i < NT; ++i) ld[((i + rot) & (NT - 1)) * (kNW * 64) + tid] = tabk[i];
#pragma unroll
        for (int i = 0; i < NT; ++i) ldv[((i + rot) & (NT - 1)) * (kNW * 64) + tid] = tabv[i];
        if constexpr (CL2 == 7) {      // C = 128: the V col image once more (attn_front.h: kVDup128)
#pragma unroll
            for (int i = 0; i < NT; ++i) ldv[((i + rot) & (NT - 1)) * (kNW * 64) + tid + kVDup128 / 16] = tabv[i];
        }
    }
    STAMP(8);
    __syncthreads();
    STAMP(1);

    float m_run = -INFINITY, l_run = 0.f;
    // parity-V: one 32 x 32 tile per subspace half; d_m = 8 form: two 16 x 16 row tiles
    typename std::conditional<D8 || D4, Acc8, v16f32[2][PV ? 1 : 2]>::type O;
    if constexpr (D8 || D4) {
        O.t[0] = v4f32{0.f, 0.f, 0.f, 0.f};
        O.t[1] = v4f32{0.f, 0.f, 0.f, 0.f};
    } else {
#pragma unroll
        for (int n = 0; n < 2; ++n)
#pragma unroll
            for (int kk = 0; kk < (PV ? 1 : 2); ++kk)
#pragma unroll
                for (int i = 0; i < 16; ++i) O[n][kk][i] = 0.f;
    }
    LAUNCH_FRONT_APPEND_STORE(128)
    unsigned sel_lo, sel_hi;      // parity-V: where a probability goes in this lane's A-operand registers
    par_selectors(lane, sel_lo, sel_hi);
    unsigned d8mx, d8my;          // d_m = 8 form: the half of the A-operand registers this lane's rows take their probability in
    d8_masks(lane, d8mx, d8my);
    if (has_res) {      // residual tile of this wave first: it needs neither codebook
        float scr[4];
        score_res_tile(rt, qb, p.scale_log2e, wave, rcnt, lane, scr);
        softmax_online<4, PV>(scr, m_run, l_run, O, G, lane);
        if constexpr (D8 || D4) value_res_tile_d4(rt, scr, d8mx, d8my, O);
        else if constexpr (PV) value_res_tile_par(rt, scr, sel_lo, sel_hi, O);
        else value_res_tile(rt, scr, O);
    }
    STAMP(2);
    const float inv_c = 1.0f / p.scale_log2e;
    SoftRef sr;
    sr.idle = ((D8 || D4) ? (c16 & 3) : c16) < G ? 0.f : -INFINITY;
    sr.set(m_run, l_run, inv_c);

    const unsigned kbase = (unsigned)q4 * (64u << CL2);      // quarter q4 of the K row image: its 16 (M = 64) / 8 (M = 32) subspaces
    const unsigned vconst0 = D4 ? ((unsigned)kVBase | ((unsigned)(lane & 15) << 3))      // V col image base | 8 n (entries of 8 bytes)
                           : D8 ? ((unsigned)kVBase | ((unsigned)(lane & 15) << 4))      // V col image base | 16 n (entries of 16 bytes)
                                : ((unsigned)kVBase | ((unsigned)(lane & 31) << (MS == 64 ? 2 : 3)));
    const unsigned vconst1 = (unsigned)kVBase | ((unsigned)((lane & 31) + 32) << 2);      // M = 64 only

    unsigned a[2][4], P[4];
    EBuf e[2];          // packed form (M = 32)
    unsigned e4[4][4];  // parity-V (M = 64): the gathers of value step i sit in e4[i & 3], two steps ahead of their MFMA
    ParA pa;
    v8f16 Acur;
    float sc[8];
    unsigned e5[2][8];  // d_m = 4 form: the four gathered entries of a value step (two column tiles x two tokens), one step ahead
#if MILLION_EXP & 32
    // development build "the launch without arithmetic" (tools/ab_build.py 32): every request, wait, barrier and the whole tail
    // stay; a unit's bytes are xor-ed into a sink instead of gathered, multiplied and soft-maxed.  What this build takes at a
    // shape is what that shape costs before the first instruction of the attention arithmetic (profiles/r04_launch_floor.txt).
    unsigned sink = 0;
#define SINK_V4(x) sink ^= (x)[0] ^ (x)[1] ^ (x)[2] ^ (x)[3]
#define KG(SL, ST)                                                                                                 \
    do {                                                                                                           \
        if ((ST) == 0) {                                                                                           \
            if constexpr (MS == 64) { SINK_V4(ring[SL].k[0]); SINK_V4(ring[SL].k[1]); }                            \
            else if constexpr (MS == 32) sink ^= ring[SL].k[0][0] ^ ring[SL].k[0][1] ^ ring[SL].k[1][0] ^ ring[SL].k[1][1]; \
            else sink ^= ring[SL].k[0] ^ ring[SL].k[1];                                                            \
        }                                                                                                          \
    } while (0)
#define KM(ST) (void)0
#define VG(SL, I)                                                                                                  \
    do {                                                                                                           \
        if ((I) == 0) {                                                                                            \
            if constexpr (D8) sink ^= ring[SL].v[0] ^ ring[SL].v[1];                                               \
            else if constexpr (D4) sink ^= ring[SL].v[0][0] ^ ring[SL].v[0][1] ^ ring[SL].v[1][0] ^ ring[SL].v[1][1]; \
            else {                                                                                                 \
                SINK_V4(ring[SL].v[0]);                                                                            \
                if constexpr (MS == 64) SINK_V4(ring[SL].v[MS == 64 ? 1 : 0]);                                     \
            }                                                                                                      \
        }                                                                                                          \
    } while (0)
#define VS(I) {}
#define VPREP() {}
#define SCORES_OUT(J) { _Pragma("unroll") for (int i = 0; i < 8; ++i) sc[i] = 0.f; (void)D; }
#define SOFTMAX_RAW() (void)0
#else
#define SOFTMAX_RAW() softmax_online_raw<8, PV>(sc, p.scale_log2e, inv_c, sr, O, G, lane)
#define KG(SL, ST) st_kgather<CL2>(ring[SL], ST, kbase, a[(ST) & 1])
    // (the first k-step of a tile takes a literal zero accumulator - an inline constant of the MFMA - instead of a zeroed D: 8 v_mov
    // per unit less)
#define KM(ST) D[(ST) >> 2] = __builtin_amdgcn_mfma_f32_16x16x32_f16(                                              \
        as_v8f16(a[(ST) & 1][0], a[(ST) & 1][1], a[(ST) & 1][2], a[(ST) & 1][3]), qb[(ST) & 3],                    \
        ((ST) & 3) == 0 ? v4f32{0.f, 0.f, 0.f, 0.f} : D[(ST) >> 2], 0, 0, 0)
    // value steps run token-step major: i -> st = 2n + s with s = i / (NV / 2), so that P serves both s = 0 steps, is
    // moved on in place (value_next_step), and then serves both s = 1 steps
#define VG(SL, I)                                                                                                  \
    do {                                                                                                           \
        if constexpr (D8) d8_vgather(ring[SL].v, (I), vconst0, e5[(I) & 1]);                                       \
        else if constexpr (D4) d4_vgather(ring[SL].v, (I), vconst0, vconst0 + 128u, e5[(I) & 1]);                  \
        else if constexpr (PV) v_gather_par(ring[SL].v, (I) >> 1, (I) & 1, vconst0, vconst1, e4[(I) & 3]);         \
        else st_vgather(ring[SL], (I), vconst0, vconst1, e[(I) & 1]);                                              \
    } while (0)
#define VS(I)                                                                                                      \
    {                                                                                                              \
        if constexpr (D8 || D4) {                                                                                  \
            d4_vstep(sc[2 * (I)], sc[2 * (I) + 1], e5[(I) & 1], d8mx, d8my, O);      /* sc: the unit's probabilities until the next SCORES_OUT */ \
        } else if constexpr (PV) {                                                                                 \
            if (((I) & 1) == 0) Acur = value_A_par(pa, (I) >> 1, sel_lo, sel_hi);                                  \
            O[(I) & 1][0] = __builtin_amdgcn_mfma_f32_32x32x16_f16(                                                \
                Acur, as_v8f16(e4[(I) & 3][0], e4[(I) & 3][1], e4[(I) & 3][2], e4[(I) & 3][3]), O[(I) & 1][0], 0, 0, 0); \
        } else {                                                                                                   \
            if ((I) == NV / 2) value_next_step(P);                                                                 \
            st_vstep(e[(I) & 1], P, (I), O);                                                                       \
        }                                                                                                          \
    }
#define VPREP()                                                                                                    \
    {                                                                                                              \
        if constexpr (D8 || D4) { }                                                                                \
        else if constexpr (PV) value_prep_par(sc, pa);                                                             \
        else value_prep(sc, P);                                                                                    \
    }
    // raw scores of round J out of the accumulators; only the unit that holds token T - 1 (wave-uniform) is masked; a
    // round whose first token is past T - 1 (only the prologue of a wave without whole rounds meets one) gives -inf
#define SCORES_OUT(J)                                                                                              \
    {                                                                                                              \
        const int t_u = t0 + (J) * t_step;                                                                         \
        if (t_u + 32 <= T) {                                                                                       \
            _Pragma("unroll") for (int i = 0; i < 8; ++i) sc[i] = D[i >> 2][i & 3];                                \
        } else {                                                                                                   \
            _Pragma("unroll") for (int i = 0; i < 8; ++i)                                                          \
                sc[i] = t_u + 8 * q4 + 4 * (i >> 2) + (i & 3) < T ? D[i >> 2][i & 3] : -INFINITY;                  \
        }                                                                                                          \
    }
#endif
    // BLOCK: the value steps of the unit in slot U4 (round J) interleaved with the 8 score stages of the unit in slot
    // U4 + 1 (round J + 1); then the first gathers of the next block, the refill of slot U4 with round J + 4 and the
    // online softmax of round J + 1.
#define BLOCK(U4, J)                                                                                               \
    {                                                                                                              \
        v4f32 D[2];                                                                                                \
        UNIT_REQ_K(U4, (J) + 4)      /* the K bytes of slot U4 (round J) were consumed by the previous block */    \
        _Pragma("unroll") for (int i = 0; i < NV; ++i) {                                                           \
            VS(i)                                                                                                  \
            __builtin_amdgcn_sched_barrier(0);                                                                     \
            if (i + VD < NV) VG(U4, i + VD); else VG(((U4) + 1) & 3, i + VD - NV);                                 \
            __builtin_amdgcn_sched_barrier(0);                                                                     \
            _Pragma("unroll") for (int k = 0; k < SPV; ++k) {                                                      \
                KM(SPV * i + k);                                                                                   \
                if (SPV * i + k + 2 < 8) KG(((U4) + 1) & 3, SPV * i + k + 2);                                      \
                else KG(((U4) + 2) & 3, SPV * i + k + 2 - 8);                                                      \
                __builtin_amdgcn_sched_barrier(0);                                                                 \
            }                                                                                                      \
        }                                                                                                          \
        UNIT_REQ_V(U4, (J) + 4)                                                                                    \
        SCORES_OUT((J) + 1)                                                                                        \
        SOFTMAX_RAW();                                                                                             \
        VPREP()                                                                                                    \
    }
#define VALUE_ALONE(U4)                                                                                            \
    _Pragma("unroll") for (int i = 0; i < NV; ++i) {                                                               \
        if (i + VD < NV) VG(U4, i + VD);                                                                           \
        VS(i)                                                                                                      \
    }
    // One unit on its own (the up to three units a wave has beyond its whole rounds of four): scores, softmax, values,
    // self-contained, so that the branch around it carries no pipeline state.
#define SINGLE(SL, J)                                                                                              \
    {                                                                                                              \
        v4f32 D[2];                                                                                                \
        KG(SL, 0);                                                                                                 \
        KG(SL, 1);                                                                                                 \
        _Pragma("unroll") for (int st = 0; st < 8; ++st) {                                                         \
            KM(st);                                                                                                \
            if (st + 2 < 8) KG(SL, st + 2);                                                                        \
        }                                                                                                          \
        SCORES_OUT(J)                                                                                              \
        SOFTMAX_RAW();                                                                                             \
        VPREP()                                                                                                    \
        _Pragma("unroll") for (int k = 0; k < VD; ++k) VG(SL, k);                                                  \
        VALUE_ALONE(SL)                                                                                            \
    }
    const int n_whole = n_mine >> 2, n_rem = n_mine & 3;      // whole rounds of four units + up to three more
    TailReq treq;
    treq.idx = 0; treq.gen = 0; treq.cen = 0; treq.base = 0; treq.done = false;
    {
        // prologue: the 8 score stages of round 0 (masked out when the wave has no whole round: its units are all
        // handled as single units below); round 2 is requested in between
        {
            v4f32 D[2];
            KG(0, 0);
            KG(0, 1);
            tail_mark_xcd(p, bh, split, wave, lane);      // this split's slot of the XCD census (see there for the placement)
#pragma unroll
            for (int st = 0; st < 8; ++st) {
                KM(st);
                if (st + 2 < 8) KG(0, st + 2);
                if (st == 4) UNIT_REQ(2, 2)
                __builtin_amdgcn_sched_barrier(0);
            }
            SCORES_OUT(0)
            if (n_whole == 0) {
#pragma unroll
                for (int i = 0; i < 8; ++i) sc[i] = -INFINITY;
            }
        }
        SOFTMAX_RAW();
        VPREP()
        STAMP(16);
        UNIT_REQ(3, 3)
        if (n_whole > 0) {
#pragma unroll
            for (int k = 0; k < VD; ++k) VG(0, k);
            KG(1, 0);
            KG(1, 1);
            // The first round's three blocks, then the loop ROTATED by three (round 4): the path of a wave with ONE whole round
            // (the headline shape at one request) joins the loop's exit with only ring slot 3 and the softmax state live.  With
            // the loop in front of these three blocks (rounds 2-3) the whole ring was live across it on that path, and the
            // parity-V build spilled 53 registers around the loop - scratch, which alone cost ~9 us per launch.
            BLOCK(0, 0)
            BLOCK(1, 1)
            BLOCK(2, 2)
            int j = 3;
            for (int w = 1; w < n_whole; ++w) {
                BLOCK(3, j)
                ++j;
                BLOCK(0, j)
                ++j;
                BLOCK(1, j)
                ++j;
                BLOCK(2, j)
                ++j;
                if (w == 1) STAMP(17);
            }
            tail_request(p, bh, p.nslots, wave, lane, treq);      // ~3 us ahead of the point where the tail needs the answers
            STAMP(19);
            VALUE_ALONE(3)
        }
        // the units beyond the whole rounds sit in ring slots 0..2 (requested by the last round's refills, or up front)
        if (n_rem > 0) SINGLE(0, 4 * n_whole)
        if (n_rem > 1) SINGLE(1, 4 * n_whole + 1)
        if (n_rem > 2) SINGLE(2, 4 * n_whole + 2)
    }
#undef SINGLE
#undef KG
#undef KM
#undef VG
#undef VS
#undef VPREP
#undef SCORES_OUT
#undef SOFTMAX_RAW
#undef BLOCK
#undef VALUE_ALONE
#undef UNIT_REQ
#undef UNIT_REQ_K
#undef UNIT_REQ_V
#if MILLION_EXP & 32
    if (sink == 0x9e3779b9u) sr.l += 1.f;      // never: keeps the sink (and the loads behind it) alive
#endif
    STAMP(3);
    merge_and_publish<MSX, PV, 128, LSE>(p, smem, b, hk, split, G, tid, lane, wave, dbg_on, O, sr.m, sr.l, treq);
#undef STAMP
}
