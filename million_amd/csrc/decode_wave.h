// decode_wave.h - what a wave of the decode MFMA kernels works with, whichever kernel it runs: vector types, LDS reads by absolute
// address, diagnostic stamps, DPP / row reductions, the online softmax, the small-accumulator forms (d_m = 8 / 4) and the
// residual-window tile.  Included by attn_mfma.hip (inside namespace million, in front of attn_tail.h, attn_stream.h and
// attn_lean.h): both kernels and the split-merge tail use it; what only one kernel uses lives with that kernel.

typedef _Float16 v8f16 __attribute__((ext_vector_type(8)));
typedef _Float16 h2 __attribute__((ext_vector_type(2)));
typedef _Float16 v4f16_t __attribute__((ext_vector_type(4)));
typedef float v4f32 __attribute__((ext_vector_type(4)));
typedef float v16f32 __attribute__((ext_vector_type(16)));
typedef unsigned v2u __attribute__((ext_vector_type(2)));
typedef unsigned v4u __attribute__((ext_vector_type(4)));

// accumulators of the d_m = 8 form: row tile h (dim position 4h + dq), lane (dq = lane >> 4, n = lane & 15): register i = head i,
// dims 8n + 4h + dq
// (d_m = 4 form: column tile j, lane (dq, n): register i = head i, dims 4 (n + 16 j) + dq)
struct Acc8 { float __attribute__((ext_vector_type(4))) t[2]; };

// LDS by absolute byte address: the dynamic LDS segment of this kernel starts at 0 (no static LDS; the
// kernel traps otherwise), so a lookup address needs no base add.
__device__ __forceinline__ unsigned lds32(unsigned addr) {
    return *(const __attribute__((address_space(3))) unsigned *)(size_t)addr;
}
__device__ __forceinline__ v2u lds64(unsigned addr) {
    return *(const __attribute__((address_space(3))) v2u *)(size_t)addr;
}
__device__ __forceinline__ v4u lds128(unsigned addr) {
    return *(const __attribute__((address_space(3))) v4u *)(size_t)addr;
}
// Diagnostic stamps go to LDS (lane 0 of each wave) and are copied out at the very end of the kernel: a global
// store per stamp would put a vmcnt(0) into the phases being timed (and a generic-pointer store a FLAT op,
// which makes hipcc wait vmcnt(0) on the non-diagnostic path too).
__device__ __forceinline__ void stamp_lds(bool on, int lane, int wave, int i) {
    if (on && lane == 0)
        *(volatile __attribute__((address_space(3))) unsigned long long *)(size_t)(kStampOff + (wave * kStampSlots + i) * 8) =
            __builtin_amdgcn_s_memrealtime();
}
__device__ __forceinline__ void stamp_lds_clear(bool on, int lane, int wave) {
    if (on && lane < kStampSlots)
        *(volatile __attribute__((address_space(3))) unsigned long long *)(size_t)(kStampOff + (wave * kStampSlots + lane) * 8) = 0ull;
}
__device__ __forceinline__ float fast_exp2(float x) { return __builtin_amdgcn_exp2f(x); }   // v_exp_f32

// Rescale of the value accumulators when a head's softmax reference moves.  alpha of head g sits in lane g; O rows (32x32
// tile, register 4 j + rho): lanes < 32 hold head 8 j + rho, lanes >= 32 head 8 j + 4 + rho; j = 1 only exists for groups
// of more than 8 query heads (wave-uniform branch).  Rows of heads >= G are scaled by whatever their idle column holds:
// they are never read.  One ds_bpermute per register row (no SGPRs: 16 v_readlane results spilled scalar registers in
// the streaming loop).
// PV = parity-V accumulators (streaming kernel, M = 64; see "parity-V", attn_stream.h): only the tiles O[n][0] exist, tile rows are
// (parity of the dim, head): register 4 j + rho of lane (h, col) = row 8 j + 4 h + rho = parity j >> 1, head 8 (j & 1) + 4 h + rho.
template <bool PV = false>
__device__ __forceinline__ void rescale_heads(v16f32 (&O)[2][PV ? 1 : 2], float alpha, int G, int lane) {
    const int sel = lane < 32 ? 0 : 16;
#pragma unroll
    for (int j = 0; j < 2; ++j) {
        if (j == 1 && G <= 8) break;
#pragma unroll
        for (int rho = 0; rho < 4; ++rho) {
            const float f = __builtin_bit_cast(float, __builtin_amdgcn_ds_bpermute(sel + 4 * (8 * j + rho), __builtin_bit_cast(int, alpha)));
#pragma unroll
            for (int n = 0; n < 2; ++n) {
                if (PV) {
                    O[n][0][4 * j + rho] *= f;
                    O[n][0][4 * (j + 2) + rho] *= f;
                } else {
#pragma unroll
                    for (int kk = 0; kk < (PV ? 1 : 2); ++kk) O[n][kk][4 * j + rho] *= f;
                }
            }
        }
    }
}
__device__ __forceinline__ v8f16 as_v8f16(unsigned a, unsigned b, unsigned c, unsigned d) {
    v4u t = {a, b, c, d};
    return __builtin_bit_cast(v8f16, t);
}

// ---- how the vector-memory queue is kept deep without fighting hipcc's waitcnt insertion ------------
// Every code / codebook / q load is a plain load the compiler can count, and NONE of them sits in a
// conditional: slots past a wave's last unit re-request that unit (L2 hits).  The
// pending-load pattern at the loop header is then identical on entry and on the back edge, and hipcc
// emits counted waits (vmcnt(12) before a unit: the three younger units stay in flight).  Versions with
// conditional refills, or with LDS-DMA for the tables, made hipcc wait vmcnt(0) and drained the ring.
//
// A scalar load (the device-resident lengths) is issued and waited for in ONE asm statement on purpose: an earlier
// version split the two to overlap the latency, and hipcc, on an unrelated edit, placed SGPR copies between the two
// statements - copies of values still in flight - which sent wild addresses to the code loads.

// Code loads address a wave-uniform 64-bit base (scalar ALU, forced into SGPRs) plus a 32-bit per-lane offset, so that
// they take the saddr + voffset form: the per-lane 64-bit pointer arithmetic of the obvious formulation was ~10 vector
// instructions per request.
typedef const __attribute__((address_space(1))) uint8_t *gptr_u8;      // global address space: an integer -> pointer
                                                                       // cast would otherwise make FLAT loads
__device__ __forceinline__ gptr_u8 uniform_ptr(const uint8_t *q) {
    const unsigned long long v = (unsigned long long)q;
    const unsigned lo = __builtin_amdgcn_readfirstlane((unsigned)v), hi = __builtin_amdgcn_readfirstlane((unsigned)(v >> 32));
    return (gptr_u8)(((unsigned long long)hi << 32) | lo);
}
typedef const __attribute__((address_space(1))) v4u *gptr_v4u;
typedef const __attribute__((address_space(1))) v2u *gptr_v2u;

// ---- residual window -------------------------------------------------------------------------------
// The window rows j = split, split + nsplit, ... < r of a split are dealt to its waves in runs of kResRows: wave w
// owns list entries idx = 16 w + i, i < kResRows (round 3; rounds 1-2 dealt them round-robin, idx = w + 8 i: with 4-7
// rows per split that made 4-7 waves load a whole 16-row tile - 12 requests each in the kernel's front - for ONE row;
// now the older, faster wave 0 takes them all), as ONE 16-row MFMA tile that the wave runs before its code
// units: scores with A = the fp16 K rows themselves, values with B = the fp16 V rows
// (k = 16 rows, cols = 32 subspaces; even / odd dims by v_perm like the looked-up centroids).  Rows past the
// list re-read the wave's first row and are masked to -inf.
struct ResTile {
    v4u k[4];          // lane (q4, c16): row c16 of the tile, dims 32*q4 + 8*s .. + 8
    unsigned v[2][8];  // lane (h, c32): rows 8*h + j, dims (2m, 2m+1) of subspace m = 32*n + c32
};

// Row pointer of list entry idx (clamped to the wave's first entry, which exists when the tile is used).
__device__ __forceinline__ long long res_row_off(const AttnParams &p, int idx, int wave, int rcnt, int split, int rstart,
                                                 int r_old, bool &is_new) {
    const int idc = idx < rcnt ? idx : kResRows * wave;
    const int j = split + idc * p.nsplit;
    int row = rstart + j;
    row = row >= p.rcap ? row - p.rcap : row;          // rstart, j < rcap: one wrap at most
    is_new = p.k_new && j == r_old;                    // fused append: the new token is window row r_old
    return (long long)row * 128;
}

template <int MS = 64>
__device__ __forceinline__ void load_res_tile(const AttnParams &p, int bh, const f16 *kr, const f16 *vr, int wave, int rcnt,
                                              int split, int rstart, int r_old, int lane, ResTile &t) {
    const int q4 = lane >> 4, c16 = lane & 15, h = lane >> 5, c32 = lane & 31;
    {
        bool is_new;
        const long long off = res_row_off(p, kResRows * wave + c16, wave, rcnt, split, rstart, r_old, is_new);
        const f16 *kp = (is_new ? p.k_new + (long long)bh * 128 : kr + off) + 32 * q4;
#pragma unroll
        for (int s = 0; s < 4; ++s) t.k[s] = *(const v4u *)(kp + 8 * s);
    }
    if constexpr (MS == 320) {     // d_m = 4 form: lane (t = q4, n = c16): k-step s_: rows 4 t + 2 s_ (+ 1), dims 4 (n + 16 j) .. + 3
#pragma unroll
        for (int s_ = 0; s_ < 2; ++s_)
#pragma unroll
            for (int rr = 0; rr < 2; ++rr) {
                bool is_new;
                const long long off = res_row_off(p, kResRows * wave + 4 * q4 + 2 * s_ + rr, wave, rcnt, split, rstart, r_old, is_new);
                const f16 *vp = (is_new ? p.v_new + (long long)bh * 128 : vr + off) + 4 * c16;
#pragma unroll
                for (int j = 0; j < 2; ++j) {
                    const v2u w = *(const v2u *)(vp + 64 * j);
                    t.v[s_][4 * j + 2 * rr + 0] = w[0];
                    t.v[s_][4 * j + 2 * rr + 1] = w[1];
                }
            }
        return;
    }
    if constexpr (MS == 16) {      // d_m = 8 form: lane (t = q4, n = c16): k-step s_: rows 4 t + 2 s_ (+ 1), dims 8 n + 4 h .. + 3
#pragma unroll
        for (int s_ = 0; s_ < 2; ++s_)
#pragma unroll
            for (int rr = 0; rr < 2; ++rr) {
                bool is_new;
                const long long off = res_row_off(p, kResRows * wave + 4 * q4 + 2 * s_ + rr, wave, rcnt, split, rstart, r_old, is_new);
                const v4u w = *(const v4u *)((is_new ? p.v_new + (long long)bh * 128 : vr + off) + 8 * c16);
                t.v[s_][2 * rr + 0] = w[0]; t.v[s_][2 * rr + 1] = w[1];              // half h = 0
                t.v[s_][4 + 2 * rr + 0] = w[2]; t.v[s_][4 + 2 * rr + 1] = w[3];      // half h = 1
            }
        return;
    }
#pragma unroll
    for (int j = 0; j < 8; ++j) {
        bool is_new;
        const long long off = res_row_off(p, kResRows * wave + 8 * h + j, wave, rcnt, split, rstart, r_old, is_new);
        if (MS == 64) {      // tile (n, kk): dim 2*(32n + c32) + kk
            const f16 *vp = (is_new ? p.v_new + (long long)bh * 128 : vr + off) + 2 * c32;
            t.v[0][j] = *(const unsigned *)vp;
            t.v[1][j] = *(const unsigned *)(vp + 64);
        } else {             // M = 32, tile (i, jj): dim 4*c32 + 2i + jj
            const f16 *vp = (is_new ? p.v_new + (long long)bh * 128 : vr + off) + 4 * c32;
            const v2u w = *(const v2u *)vp;
            t.v[0][j] = w[0];
            t.v[1][j] = w[1];
        }
    }
}

// scores of the tile: sc[rho] = row 4*q' + rho for the head of this lane's column
template <class RT>      // ResTile / ResTileLean (lean kernel): the K rows are laid out alike
__device__ __forceinline__ void score_res_tile(const RT &t, const v8f16 (&qb)[4], float scale_log2e, int wave, int rcnt,
                                               int lane, float (&sc)[4]) {
    const int q4 = lane >> 4;
    v4f32 D = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
    for (int s = 0; s < 4; ++s)
        D = __builtin_amdgcn_mfma_f32_16x16x32_f16(__builtin_bit_cast(v8f16, t.k[s]), qb[s], D, 0, 0, 0);
#pragma unroll
    for (int rho = 0; rho < 4; ++rho)
        sc[rho] = (kResRows * wave + 4 * q4 + rho) < rcnt ? D[rho] * scale_log2e : -INFINITY;
}

// O += P (heads x 16 rows) * V rows.  pr[rho] = probability of row 4*q' + rho for the head of this lane's column.
__device__ __forceinline__ void value_res_tile(const ResTile &t, const float (&pr)[4], v16f32 (&O)[2][2]) {
    h2 t0 = {(f16)pr[0], (f16)pr[1]}, t1 = {(f16)pr[2], (f16)pr[3]};
    const v2u y0 = swap16_self(__builtin_bit_cast(unsigned, t0));     // [0]: rows 2h of the score layout, [1]: rows 2h + 1
    const v2u y1 = swap16_self(__builtin_bit_cast(unsigned, t1));
    const unsigned y00 = y0[0], y01 = y0[1], y10 = y1[0], y11 = y1[1];
    const v8f16 A = as_v8f16(y00, y10, y01, y11);                     // rows 8h + (0,1), (2,3), (4,5), (6,7)
#pragma unroll
    for (int n = 0; n < 2; ++n) {
        const unsigned(&e)[8] = t.v[n];
        const v8f16 B0 = as_v8f16(__builtin_amdgcn_perm(e[1], e[0], 0x05040100u), __builtin_amdgcn_perm(e[3], e[2], 0x05040100u),
                                  __builtin_amdgcn_perm(e[5], e[4], 0x05040100u), __builtin_amdgcn_perm(e[7], e[6], 0x05040100u));
        const v8f16 B1 = as_v8f16(__builtin_amdgcn_perm(e[1], e[0], 0x07060302u), __builtin_amdgcn_perm(e[3], e[2], 0x07060302u),
                                  __builtin_amdgcn_perm(e[5], e[4], 0x07060302u), __builtin_amdgcn_perm(e[7], e[6], 0x07060302u));
        O[n][0] = __builtin_amdgcn_mfma_f32_32x32x16_f16(A, B0, O[n][0], 0, 0, 0);
        O[n][1] = __builtin_amdgcn_mfma_f32_32x32x16_f16(A, B1, O[n][1], 0, 0, 0);
    }
}
// residual tile in the parity form: t.v[n][j] (rows 8h + j, dims (2m, 2m + 1)) IS the B operand of step s = j >> 2; pr[rho] =
// probability of row 4 q4 + rho = 8h + 4p' + rho: step 0's rows sit in the even lane rows, step 1's in the odd ones
__device__ __forceinline__ void value_res_tile_par(const ResTile &t, const float (&pr)[4], unsigned sel_lo, unsigned sel_hi, v16f32 (&O)[2][1]) {
    h2 t0 = {(f16)pr[0], (f16)pr[1]}, t1 = {(f16)pr[2], (f16)pr[3]};
    const v2u y0 = swap16_self(__builtin_bit_cast(unsigned, t0));
    const v2u y1 = swap16_self(__builtin_bit_cast(unsigned, t1));
    const unsigned e0 = y0[0], f0 = y0[1], e1 = y1[0], f1 = y1[1];
#pragma unroll
    for (int s = 0; s < 2; ++s) {
        const unsigned w0 = s ? f0 : e0, w1 = s ? f1 : e1;
        const v8f16 A = as_v8f16(__builtin_amdgcn_perm(0u, w0, sel_lo), __builtin_amdgcn_perm(0u, w0, sel_hi),
                                 __builtin_amdgcn_perm(0u, w1, sel_lo), __builtin_amdgcn_perm(0u, w1, sel_hi));
#pragma unroll
        for (int n = 0; n < 2; ++n)
            O[n][0] = __builtin_amdgcn_mfma_f32_32x32x16_f16(A, as_v8f16(t.v[n][4 * s], t.v[n][4 * s + 1], t.v[n][4 * s + 2], t.v[n][4 * s + 3]),
                                                             O[n][0], 0, 0, 0);
    }
}

// 16-lane row reductions by DPP (quad swaps, half-row mirror, row mirror), then the four rows by the row swaps
#define MILLION_DPP(x, CTRL) __builtin_bit_cast(float, __builtin_amdgcn_update_dpp(0, __builtin_bit_cast(int, (x)), (CTRL), 0xf, 0xf, false))
__device__ __forceinline__ float wave_max_valu(float x) {
    x = fmaxf(x, MILLION_DPP(x, 0xB1));      // quad_perm [1,0,3,2]
    x = fmaxf(x, MILLION_DPP(x, 0x4E));      // quad_perm [2,3,0,1]
    x = fmaxf(x, MILLION_DPP(x, 0x141));     // row_half_mirror
    x = fmaxf(x, MILLION_DPP(x, 0x140));     // row_mirror
    return rows_max(x);
}
__device__ __forceinline__ float wave_sum_valu(float x) {
    x += MILLION_DPP(x, 0xB1);
    x += MILLION_DPP(x, 0x4E);
    x += MILLION_DPP(x, 0x141);
    x += MILLION_DPP(x, 0x140);
    return rows_sum(x);
}

// ---- d_m = 8 form (M = 16, streaming kernel, G <= 4; round 4) ----------------------------------------------------------
// A 16-byte codebook entry is 8 dims of ONE token and ONE subspace: exactly one lane's 8 reduction slots of a 16x16x32 operand.
//   scores: A[row = token][k = (quarter q4, dim 8)] = the gathered K entry of subspace 4 q4 + s in k-step s; B = the query heads,
//           REPLICATED over the four column groups (column c = 4 dq + g holds head g): the score tile then has head g's
//           probabilities in every lane row the value operand wants them in - no lane movement at all;
//   values: a 16-byte V entry is handled as its two 8-byte halves (dims 4 h .. 4 h + 3, h = 0 / 1) in the d_m = 4 form below: the
//           reduction index is (token of 2, dim position of 4), B = the halves h of the two tokens' entries (two ds_read_b64), A
//           carries the two tokens' probabilities at dim position dq (lane-constant masks), one product per half:
//           D_h[(dq, g)][n] = out[g][8 n + 4 h + dq].  (First version: whole entries by ds_read_b128, reduction index (token of 4,
//           dim position of 8), A = {x, y, 0, 0} / {0, 0, x, y} for the two row tiles: twice the value MFMAs, and hipcc rebuilt
//           the zero-padded operands with 8 v_mov per step.)
// Per 32-token unit: 8 gathers (ds_read_b128) + 16 (ds_read_b64), 8 score + 8 value MFMAs (16x16x32), 8 accumulator registers, no
// pack and no cross-lane instruction.
__device__ __forceinline__ void d8_masks(int lane, unsigned &mx, unsigned &my) {
    const int dq = (lane >> 2) & 3;      // column group of this lane = dim position (mod 4) of its rows
    mx = dq == 0 ? 0x0000ffffu : dq == 1 ? 0xffff0000u : 0u;
    my = dq == 2 ? 0x0000ffffu : dq == 3 ? 0xffff0000u : 0u;
}
// ---- d_m = 4 form (M = 32, G <= 4): the same idea with 8-byte entries.  A lane's 8 reduction slots are TWO tokens x 4 dim
// positions: k-step s of a 16-token tile takes tile rows 4 t + 2 s and 4 t + 2 s + 1 (t = lane >> 4) - registers 2 s, 2 s + 1 of the
// lane's own scores; the B operand is the two gathered entries of those rows, for subspace n (column tile 0) and n + 16 (tile 1);
// rows = (dim position dq, head g): ONE row tile.  Per unit: 16 + 16 gathers (ds_read_b64), 8 + 8 MFMAs (16x16x32), 8
// accumulator registers (the packed form: 8 + 8 MFMAs of which the value ones are 32x32x16, 48 pack v_perm, 64 accumulators).
__device__ __forceinline__ void d4_vstep(float p0, float p1, const unsigned (&e)[8], unsigned mx, unsigned my, Acc8 &O) {
    const h2 a0 = {(f16)p0, (f16)p0}, a1 = {(f16)p1, (f16)p1};
    const unsigned w0 = __builtin_bit_cast(unsigned, a0), w1 = __builtin_bit_cast(unsigned, a1);
    const v8f16 A = as_v8f16(w0 & mx, w0 & my, w1 & mx, w1 & my);
    O.t[0] = __builtin_amdgcn_mfma_f32_16x16x32_f16(A, as_v8f16(e[0], e[1], e[2], e[3]), O.t[0], 0, 0, 0);
    O.t[1] = __builtin_amdgcn_mfma_f32_16x16x32_f16(A, as_v8f16(e[4], e[5], e[6], e[7]), O.t[1], 0, 0, 0);
}
// residual tile: t.v[s][4 j + ..] = (row 4 t + 2 s, row 4 t + 2 s + 1) x dims 4 (n + 16 j) .. + 3
__device__ __forceinline__ void value_res_tile_d4(const ResTile &t, const float (&pr)[4], unsigned mx, unsigned my, Acc8 &O) {
#pragma unroll
    for (int s_ = 0; s_ < 2; ++s_) d4_vstep(pr[2 * s_], pr[2 * s_ + 1], t.v[s_], mx, my, O);
}
// rescale of the accumulators: register i belongs to head i, whose alpha sits in lane i of this lane's quad
__device__ __forceinline__ void rescale_acc(Acc8 &O, float alpha, int, int) {
    const float f0 = MILLION_DPP(alpha, 0x00), f1 = MILLION_DPP(alpha, 0x55), f2 = MILLION_DPP(alpha, 0xAA), f3 = MILLION_DPP(alpha, 0xFF);
#pragma unroll
    for (int h = 0; h < 2; ++h) { O.t[h][0] *= f0; O.t[h][1] *= f1; O.t[h][2] *= f2; O.t[h][3] *= f3; }
}
template <int KK>
__device__ __forceinline__ void rescale_acc(v16f32 (&O)[2][KK], float alpha, int G, int lane) { rescale_heads<KK == 1>(O, alpha, G, lane); }

// online softmax over N new scores of this lane's column (head): updates (m_run, l_run), rescales O when a
// running maximum moves, turns the scores into probabilities in place
template <int N, bool PV = false, class ACC>
__device__ __forceinline__ void softmax_online(float (&sc)[N], float &m_run, float &l_run, ACC &O, int G, int lane) {
    float mx = sc[0];
#pragma unroll
    for (int i = 1; i < N; ++i) mx = fmaxf(mx, sc[i]);
    mx = rows_max(mx);
    const float m_new = fmaxf(m_run, mx);
    const float m_safe = m_new > -INFINITY ? m_new : 0.f;
    const float alpha = fast_exp2(m_run - m_safe);
    if (__any(m_new > m_run && m_run > -INFINITY)) {
        rescale_acc(O, alpha, G, lane);
    }
    float ls = 0.f;
#pragma unroll
    for (int i = 0; i < N; ++i) {
        sc[i] = fast_exp2(sc[i] - m_safe);
        ls += sc[i];
    }
    l_run = l_run * alpha + ls;
    m_run = m_new;
}

// same on RAW scores (q.k, masked to -inf where needed): the 1/sqrt(d)*log2(e) factor c > 0 is folded into the exp2
// argument (one fma per score instead of a multiply and a subtract), the running maximum stays in the scaled domain
// v_max3_f32 without the two canonicalising v_max x, x that fmaxf() of an MFMA result costs under IEEE mode (the operands
// are never signalling NaNs); plain asm, not volatile: the scheduler may move it
__device__ __forceinline__ float max3_raw(float a, float b, float c) {
    float r;
    asm("v_max3_f32 %0, %1, %2, %3" : "=v"(r) : "v"(a), "v"(b), "v"(c));
    return r;
}
// Softmax state of this lane's head in the streaming kernel.  m is the softmax REFERENCE, not necessarily the running
// maximum: it moves (cross-lane maximum, alpha, rescale of O and l) only when a raw score of the unit exceeds thr_raw =
// (m + 2^3) / c, i.e. when a probability would exceed 2^8 (fp16 operand of the value MFMA: exact up to 2^15).  The common
// unit needs no cross-lane reduction: four v_max3, one compare, a wave-uniform branch.  Any reference gives the same
// softmax; the merges downstream only need (m, l, O) to be consistent.  neg_ref = -(m, or 0 while m = -inf) and thr_raw
// are kept in registers so that the common path recomputes neither.
struct SoftRef {
    float m, l, neg_ref, thr_raw;
    float idle = 0.f;      // -inf in the lanes of score columns >= G (no query head): their probabilities come out as exact zeros, so
                           // the idle rows of the value MFMA's A operand multiply zeros (round 4: the MFMAs set the chip's clock -
                           // tools/micro/core_micro.hip "MFMA -> 1 VALU": 1.80 -> 2.31 GHz - and zero operands draw less)
    __device__ __forceinline__ void set(float m_, float l_, float inv_c) {
        m = m_; l = l_;
        neg_ref = (m_ > -INFINITY ? -m_ : 0.f) + idle;
        thr_raw = (m_ + 8.0f) * inv_c;          // -inf while nothing has been seen: the first finite score moves it
    }
};
template <int N, bool PV = false, class ACC>
__device__ __forceinline__ void softmax_online_raw(float (&sc)[N], float c, float inv_c, SoftRef &st, ACC &O, int G, int lane) {
    static_assert(N == 8, "one 32-token unit: 8 scores per lane");
    float mx = max3_raw(sc[0], sc[1], sc[2]);
    mx = max3_raw(mx, sc[3], sc[4]);
    mx = max3_raw(mx, sc[5], sc[6]);
    mx = max3_raw(mx, sc[7], sc[7]);
    if (__any(mx > st.thr_raw)) {
        const float m_new = fmaxf(st.m, rows_max(mx) * c);
        const float m_safe = m_new > -INFINITY ? m_new : 0.f;
        const float alpha = fast_exp2(st.m - m_safe);
        if (__any(m_new > st.m && st.m > -INFINITY)) {
            rescale_acc(O, alpha, G, lane);
        }
        st.set(m_new, st.l * alpha, inv_c);
    }
    float ls = 0.f;
#pragma unroll
    for (int i = 0; i < N; ++i) {
        sc[i] = fast_exp2(fmaf(sc[i], c, st.neg_ref));
        ls += sc[i];
    }
    st.l += ls;
}
