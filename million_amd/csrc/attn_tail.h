// attn_tail.h - the split-merge tail of the decode MFMA kernels.  Included by attn_mfma.hip (inside namespace million, behind
// decode_wave.h): attn_stream_kernel and attn_lean_kernel both end in merge_and_publish.  tests/test_host_logic.py models the
// protocol on the CPU.
// =====================================================================================================
// Tail shared by the MFMA kernels (round 3): wave partials -> LDS -> the split's partial -> workspace -> merge.
//
// Round 2 handed the split partials over through MEMORY: write-through (sc1) stores, drain, barrier, one returning
// ticket atomic, barrier, and in the last arriver 64 KiB of sc1 loads by one workgroup - three dependent fabric round
// trips, 3.4 us of an 18 us launch (profiles/r02_stamps.txt).  Now (protocol measured in isolation by
// tools/micro/l2_handoff.hip -> profiles/r03_l2_handoff.txt):
//   * the kernel deals all splits of a (b, kv head) to ONE XCD (workgroup i runs on XCD i % 8).  A plain store is in
//     that XCD's L2 when its vmcnt retires, and an sc1 load issued on the same XCD is served from there (it bypasses
//     only the L1): a same-XCD hand-off never leaves the chiplet.  Whether the placement really holds is checked, not
//     assumed: in its prologue every workgroup MARKS its slot of the (b, kv head)'s census line with its XCC id (one
//     write-through 4-byte store), and at the start of its tail it reads the line: only if all nsplit slots carry its own
//     XCC id does it store its partial plain; otherwise (another XCD, or a workgroup that has not started yet)
//     write-through (sc1), which any XCD can read.  Loads and polls are sc1 in both cases;
//   * nobody waits for a ticket: the arrival index is requested ~3 us ahead of the tail (wave 7, which stores nothing);
//     the storing waves drain their stores, and behind the workgroup barrier they then join the split's FLAG (= generation
//     + 1) is raised; the workgroup whose index is ns - 1 is the merger (round 4: the only one): its waves poll the flags
//     (lane = split, bounded) and merge the query heads, four waves per head and two heads per pass - 16 KiB of loads per
//     head, wave reductions by DPP / row swaps, no LDS, no barrier.  Every workgroup it waits for has taken its index, so
//     it is resident, past its loop and waits for nothing: the polls end under any dispatch order and any residency.  A
//     poll that runs out of its bound is COUNTED (g_tail_faults, million_debug_tail_faults) and the heads are written as
//     NaN, never as the sum of stale partials;
//   * the workgroup with the highest index clears the census line and the counter and advances the generation once its
//     own poll has seen every flag (all census reads and stores of the launch are behind those flags);
//   * nsplit = 1: the only workgroup normalises and writes the output itself.
//
// Window-length advance (fused append with device-resident lengths: r += 1 once per launch and request).  r may move only
// when every workgroup of the request has read its lengths, and exactly one workgroup may move it: the primaries of the
// request's nh_k (virtual) kv heads take a SECOND-LEVEL ticket on ws_cnt2[b], and the one that draws nh_k - 1 puts that
// word back to 0 and bumps r.  Through round 5 this sat at the very end of the tail, behind the primary's polls, merge and
// `out` stores: a returning atomic on a word that primaries on eight XCDs hit, then in the last of them a store, a load
// of r, an add and a store - two dependent fabric round trips behind the end of the launch's last merge, i.e. on the
// critical path of every step-form launch and of no other call form (profiles/ab_decode_advance.txt).  Now:
//   * the ticket is REQUESTED as soon as the workgroup knows that it is the primary - behind the barrier that makes its
//     arrival index visible, in front of the flag polls and the merge.  Why that is early enough to be safe: a workgroup
//     takes its first-level index in tail_request, which it reaches behind its codebook barrier, and every wave of it has
//     executed LAUNCH_FRONT_LENGTHS - the only place where either MFMA kernel reads dev_lengths - in front of that barrier.
//     So idx == ns - 1 already says that all ns workgroups of the pair have read their lengths; a workgroup that is not
//     dispatched yet has taken no index, so no primary exists before it has.  The request's last second-level ticket
//     therefore says the same for every pair of the request.  Nothing else in the launch reads r (the append row's slot
//     comes from the registers of the front);
//   * it is a buffer atomic of wave kNW - 1, issued early and looked at late, like the first-level ticket: with helpers
//     (nm = G = 4) waves 4 - 7 of a merger have no head to merge, so that wave waits for the answer while the others poll
//     and merge (~1.4 us) and bumps r before they are done.  With one merger (grids larger than the chip), and where the
//     primary takes over a helper's head, wave kNW - 1 polls and merges itself: its poll loads retire in order behind the
//     returning atomic, so the first poll's wait is also the wait for the ticket - there the round trip runs IN FRONT of
//     the wave's poll, not beside it; what is saved in that case is the second trip (no load of r) and that the wave's
//     merge is not in front of the request.  ns = 1: the round trip follows the output stores, as before;
//   * the last arriver does not load r: it stores 0 to the ticket word and issues an atomic add of 1 on the RAW device word
//     (not the clamped value the launch computed with) whose result nobody uses - nothing the end of the kernel waits for
//     beyond what the `out` stores already cost.  The ticket word is at rest when the launch ends (common.h), so the tile
//     and scalar kernels, which take the same ticket behind their merge (common.h: ticket_and_merge), can alternate with
//     these on one workspace.  No spin, no poll and no wait on another workgroup was added.
// tests/test_decode_advance.py: back-to-back step-form launches on every path, and a CPU model over every interleaving.
// =====================================================================================================
__device__ __forceinline__ unsigned *tail_rec(const AttnParams &p, int bh) { return (unsigned *)p.ws_cnt + (long long)bh * kRecWords; }
__device__ __forceinline__ unsigned *tail_flags(const AttnParams &p, int bh) { return p.ws_flags + (long long)bh * (2 * kFlagWords); }
__device__ __forceinline__ unsigned tail_xcc() { return __builtin_amdgcn_s_getreg(6164) & 7u; }      // hwreg(HW_REG_XCC_ID, 0, 4)

// Census mark: thread 0, write-through (every XCD must be able to read it, and no copy may linger dirty in an L2 when the
// last workgroup clears the line), in a wave-uniform branch of wave 0.  hipcc sizes wave 0's later vmcnt waits as if the
// store had not been issued, so wave 0's next wait for an OLDER load also waits for this store's acknowledgement: it is
// placed in the prologue behind the first gathers, where that next wait is ~1 us away, in the wave that reaches the
// wave-merge barrier 1.6 us early anyway.  The same wave drains it (vmcnt(0)) before this workgroup's flag goes up.
// (First form of this tail: a returning start-counter atomic, a census atomic and a generation load up here, by all eight
// waves: 512 same-line memory-side operations per (b, kv head) queued at one channel and launches took 20-25 us; by one
// lane: the body still ran 1.4 us longer.)
__device__ __forceinline__ void tail_mark_xcd(const AttnParams &p, int bh, int split, int wave, int lane) {
    if (wave == 0) {
        if (lane == 0) {
            __hip_atomic_store(tail_flags(p, bh) + kFlagWords + split, tail_xcc() + 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            // diagnostics (million_set_force_generic(4)): every helper "has given up" before anybody's ticket
            if (p.tail_test == 1) __hip_atomic_fetch_or(tail_rec(p, bh) + 2, 0xffu, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        }
    }
}

// The tail's three requests - census line (wave 0, lane = split), arrival index (returning atomic) and generation (thread
// (kNW-1)*64) - issued ~3 us ahead of the tail, between the last blocks of the streaming loop: under the full code stream a
// memory round trip takes 2-3 us, more than the wave merge hides (the census read at the start of the tail held barrier B
// for 0.7 us).  Every lane of every wave issues the three instructions - no branch between two blocks of the pipeline, and
// no conditional vector-memory operation for hipcc's wait counting - but only the lanes named above address inside the
// descriptors; the hardware drops out-of-range lanes (loads return 0).
struct TailReq {
    int idx;        // RAW ticket word as the atomic returned it: give-up bits [7:0], arrival count [31:8] (see merge_and_publish)
    unsigned gen, cen, base;
    int nm, tt;     // mergers per (b, kv head) and the tail's test mode: kernel arguments, read here - not on the tail's critical path
    bool done;      // wave-uniform: false = this wave never passed the early request point (it had no whole round)
};
__device__ __forceinline__ void tail_request(const AttnParams &p, int bh, int ns, int wave, int lane, TailReq &t) {
    constexpr int kOut = 1 << 20;
    __amdgpu_buffer_rsrc_t rr = __builtin_amdgcn_make_buffer_rsrc((void *)tail_rec(p, bh), 0, kRecWords * 4, 0x00020000);
    __amdgpu_buffer_rsrc_t rc = __builtin_amdgcn_make_buffer_rsrc((void *)(tail_flags(p, bh) + kFlagWords), 0, kFlagWords * 4, 0x00020000);
    const bool one = wave == kNW - 1 && lane == 0;
    t.cen = __builtin_amdgcn_raw_buffer_load_b32(rc, wave == 0 ? (lane < ns ? lane : 0) * 4 : kOut, 0, 16);
    t.idx = __builtin_amdgcn_raw_ptr_buffer_atomic_add_i32(256, rr, one ? 2 * 4 : kOut, 0, 0);
    t.gen = __builtin_amdgcn_raw_buffer_load_b32(rr, one ? 3 * 4 : kOut, 0, 16);
    t.base = __builtin_amdgcn_raw_buffer_load_b32(rr, one ? 4 * 4 : kOut, 0, 16);
    t.nm = ns > 1 ? (p.nmerge < ns ? (p.nmerge > 0 ? p.nmerge : 1) : ns) : 1;
    t.tt = p.tail_test;
    t.done = true;
}

// Count of merges that gave up waiting for a split's flag (million_debug_tail_faults): never non-zero unless a workgroup of the
// launch died or the workspace was not zeroed; the heads concerned are written as NaN, never as a stale partial's sum.
__device__ unsigned g_tail_faults = 0;

// One query head is merged by FOUR waves: wave part (0..3) owns outputs [32 part, 32 part + 32) of the head; its lane
// (h, q8) owns float4 q8 of those for the splits s = h (mod 8): ns / 8 16-byte loads per lane, the eight split subsets are
// summed with DPP / row swaps.  (A two-heads-per-pass variant - both heads' loads in flight before the first reduction - paid
// when ONE workgroup merged every head; with the helpers back each merger has one head per wave group and the second
// instantiation only made the cold tail longer.)
template <int DD = 128, bool LSE = false>      // DD = d: rows of 64 dims (lean kernel, d = 64) keep two of the four waves of a head busy
__device__ __forceinline__ void tail_merge_head(const AttnParams &p, int b, int hk, int g, int part, int ns, const float *src, int lane,
                                                bool fault) {
    if (32 * part >= DD) return;      // wave-uniform
    const int q8 = lane & 7, h = lane >> 3;
    __amdgpu_buffer_rsrc_t rsrc = __builtin_amdgcn_make_buffer_rsrc((void *)src, 0, 0x7fffffff, 0x00020000);
    // softmax weights of the splits (lane = split)
    const bool on = lane < ns;
    const int sl = on ? lane : 0;
    const float m1 = __builtin_bit_cast(float, __builtin_amdgcn_raw_buffer_load_b32(rsrc, (sl * p.slot_floats + p.G * DD + g) * 4, 0, 16));
    const float l1 = __builtin_bit_cast(float, __builtin_amdgcn_raw_buffer_load_b32(rsrc, (sl * p.slot_floats + p.G * DD + p.G + g) * 4, 0, 16));
    v4u v[8];
#pragma unroll
    for (int k = 0; k < 8; ++k) {
        const int slot = 8 * k + h;
        const int sc = slot < ns ? slot : ns - 1;                      // clamped: never a conditional load (weight 0)
        if (k < 4 || ns > 32)                                          // wave-uniform: the second half only for more than 32 splits
            v[k] = __builtin_amdgcn_raw_buffer_load_b128(rsrc, (sc * p.slot_floats + g * DD + 32 * part + 4 * q8) * 4, 0, 16);
        else
            v[k] = v4u{0, 0, 0, 0};
    }
    const float m0 = on ? m1 : -INFINITY;
    const float l0 = on ? l1 : 0.f;
    const float mx = wave_max_valu(m0);
    const float ms_ = mx > -INFINITY ? mx : 0.f;
    const float w0 = fast_exp2(m0 - ms_);                               // -inf -> 0 (lanes >= ns: 0)
    // unnormalised sum first, 1 / (sum of w l) at the end: the denominator's reduction runs beside the accumulation
    v4f32 acc = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
    for (int k = 0; k < 8; ++k) {
        const float w = __builtin_bit_cast(float, __builtin_amdgcn_ds_bpermute(4 * (8 * k + h), __builtin_bit_cast(int, w0)));
        acc += w * __builtin_bit_cast(v4f32, v[k]);
    }
    const float den = wave_sum_valu(w0 * l0);
    // nothing to attend to: 0; a merge that gave up on a flag: NaN, never a stale partial's sum
    const float inv = fault ? __builtin_nanf("") : den > 0.f ? __builtin_amdgcn_rcpf(den) : 0.f;
    // sum over the eight split subsets: lanes l, l ^ 8 (same 16-lane row), then the four rows
#pragma unroll
    for (int c = 0; c < 4; ++c) {
        float x = acc[c];
        x += MILLION_DPP(x, 0x128);      // row_ror:8
        acc[c] = rows_sum(x) * inv;
    }
    if (lane < 8) {
        typedef f16 h4 __attribute__((ext_vector_type(4)));
        const h4 o = {(f16)acc[0], (f16)acc[1], (f16)acc[2], (f16)acc[3]};
        *(h4 *)(p.out + ((long long)b * p.nh + head0(p, hk) + g) * DD + 32 * part + 4 * q8) = o;
    }
    // the head's lse from the maximum and the denominator every lane of this wave holds: one lane of the wave that owns the head's
    // first 32 dims; a merge that gave up: NaN, like `out`
    if constexpr (LSE) { if (part == 0 && lane == 0) store_lse(p, b, hk, g, fault ? __builtin_nanf("") : lse_of(ms_, den)); }
}

template <int MS = 64, bool PV = false, int DD = 128, bool LSE = false, class ACC>
__device__ __forceinline__ void merge_and_publish(const AttnParams &p, char *smem, int b, int hk, int split, int G, int tid,
                                                  int lane, int wave, bool dbg_on, ACC &O, float m_run, float l_run, TailReq &treq) {
#define STAMP(i) stamp_lds(dbg_on, lane, wave, i)
    const int ns = p.nslots;
    const int bh = b * p.nh_k + hk;
    // LDS words by absolute address (a generic pointer made these FLAT accesses): [1] arrival index, [2] generation,
    // [3] 1 = every split of this (b, kv head) runs on this XCD, [5] give-up bits as this workgroup's ticket returned them,
    // [6] count base of this launch (common.h: record words [2] and [4])
    typedef volatile __attribute__((address_space(3))) int *lds_int_p;
    const lds_int_p tl = (lds_int_p)(size_t)kPartOff;
    // ---- census line / arrival index / generation: requested ~3 us ago by the streaming loop (tail_request); a wave that
    //      had no whole round asks now ----
    if (!treq.done) tail_request(p, bh, ns, wave, lane, treq);
    const unsigned raw_v = (unsigned)treq.idx;
    const int idx_v = (int)(((raw_v >> 8) - treq.base) & 0xffffffu);      // arrival index of this workgroup within this launch
    const unsigned gen_v = treq.gen, cen_v = treq.cen;
    // ---- merge the waves of this workgroup through LDS (tables are dead after the barrier) ----
    l_run = rows_sum(l_run);
    __syncthreads();
    STAMP(4);
    if (wave == 0) {
        const bool all_here = __all(cen_v == tail_xcc() + 1u);
        if (lane == 0) tl[3] = all_here ? 1 : 0;
    }
    const int wstride = G * DD + 2 * kMaxGMfma;           // floats per wave (G = 16: 65 KiB for the 8 waves, the dead tables' space)
    float *scr_l = (float *)smem;
    float *mine = scr_l + wave * wstride;
    {
        const bool hi = lane >= 32;
        const int c32 = lane & 31;
        if constexpr (MS == 640) {     // lean kernel (z-rows): accumulator pi, lane (rg = lane >> 4, n = lane & 15), register i = head i:
                                       // row 4 rg + i = (z = rg >> 1, parity rg & 1, head i), column n = subspace 32 pi + 16 z + n
#pragma unroll
            for (int j = 0; j < DD / 64; ++j)
#pragma unroll
                for (int i = 0; i < 4; ++i)
                    if (i < G) mine[i * DD + 64 * j + 32 * (lane >> 5) + 2 * (lane & 15) + ((lane >> 4) & 1)] = O.t[j][i];
        } else
        if constexpr (MS == 320) {     // d_m = 4 form: column tile j, lane (dq = lane >> 4, n = lane & 15), register i = head i
#pragma unroll
            for (int j = 0; j < DD / 64; ++j)
#pragma unroll
                for (int i = 0; i < 4; ++i)
                    if (i < G) mine[i * DD + 4 * ((lane & 15) + 16 * j) + (lane >> 4)] = O.t[j][i];
        } else
        if constexpr (MS == 16) {      // d_m = 8 form: row tile h, lane (dq = lane >> 4, n = lane & 15), register i = head i
#pragma unroll
            for (int h = 0; h < 2; ++h)
#pragma unroll
                for (int i = 0; i < 4; ++i)
                    if (i < G) mine[i * 128 + 8 * (lane & 15) + 4 * h + (lane >> 4)] = O.t[h][i];
        } else
        if constexpr (PV) {      // parity-V tiles O[n][0]: register 4 j + rho = row 8 j + 4 hi + rho = (parity j >> 1, head 8 (j & 1) + 4 hi + rho)
#pragma unroll
            for (int j = 0; j < 4; ++j)
#pragma unroll
                for (int rho = 0; rho < 4; ++rho) {
                    const int g = 8 * (j & 1) + (hi ? 4 + rho : rho);
                    if (g < G) {
#pragma unroll
                        for (int n = 0; n < 2; ++n) mine[g * 128 + 2 * (32 * n + c32) + (j >> 1)] = O[n][0][4 * j + rho];
                    }
                }
        } else if constexpr (MS != 16 && MS != 320 && MS != 640) {
#pragma unroll
        for (int j = 0; j < 2; ++j)                      // tile rows 8 j + 4 hi + rho = register 4 j + rho; j = 1: groups above 8 heads
#pragma unroll
            for (int rho = 0; rho < 4; ++rho) {
                const int g = 8 * j + (hi ? 4 + rho : rho);
                if (g < G) {
#pragma unroll
                    for (int n = 0; n < 2; ++n)
#pragma unroll
                        for (int kk = 0; kk < (PV ? 1 : 2); ++kk)
                            mine[g * 128 + (MS == 64 ? 2 * (32 * n + c32) + kk : 4 * c32 + 2 * n + kk)] = O[n][kk][4 * j + rho];
                }
            }
        }
        if (lane < G) {                                  // lane g: row q' = 0, col g
            mine[G * DD + lane] = m_run;
            mine[G * DD + kMaxGMfma + lane] = l_run;
        }
    }
    __syncthreads();
    // a thread combines the 8 wave partials of 4 consecutive output elements (16-byte LDS reads) and publishes them
    // straight from registers with one 16-byte store into this split's workspace slot: plain (stays in this XCD's L2)
    // when the census says every workgroup of this (b, kv head) runs on this XCD, write-through (sc1) otherwise
    const bool same_xcd = tl[3] != 0;
    const int nsw = (G * (DD / 4) + 63) >> 6;            // waves that store
    float *dst = slot_ptr(p, b, hk, split);
    {
        __amdgpu_buffer_rsrc_t rsrc = __builtin_amdgcn_make_buffer_rsrc((void *)dst, 0, 0x7fffffff, 0x00020000);
        for (int q = tid; q < G * (DD / 4); q += kNW * 64) {
            const int g = q / (DD / 4);
            float mw[kNW], lw[kNW];
            v4f32 vw[kNW];
#pragma unroll
            for (int w = 0; w < kNW; ++w) {
                mw[w] = scr_l[w * wstride + G * DD + g];
                vw[w] = *(const v4f32 *)(scr_l + w * wstride + 4 * q);
                lw[w] = scr_l[w * wstride + G * DD + kMaxGMfma + g];
            }
            float Mx = mw[0];
#pragma unroll
            for (int w = 1; w < kNW; ++w) Mx = fmaxf(Mx, mw[w]);
            const float Ms = Mx > -INFINITY ? Mx : 0.f;
            v4f32 acc = {0.f, 0.f, 0.f, 0.f};
            float lsum = 0.f;
#pragma unroll
            for (int w = 0; w < kNW; ++w) {
                const float f = fast_exp2(mw[w] - Ms);      // -inf -> 0
                acc += f * vw[w];
                lsum = fmaf(f, lw[w], lsum);
            }
            if (ns == 1) {      // the only split of this (b, kv head): normalise and write the output (nothing to attend to: 0)
                const float inv = lsum > 0.f ? 1.0f / lsum : 0.f;
                typedef f16 h4 __attribute__((ext_vector_type(4)));
                const h4 o = {(f16)(acc[0] * inv), (f16)(acc[1] * inv), (f16)(acc[2] * inv), (f16)(acc[3] * inv)};
                *(h4 *)(p.out + ((long long)b * p.nh + head0(p, hk)) * DD + 4 * q) = o;
                if constexpr (LSE) { if (q % (DD / 4) == 0) store_lse(p, b, hk, g, lse_of(Ms, lsum)); }      // the head's first thread
            } else if (same_xcd) {
                __builtin_amdgcn_raw_buffer_store_b128(__builtin_bit_cast(v4u, acc), rsrc, q * 16, 0, 0);
                if (q % (DD / 4) == 0) {      // (a slot is laid out for p.G heads: the last part of an odd head group holds fewer, G < p.G)
                    dst[p.G * DD + g] = Mx;
                    dst[p.G * DD + p.G + g] = lsum;
                }
            } else {
                __builtin_amdgcn_raw_buffer_store_b128(__builtin_bit_cast(v4u, acc), rsrc, q * 16, 0, 16 /* sc1 */);
                if (q % (DD / 4) == 0) {
                    st_agent(dst + p.G * DD + g, Mx);
                    st_agent(dst + p.G * DD + p.G + g, lsum);
                }
            }
        }
    }
    STAMP(5);
    if (wave == kNW - 1 && lane == 0) { tl[1] = idx_v; tl[2] = (int)gen_v; tl[5] = (int)(raw_v & 0xffu); tl[6] = (int)treq.base; }      // the index, the generation, the give-up bits and the base have arrived
    // a storing wave's partial is out of the CU (in L2, or in memory) when its vmcnt retires; the flag is raised behind the
    // barrier every storing wave then joins (cdna_hip_programming.md Guideline 16, R1)
    if (ns > 1 && wave < nsw) asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    __syncthreads();      // wave scratch is dead; index and generation are visible to every wave
    MILLION_STAMP(p, 10);
    const int idx = tl[1];
    const unsigned want = (unsigned)tl[2] + 1u;
    if (ns > 1 && tid == 0) {
        __amdgpu_buffer_rsrc_t rf = __builtin_amdgcn_make_buffer_rsrc((void *)tail_flags(p, bh), 0, kFlagWords * 4, 0x00020000);
        if (same_xcd) __builtin_amdgcn_raw_buffer_store_b32(want, rf, split * 4, 0, 0);
        else __builtin_amdgcn_raw_buffer_store_b32(want, rf, split * 4, 0, 16 /* sc1 */);
    }
    if (p.dbg && tid == 0)      // diagnostics: slot 12 = 1 + "stored plain (every split on this XCD)", slot 13 = 1 + arrival index
        { unsigned long long *d_ = p.dbg + ((long long)blockIdx.y * gridDim.x + blockIdx.x) * kStampWaves * kStampSlots; d_[12] = 1 + (same_xcd ? 1 : 0); d_[13] = 1 + idx; }
    // ---- window-length advance of a fused append with device-resident lengths: the second-level ticket (ws_cnt2[b], one per
    //      request; all nh_k primaries of the request hit this word, from eight XCDs) is REQUESTED here, in front of the polls
    //      and the merge, and its answer is looked at behind them (see "Window-length advance" in the header).  Wave kNW - 1 of
    //      a primary asks: with helpers (nm = G = 4) waves 4 - 7 of a merger have no head, so the round trip runs beside the
    //      other waves' merge and this wave bumps r while they still merge; with one merger the wave polls and merges too, and
    //      its first poll waits for the answer as well (in-order returns).  Every lane of the wave issues the instruction; only
    //      lane 0 of a primary's wave addresses inside the descriptor (one word; none in a workgroup that is no primary): the
    //      hardware drops the rest. ----
#if !(MILLION_EXP & 64)      // (A/B: no advance at all - what the step form pays for it, profiles/ab_decode_advance.txt)
    // (kernel-uniform branch: a launch that does not advance r - plain, append-only, device lengths only - keeps the
    //  instruction stream it had.  Without it every workgroup of those launches issued one atomic the hardware drops, and its
    //  wait: measured +0.04 .. +0.14 us on their medians at one request, inside their band, profiles/ab_decode_advance.txt)
    const bool adv_wave = wave == kNW - 1 && p.k_new && p.dev_lengths_w;
    const bool adv_mine = idx == ns - 1;      // workgroup-uniform
    int adv_t2 = 0;
    if (adv_wave) {
        MILLION_STAMP(p, 14);
        __amdgpu_buffer_rsrc_t r2 = __builtin_amdgcn_make_buffer_rsrc((void *)(p.ws_cnt2 + b), 0, adv_mine ? 4 : 0, 0x00020000);
        adv_t2 = __builtin_amdgcn_raw_ptr_buffer_atomic_add_i32(1, r2, lane == 0 ? 0 : (1 << 20), 0, 0);
    }
#endif
    // ---- the merge (round 4).  The workgroup whose arrival index is ns - 1 - the PRIMARY - is responsible for every head:
    //      every workgroup it waits for has taken its index, i.e. is resident, on its way to its own flag store, and waits
    //      for nothing itself, so its polls end under ANY dispatch order and residency.  The nm - 1 workgroups that arrived
    //      just before it are HELPERS (merger k = idx - (ns - nm) takes heads k, k + nm, ...).  A helper needs the flags of
    //      workgroups that arrived AFTER it and may not even be dispatched (more workgroups than resident slots; two launches
    //      sharing the chip), so its patience is BOUNDED (48 polls of the flags, ~30 us).  What happens then is decided on ONE
    //      word, the ticket word of the (b, kv head): arrival count in bits 31:8 (a ticket is an atomic add of 256), give-up
    //      bits 7:0.  A helper wave out of patience ORs bit k in and looks at the count the atomic returns: incomplete - the
    //      last ticket comes later and RETURNS the bit to the primary (fetched ~3 us before its tail): leave, the primary merges
    //      head k too; complete - every workgroup is resident, the flags will come: poll on and merge.  Atomics on one word are
    //      serialised, so there is no window between the two cases, and nobody polls anybody's status.  The count is never
    //      reset (a straggling wave must never read a count that looks incomplete): a launch's indices are counted from
    //      `base`, which the primary moves on by ns at the end, together with the generation; it also clears the bits (one set
    //      behind the clear costs the next launch's primary a redundant merge of the same values, nothing else).
    //      (Round 3 let all nm mergers wait for flags without bound: when every resident workgroup is such a merger the launch
    //      stalls for the spin bound and merges stale partials.  The primary alone pulls all 64 KiB of a (b, kv head)'s
    //      partials through ONE CU: +1.2 us per launch at one request; helpers that report through status words the primary
    //      polls: +0.8 us, profiles/r04_ab_merge.txt.)  The host sets nmerge = 1 when the grid does not fit the chip.
    //      Every merging wave polls the flags itself (lane = split) and merges behind its own match; four waves per head:
    //      waves 0-3 heads k, k + 2 nm, ..., waves 4-7 heads k + nm, k + 3 nm, ... ----
    const int nm = treq.nm;
    const int km = idx - (ns - nm);                          // merger number; nm - 1 = the primary
    if (ns > 1 && km >= 0) {
        const bool primary = idx == ns - 1;
        const float *src = p.ws_part + (long long)bh * ns * p.slot_floats;
        __amdgpu_buffer_rsrc_t rf = __builtin_amdgcn_make_buffer_rsrc((void *)tail_flags(p, bh), 0, kFlagWords * 4, 0x00020000);
        const int fo = (lane < ns ? lane : 0) * 4;
        const int tt = treq.tt;
        // The common path is short and straight (this code runs once per workgroup from a cold instruction cache: round 4
        // measured +0.3 us from the barrier to "flags seen" and +0.35 us over the merge for a tail with loops over head masks
        // and kernel arguments read here): poll, merge; what happens when a helper's patience runs out, and the primary's
        // extra heads, sit behind unlikely branches.
        int state = 0;      // 0 = not polled, 1 = every flag seen, 2 = fault, 3 = gave up
        for (int g = km + (wave >> 2) * nm; g < G; g += 2 * nm) {
            if (state == 0) {
                // a helper's patience: ~30 us of polls (test modes: none); the primary's: the fault bound
                const int bound = primary ? (1 << 20) : (tt ? 0 : 48);
                state = 2;
                for (int spin = 0; spin < bound; ++spin) {
                    const unsigned f = __builtin_amdgcn_raw_buffer_load_b32(rf, fo, 0, 16);
                    if (__all(f == want)) { state = 1; break; }
                    __builtin_amdgcn_s_sleep(1);
                }
                if (__builtin_expect(state != 1 && !primary, 0)) {
                    // out of patience (this WAVE: the decision needs no barrier).  An atomic OR of bit km into the ticket word:
                    // if it returns an incomplete count the primary's ticket comes later and returns the bit - leave; if the
                    // count is complete every workgroup is resident and the flags will come - poll on to the fault bound and
                    // merge (the primary may have seen a bit another wave of this workgroup set: it then merges the head as
                    // well, same values).  A bit set after the primary's clear survives into the next launch and costs its
                    // primary one merge more, nothing else.  Test mode 1: the bits were all set in the prologue.
                    unsigned old = 0;
                    if (tt != 1 && lane == 0) old = __hip_atomic_fetch_or(tail_rec(p, bh) + 2, 1u << km, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
                    old = (unsigned)__builtin_amdgcn_readfirstlane((int)old);
                    if (tt == 1 || (((old >> 8) - (unsigned)tl[6]) & 0xffffffu) < (unsigned)ns) state = 3;
                    else
                        for (int spin = 0; spin < (1 << 20); ++spin) {
                            const unsigned f = __builtin_amdgcn_raw_buffer_load_b32(rf, fo, 0, 16);
                            if (__all(f == want)) { state = 1; break; }
                            __builtin_amdgcn_s_sleep(1);
                        }
                }
                MILLION_STAMP(p, 11);
                if (state == 3) break;
                if (__builtin_expect(state == 2, 0) && lane == 0) atomicAdd(&g_tail_faults, 1u);      // this wave's outputs are written as NaN
            }
            tail_merge_head<DD, LSE>(p, b, hk, g, wave & 3, ns, src, lane, state == 2);
        }
        // the primary also merges the heads of the helpers that gave up before it took its index (bits of its own ticket):
        // heads h, h + nm, ... of helper h, the same four-waves-per-head split
        const unsigned gave = primary ? (unsigned)tl[5] & ((1u << (nm - 1)) - 1u) : 0u;
        if (__builtin_expect(gave != 0, 0)) {
            if (state == 0) {      // waves 4-7 of a primary with one head of its own have not polled yet
                state = 2;
                for (int spin = 0; spin < (1 << 20); ++spin) {
                    const unsigned f = __builtin_amdgcn_raw_buffer_load_b32(rf, fo, 0, 16);
                    if (__all(f == want)) { state = 1; break; }
                    __builtin_amdgcn_s_sleep(1);
                }
                if (state == 2 && lane == 0) atomicAdd(&g_tail_faults, 1u);
            }
            int pos = 0;
            for (int h = 0; h < nm - 1; ++h)
                if (gave >> h & 1u)
                    for (int g = h; g < G; g += nm) {
                        if ((pos & 1) == (wave >> 2)) tail_merge_head<DD, LSE>(p, b, hk, g, wave & 3, ns, src, lane, state == 2);
                        ++pos;
                    }
        }
    }
    if (idx == ns - 1 && tid == 0) {
        // the workgroup that arrived last: its wave 0 has seen every flag of this launch (or ns == 1), so every workgroup of
        // this (b, kv head) has read the census line and the generation and stored its partial
        unsigned *rec = tail_rec(p, bh);
        __hip_atomic_fetch_and(rec + 2, ~0xffu, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);      // give-up bits off; the count stays
        __hip_atomic_store(rec + 4, ((unsigned)tl[6] + (unsigned)ns) & 0xffffffu, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        __hip_atomic_store(rec + 3, want, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    }
#if !(MILLION_EXP & 64)
    // the answer of the second-level ticket (requested in front of the merge): the primary that took the request's last one
    // puts the ticket word back to rest and bumps the raw r - a store and an add that returns nothing: nobody waits for either
    if (adv_wave) {
        if (lane == 0 && adv_mine && adv_t2 == p.nh_k - 1) {
            __hip_atomic_store(p.ws_cnt2 + b, 0, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            (void)__hip_atomic_fetch_add(p.dev_lengths_w + b * 4 + 1, 1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        }
        MILLION_STAMP(p, 15);
    }
#endif
    if (idx == ns - 1 && wave == 0) {      // census line back to zero, behind this wave's own poll (write-through: the next launch may run anywhere)
        __amdgpu_buffer_rsrc_t rc = __builtin_amdgcn_make_buffer_rsrc((void *)(tail_flags(p, bh) + kFlagWords), 0, kFlagWords * 4, 0x00020000);
        __builtin_amdgcn_raw_buffer_store_b32(0u, rc, lane * 4, 0, 16 /* sc1 */);
    }
    MILLION_STAMP(p, 6);
    if (dbg_on && lane < kStampSlots) {              // copy this wave's LDS stamps out (slots it wrote)
        const unsigned long long v =
            *(volatile __attribute__((address_space(3))) unsigned long long *)(size_t)(kStampOff + (wave * kStampSlots + lane) * 8);
        if (v) p.dbg[(((long long)blockIdx.y * gridDim.x + blockIdx.x) * kStampWaves + wave) * kStampSlots + lane] = v;
    }
#undef STAMP
}
