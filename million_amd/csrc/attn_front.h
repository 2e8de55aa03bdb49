// attn_front.h - the launch front of the decode MFMA kernels: which workgroup a (b, kv head, split) is, what a wave of it
// reads, what may be read past T, and who appends.  Included by attn_mfma.hip (inside namespace million, behind attn_tail.h, in
// front of attn_stream.h and attn_lean.h).  This contract must agree with the planner (plan_attn_mfma: grid, nsplit, the 64
// rounds a wave preloads ids for, virtual kv heads) and with the workspace layout (million_api.hip); it is written here once.
//
// The steps are statement macros, not functions: they declare the wave-uniform values below as plain locals of the kernel, so
// both kernels compile the text they compiled when each carried its own copy (every instance keeps its registers and spills:
// profiles/ab_decode_front.txt; the same steps as functions over a struct, or over locals passed by reference, reach hipcc's
// early passes as memory and moved the scalar allocation of 28 of 32 instances).  A kernel expands them in the order in which
// the loads must be issued - the CU's load path takes ~28 cycles per 1-KiB wave request, in order: what is requested first is
// there first:
//     LAUNCH_FRONT_PLACE | (LDS base check, stamps) | LAUNCH_FRONT_PAGE_IDS | (the kernel's own query operand; lean kernel: ONE
//     request of wave 0 for the workgroup's query rows, which go to LDS with the codebook images) |
//     LAUNCH_FRONT_NEW_ROW_AND_TABLES | LAUNCH_FRONT_LENGTHS | ... LDS images, barrier ... | LAUNCH_FRONT_APPEND_STORE
// They expect the kernel's p (AttnParams), tid, lane, wave and kNW / kResRows, and leave:
//   split, bh, b, hk        hk, bh: VIRTUAL when the launch splits the query heads of a kv head into parts
//   part, hkr, bhr          this workgroup's part; the REAL kv head / pair: what codes, page ids, window rows and new rows are indexed by
//   G                       query heads of this workgroup (the last part of an odd head group holds fewer than p.G)
//   k_paged, v_ident, ids64 the layout, by MODE: 0: K and V paged, int32 ids (PagedPQCache).  1: row-major K, V in dense scratch
//                           pages (the reference's 10-arg layout after the transpose).  2: anything else, by run-time flags
//   pg0, pg_step, tin       the wave reads page pg0 + j * pg_step in round j, tokens [tin, tin + (1 << UL)) of it
//   vpk, vpv                page ids of rounds 0..63 (lane = round)
//   append_wave, new_k, new_v   the wave that stores the call's new K / V row into the window (fused append), and the row
//   tabk[NT], tabv[NT], rot the codebook pieces of this thread, rotated so that workgroups start on different channels
//   T, r_old, rstart, r     context length, window rows before / after the append, first window row (clamped: clamp_lengths)
//   t0, t_step              first token of round 0, tokens between rounds
//   n_mine, j_last, T_ld    rounds (= units) of this wave (host: <= 64), the last of them (or 0), max(T, 1)
//   rcnt, has_res, kr, vr   window rows of this split, whether this wave has some (load_res_tile), the window of (b, real kv head)
// The differences between the kernels are compile-time arguments (no run-time branch on "which kernel": this code runs from a
// cold instruction cache and every branch of it is on the launch's critical path, see attn_lean.h on FL):
//   UL     log2 of the tokens of a unit: 5 (streaming kernel) or 6 (lean kernel)
//   DR     f16 per row of the window and of the new K / V row: d (a wave's 64 lanes carry two each: 2 * lane < DR guards the row)
//   PARTS  the instance carries the code for query-head parts (AttnParams::nhk_real)
//
// Units are dealt to (split, wave) by PAGE, strided: page (j * ppr + wave / upp) * nsplit + split goes to round j of the wave
// (upp = units per page, ppr = 8 / upp pages per workgroup and round), so where a wave reads does not depend on the context
// length T - only HOW MANY units it has does.  A page is never shared between workgroups, so rows past T - 1 of the last unit
// stay inside an allocated page: no row clamping on paged K.  A request for a round past a wave's last unit re-requests that unit
// (LAUNCH_FRONT_ROUND: L2 hits, never consumed), so that no code load sits in a conditional.  Such a request still takes its
// ~28 cycles per wave request of the CU's in-order load path, so a loop should not issue it where it can know better: the lean
// kernel's last block requests nothing (attn_lean.h: BLOCK_LAST; its only clamped requests are the prologue's round 1 in waves
// with fewer than two units); the streaming kernel's blocks still re-request.

// C = 128: the V col image is written to LDS a second time kVDup128 bytes above the first (code c at kVBase + 256 c in every
// form), where the code bytes 128 .. 255 of masked tokens land (the gathers take the byte unmasked): they gather row c - 128, a
// finite centroid times probability 0 - not an unwritten LDS word, which may be NaN (0 x NaN = NaN in the value MFMA).  An AND
// of every V code word with 0x7f7f7f7f does the same in the loop; the copy costs NT / 2 stores in the prologue only.  (K: the
// second half of a row is read only by code bytes >= 128 - tokens past T, never valid ones - and such scores are masked by a
// select.)  Each kernel's LDS image writer applies it to its own image (dense: streaming kernel; spread or padded: lean).
constexpr unsigned kVDup128 = 32768u;

// 1. Workgroup i of a grid lands on XCD i % 8 (tools/micro/xcc_map.hip).  With a multiple of 8 (b, kv head) pairs the pairs are
// dealt over the linear id first, so ALL splits of a pair run on one XCD and the last arriver can read the partials through its
// own L2 (attn_tail.h checks the placement at run time, it is never assumed).  (dl: the host's lengths, see step 4.)
#define LAUNCH_FRONT_PLACE(MODE, PARTS)                                                                                            \
    int split = blockIdx.x, bh = blockIdx.y;                                                                                       \
    if ((gridDim.y & 7) == 0) {                                                                                                    \
        const int id = blockIdx.y * gridDim.x + blockIdx.x;                                                                        \
        bh = id % (int)gridDim.y;                                                                                                  \
        split = id / (int)gridDim.y;                                                                                               \
    }                                                                                                                              \
    const int b = bh / p.nh_k, hk = bh % p.nh_k;                                                                                   \
    const int part = (PARTS) ? head_part(p, hk) : 0, hkr = hk - part * p.nhk_mul;                                                  \
    const int bhr = (PARTS) ? bh - (b * p.hparts_m1 + part) * p.nhk_mul : bh;                                                      \
    const int G = (PARTS) && p.nhk_mul ? min(p.G, p.G_all - part * p.G) : p.G;                                                     \
    const bool k_paged = MODE == 0 ? true : MODE == 1 ? false : (p.k_paged != 0);                                                  \
    const bool v_ident = MODE == 0 ? false : MODE == 1 ? true : (p.v_identity != 0);                                               \
    const bool ids64 = MODE == 2 ? (p.ids64 != 0) : false;                                                                         \
    typedef int v4i __attribute__((ext_vector_type(4)));                                                                           \
    v4i dl = {p.T, p.r, p.rstart, 0};

// 2. The page ids of a wave's first 64 rounds are ONE vector load (lane = round), the oldest loads of the wave; each unit's id
// is then a v_readlane.  No scalar-cache round trip sits between the kernel start and the first code request, device-resident
// lengths included (round 1: lengths -> split range -> page ids -> codes, two dependent s_load round trips).
#ifdef MILLION_DEBUG_CHECK_IDS      // lane = round: entries of pages beyond the context (host bound) are preloaded but never used
#define LAUNCH_FRONT_CHECK_IDS()                                                                                                   \
    {                                                                                                                              \
        const bool live = pg0 + lane * pg_step < p.n_pages_cap && ((long long)(pg0 + lane * pg_step) << p.ps_shift) < p.T;         \
        if (k_paged) vpk = MILLION_CHECK_KID(p, ids64 ? (long long)p.k_ids64[idx] : (long long)vpk, live);                         \
        if (!v_ident) vpv = MILLION_CHECK_VID(p, ids64 ? (long long)p.v_ids64[idx] : (long long)vpv, live);                        \
    }
#else
#define LAUNCH_FRONT_CHECK_IDS()
#endif
#define LAUNCH_FRONT_PAGE_IDS(UL)                                                                                                  \
    const int ups = p.ps_shift - (UL);                    /* log2(units per page) */                                               \
    const int wp = wave >> ups, uw = wave & ((1 << ups) - 1);                                                                      \
    const int pg0 = wp * p.nsplit + split;                                                                                         \
    const int pg_step = p.nsplit << (3 - ups);                                                                                     \
    const int tin = uw << (UL);                                                                                                    \
    int vpk = 0, vpv = 0;                                                                                                          \
    {                                                                                                                              \
        int pgl = pg0 + lane * pg_step;                                                                                            \
        pgl = pgl < p.n_pages_cap ? pgl : p.n_pages_cap - 1;                                                                       \
        const long long idx = (long long)bhr * p.n_pages_cap + pgl;                                                                \
        if (k_paged) vpk = ids64 ? (int)p.k_ids64[idx] : p.k_ids32[idx];                                                           \
        if (v_ident) vpv = (int)idx;                                                                                               \
        else vpv = ids64 ? (int)p.v_ids64[idx] : p.v_ids32[idx];                                                                   \
        LAUNCH_FRONT_CHECK_IDS()                                                                                                   \
    }

// 3. The new row (the last wave of split 0 and part 0 appends), then both codebooks, NT 16-byte pieces of each image per thread:
// they go out before anything that depends on a length or a page id.  (Through round 2 the V codebook was requested during the
// prologue and had a barrier of its own: 18.6 -> 18.2 us at one request with it up here.)
#define LAUNCH_FRONT_NEW_ROW_AND_TABLES(DR, NT)                                                                                    \
    const bool append_wave = p.k_new && split == 0 && wave == kNW - 1 && part == 0;                                                \
    h2 new_k = {}, new_v = {};                                                                                                     \
    if (append_wave && 2 * lane < (DR)) {                                                                                          \
        new_k = *(const h2 *)(p.k_new + (long long)bhr * (DR) + 2 * lane);                                                         \
        new_v = *(const h2 *)(p.v_new + (long long)bhr * (DR) + 2 * lane);                                                         \
    }                                                                                                                              \
    v4u tabk[NT], tabv[NT];                                                                                                        \
    const int rot = (blockIdx.x + 5 * blockIdx.y) & ((NT) - 1);                                                                    \
    {                                                                                                                              \
        const v4u *ks = (const v4u *)p.k_tab;                                                                                      \
        _Pragma("unroll") for (int i = 0; i < (NT); ++i) tabk[i] = ks[((i + rot) & ((NT) - 1)) * (kNW * 64) + tid];                \
        const v4u *vs = (const v4u *)p.v_tab_col;      /* the V codebook right behind it: one barrier serves both */               \
        _Pragma("unroll") for (int i = 0; i < (NT); ++i) tabv[i] = vs[((i + rot) & ((NT) - 1)) * (kNW * 64) + tid];                \
    }

// 4. The lengths - device-resident ones by a scalar load, issued and waited for in ONE statement (decode_wave.h: the note on the
// vector-memory queue) - and what follows from them: only the masks, the round count and the window (dealt to the split's waves
// in runs of kResRows, see load_res_tile) depend on them.
#define LAUNCH_FRONT_LENGTHS()                                                                                                     \
    if (p.dev_lengths)                                                                                                             \
        asm volatile("s_load_dwordx4 %0, %1, %2\n\ts_waitcnt lgkmcnt(0)" : "=&s"(dl) : "s"(p.dev_lengths), "s"((unsigned)b * 16u) : "memory"); \
    int T = dl[0], r_old = dl[1], rstart = dl[2];                                                                                  \
    clamp_lengths(p, T, r_old, rstart);                                                                                            \
    const int r = r_old + (p.k_new ? 1 : 0);                                                                                       \
    const int t0 = (pg0 << p.ps_shift) + tin;                                                                                      \
    const int t_step = pg_step << p.ps_shift;                                                                                      \
    const int n_mine = T > t0 ? (T - t0 + t_step - 1) / t_step : 0;                                                                \
    const int j_last = n_mine > 0 ? n_mine - 1 : 0;                                                                                \
    const int T_ld = T > 0 ? T : 1;                                                                                                \
    const int rcnt = split < r ? (r - split + p.nsplit - 1) / p.nsplit : 0;                                                        \
    const bool has_res = kResRows * wave < rcnt;                                                                                   \
    const f16 *kr = p.k_res + b * p.res_sb + hkr * p.res_sh;                                                                       \
    const f16 *vr = p.v_res + b * p.res_sb + hkr * p.res_sh;

// 5. Fused append: the new token becomes window row r_old.
#define LAUNCH_FRONT_APPEND_STORE(DR)                                                                                              \
    if (append_wave && 2 * lane < (DR)) {                                                                                          \
        int row_n = rstart + r_old;                                                                                                \
        row_n = row_n >= p.rcap ? row_n - p.rcap : row_n;                                                                          \
        const long long o = b * p.res_sb + hkr * p.res_sh + (long long)row_n * (DR) + 2 * lane;                                    \
        *(h2 *)(p.k_res_w + o) = new_k;                                                                                            \
        *(h2 *)(p.v_res_w + o) = new_v;                                                                                            \
    }

// round J of this wave, or its last one
#define LAUNCH_FRONT_ROUND(J) ((J) < n_mine ? (J) : j_last)
