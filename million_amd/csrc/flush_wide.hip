// flush_wide.hip — the window flush of a paged cache with 9 .. 12-bit codes in one encode launch (million_pq_flush_wide), for
// uint16 pages and packed pages, gfx950.
//
// million_pq_flush (encode.hip) is uint8-only; a wide cache flushed with two million_pq_encode launches, in which a wave scans
// 4 subspaces x C centroids one after the other (64 waves per side at M = 32: 16 384 dependent tests each at C = 4096), with T
// and the ring start taken from the host.  Here the oldest n rows of every request's K and V ring window become tokens
// [T, T + n) of its pages in ONE launch that reads {T, r, start} on the device (load_len_row: clamped, never trusted) and skips
// the requests with r < min_r, followed by a one-thread-per-request launch that advances the rows of those that flushed:
// stream order is all the ordering there is (the pattern of million_pq_store_ragged: no ticket, no atomics, no polls).
//
// Mapping.  A workgroup = (block of 64 tokens, side, kv head, group of 4 consecutive subspaces), 16 waves: wave = (subspace of
// the group, quarter of the centroid range), lane = token.  The four subspaces of a token meet in one workgroup because a packed
// page keeps the high bits of 4 (hb = 2) or 2 (hb = 4) consecutive subspaces of a token in one byte: wave 0 gathers the 16
// candidates of its token through LDS and stores them with store_codes4_wide (code_pages.h), as every writer of wide pages does
// - every byte written belongs to one token, all stores are plain vector stores.
// A wave never scans more than C / 4 centroids, and it never reads the fp16 row through the scalar cache: it stages its quarter
// chunk by chunk (128 centroids: one 8- or 16-byte vector load per lane, issued one chunk ahead, widened to fp32 by all 64 lanes
// at once) in 2 KiB of LDS of its own and reads it back with wave-uniform (broadcast) ds_reads - pq_scan_lds_chunk (pq_scan.h):
// d_m + 2 d_m - 1 + 3 vector instructions per test, the conversions paid once per 64 tests.  Own chunk, own wave: LDS order
// suffices, no workgroup barrier before the one in front of the gather.  LDS: 16 x 2 KiB + 8 KiB of candidates = 40 KiB.
// No load sits in a lane-conditional: dead lanes (t >= n, a token past the table) read a clamped row and a clamped page-table
// entry and drop their store; the next chunk's load is clamped to the last chunk.  A block whose first token lies past the
// table, and every workgroup of a request that takes no part, leaves before its first vector load and before any barrier.
// Codes are those of million_pq_encode / million_pq_encode_packed bit for bit: the same IEEE operations in the same order per
// (row, centroid), strict '<' over increasing c within a quarter, quarters combined in centroid order.
//
// Several layers, and encode-ahead (million_pq_flush_wide_layers).  The layers of a cache lie side by side (windows, page tables,
// length rows: a stride each; pools and codebooks shared), grid z covers the (layer, request, kv head, side) units, and the body
// above - flush_wide_unit, templated on the number of centroid parts - has two more instances behind one kernel with a unit loop:
//   * PARTS = 4, advance = 1: the 16-wave workgroup above, every unit in the grid, then ONE advance launch with a thread per
//     (layer, request).  A flush the attention waits for: it may own the CUs.
//   * PARTS = 1, advance = 0 (encode-ahead): the rows become tokens [T, T + n) and nothing else changes - no advance launch, no
//     write to dev_lengths; min_r then means "rows present".  This form runs BESIDE a step's wide attention launches, as
//     pq_flush_kernel (encode.hip) runs beside the 8-bit ones, so it is a 4-wave workgroup, one wave per SIMD: wave = one of the
//     group's four subspaces, scanning that subspace's WHOLE centroid range chunk by chunk through its own 2 KiB of LDS - one
//     running (best, best_c) under strict '<' over increasing c, which is by construction what the four quarters combined in
//     centroid order give.  The four waves still meet in wave 0 for the packed high byte.  LDS: 4 x 2 KiB + 1 KiB of candidates.
//     Only `pairs_in_flight` (layer, request) pairs are in the grid; the workgroups walk the others (zi += gridDim.z), a
//     workgroup barrier between two units (the candidates of the last unit are read by wave 0 while the others would write the
//     next).  A unit that takes no part is left by every wave alike, before its first vector load and before any barrier.
//     While the attention launches of the step run, they append a row and add 1 to r of the rows this kernel reads: T and the ring
//     start do not move in a step without a flush, r only grows past min_r, and the rows encoded here are the oldest ones, which the
//     append never touches - so either value of r gives the same codes in the same bytes.
// Register budget beside attn_wide_kernel (8 waves per workgroup, 2 per SIMD; -Rpass-analysis=kernel-resource-usage, ROCm 7.2).
// d = 128: 198 .. 206 VGPRs at d_m = 2, 167 .. 175 at d_m = 4, allocated in eights: one attention workgroup per CU holds at most
// 2 x 208 = 416 of a SIMD's 512 registers, a second one never fits, and 96 stay free: an encode-ahead wave of <= 96 VGPRs (the
// instances here: 67 at d_m = 2, 63 at d_m = 4 - 72 and 64 allocated; no scratch, no spills) sits on every SIMD beside the attention
// waves, and a new attention workgroup (416) still fits while it is resident (72 + 416 <= 512); a second encode-ahead workgroup on
// the CU (2 x 64 > 96) would hold registers the next attention workgroup needs - hence about one workgroup per CU in flight.
// LDS: ~50 KiB + 5 KiB (d_m = 2) or 9 KiB (d_m = 4) of 160.  d = 64: the attention kernel takes
// 104 .. 121 VGPRs and TWO workgroups per CU (4 waves per SIMD): 4 x 120 = 480 at best, 4 x 128 = 512 for the packed d_m = 2
// instances - the register file is full or 32 short of an encode-ahead wave, which there waits for an attention workgroup to leave
// and takes the place of the next one for its duration.
#include "code_pages.h"
#include "pq_scan.h"

#pragma clang fp contract(off)

namespace million {

constexpr int kFwSub = 4;          // subspaces per workgroup
constexpr int kFwParts = 4;        // parts of the centroid range
constexpr int kFwWaves = kFwSub * kFwParts;
constexpr int kFwChunk = 128;      // centroids a wave stages at a time (C / kFwParts is a multiple: C >= 512)

struct FlushWideParams {
    const f16 *k_rows, *v_rows;       // windows (bs, nh_k, rcap, d)
    const f16 *k_cents, *v_cents;     // (M, C, d_m) fp16
    uint8_t *k_pool, *v_pool;
    const int *page_ids;              // (bs, nh_k, n_pages_cap)
    const int *dev_lengths;           // (bs, 4) or null: tok0 / xrow_start
    long long xsb, xsh, xsn;
    int bs, nh_k, n, M, C;
    int rcap, min_r;
    int tok0, xrow_start;
    int page_size, ps_shift, n_pages_cap, cap_tok;
    int packed;
    // million_pq_flush_wide_layers: element strides between the layers' windows, page tables and length rows; one layer: 0
    long long x_ls, ids_ls, len_ls;
    int n_layers;
};

// One unit = (layer, request, kv head, side) of one workgroup (token block blockIdx.x, subspace group blockIdx.y); PARTS = parts of
// the centroid range = waves per subspace.  layer is 0 (a literal) in the one-layer kernel.  A `return` here ends the unit.
// page_size and M are p's as the store at the end takes them (see pq_flush_wide_layers_kernel).
template <int DM, int PARTS>
__device__ __forceinline__ void flush_wide_unit(const FlushWideParams &p, const bool vside, const int layer, const int b, const int hk,
                                                const int page_size, const int M) {
    typedef f16 hvec __attribute__((ext_vector_type(DM)));
    typedef f16 hvec2 __attribute__((ext_vector_type(2 * DM)));
    __shared__ __attribute__((aligned(16))) float rows[kFwSub * PARTS][kFwChunk * DM];
    __shared__ float cand_d[kFwSub][PARTS][64];
    __shared__ int cand_c[kFwSub][PARTS][64];
    const int lane = threadIdx.x & 63;
    const int w = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
    const int s = w & (kFwSub - 1), part = w / kFwSub;
    const int m0 = blockIdx.y * kFwSub;
    const int bh = b * p.nh_k + hk;
    int T = p.tok0, st = p.xrow_start;
    if (p.dev_lengths) {
        // through the constant address space: T and the start are not written while this kernel runs (the advance is the next
        // launch; a decode step beside an encode-ahead launch moves r alone, see the header)
        typedef const __attribute__((address_space(4))) int *const_p;
        int r;
        load_len_row((const_p)(p.dev_lengths + layer * p.len_ls + 4 * b), p.cap_tok, p.rcap, p.rcap, T, r, st);
        if (r < p.min_r) return;      // the request takes no part: nothing of it is read beyond the row
    }
    // 0 <= T <= cap_tok (clamped, or checked by the host): no sum below can wrap (cap_tok + page_size fits an int, host check)
    const int j0 = blockIdx.x * 64;
    if (T + j0 >= p.cap_tok) return;      // every token of the block lies past the table
    const int t = j0 + lane;
    const bool valid = t < p.n;
    const int tc = valid ? t : p.n - 1;
    float x[DM];
    {
        const f16 *xp = (vside ? p.v_rows : p.k_rows) + layer * p.x_ls + b * p.xsb + hk * p.xsh + (long long)((st + tc) % p.rcap) * p.xsn + (m0 + s) * DM;
        const hvec xv = *(const hvec *)xp;
#pragma unroll
        for (int k = 0; k < DM; ++k) x[k] = (float)xv[k];
    }
    // destination: token T + tc.  The page index of a dead or dropped lane is clamped to a page that receives a token of this
    // block (the block's first token lies inside the table)
    const int tok = T + tc;
    const int page = tok >> p.ps_shift;
    const bool keep = valid && page < p.n_pages_cap;
    const long long pid = p.page_ids[layer * p.ids_ls + (long long)bh * p.n_pages_cap + (page < p.n_pages_cap ? page : p.n_pages_cap - 1)];

    // this wave's quarter of the subspace's centroids, chunk by chunk through its own LDS
    const f16 *tab = (vside ? p.v_cents : p.k_cents) + (long long)(m0 + s) * p.C * DM;
    const int cq = p.C / PARTS;
    const int c0 = part * cq, nch = cq / kFwChunk;
    float *mine = rows[w];
    float best = INFINITY;
    int best_c = c0;
    hvec2 nxt = *(const hvec2 *)(tab + (long long)(c0 + 2 * lane) * DM);      // lane: centroids c0 + 2 lane, + 1
    for (int ch = 0; ch < nch; ++ch) {
        const int cb = c0 + ch * kFwChunk;
        const hvec2 cur = nxt;
        const int cn = ch + 1 < nch ? cb + kFwChunk : cb;      // clamped, not predicated
        nxt = *(const hvec2 *)(tab + (long long)(cn + 2 * lane) * DM);
#pragma unroll
        for (int k = 0; k < 2 * DM; ++k) mine[2 * lane * DM + k] = (float)cur[k];
        __builtin_amdgcn_wave_barrier();
        pq_scan_lds_chunk<DM, (DM <= 2 ? 16 : 8)>(x, mine, kFwChunk, cb, best, best_c);
        __builtin_amdgcn_wave_barrier();
    }
    if constexpr (PARTS > 1) cand_d[s][part][lane] = best;
    cand_c[s][part][lane] = best_c;
    __syncthreads();
    if (w != 0 || !keep) return;
    // wave 0, lane = token: the parts of each subspace in centroid order, strict '<': the lowest index wins exact ties
    unsigned c4[kFwSub];
#pragma unroll
    for (int j = 0; j < kFwSub; ++j) {
        int bc = cand_c[j][0][lane];
        float bd = PARTS > 1 ? cand_d[j][0][lane] : 0.f;
#pragma unroll
        for (int q = 1; q < PARTS; ++q) {
            const float dj = cand_d[j][q][lane];
            const int cj = cand_c[j][q][lane];
            bc = dj < bd ? cj : bc;
            bd = fminf(bd, dj);
        }
        c4[j] = (unsigned)bc;
    }
    store_codes4_wide(vside ? p.v_pool : p.k_pool, pid, tok & (page_size - 1), m0, c4, vside, page_size, M, p.C, p.packed);
}

template <int DM>
__global__ __launch_bounds__(kFwWaves * 64) void pq_flush_wide_kernel(FlushWideParams p) {
    const int bh = blockIdx.z >> 1;
    flush_wide_unit<DM, kFwParts>(p, blockIdx.z & 1, 0, bh / p.nh_k, bh % p.nh_k, p.page_size, p.M);      // the side is workgroup-uniform
}

// The layered forms: grid z holds every unit (advance: PARTS = 4) or the units of the pairs in flight, whose workgroups walk the
// other pairs (encode-ahead: PARTS = 1).  blockIdx.z = (pair in flight * nh_k + hk) * 2 + side with pair = layer * bs + b, and
// gridDim.z = pairs in flight * 2 nh_k: a workgroup keeps its head and side (and with them its window, codebook and pool) and
// walks pairs.  The barrier keeps a unit's candidates until wave 0 has read them.  The store's address terms are functions of
// (page_size, M, C, blockIdx.y) alone; hoisted out of the loop they are held in SGPRs across the scan and the d_m = 2 instances
// spill 8 of them (ROCm 7.2), so the page size and M reach the store as values the compiler cannot follow.
template <int DM, int PARTS>
__global__ __launch_bounds__(kFwSub * PARTS * 64) void pq_flush_wide_layers_kernel(FlushWideParams p) {
    const int per = 2 * p.nh_k, hs = blockIdx.z % per;
    const int pairs = p.n_layers * p.bs, step = gridDim.z / per;
    for (int zi = blockIdx.z / per; zi < pairs; zi += step) {
        int page_size = p.page_size, M = p.M;
        asm volatile("" : "+s"(page_size), "+s"(M));
        flush_wide_unit<DM, PARTS>(p, hs & 1, zi / p.bs, zi % p.bs, hs >> 1, page_size, M);
        __syncthreads();
    }
}

// The rows of a request that flushed (the same clamped r >= min_r) move on - T += n, r -= n, start = (start + n) % rcap, no sum or
// difference able to wrap; word 3 is not touched.
__device__ __forceinline__ void flush_wide_advance_row(int *row, int n, int cap_tok, int rcap, int min_r) {
    int T, r, st;
    load_len_row((const int *)row, cap_tok, rcap, rcap, T, r, st);
    if (r < min_r) return;
    row[0] = T > cap_tok - n ? cap_tok : T + n;
    row[1] = r < n ? 0 : r - n;
    row[2] = (int)(((unsigned)st + (unsigned)n) % (unsigned)rcap);
}

// One thread per request, after the encode launch on the same stream
__global__ void flush_wide_advance_kernel(int *dev_lengths, int bs, int n, int cap_tok, int rcap, int min_r) {
    const int b = blockIdx.x * blockDim.x + threadIdx.x;
    if (b >= bs) return;
    flush_wide_advance_row(dev_lengths + 4 * b, n, cap_tok, rcap, min_r);
}

// ... per (layer, request): ONE launch for the layers of million_pq_flush_wide_layers
__global__ void flush_wide_advance_layers_kernel(int *dev_lengths, long long len_ls, int n_layers, int bs, int n, int cap_tok, int rcap, int min_r) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n_layers * bs) return;
    flush_wide_advance_row(dev_lengths + (i / bs) * len_ls + 4 * (i % bs), n, cap_tok, rcap, min_r);
}

}  // namespace million

using namespace million;

namespace {

struct FlushWideLayers { int n_layers; long long x_ls, ids_ls, len_ls; };      // one layer: {1, 0, 0, 0}

// The checks of both entries, in one order (shape and argument errors before any look at a pointer's value), and the kernel
// parameters.  true: launch; false: return rc (an error, or MILLION_OK: nothing to flush).
bool flush_wide_front(const char *who, const million_encode_desc *desc, const void *k_rows, const void *v_rows, const void *k_cents,
                      const void *v_cents, void *k_pool, void *v_pool, const int32_t *page_ids, int32_t *dev_lengths, int resid_cap,
                      int min_r, int packed, const FlushWideLayers &ly, int pairs_in_flight, FlushWideParams &p, int &rc) {
    rc = MILLION_ERR_ARG;
    if (!desc || desc->struct_size != sizeof(million_encode_desc)) { set_error("%s: bad desc / struct_size", who); return false; }
    const million_encode_desc &d = *desc;
    rc = MILLION_ERR_SHAPE;
    if (d.bs <= 0 || d.nh_k <= 0 || d.n < 0 || ly.n_layers < 0) { set_error("%s: bs=%d nh_k=%d n=%d n_layers=%d", who, d.bs, d.nh_k, d.n, ly.n_layers); return false; }
    if (!wide_geometry(d.d, d.M, d.C, 1) || (packed && d.M % 4)) {
        set_error("%s: d=%d M=%d C=%d (d 64 / 128, d / M 2 or 4, C 512 / 1024 / 2048 / 4096; packed pages: M a multiple of 4)", who, d.d, d.M, d.C);
        return false;
    }
    int ps_shift;
    if (!page_shift(who, d.page_size, ps_shift)) return false;
    if (d.n > d.page_size) { set_error("%s: n=%d exceeds page_size=%d", who, d.n, d.page_size); return false; }
    if (d.n_pages_cap <= 0 || (long long)d.n_pages_cap * d.page_size + d.page_size > 0x7fffffffLL || (long long)d.bs * d.nh_k * d.n_pages_cap > 0x7fffffffLL) {
        set_error("%s: n_pages_cap=%d (page table of %lld entries)", who, d.n_pages_cap, (long long)d.bs * d.nh_k * d.n_pages_cap);
        return false;
    }
    if ((long long)(ly.n_layers > 1 ? ly.n_layers : 1) * d.bs * d.nh_k * 2 > 65535) {
        set_error("%s: n_layers * bs * nh_k = %lld exceeds the grid (32767)", who, (long long)(ly.n_layers > 1 ? ly.n_layers : 1) * d.bs * d.nh_k);
        return false;
    }
    rc = MILLION_ERR_ARG;
    if (d.dst_layout != MILLION_CODES_KPAGES) { set_error("%s: dst_layout must be MILLION_CODES_KPAGES (the V side is written as VPAGES)", who); return false; }
    if (resid_cap <= 0 || resid_cap < d.n || d.x_row_mod != resid_cap) {
        set_error("%s: resid_cap=%d (> 0, >= n = %d, and desc->x_row_mod = %d must equal it)", who, resid_cap, d.n, d.x_row_mod);
        return false;
    }
    if ((const int32_t *)dev_lengths != d.dev_lengths) { set_error("%s: dev_lengths must equal desc->dev_lengths (or both null)", who); return false; }
    if (min_r < 0 || min_r > resid_cap) { set_error("%s: min_r=%d outside [0, resid_cap]", who, min_r); return false; }
    if (pairs_in_flight < 0) { set_error("%s: pairs_in_flight=%d (0: the library's rule)", who, pairs_in_flight); return false; }
    const int cap_tok = d.n_pages_cap * d.page_size;
    if (!dev_lengths) {
        if (d.dst_token_start < 0 || (long long)d.dst_token_start + d.n > cap_tok) { set_error("%s: dst_token_start=%d, page table too short", who, d.dst_token_start); return false; }
        if (d.x_row_start < 0 || d.x_row_start >= resid_cap) { set_error("%s: x_row_start=%d outside [0, resid_cap)", who, d.x_row_start); return false; }
    }
    rc = MILLION_OK;
    if (d.n == 0 || ly.n_layers == 0) return false;      // nothing to flush, whatever the pointers
    rc = MILLION_ERR_ARG;
    if (!k_rows || !v_rows || !k_cents || !v_cents || !k_pool || !v_pool || !page_ids) { set_error("%s: null rows / codebooks / pools / page_ids", who); return false; }
    rc = MILLION_ERR_ALIGN;
    if (((uintptr_t)k_rows | (uintptr_t)v_rows | (uintptr_t)k_cents | (uintptr_t)v_cents | (uintptr_t)k_pool | (uintptr_t)v_pool) & 15) {
        set_error("%s: rows, codebooks and pools must be 16-byte aligned", who);
        return false;
    }
    if (((uintptr_t)page_ids | (uintptr_t)dev_lengths) & 3) { set_error("%s: page_ids / dev_lengths must be 4-byte aligned", who); return false; }
    if ((d.x_stride_b | d.x_stride_h | d.x_stride_n | ly.x_ls) & 7) { set_error("%s: fp16 strides must be multiples of 8 elements (16-byte rows)", who); return false; }
    p.k_rows = (const f16 *)k_rows; p.v_rows = (const f16 *)v_rows;
    p.k_cents = (const f16 *)k_cents; p.v_cents = (const f16 *)v_cents;
    p.k_pool = (uint8_t *)k_pool; p.v_pool = (uint8_t *)v_pool;
    p.page_ids = page_ids; p.dev_lengths = dev_lengths;
    p.xsb = d.x_stride_b; p.xsh = d.x_stride_h; p.xsn = d.x_stride_n;
    p.bs = d.bs; p.nh_k = d.nh_k; p.n = d.n; p.M = d.M; p.C = d.C;
    p.rcap = resid_cap; p.min_r = min_r;
    p.tok0 = d.dst_token_start; p.xrow_start = d.x_row_start;
    p.page_size = d.page_size; p.ps_shift = ps_shift; p.n_pages_cap = d.n_pages_cap; p.cap_tok = cap_tok;
    p.packed = packed ? 1 : 0;
    p.x_ls = ly.x_ls; p.ids_ls = ly.ids_ls; p.len_ls = ly.len_ls; p.n_layers = ly.n_layers;
    rc = MILLION_OK;
    return true;
}

int flush_wide_launched(const char *who, const char *what) {
    const hipError_t e = hipGetLastError();
    if (e == hipSuccess) return MILLION_OK;
    set_error("%s %slaunch: %s", who, what, hipGetErrorString(e));
    return MILLION_ERR_LAUNCH;
}

}  // namespace

extern "C" int million_pq_flush_wide(const million_encode_desc *desc, const void *k_rows, const void *v_rows, const void *k_cents,
                                     const void *v_cents, void *k_pool, void *v_pool, const int32_t *page_ids, int32_t *dev_lengths,
                                     int resid_cap, int min_r, int packed, million_stream_t stream) {
    FlushWideParams p;
    int rc;
    if (!flush_wide_front("flush_wide", desc, k_rows, v_rows, k_cents, v_cents, k_pool, v_pool, page_ids, dev_lengths, resid_cap, min_r, packed,
                          {1, 0, 0, 0}, 0, p, rc)) return rc;
    const dim3 grid((p.n + 63) / 64, p.M / kFwSub, p.bs * p.nh_k * 2);
    hipStream_t s = (hipStream_t)stream;
    if (desc->d / p.M == 2) hipLaunchKernelGGL(pq_flush_wide_kernel<2>, grid, dim3(kFwWaves * 64), 0, s, p);
    else hipLaunchKernelGGL(pq_flush_wide_kernel<4>, grid, dim3(kFwWaves * 64), 0, s, p);
    if ((rc = flush_wide_launched("flush_wide", "")) != MILLION_OK || !dev_lengths) return rc;      // host lengths: nothing to advance
    hipLaunchKernelGGL(flush_wide_advance_kernel, dim3((p.bs + 63) / 64), dim3(64), 0, s, dev_lengths, p.bs, p.n, p.cap_tok, resid_cap, min_r);
    return flush_wide_launched("flush_wide", "advance ");
}

extern "C" int million_pq_flush_wide_layers(const million_encode_desc *desc, const void *k_rows, const void *v_rows, const void *k_cents,
                                            const void *v_cents, void *k_pool, void *v_pool, const int32_t *page_ids, int32_t *dev_lengths,
                                            int resid_cap, int min_r, int n_layers, int64_t rows_layer_stride, int64_t ids_layer_stride,
                                            int64_t lengths_layer_stride, int advance, int packed, int pairs_in_flight,
                                            million_stream_t stream) {
    const char *const who = "flush_wide_layers";
    FlushWideParams p;
    int rc;
    if (!flush_wide_front(who, desc, k_rows, v_rows, k_cents, v_cents, k_pool, v_pool, page_ids, dev_lengths, resid_cap, min_r, packed,
                          {n_layers, rows_layer_stride, ids_layer_stride, lengths_layer_stride}, pairs_in_flight, p, rc)) return rc;
    const int tblocks = (p.n + 63) / 64, groups = p.M / kFwSub, pairs = n_layers * p.bs;
    const bool dm2 = desc->d / p.M == 2;
    hipStream_t s = (hipStream_t)stream;
    if (advance) {
        // a flush the attention waits for: every unit in the grid, the 16-wave workgroup
        const dim3 grid(tblocks, groups, pairs * p.nh_k * 2);
        if (dm2) hipLaunchKernelGGL((pq_flush_wide_layers_kernel<2, kFwParts>), grid, dim3(kFwWaves * 64), 0, s, p);
        else hipLaunchKernelGGL((pq_flush_wide_layers_kernel<4, kFwParts>), grid, dim3(kFwWaves * 64), 0, s, p);
        if ((rc = flush_wide_launched(who, "")) != MILLION_OK || !dev_lengths) return rc;      // host lengths: nothing to advance
        hipLaunchKernelGGL(flush_wide_advance_layers_kernel, dim3((pairs + 63) / 64), dim3(64), 0, s, dev_lengths, p.len_ls, n_layers, p.bs, p.n,
                           p.cap_tok, resid_cap, min_r);
        return flush_wide_launched(who, "advance ");
    }
    // encode-ahead: the 4-wave workgroup, (layer, request) pairs in flight as given, or launch_flush's rule (encode.hip): as many as
    // keep about ONE workgroup per CU in flight - what fits beside an attention workgroup (the file header); the workgroups walk
    // the remaining pairs
    int gz = pairs_in_flight;
    if (gz == 0) gz = (int)(device_cus() / ((long long)tblocks * groups * p.nh_k * 2));
    gz = gz < 1 ? 1 : gz > pairs ? pairs : gz;
    const dim3 grid(tblocks, groups, gz * p.nh_k * 2);
    if (dm2) hipLaunchKernelGGL((pq_flush_wide_layers_kernel<2, 1>), grid, dim3(kFwSub * 64), 0, s, p);
    else hipLaunchKernelGGL((pq_flush_wide_layers_kernel<4, 1>), grid, dim3(kFwSub * 64), 0, s, p);
    return flush_wide_launched(who, "");
}
