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
};

template <int DM>
__global__ __launch_bounds__(kFwWaves * 64) void pq_flush_wide_kernel(FlushWideParams p) {
    typedef f16 hvec __attribute__((ext_vector_type(DM)));
    typedef f16 hvec2 __attribute__((ext_vector_type(2 * DM)));
    __shared__ __attribute__((aligned(16))) float rows[kFwWaves][kFwChunk * DM];
    __shared__ float cand_d[kFwSub][kFwParts][64];
    __shared__ int cand_c[kFwSub][kFwParts][64];
    const int lane = threadIdx.x & 63;
    const int w = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
    const int s = w & (kFwSub - 1), part = w / kFwSub;
    const int m0 = blockIdx.y * kFwSub;
    const bool vside = blockIdx.z & 1;      // workgroup-uniform
    const int bh = blockIdx.z >> 1;
    const int b = bh / p.nh_k, hk = bh % p.nh_k;
    int T = p.tok0, st = p.xrow_start;
    if (p.dev_lengths) {
        // through the constant address space: the rows are not written while this kernel runs (the advance is the next launch)
        typedef const __attribute__((address_space(4))) int *const_p;
        int r;
        load_len_row((const_p)(p.dev_lengths + 4 * b), p.cap_tok, p.rcap, p.rcap, T, r, st);
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
        const f16 *xp = (vside ? p.v_rows : p.k_rows) + b * p.xsb + hk * p.xsh + (long long)((st + tc) % p.rcap) * p.xsn + (m0 + s) * DM;
        const hvec xv = *(const hvec *)xp;
#pragma unroll
        for (int k = 0; k < DM; ++k) x[k] = (float)xv[k];
    }
    // destination: token T + tc.  The page index of a dead or dropped lane is clamped to a page that receives a token of this
    // block (the block's first token lies inside the table)
    const int tok = T + tc;
    const int page = tok >> p.ps_shift;
    const bool keep = valid && page < p.n_pages_cap;
    const long long pid = p.page_ids[(long long)bh * p.n_pages_cap + (page < p.n_pages_cap ? page : p.n_pages_cap - 1)];

    // this wave's quarter of the subspace's centroids, chunk by chunk through its own LDS
    const f16 *tab = (vside ? p.v_cents : p.k_cents) + (long long)(m0 + s) * p.C * DM;
    const int cq = p.C / kFwParts;
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
    cand_d[s][part][lane] = best;
    cand_c[s][part][lane] = best_c;
    __syncthreads();
    if (w != 0 || !keep) return;
    // wave 0, lane = token: the parts of each subspace in centroid order, strict '<': the lowest index wins exact ties
    unsigned c4[kFwSub];
#pragma unroll
    for (int j = 0; j < kFwSub; ++j) {
        float bd = cand_d[j][0][lane];
        int bc = cand_c[j][0][lane];
#pragma unroll
        for (int q = 1; q < kFwParts; ++q) {
            const float dj = cand_d[j][q][lane];
            const int cj = cand_c[j][q][lane];
            bc = dj < bd ? cj : bc;
            bd = fminf(bd, dj);
        }
        c4[j] = (unsigned)bc;
    }
    store_codes4_wide(vside ? p.v_pool : p.k_pool, pid, tok & (p.page_size - 1), m0, c4, vside, p.page_size, p.M, p.C, p.packed);
}

// One thread per request, after the encode launch on the same stream: the rows of the requests that flushed (the same clamped
// r >= min_r) move on - T += n, r -= n, start = (start + n) % rcap, no sum or difference able to wrap; word 3 is not touched.
__global__ void flush_wide_advance_kernel(int *dev_lengths, int bs, int n, int cap_tok, int rcap, int min_r) {
    const int b = blockIdx.x * blockDim.x + threadIdx.x;
    if (b >= bs) return;
    int T, r, st;
    load_len_row((const int *)dev_lengths + 4 * b, cap_tok, rcap, rcap, T, r, st);
    if (r < min_r) return;
    dev_lengths[4 * b] = T > cap_tok - n ? cap_tok : T + n;
    dev_lengths[4 * b + 1] = r < n ? 0 : r - n;
    dev_lengths[4 * b + 2] = (int)(((unsigned)st + (unsigned)n) % (unsigned)rcap);
}

}  // namespace million

using namespace million;

extern "C" int million_pq_flush_wide(const million_encode_desc *desc, const void *k_rows, const void *v_rows, const void *k_cents,
                                     const void *v_cents, void *k_pool, void *v_pool, const int32_t *page_ids, int32_t *dev_lengths,
                                     int resid_cap, int min_r, int packed, million_stream_t stream) {
    if (!desc || desc->struct_size != sizeof(million_encode_desc)) { set_error("flush_wide: bad desc / struct_size"); return MILLION_ERR_ARG; }
    const million_encode_desc &d = *desc;
    if (d.bs <= 0 || d.nh_k <= 0 || d.n < 0) { set_error("flush_wide: bs=%d nh_k=%d n=%d", d.bs, d.nh_k, d.n); return MILLION_ERR_SHAPE; }
    if (!wide_geometry(d.d, d.M, d.C, 1) || (packed && d.M % 4)) {
        set_error("flush_wide: d=%d M=%d C=%d (d 64 / 128, d / M 2 or 4, C 512 / 1024 / 2048 / 4096; packed pages: M a multiple of 4)", d.d, d.M, d.C);
        return MILLION_ERR_SHAPE;
    }
    int ps_shift;
    if (!page_shift("flush_wide", d.page_size, ps_shift)) return MILLION_ERR_SHAPE;
    if (d.n > d.page_size) { set_error("flush_wide: n=%d exceeds page_size=%d", d.n, d.page_size); return MILLION_ERR_SHAPE; }
    if (d.n_pages_cap <= 0 || (long long)d.n_pages_cap * d.page_size + d.page_size > 0x7fffffffLL || (long long)d.bs * d.nh_k * d.n_pages_cap > 0x7fffffffLL) {
        set_error("flush_wide: n_pages_cap=%d (page table of %lld entries)", d.n_pages_cap, (long long)d.bs * d.nh_k * d.n_pages_cap);
        return MILLION_ERR_SHAPE;
    }
    if ((long long)d.bs * d.nh_k * 2 > 65535) { set_error("flush_wide: bs * nh_k = %lld exceeds the grid (32767)", (long long)d.bs * d.nh_k); return MILLION_ERR_SHAPE; }
    if (d.dst_layout != MILLION_CODES_KPAGES) { set_error("flush_wide: dst_layout must be MILLION_CODES_KPAGES (the V side is written as VPAGES)"); return MILLION_ERR_ARG; }
    if (resid_cap <= 0 || resid_cap < d.n || d.x_row_mod != resid_cap) {
        set_error("flush_wide: resid_cap=%d (> 0, >= n = %d, and desc->x_row_mod = %d must equal it)", resid_cap, d.n, d.x_row_mod);
        return MILLION_ERR_ARG;
    }
    if ((const int32_t *)dev_lengths != d.dev_lengths) { set_error("flush_wide: dev_lengths must equal desc->dev_lengths (or both null)"); return MILLION_ERR_ARG; }
    if (min_r < 0 || min_r > resid_cap) { set_error("flush_wide: min_r=%d outside [0, resid_cap]", min_r); return MILLION_ERR_ARG; }
    const int cap_tok = d.n_pages_cap * d.page_size;
    if (!dev_lengths) {
        if (d.dst_token_start < 0 || (long long)d.dst_token_start + d.n > cap_tok) { set_error("flush_wide: dst_token_start=%d, page table too short", d.dst_token_start); return MILLION_ERR_ARG; }
        if (d.x_row_start < 0 || d.x_row_start >= resid_cap) { set_error("flush_wide: x_row_start=%d outside [0, resid_cap)", d.x_row_start); return MILLION_ERR_ARG; }
    }
    if (d.n == 0) return MILLION_OK;      // nothing to flush, whatever the pointers
    if (!k_rows || !v_rows || !k_cents || !v_cents || !k_pool || !v_pool || !page_ids) { set_error("flush_wide: null rows / codebooks / pools / page_ids"); return MILLION_ERR_ARG; }
    if (((uintptr_t)k_rows | (uintptr_t)v_rows | (uintptr_t)k_cents | (uintptr_t)v_cents | (uintptr_t)k_pool | (uintptr_t)v_pool) & 15) {
        set_error("flush_wide: rows, codebooks and pools must be 16-byte aligned");
        return MILLION_ERR_ALIGN;
    }
    if (((uintptr_t)page_ids | (uintptr_t)dev_lengths) & 3) { set_error("flush_wide: page_ids / dev_lengths must be 4-byte aligned"); return MILLION_ERR_ALIGN; }
    if ((d.x_stride_b | d.x_stride_h | d.x_stride_n) & 7) { set_error("flush_wide: fp16 strides must be multiples of 8 elements (16-byte rows)"); return MILLION_ERR_ALIGN; }
    FlushWideParams p;
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
    const dim3 grid((d.n + 63) / 64, d.M / kFwSub, d.bs * d.nh_k * 2);
    hipStream_t s = (hipStream_t)stream;
    if (d.d / d.M == 2) hipLaunchKernelGGL(pq_flush_wide_kernel<2>, grid, dim3(kFwWaves * 64), 0, s, p);
    else hipLaunchKernelGGL(pq_flush_wide_kernel<4>, grid, dim3(kFwWaves * 64), 0, s, p);
    hipError_t e = hipGetLastError();
    if (e != hipSuccess) { set_error("flush_wide launch: %s", hipGetErrorString(e)); return MILLION_ERR_LAUNCH; }
    if (!dev_lengths) return MILLION_OK;      // host lengths: nothing to advance
    hipLaunchKernelGGL(flush_wide_advance_kernel, dim3((d.bs + 63) / 64), dim3(64), 0, s, dev_lengths, d.bs, d.n, cap_tok, resid_cap, min_r);
    e = hipGetLastError();
    if (e != hipSuccess) { set_error("flush_wide advance launch: %s", hipGetErrorString(e)); return MILLION_ERR_LAUNCH; }
    return MILLION_OK;
}
