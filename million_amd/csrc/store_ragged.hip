// store_ragged.hip — the store step of a ragged batch in one launch (million_pq_store_ragged), gfx950.
//
// Behind a ragged attention launch (million_pq_chunk_attn with dev_lengths / dev_n_q, million_prefill_attn with dev_spans)
// PagedPQCache._store was a host loop: per slot up to four million_pq_encode launches (K and V of the window in ring order,
// K and V of the new rows) and a host-to-device copy of the slot's lengths row, each with host values baked in.  Here every
// request of the batch is stored by ONE encode launch that reads {T, r, start} and n_b on the device, followed by a
// one-thread-per-request launch that advances the lengths rows: stream order is all the ordering there is (the pattern of
// chunk_merge_kernel: two plain launches, no atomics, tickets or polls).
//
// Per request b (values clamped: ps_load_row of paged_store.h, load_len_row of common.h): r + n_b source rows - row j < r is
// window row (start + j) % resid_cap, row j >= r is new row j - r - and source row j becomes token T + j of the request's K pages
// and transposed V pages.  The encode launch is paged_store_kernel<DM, StoreRaggedParams> (paged_store.h: mapping, grid, early exits); the
// advance kernel and the entry point are here.
#include "paged_store.h"

#pragma clang fp contract(off)

namespace million {

struct StoreRaggedParams {
    static constexpr bool kCommit = false;
    PagedStoreSide k, v;        // new rows (bs, nh_k, n_bound, d), window (bs, nh_k, resid_cap, d)
    const int *page_ids;        // (bs, nh_k, n_pages_cap)
    const int *dev_lengths;     // (bs, 4)
    const int *dev_n;           // (bs,)
    long long wsb, wsh;
    int bs, nh_k, d, M, C;
    int n_bound, rcap;
    int page_size, ps_shift, n_pages_cap, cap_tok;
    __device__ __forceinline__ PagedStoreSide side(bool vside) const {
        return {vside ? v.new_rows : k.new_rows, vside ? v.win : k.win, vside ? v.cents32 : k.cents32, vside ? v.pool : k.pool,
                vside ? v.nsb : k.nsb, vside ? v.nsh : k.nsh, vside ? v.nsn : k.nsn};
    }
};

// One thread per request, after the encode launch on the same stream: T <- min(T + r + n, cap_tok), r <- 0, start <- 0 from
// the clamped values; word 3 and the rows with n = 0 are not touched.
__global__ void store_ragged_advance_kernel(int *dev_lengths, const int *dev_n, int bs, int cap_tok, int rcap, int n_bound) {
    const int b = blockIdx.x * blockDim.x + threadIdx.x;
    if (b >= bs) return;
    int T, r, st;
    load_len_row((const int *)dev_lengths + 4 * b, cap_tok, rcap, rcap, T, r, st);
    const int n = clamp_count(dev_n[b], n_bound);
    if (n == 0) return;
    const long long Tn = (long long)T + r + n;
    dev_lengths[4 * b] = Tn > cap_tok ? cap_tok : (int)Tn;
    dev_lengths[4 * b + 1] = 0;
    dev_lengths[4 * b + 2] = 0;
}

// ---- the same store over uint16 pages and packed pages (million_pq_store_ragged_wide): codes of 512 .. 4096 centroids.
// A kernel of its own rather than a third parameter block of paged_store_kernel: the scan reads the plain fp16 codebook
// (pq_scan_sgpr<DM, f16>: wide formats have no prepared image) and the store is pq_encode_kernel<DM, false, uint16_t[, PACKED]>'s,
// and the instances of the store and the commit stay what they are (paged_store.h: a merged block regrouped their argument
// loads once).  Mapping, grid rule, early exits, clamps and the source-row selection are paged_store_kernel's word for word;
// the helpers (ps_load_row, pq_scan_sgpr) and the advance kernel above are shared.
struct StoreRaggedWideSide {
    const f16 *new_rows, *win, *cents;      // cents: (M, C, d_m) fp16
    uint8_t *pool;                          // uint16 pages as bytes, or packed pages
    long long nsb, nsh, nsn;
};
struct StoreRaggedWideParams {
    StoreRaggedWideSide k, v;
    const int *page_ids;
    const int *dev_lengths;
    const int *dev_n;
    long long wsb, wsh;
    int bs, nh_k, d, M, C;
    int n_bound, rcap;
    int page_size, ps_shift, n_pages_cap, cap_tok;
    int packed;
    __device__ __forceinline__ StoreRaggedWideSide side(bool vside) const {
        return {vside ? v.new_rows : k.new_rows, vside ? v.win : k.win, vside ? v.cents : k.cents, vside ? v.pool : k.pool,
                vside ? v.nsb : k.nsb, vside ? v.nsh : k.nsh, vside ? v.nsn : k.nsn};
    }
};

template <int DM>
__global__ __launch_bounds__(kPsBlock) void store_ragged_wide_kernel(StoreRaggedWideParams p) {
    const int lane = threadIdx.x & 63;
    const int mg = __builtin_amdgcn_readfirstlane((int)(blockIdx.y * (kPsBlock / 64) + (threadIdx.x >> 6)));
    const int m0 = mg * kPsSub;
    const bool vside = blockIdx.z & 1;    // workgroup-uniform
    const StoreRaggedWideSide sd = p.side(vside);
    const int bh = blockIdx.z >> 1;
    const int b = bh / p.nh_k, hk = bh % p.nh_k;
    if (m0 >= p.M) return;
    int T, r, st, n;
    {
        typedef const __attribute__((address_space(4))) int *const_p;      // scalar loads: neither array is written by this launch
        ps_load_row((const_p)(p.dev_lengths + 4 * b), (const_p)p.dev_n, b, p, T, r, st, n);
    }
    if (n == 0) return;               // the request takes no part: nothing of it is read beyond those words
    const int rows = r + n;
    const int j0 = blockIdx.x * 64;
    // a block past the request's rows, a block whose first token lies past the page table
    if (j0 >= rows || ((T + j0) >> p.ps_shift) >= p.n_pages_cap) return;
    const int j = j0 + lane;
    const bool valid = j < rows;
    const int jc = valid ? j : rows - 1;
    // source row: the address is selected, the load is one
    const int rmod = p.rcap > 0 ? p.rcap : 1;
    const long long off_w = b * p.wsb + hk * p.wsh + (long long)((st + jc) % rmod) * p.d;
    const long long off_n = b * sd.nsb + hk * sd.nsh + (long long)(jc - r) * sd.nsn;
    const f16 *xp = (jc < r ? sd.win + off_w : sd.new_rows + off_n) + m0 * DM;
    float x[kPsSub][DM];
#pragma unroll
    for (int s = 0; s < kPsSub; ++s)
#pragma unroll
        for (int k = 0; k < DM; ++k) x[s][k] = (float)xp[s * DM + k];
    // destination: token T + jc; the page index of a dead or dropped lane is clamped to a page that receives a token of this block
    const int tok = T + jc;
    const int page = tok >> p.ps_shift;
    const bool keep = valid && page < p.n_pages_cap;
    const long long pid = p.page_ids[(long long)bh * p.n_pages_cap + (page < p.n_pages_cap ? page : p.n_pages_cap - 1)];

    unsigned c4[kPsSub];
    const f16 *__restrict__ tab = sd.cents;
#pragma unroll
    for (int s = 0; s < kPsSub; ++s) {
        float best = INFINITY;
        int best_c = 0;
        pq_scan_sgpr<DM>(x[s], tab + (long long)(m0 + s) * p.C * DM, p.C, best, best_c);   // wave-uniform rows
        c4[s] = (unsigned)best_c;
    }
    if (!keep) return;
    const int off = tok & (p.page_size - 1);
    if (!p.packed) {
        uint16_t *dst = (uint16_t *)sd.pool;
        if (!vside) {
            // K page (page_size, M): the token's 4 codes are one aligned 64-bit store (M and m0 are multiples of 4)
            const unsigned long long codes = (unsigned long long)c4[0] | (unsigned long long)c4[1] << 16 | (unsigned long long)c4[2] << 32 |
                                             (unsigned long long)c4[3] << 48;
            *(unsigned long long *)(dst + (pid * p.page_size + off) * p.M + m0) = codes;
        } else {
            // transposed V page (M, page_size): four lane-contiguous 16-bit rows
#pragma unroll
            for (int s = 0; s < kPsSub; ++s) dst[(pid * p.M + m0 + s) * p.page_size + off] = (uint16_t)c4[s];
        }
        return;
    }
    // packed page: 4 low bytes, and one whole byte (2 high bits per code) or two (4 high bits) of the high plane - every byte
    // written belongs to this token alone
    const int hb = packed_hi_bits(p.C);
    uint8_t *pg = sd.pool + pid * packed_page_bytes(p.page_size, p.M, p.C);
    uint8_t *hi_plane = pg + p.page_size * p.M;
    unsigned lo = 0, hi = 0;
#pragma unroll
    for (int s = 0; s < kPsSub; ++s) {
        lo |= (c4[s] & 0xffu) << (8 * s);
        hi |= ((c4[s] >> 8) & ((1u << hb) - 1u)) << (hb * s);
    }
    if (!vside) {
        *(unsigned *)(pg + off * p.M + m0) = lo;
        if (hb == 2) hi_plane[off * (p.M / 4) + m0 / 4] = (uint8_t)hi;
        else *(unsigned short *)(hi_plane + off * (p.M / 2) + m0 / 2) = (unsigned short)hi;
    } else {
#pragma unroll
        for (int s = 0; s < kPsSub; ++s) pg[(m0 + s) * p.page_size + off] = (uint8_t)c4[s];
        if (hb == 2) hi_plane[(m0 / 4) * p.page_size + off] = (uint8_t)hi;
        else {
            hi_plane[(m0 / 2) * p.page_size + off] = (uint8_t)hi;
            hi_plane[(m0 / 2 + 1) * p.page_size + off] = (uint8_t)(hi >> 8);
        }
    }
}

}  // namespace million

using namespace million;

extern "C" int million_pq_store_ragged_wide(const million_store_ragged_desc *desc, const void *k_new, const void *v_new,
                                            const void *k_resid, const void *v_resid, const void *k_cents, const void *v_cents,
                                            void *k_pool, void *v_pool, const int32_t *page_ids, int32_t *dev_lengths,
                                            const int32_t *dev_n, int packed, million_stream_t stream) {
    if (!desc || desc->struct_size != sizeof(million_store_ragged_desc)) { set_error("store_ragged_wide: bad desc / struct_size"); return MILLION_ERR_ARG; }
    const million_store_ragged_desc &d = *desc;
    if (d.bs <= 0 || d.nh_k <= 0 || d.n_bound < 0) { set_error("store_ragged_wide: bs=%d nh_k=%d n_bound=%d", d.bs, d.nh_k, d.n_bound); return MILLION_ERR_SHAPE; }
    int ps_shift;
    if (!wide_geometry(d.d, d.M, d.C, 1) || (packed && d.M % 4)) {
        set_error("store_ragged_wide: d=%d M=%d C=%d (d 64 / 128, d / M 2 or 4, C 512 / 1024 / 2048 / 4096; packed pages: M a multiple of 4)", d.d, d.M, d.C);
        return MILLION_ERR_SHAPE;
    }
    if (!page_shift("store_ragged_wide", d.page_size, ps_shift)) return MILLION_ERR_SHAPE;
    if (d.n_pages_cap <= 0 || (long long)d.n_pages_cap * d.page_size + d.resid_cap + d.n_bound > 0x7fffffffLL || (long long)d.bs * d.nh_k * d.n_pages_cap > 0x7fffffffLL) {
        set_error("store_ragged_wide: n_pages_cap=%d (page table of %lld entries)", d.n_pages_cap, (long long)d.bs * d.nh_k * d.n_pages_cap);
        return MILLION_ERR_SHAPE;
    }
    if ((long long)d.bs * d.nh_k * 2 > 65535) { set_error("store_ragged_wide: bs * nh_k = %lld exceeds the grid (32767)", (long long)d.bs * d.nh_k); return MILLION_ERR_SHAPE; }
    if (d.resid_cap < 0) { set_error("store_ragged_wide: resid_cap=%d", d.resid_cap); return MILLION_ERR_ARG; }
    if (d.n_bound == 0) return MILLION_OK;      // no request can have a row: nothing to do, whatever the pointers
    if (!dev_n) { set_error("store_ragged_wide: null dev_n (the row count of every request is read on the device)"); return MILLION_ERR_ARG; }
    if (!dev_lengths) { set_error("store_ragged_wide: null dev_lengths"); return MILLION_ERR_ARG; }
    if (d.resid_cap > 0 && (!k_resid || !v_resid)) { set_error("store_ragged_wide: null window with resid_cap=%d", d.resid_cap); return MILLION_ERR_ARG; }
    if (!k_cents || !v_cents) { set_error("store_ragged_wide: null codebook (the plain (M, C, d_m) fp16 tensors: the call needs both)"); return MILLION_ERR_ARG; }
    if (!k_new || !v_new || !k_pool || !v_pool || !page_ids) { set_error("store_ragged_wide: null new rows / pools / page_ids"); return MILLION_ERR_ARG; }
    if (((uintptr_t)k_new | (uintptr_t)v_new | (uintptr_t)k_resid | (uintptr_t)v_resid | (uintptr_t)k_cents | (uintptr_t)v_cents | (uintptr_t)k_pool | (uintptr_t)v_pool) & 15) {
        set_error("store_ragged_wide: rows, windows, codebooks and pools must be 16-byte aligned");
        return MILLION_ERR_ALIGN;
    }
    if (((uintptr_t)page_ids | (uintptr_t)dev_lengths | (uintptr_t)dev_n) & 3) { set_error("store_ragged_wide: page_ids / dev_lengths / dev_n must be 4-byte aligned"); return MILLION_ERR_ALIGN; }
    if ((d.kn_stride_b | d.kn_stride_h | d.kn_stride_n | d.vn_stride_b | d.vn_stride_h | d.vn_stride_n | d.resid_stride_b | d.resid_stride_h) & 7) {
        set_error("store_ragged_wide: fp16 strides must be multiples of 8 elements (16-byte rows)");
        return MILLION_ERR_ALIGN;
    }
    StoreRaggedWideParams p;
    memset(&p, 0, sizeof(p));
    p.page_ids = page_ids; p.dev_lengths = dev_lengths; p.dev_n = dev_n;
    p.bs = d.bs; p.nh_k = d.nh_k; p.d = d.d; p.M = d.M; p.C = d.C;
    p.n_bound = d.n_bound; p.rcap = d.resid_cap;
    p.page_size = d.page_size; p.ps_shift = ps_shift;
    p.n_pages_cap = d.n_pages_cap; p.cap_tok = d.n_pages_cap * d.page_size;
    p.packed = packed ? 1 : 0;
    p.k.new_rows = (const f16 *)k_new; p.v.new_rows = (const f16 *)v_new;
    p.k.win = (const f16 *)k_resid; p.v.win = (const f16 *)v_resid;
    p.k.cents = (const f16 *)k_cents; p.v.cents = (const f16 *)v_cents;
    p.k.pool = (uint8_t *)k_pool; p.v.pool = (uint8_t *)v_pool;
    p.k.nsb = d.kn_stride_b; p.k.nsh = d.kn_stride_h; p.k.nsn = d.kn_stride_n;
    p.v.nsb = d.vn_stride_b; p.v.nsh = d.vn_stride_h; p.v.nsn = d.vn_stride_n;
    p.wsb = d.resid_stride_b; p.wsh = d.resid_stride_h;
    const int groups = d.M / kPsSub;
    const dim3 grid(((long long)d.resid_cap + d.n_bound + 63) / 64, (groups + kPsBlock / 64 - 1) / (kPsBlock / 64), d.bs * d.nh_k * 2);
    hipStream_t s = (hipStream_t)stream;
    if (d.d / d.M == 2) hipLaunchKernelGGL(store_ragged_wide_kernel<2>, grid, dim3(kPsBlock), 0, s, p);
    else hipLaunchKernelGGL(store_ragged_wide_kernel<4>, grid, dim3(kPsBlock), 0, s, p);
    hipError_t e = hipGetLastError();
    if (e != hipSuccess) { set_error("store_ragged_wide launch: %s", hipGetErrorString(e)); return MILLION_ERR_LAUNCH; }
    hipLaunchKernelGGL(store_ragged_advance_kernel, dim3((d.bs + 63) / 64), dim3(64), 0, s, dev_lengths, dev_n, d.bs, p.cap_tok,
                       d.resid_cap, d.n_bound);
    e = hipGetLastError();
    if (e != hipSuccess) { set_error("store_ragged_wide advance launch: %s", hipGetErrorString(e)); return MILLION_ERR_LAUNCH; }
    return MILLION_OK;
}

extern "C" int million_pq_store_ragged(const million_store_ragged_desc *desc, const void *k_new, const void *v_new,
                                       const void *k_resid, const void *v_resid, const void *k_cents_prepared,
                                       const void *v_cents_prepared, void *k_pool, void *v_pool, const int32_t *page_ids,
                                       int32_t *dev_lengths, const int32_t *dev_n, million_stream_t stream) {
    if (!desc || desc->struct_size != sizeof(million_store_ragged_desc)) { set_error("store_ragged: bad desc / struct_size"); return MILLION_ERR_ARG; }
    const million_store_ragged_desc &d = *desc;
    if (d.bs <= 0 || d.nh_k <= 0 || d.n_bound < 0) { set_error("store_ragged: bs=%d nh_k=%d n_bound=%d", d.bs, d.nh_k, d.n_bound); return MILLION_ERR_SHAPE; }
    int ps_shift;
    if (!u8_geometry("store_ragged", d.d, d.M, d.C) || !page_shift("store_ragged", d.page_size, ps_shift)) return MILLION_ERR_SHAPE;
    if (d.n_pages_cap <= 0 || (long long)d.n_pages_cap * d.page_size + d.resid_cap + d.n_bound > 0x7fffffffLL || (long long)d.bs * d.nh_k * d.n_pages_cap > 0x7fffffffLL) {
        set_error("store_ragged: n_pages_cap=%d (page table of %lld entries)", d.n_pages_cap, (long long)d.bs * d.nh_k * d.n_pages_cap);
        return MILLION_ERR_SHAPE;
    }
    if ((long long)d.bs * d.nh_k * 2 > 65535) { set_error("store_ragged: bs * nh_k = %lld exceeds the grid (32767)", (long long)d.bs * d.nh_k); return MILLION_ERR_SHAPE; }
    if (d.resid_cap < 0) { set_error("store_ragged: resid_cap=%d", d.resid_cap); return MILLION_ERR_ARG; }
    if (d.n_bound == 0) return MILLION_OK;      // no request can have a row: nothing to do, whatever the pointers
    if (!dev_n) { set_error("store_ragged: null dev_n (the row count of every request is read on the device)"); return MILLION_ERR_ARG; }
    if (!dev_lengths) { set_error("store_ragged: null dev_lengths"); return MILLION_ERR_ARG; }
    if (d.resid_cap > 0 && (!k_resid || !v_resid)) { set_error("store_ragged: null window with resid_cap=%d", d.resid_cap); return MILLION_ERR_ARG; }
    if (!k_cents_prepared || !v_cents_prepared) { set_error("store_ragged: null prepared codebook (million_prepare_cents: the call needs both)"); return MILLION_ERR_ARG; }
    if (!k_new || !v_new || !k_pool || !v_pool || !page_ids) { set_error("store_ragged: null new rows / pools / page_ids"); return MILLION_ERR_ARG; }
    StoreRaggedParams p;
    const int rc = paged_store_fill("store_ragged", p, d.bs, d.nh_k, d.d, d.M, d.C, d.n_bound, d.resid_cap, d.page_size, ps_shift, d.n_pages_cap,
                                    (uintptr_t)k_new | (uintptr_t)v_new | (uintptr_t)k_resid | (uintptr_t)v_resid | (uintptr_t)k_cents_prepared |
                                        (uintptr_t)v_cents_prepared | (uintptr_t)k_pool | (uintptr_t)v_pool,
                                    page_ids, dev_lengths, dev_n);
    if (rc != MILLION_OK) return rc;
    if ((d.kn_stride_b | d.kn_stride_h | d.kn_stride_n | d.vn_stride_b | d.vn_stride_h | d.vn_stride_n | d.resid_stride_b | d.resid_stride_h) & 7) {
        set_error("store_ragged: fp16 strides must be multiples of 8 elements (16-byte rows)");
        return MILLION_ERR_ALIGN;
    }
    const int dm = d.d / d.M;
    p.k.new_rows = (const f16 *)k_new; p.v.new_rows = (const f16 *)v_new;
    p.k.win = (const f16 *)k_resid; p.v.win = (const f16 *)v_resid;
    p.k.cents32 = prepared_cents32(k_cents_prepared, d.M, d.C, dm);
    p.v.cents32 = prepared_cents32(v_cents_prepared, d.M, d.C, dm);
    p.k.pool = (uint8_t *)k_pool; p.v.pool = (uint8_t *)v_pool;
    p.k.nsb = d.kn_stride_b; p.k.nsh = d.kn_stride_h; p.k.nsn = d.kn_stride_n;
    p.v.nsb = d.vn_stride_b; p.v.nsh = d.vn_stride_h; p.v.nsn = d.vn_stride_n;
    p.wsb = d.resid_stride_b; p.wsh = d.resid_stride_h;
    const int groups = d.M / kPsSub;
    const dim3 grid(((long long)d.resid_cap + d.n_bound + 63) / 64, (groups + kPsBlock / 64 - 1) / (kPsBlock / 64), d.bs * d.nh_k * 2);
    hipStream_t s = (hipStream_t)stream;
    if (!dispatch_dm(dm, [&](auto w) { hipLaunchKernelGGL((paged_store_kernel<w(), StoreRaggedParams>), grid, dim3(kPsBlock), 0, s, p); })) {
        set_error("store_ragged: d/M=%d unsupported (1,2,4,8)", dm);
        return MILLION_ERR_SHAPE;
    }
    hipError_t e = hipGetLastError();
    if (e != hipSuccess) { set_error("store_ragged launch: %s", hipGetErrorString(e)); return MILLION_ERR_LAUNCH; }
    hipLaunchKernelGGL(store_ragged_advance_kernel, dim3((d.bs + 63) / 64), dim3(64), 0, s, dev_lengths, dev_n, d.bs, p.cap_tok,
                       d.resid_cap, d.n_bound);
    e = hipGetLastError();
    if (e != hipSuccess) { set_error("store_ragged advance launch: %s", hipGetErrorString(e)); return MILLION_ERR_LAUNCH; }
    return MILLION_OK;
}
