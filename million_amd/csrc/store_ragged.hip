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

}  // namespace million

using namespace million;

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
