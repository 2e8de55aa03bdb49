// store_ragged.hip — the store step of a ragged batch in one launch (million_pq_store_ragged for 8-bit codes,
// million_pq_store_ragged_wide for codes of 9 .. 12 bits in uint16 pages or packed pages), gfx950.
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
// and transposed V pages.  The encode launch is paged_store_kernel<DM, P> (paged_store.h: mapping, grid, early exits) with one
// of the two parameter blocks below - the wide one scans the plain fp16 codebook and stores through code_pages.h; the advance
// kernel, the host front both entry points share (store_ragged_front) and the entry points are here.
#include "paged_store.h"

#pragma clang fp contract(off)

namespace million {

struct StoreRaggedParams {
    static constexpr bool kCommit = false;
    static constexpr bool kWide = false;
    PagedStoreSide k, v;        // new rows (bs, nh_k, n_bound, d), window (bs, nh_k, resid_cap, d)
    const int *page_ids;        // (bs, nh_k, n_pages_cap)
    const int *dev_lengths;     // (bs, 4)
    const int *dev_n;           // (bs,)
    long long wsb, wsh;
    int bs, nh_k, d, M, C;
    int n_bound, rcap;
    int page_size, ps_shift, n_pages_cap, cap_tok;
    __device__ __forceinline__ PagedStoreSide side(bool vside) const {
        return {vside ? v.new_rows : k.new_rows, vside ? v.win : k.win, vside ? v.cents : k.cents, vside ? v.pool : k.pool,
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

// The same block for wide codes (512 .. 4096 centroids): the sides carry the plain (M, C, d_m) fp16 codebook, the pools are
// uint16 pages (as bytes) or packed pages
struct StoreRaggedWideParams {
    static constexpr bool kCommit = false;
    static constexpr bool kWide = true;
    PagedStoreSideT<f16> k, v;
    const int *page_ids;
    const int *dev_lengths;
    const int *dev_n;
    long long wsb, wsh;
    int bs, nh_k, d, M, C;
    int n_bound, rcap;
    int page_size, ps_shift, n_pages_cap, cap_tok;
    int packed;
    __device__ __forceinline__ PagedStoreSideT<f16> side(bool vside) const {
        return {vside ? v.new_rows : k.new_rows, vside ? v.win : k.win, vside ? v.cents : k.cents, vside ? v.pool : k.pool,
                vside ? v.nsb : k.nsb, vside ? v.nsh : k.nsh, vside ? v.nsn : k.nsn};
    }
};

// Host: everything the two entry points share - the refusals in their one order, the parameter fill, the grid and the two
// launches.  `who` names the entry point in the messages, `cents_kind` its codebooks in the null-pointer message; geometry(d)
// is the entry point's own shape check (false: refused, its words set); finish(p, grid, s) puts the entry point's codebook
// pointers (and format) into p and launches its instance of paged_store_kernel (false: no instance for this d / M).
template <class P, class Geometry, class Finish>
static int store_ragged_front(const char *who, const char *cents_kind, const million_store_ragged_desc *desc, const void *k_new,
                              const void *v_new, const void *k_resid, const void *v_resid, const void *k_cents, const void *v_cents,
                              void *k_pool, void *v_pool, const int32_t *page_ids, int32_t *dev_lengths, const int32_t *dev_n,
                              million_stream_t stream, Geometry geometry, Finish finish) {
    if (!desc || desc->struct_size != sizeof(million_store_ragged_desc)) { set_error("%s: bad desc / struct_size", who); return MILLION_ERR_ARG; }
    const million_store_ragged_desc &d = *desc;
    if (d.bs <= 0 || d.nh_k <= 0 || d.n_bound < 0) { set_error("%s: bs=%d nh_k=%d n_bound=%d", who, d.bs, d.nh_k, d.n_bound); return MILLION_ERR_SHAPE; }
    int ps_shift;
    if (!geometry(d) || !page_shift(who, d.page_size, ps_shift)) return MILLION_ERR_SHAPE;
    if (d.n_pages_cap <= 0 || (long long)d.n_pages_cap * d.page_size + d.resid_cap + d.n_bound > 0x7fffffffLL || (long long)d.bs * d.nh_k * d.n_pages_cap > 0x7fffffffLL) {
        set_error("%s: n_pages_cap=%d (page table of %lld entries)", who, d.n_pages_cap, (long long)d.bs * d.nh_k * d.n_pages_cap);
        return MILLION_ERR_SHAPE;
    }
    if ((long long)d.bs * d.nh_k * 2 > 65535) { set_error("%s: bs * nh_k = %lld exceeds the grid (32767)", who, (long long)d.bs * d.nh_k); return MILLION_ERR_SHAPE; }
    if (d.resid_cap < 0) { set_error("%s: resid_cap=%d", who, d.resid_cap); return MILLION_ERR_ARG; }
    if (d.n_bound == 0) return MILLION_OK;      // no request can have a row: nothing to do, whatever the pointers
    if (!dev_n) { set_error("%s: null dev_n (the row count of every request is read on the device)", who); return MILLION_ERR_ARG; }
    if (!dev_lengths) { set_error("%s: null dev_lengths", who); return MILLION_ERR_ARG; }
    if (d.resid_cap > 0 && (!k_resid || !v_resid)) { set_error("%s: null window with resid_cap=%d", who, d.resid_cap); return MILLION_ERR_ARG; }
    if (!k_cents || !v_cents) { set_error("%s: null %s", who, cents_kind); return MILLION_ERR_ARG; }
    if (!k_new || !v_new || !k_pool || !v_pool || !page_ids) { set_error("%s: null new rows / pools / page_ids", who); return MILLION_ERR_ARG; }
    P p;
    const int rc = paged_store_fill(who, p, d.bs, d.nh_k, d.d, d.M, d.C, d.n_bound, d.resid_cap, d.page_size, ps_shift, d.n_pages_cap,
                                    (uintptr_t)k_new | (uintptr_t)v_new | (uintptr_t)k_resid | (uintptr_t)v_resid | (uintptr_t)k_cents |
                                        (uintptr_t)v_cents | (uintptr_t)k_pool | (uintptr_t)v_pool,
                                    page_ids, dev_lengths, dev_n);
    if (rc != MILLION_OK) return rc;
    if ((d.kn_stride_b | d.kn_stride_h | d.kn_stride_n | d.vn_stride_b | d.vn_stride_h | d.vn_stride_n | d.resid_stride_b | d.resid_stride_h) & 7) {
        set_error("%s: fp16 strides must be multiples of 8 elements (16-byte rows)", who);
        return MILLION_ERR_ALIGN;
    }
    p.k.new_rows = (const f16 *)k_new; p.v.new_rows = (const f16 *)v_new;
    p.k.win = (const f16 *)k_resid; p.v.win = (const f16 *)v_resid;
    p.k.pool = (uint8_t *)k_pool; p.v.pool = (uint8_t *)v_pool;
    p.k.nsb = d.kn_stride_b; p.k.nsh = d.kn_stride_h; p.k.nsn = d.kn_stride_n;
    p.v.nsb = d.vn_stride_b; p.v.nsh = d.vn_stride_h; p.v.nsn = d.vn_stride_n;
    p.wsb = d.resid_stride_b; p.wsh = d.resid_stride_h;
    const int groups = d.M / kPsSub;
    const dim3 grid(((long long)d.resid_cap + d.n_bound + 63) / 64, (groups + kPsBlock / 64 - 1) / (kPsBlock / 64), d.bs * d.nh_k * 2);
    hipStream_t s = (hipStream_t)stream;
    if (!finish(p, grid, s)) { set_error("%s: d/M=%d unsupported (1,2,4,8)", who, d.d / d.M); return MILLION_ERR_SHAPE; }
    hipError_t e = hipGetLastError();
    if (e != hipSuccess) { set_error("%s launch: %s", who, hipGetErrorString(e)); return MILLION_ERR_LAUNCH; }
    hipLaunchKernelGGL(store_ragged_advance_kernel, dim3((d.bs + 63) / 64), dim3(64), 0, s, dev_lengths, dev_n, d.bs, p.cap_tok,
                       d.resid_cap, d.n_bound);
    e = hipGetLastError();
    if (e != hipSuccess) { set_error("%s advance launch: %s", who, hipGetErrorString(e)); return MILLION_ERR_LAUNCH; }
    return MILLION_OK;
}

}  // namespace million

using namespace million;

extern "C" int million_pq_store_ragged_wide(const million_store_ragged_desc *desc, const void *k_new, const void *v_new,
                                            const void *k_resid, const void *v_resid, const void *k_cents, const void *v_cents,
                                            void *k_pool, void *v_pool, const int32_t *page_ids, int32_t *dev_lengths,
                                            const int32_t *dev_n, int packed, million_stream_t stream) {
    return store_ragged_front<StoreRaggedWideParams>(
        "store_ragged_wide", "codebook (the plain (M, C, d_m) fp16 tensors: the call needs both)", desc, k_new, v_new, k_resid, v_resid,
        k_cents, v_cents, k_pool, v_pool, page_ids, dev_lengths, dev_n, stream,
        [&](const million_store_ragged_desc &d) {
            if (wide_geometry(d.d, d.M, d.C, 1) && !(packed && d.M % 4)) return true;
            set_error("store_ragged_wide: d=%d M=%d C=%d (d 64 / 128, d / M 2 or 4, C 512 / 1024 / 2048 / 4096; packed pages: M a multiple of 4)", d.d, d.M, d.C);
            return false;
        },
        [&](StoreRaggedWideParams &p, dim3 grid, hipStream_t s) {
            p.k.cents = (const f16 *)k_cents; p.v.cents = (const f16 *)v_cents;
            p.packed = packed ? 1 : 0;
            if (p.d / p.M == 2) hipLaunchKernelGGL((paged_store_kernel<2, StoreRaggedWideParams>), grid, dim3(kPsBlock), 0, s, p);
            else hipLaunchKernelGGL((paged_store_kernel<4, StoreRaggedWideParams>), grid, dim3(kPsBlock), 0, s, p);
            return true;      // wide_geometry: d / M is 2 or 4
        });
}

extern "C" int million_pq_store_ragged(const million_store_ragged_desc *desc, const void *k_new, const void *v_new,
                                       const void *k_resid, const void *v_resid, const void *k_cents_prepared,
                                       const void *v_cents_prepared, void *k_pool, void *v_pool, const int32_t *page_ids,
                                       int32_t *dev_lengths, const int32_t *dev_n, million_stream_t stream) {
    return store_ragged_front<StoreRaggedParams>(
        "store_ragged", "prepared codebook (million_prepare_cents: the call needs both)", desc, k_new, v_new, k_resid, v_resid,
        k_cents_prepared, v_cents_prepared, k_pool, v_pool, page_ids, dev_lengths, dev_n, stream,
        [](const million_store_ragged_desc &d) { return u8_geometry("store_ragged", d.d, d.M, d.C); },
        [&](StoreRaggedParams &p, dim3 grid, hipStream_t s) {
            const int dm = p.d / p.M;
            p.k.cents = prepared_cents32(k_cents_prepared, p.M, p.C, dm);
            p.v.cents = prepared_cents32(v_cents_prepared, p.M, p.C, dm);
            return dispatch_dm(dm, [&](auto w) { hipLaunchKernelGGL((paged_store_kernel<w(), StoreRaggedParams>), grid, dim3(kPsBlock), 0, s, p); });
        });
}
