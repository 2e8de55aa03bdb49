// window_commit.hip — append the accepted rows of a draft verification to the residual windows of a paged cache, every layer in
// one call (million_window_commit, include/million_hip.h), gfx950.
//
// Request b accepted a_b = dev_n[b] of the rows in k_new / v_new (layers, bs, nh_k, n_bound, d).  The cache is left exactly as a_b
// decode steps would have left it, where a decode step is "if the window is full, flush its oldest page_size rows; append".  A
// flush encodes the oldest rows and a code depends on its row and the codebook alone, so the a_b steps have a closed form, per
// (layer, b) with the clamped {T, r, start} of the request's lengths row (load_len_row, common.h):
//   source sequence  S = [the r window rows in ring order; the a new rows];
//   F = ceil((r + a - cap) / page_size) if r + a > cap else 0 (0 or 1: n_bound <= page_size), f = F * page_size;
//   S[0, f) becomes tokens [T, T + f) of the K pages and the transposed V pages; the new rows with source index >= f go to ring
//   slot (start + r + i) % cap; then T += f, r += a - f, start = (start + f) % cap.  Word 3 is not touched.
// Two plain launches on one stream (the pattern of store_ragged.hip: no atomics, tickets or polls):
//   1. paged_store_kernel<DM, WindowCommitParams> (paged_store.h), the kernel of million_pq_store_ragged with S[0, f) for its
//      rows (lane = token, a wave owns 4 consecutive subspaces, the scan of pq_scan.h over the fp32 row image read through the
//      scalar cache), so the codes are what million_pq_flush writes.  The grid is a function of the bounds alone; a block of a
//      request with f = 0 leaves before its first vector load.
//   2. window_commit_append_kernel: one workgroup per (layer, b) copies the rows that stay in the window and then advances the
//      lengths row.  It comes second because the ring slots it writes may hold rows the first launch reads; inside it every
//      thread has read the lengths row before the barrier that precedes the one thread's write.
// A request whose T + f would pass the page table is left untouched by both launches.
// million_window_commit_rows (the accepted path of a draft tree) is the same two launches with one indirection: new row i of
// request b is staged row dev_rows[b][i], index and entry clamped on the device (ps_new_row, paged_store.h; CommitRowsParams).
// million_window_commit_wide / million_window_commit_rows_wide are the same two launches over uint16 pages or packed pages (codes
// of 512 .. 4096 centroids): launch 1 with the P::kWide blocks below - the scan over the plain fp16 codebook, the token store of
// code_pages.h, so the codes are million_pq_flush_wide's - and launch 2 the append kernels above, which see fp16 rows and the
// lengths rows only.
#include "paged_store.h"

#pragma clang fp contract(off)

namespace million {

namespace {

constexpr int kWcBlock = 256;
constexpr int kWcMaxRows = 16;      // new rows per request, at most

struct WindowCommitParams {
    static constexpr bool kCommit = true;
    static constexpr bool kRows = false;
    static constexpr bool kWide = false;
    const f16 *k_new, *v_new;       // (layers, bs, nh_k, n_bound, d)
    f16 *k_win, *v_win;             // (layers, bs, nh_k, rcap, d), each layer contiguous
    const float *k_cents32, *v_cents32;
    uint8_t *k_pool, *v_pool;
    const int *page_ids;            // (layers, bs, nh_k, n_pages_cap)
    int *dev_lengths;               // (layers, bs, 4)
    const int *dev_n;               // (bs,)
    long long nsl, nsb, nsh, nsn;   // the new rows' strides, fp16 elements
    long long ids_ls, win_ls, len_ls;
    int n_layers, bs, nh_k, d, M, C;
    int n_bound, rcap;
    int page_size, ps_shift, n_pages_cap, cap_tok, n_pool;
    int groups_y;                   // grid.y per layer
    __device__ __forceinline__ PagedStoreSide side(bool vside) const {
        return {vside ? v_new : k_new, vside ? v_win : k_win, vside ? v_cents32 : k_cents32, vside ? v_pool : k_pool, nsb, nsh, nsn};
    }
};

// million_window_commit_rows: new row i of request b is staged row dev_rows[b][i] (ps_new_row, paged_store.h)
struct CommitRowsParams : WindowCommitParams {
    static constexpr bool kRows = true;
    const int *dev_rows;            // (bs, n_bound)
};

// million_window_commit_wide / million_window_commit_rows_wide: the first launch over uint16 pages or packed pages.  The sides
// carry the plain (M, C, d_m) fp16 codebooks (P::kWide: the scan reads them, the token store is store_codes4_wide); every other
// word is the commit's.  The append launch takes the WindowCommitParams / CommitRowsParams these blocks begin with.
struct WindowCommitWideParams : WindowCommitParams {
    static constexpr bool kWide = true;
    const f16 *k_cents, *v_cents;
    int packed;
    __device__ __forceinline__ PagedStoreSideT<f16> side(bool vside) const {
        return {vside ? v_new : k_new, vside ? v_win : k_win, vside ? v_cents : k_cents, vside ? v_pool : k_pool, nsb, nsh, nsn};
    }
};
struct CommitRowsWideParams : WindowCommitWideParams {
    static constexpr bool kRows = true;
    const int *dev_rows;            // (bs, n_bound)
};

typedef unsigned wv4 __attribute__((ext_vector_type(4)));

template <class P>
__device__ __forceinline__ void window_commit_append_body(const P &p) {
    const int l = blockIdx.x / p.bs, b = blockIdx.x % p.bs;
    int *row = p.dev_lengths + l * p.len_ls + 4ll * b;
    int T, r, st, a, f;
    bool ok;
    ps_load_row((const int *)row, p.dev_n, b, p, T, r, st, a);
    ps_commit_flush(p, T, r, a, f, ok);
    __syncthreads();      // every thread holds the row: thread 0 may write it
    if (a == 0 || !ok) return;
    const int vpr = p.d >> 3;      // 16-byte vectors per row
    const int total = p.nh_k * a * 2 * vpr;
    for (int t = threadIdx.x; t < total; t += kWcBlock) {
        const int col = t % vpr;
        const bool vside = (t / vpr) & 1;
        const int i = (t / (2 * vpr)) % a;
        const int hk = t / (2 * vpr * a);
        if (r + i < f) continue;      // the row became a token in the first launch
        const int slot = (st + r + i) % p.rcap;
        const f16 *src = (vside ? p.v_new : p.k_new) + l * p.nsl + b * p.nsb + hk * p.nsh + (long long)ps_new_row(p, b, i) * p.nsn + 8 * col;
        f16 *dst = (vside ? p.v_win : p.k_win) + l * p.win_ls + (((long long)b * p.nh_k + hk) * p.rcap + slot) * p.d + 8 * col;
        *(wv4 *)dst = *(const wv4 *)src;
    }
    if (threadIdx.x == 0) {
        row[0] = T + f;
        row[1] = r + a - f;
        row[2] = (st + f) % p.rcap;
    }
}

__global__ __launch_bounds__(kWcBlock) void window_commit_append_kernel(WindowCommitParams p) { window_commit_append_body(p); }

__global__ __launch_bounds__(kWcBlock) void window_commit_rows_append_kernel(CommitRowsParams p) { window_commit_append_body(p); }

}  // namespace

}  // namespace million

using namespace million;

// Validation and parameter fill shared by the two entries; `who` names the entry in the messages.  No HIP call.
// P::kWide: the codebooks are the plain fp16 ones and the geometry is the wide formats' (packed: the pools hold packed pages).
template <class P>
static int window_commit_fill(const char *who, const million_window_commit_desc *desc, const void *k_new, const void *v_new, void *k_resid,
                              void *v_resid, const void *k_cents_prepared, const void *v_cents_prepared, void *k_pool, void *v_pool,
                              const int32_t *page_ids, int32_t *dev_lengths, const int32_t *dev_n, P &p, int &dm, int packed = 0) {
    if (!desc || desc->struct_size != sizeof(million_window_commit_desc)) { set_error("%s: bad desc / struct_size", who); return MILLION_ERR_ARG; }
    const million_window_commit_desc &d = *desc;
    if (d.n_layers <= 0 || d.bs <= 0 || d.nh_k <= 0) { set_error("%s: n_layers=%d bs=%d nh_k=%d", who, d.n_layers, d.bs, d.nh_k); return MILLION_ERR_SHAPE; }
    int ps_shift;
    if constexpr (P::kWide) {
        if (!wide_geometry(d.d, d.M, d.C, 1) || (packed && d.M % 4)) {
            set_error("%s: d=%d M=%d C=%d (d 64 / 128, d / M 2 or 4, C 512 / 1024 / 2048 / 4096; packed pages: M a multiple of 4)", who, d.d, d.M, d.C);
            return MILLION_ERR_SHAPE;
        }
    } else if (!u8_geometry(who, d.d, d.M, d.C)) return MILLION_ERR_SHAPE;
    if (!page_shift(who, d.page_size, ps_shift)) return MILLION_ERR_SHAPE;
    if (d.n_bound < 1 || d.n_bound > kWcMaxRows || d.n_bound > d.page_size) {
        set_error("%s: n_bound=%d (1 .. %d, at most page_size=%d: one flush per request)", who, d.n_bound, kWcMaxRows, d.page_size);
        return MILLION_ERR_SHAPE;
    }
    if (d.resid_cap < d.page_size || (long long)d.resid_cap * d.d > 0x7fffffffLL) { set_error("%s: resid_cap=%d (at least page_size=%d)", who, d.resid_cap, d.page_size); return MILLION_ERR_SHAPE; }
    if (d.n_pages_cap <= 0 || d.n_pool <= 0 || (long long)d.n_pages_cap * d.page_size + d.resid_cap + d.n_bound > 0x7fffffffLL ||
        (long long)d.bs * d.nh_k * d.n_pages_cap > 0x7fffffffLL) {
        set_error("%s: n_pages_cap=%d n_pool=%d (page table of %lld entries)", who, d.n_pages_cap, d.n_pool, (long long)d.bs * d.nh_k * d.n_pages_cap);
        return MILLION_ERR_SHAPE;
    }
    dm = d.d / d.M;
    const int groups_y = (d.M / kPsSub + kWcBlock / 64 - 1) / (kWcBlock / 64);
    if ((long long)d.bs * d.nh_k * 2 > 65535 || (long long)d.n_layers * groups_y > 65535 || (long long)d.n_layers * d.bs > 0x7fffffffLL) {
        set_error("%s: bs * nh_k = %lld (at most 32767), n_layers=%d exceed the grid", who, (long long)d.bs * d.nh_k, d.n_layers);
        return MILLION_ERR_SHAPE;
    }
    if (dm != 1 && dm != 2 && dm != 4 && dm != 8) { set_error("%s: d/M=%d unsupported (1,2,4,8)", who, dm); return MILLION_ERR_SHAPE; }
    if (d.ids_layer_stride < 0 || d.rows_layer_stride < 0 || d.lengths_layer_stride < 0 ||
        (d.n_layers > 1 && (d.lengths_layer_stride < 4LL * d.bs || d.ids_layer_stride < (long long)d.bs * d.nh_k * d.n_pages_cap ||
                            d.rows_layer_stride < (long long)d.bs * d.nh_k * d.resid_cap * d.d))) {
        set_error("%s: layer strides %lld / %lld / %lld shorter than a layer", who, (long long)d.ids_layer_stride, (long long)d.rows_layer_stride,
                  (long long)d.lengths_layer_stride);
        return MILLION_ERR_ARG;
    }
    if (!dev_n || !dev_lengths) { set_error("%s: null dev_n / dev_lengths (every per-request value is read on the device)", who); return MILLION_ERR_ARG; }
    if (!k_new || !v_new || !k_resid || !v_resid) { set_error("%s: null new rows / windows", who); return MILLION_ERR_ARG; }
    if (!k_cents_prepared || !v_cents_prepared) {
        set_error(P::kWide ? "%s: null codebook (the plain (M, C, d_m) fp16 tensors: the call needs both)" : "%s: null prepared codebook (million_prepare_cents: the call needs both)", who);
        return MILLION_ERR_ARG;
    }
    if (!k_pool || !v_pool || !page_ids) { set_error("%s: null pools / page_ids", who); return MILLION_ERR_ARG; }
    const int rc = paged_store_fill(who, p, d.bs, d.nh_k, d.d, d.M, d.C, d.n_bound, d.resid_cap, d.page_size, ps_shift, d.n_pages_cap,
                                    (uintptr_t)k_new | (uintptr_t)v_new | (uintptr_t)k_resid | (uintptr_t)v_resid | (uintptr_t)k_cents_prepared |
                                        (uintptr_t)v_cents_prepared | (uintptr_t)k_pool | (uintptr_t)v_pool,
                                    page_ids, dev_lengths, dev_n);
    if (rc != MILLION_OK) return rc;
    if ((d.new_stride_l | d.new_stride_b | d.new_stride_h | d.new_stride_n | d.rows_layer_stride) & 7) {
        set_error("%s: fp16 strides must be multiples of 8 elements (16-byte rows)", who);
        return MILLION_ERR_ALIGN;
    }
    p.k_new = (const f16 *)k_new; p.v_new = (const f16 *)v_new;
    p.k_win = (f16 *)k_resid; p.v_win = (f16 *)v_resid;
    if constexpr (P::kWide) {
        p.k_cents = (const f16 *)k_cents_prepared; p.v_cents = (const f16 *)v_cents_prepared;
        p.packed = packed ? 1 : 0;
    } else {
        p.k_cents32 = prepared_cents32(k_cents_prepared, d.M, d.C, dm);
        p.v_cents32 = prepared_cents32(v_cents_prepared, d.M, d.C, dm);
    }
    p.k_pool = (uint8_t *)k_pool; p.v_pool = (uint8_t *)v_pool;
    p.nsl = d.new_stride_l; p.nsb = d.new_stride_b; p.nsh = d.new_stride_h; p.nsn = d.new_stride_n; p.ids_ls = d.ids_layer_stride; p.win_ls = d.rows_layer_stride; p.len_ls = d.lengths_layer_stride;
    p.n_layers = d.n_layers; p.n_pool = d.n_pool;
    p.groups_y = groups_y;
    return MILLION_OK;
}

extern "C" int million_window_commit(const million_window_commit_desc *desc, const void *k_new, const void *v_new, void *k_resid,
                                     void *v_resid, const void *k_cents_prepared, const void *v_cents_prepared, void *k_pool,
                                     void *v_pool, const int32_t *page_ids, int32_t *dev_lengths, const int32_t *dev_n,
                                     million_stream_t stream) {
    WindowCommitParams p;
    int dm;
    const int rc = window_commit_fill("window_commit", desc, k_new, v_new, k_resid, v_resid, k_cents_prepared, v_cents_prepared, k_pool, v_pool,
                                      page_ids, dev_lengths, dev_n, p, dm);
    if (rc != MILLION_OK) return rc;
    const million_window_commit_desc &d = *desc;
    const dim3 grid((d.page_size + 63) / 64, d.n_layers * p.groups_y, d.bs * d.nh_k * 2);
    hipStream_t s = (hipStream_t)stream;
    dispatch_dm(dm, [&](auto w) { hipLaunchKernelGGL((paged_store_kernel<w(), WindowCommitParams>), grid, dim3(kWcBlock), 0, s, p); });
    hipError_t e = hipGetLastError();
    if (e != hipSuccess) { set_error("window_commit encode launch: %s", hipGetErrorString(e)); return MILLION_ERR_LAUNCH; }
    hipLaunchKernelGGL(window_commit_append_kernel, dim3(d.n_layers * d.bs), dim3(kWcBlock), 0, s, p);
    e = hipGetLastError();
    if (e != hipSuccess) { set_error("window_commit append launch: %s", hipGetErrorString(e)); return MILLION_ERR_LAUNCH; }
    return MILLION_OK;
}

extern "C" int million_window_commit_rows(const million_window_commit_desc *desc, const void *k_new, const void *v_new, void *k_resid,
                                          void *v_resid, const void *k_cents_prepared, const void *v_cents_prepared, void *k_pool,
                                          void *v_pool, const int32_t *page_ids, int32_t *dev_lengths, const int32_t *dev_n,
                                          const int32_t *dev_rows, million_stream_t stream) {
    CommitRowsParams p;
    int dm;
    const int rc = window_commit_fill("window_commit_rows", desc, k_new, v_new, k_resid, v_resid, k_cents_prepared, v_cents_prepared, k_pool,
                                      v_pool, page_ids, dev_lengths, dev_n, p, dm);
    if (rc != MILLION_OK) return rc;
    if (!dev_rows) { set_error("window_commit_rows: null dev_rows (million_window_commit is the entry without row indices)"); return MILLION_ERR_ARG; }
    if ((uintptr_t)dev_rows & 3) { set_error("window_commit_rows: dev_rows must be 4-byte aligned"); return MILLION_ERR_ALIGN; }
    p.dev_rows = dev_rows;
    const million_window_commit_desc &d = *desc;
    const dim3 grid((d.page_size + 63) / 64, d.n_layers * p.groups_y, d.bs * d.nh_k * 2);
    hipStream_t s = (hipStream_t)stream;
    dispatch_dm(dm, [&](auto w) { hipLaunchKernelGGL((paged_store_kernel<w(), CommitRowsParams>), grid, dim3(kWcBlock), 0, s, p); });
    hipError_t e = hipGetLastError();
    if (e != hipSuccess) { set_error("window_commit_rows encode launch: %s", hipGetErrorString(e)); return MILLION_ERR_LAUNCH; }
    hipLaunchKernelGGL(window_commit_rows_append_kernel, dim3(d.n_layers * d.bs), dim3(kWcBlock), 0, s, p);
    e = hipGetLastError();
    if (e != hipSuccess) { set_error("window_commit_rows append launch: %s", hipGetErrorString(e)); return MILLION_ERR_LAUNCH; }
    return MILLION_OK;
}

// The two launches of the wide entries: paged_store_kernel with the wide block (d / M is 2 or 4: wide_geometry), then the append
// launch of the 8-bit entries over the block's WindowCommitParams / CommitRowsParams part.
template <class P, class Append, class AppendParams>
static int window_commit_wide_launch(const char *who, const million_window_commit_desc &d, const P &p, int dm, Append append, const AppendParams &pa,
                                     hipStream_t s) {
    const dim3 grid((d.page_size + 63) / 64, d.n_layers * p.groups_y, d.bs * d.nh_k * 2);
    if (dm == 2) hipLaunchKernelGGL((paged_store_kernel<2, P>), grid, dim3(kWcBlock), 0, s, p);
    else hipLaunchKernelGGL((paged_store_kernel<4, P>), grid, dim3(kWcBlock), 0, s, p);
    hipError_t e = hipGetLastError();
    if (e != hipSuccess) { set_error("%s encode launch: %s", who, hipGetErrorString(e)); return MILLION_ERR_LAUNCH; }
    hipLaunchKernelGGL(append, dim3(d.n_layers * d.bs), dim3(kWcBlock), 0, s, pa);
    e = hipGetLastError();
    if (e != hipSuccess) { set_error("%s append launch: %s", who, hipGetErrorString(e)); return MILLION_ERR_LAUNCH; }
    return MILLION_OK;
}

extern "C" int million_window_commit_wide(const million_window_commit_desc *desc, const void *k_new, const void *v_new, void *k_resid,
                                          void *v_resid, const void *k_cents, const void *v_cents, void *k_pool, void *v_pool,
                                          const int32_t *page_ids, int32_t *dev_lengths, const int32_t *dev_n, int packed,
                                          million_stream_t stream) {
    WindowCommitWideParams p;
    int dm;
    const int rc = window_commit_fill("window_commit_wide", desc, k_new, v_new, k_resid, v_resid, k_cents, v_cents, k_pool, v_pool, page_ids,
                                      dev_lengths, dev_n, p, dm, packed);
    if (rc != MILLION_OK) return rc;
    return window_commit_wide_launch("window_commit_wide", *desc, p, dm, window_commit_append_kernel, (const WindowCommitParams &)p, (hipStream_t)stream);
}

extern "C" int million_window_commit_rows_wide(const million_window_commit_desc *desc, const void *k_new, const void *v_new, void *k_resid,
                                               void *v_resid, const void *k_cents, const void *v_cents, void *k_pool, void *v_pool,
                                               const int32_t *page_ids, int32_t *dev_lengths, const int32_t *dev_n,
                                               const int32_t *dev_rows, int packed, million_stream_t stream) {
    CommitRowsWideParams p;
    int dm;
    const int rc = window_commit_fill("window_commit_rows_wide", desc, k_new, v_new, k_resid, v_resid, k_cents, v_cents, k_pool, v_pool,
                                      page_ids, dev_lengths, dev_n, p, dm, packed);
    if (rc != MILLION_OK) return rc;
    if (!dev_rows) { set_error("window_commit_rows_wide: null dev_rows (million_window_commit_wide is the entry without row indices)"); return MILLION_ERR_ARG; }
    if ((uintptr_t)dev_rows & 3) { set_error("window_commit_rows_wide: dev_rows must be 4-byte aligned"); return MILLION_ERR_ALIGN; }
    p.dev_rows = dev_rows;
    CommitRowsParams pa;
    (WindowCommitParams &)pa = (const WindowCommitParams &)p;
    pa.dev_rows = dev_rows;
    return window_commit_wide_launch("window_commit_rows_wide", *desc, p, dm, window_commit_rows_append_kernel, pa, (hipStream_t)stream);
}
