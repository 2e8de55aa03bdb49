// window_commit.hip — append the accepted rows of a draft verification to the residual windows of a paged cache, every layer in
// one call (million_window_commit, include/million_hip.h), gfx950.
//
// Request b accepted a_b = dev_n[b] of the rows in k_new / v_new (layers, bs, nh_k, n_bound, d).  The cache is left exactly as a_b
// decode steps would have left it, where a decode step is "if the window is full, flush its oldest page_size rows; append".  A
// flush encodes the oldest rows and a code depends on its row and the codebook alone, so the a_b steps have a closed form, per
// (layer, b) with the clamped {T, r, start} of the request's lengths row (sr_load_row's clamps):
//   source sequence  S = [the r window rows in ring order; the a new rows];
//   F = ceil((r + a - cap) / page_size) if r + a > cap else 0 (0 or 1: n_bound <= page_size), f = F * page_size;
//   S[0, f) becomes tokens [T, T + f) of the K pages and the transposed V pages; the new rows with source index >= f go to ring
//   slot (start + r + i) % cap; then T += f, r += a - f, start = (start + f) % cap.  Word 3 is not touched.
// Two plain launches on one stream (the pattern of store_ragged.hip: no atomics, tickets or polls):
//   1. window_commit_encode_kernel: pq_store_ragged_kernel's mapping (lane = token, a wave owns 4 consecutive subspaces, the scan
//      of pq_scan.h over the fp32 row image read through the scalar cache), so the codes are what million_pq_flush writes.  The
//      grid is a function of the bounds alone; a block of a request with f = 0 leaves before its first vector load.
//   2. window_commit_append_kernel: one workgroup per (layer, b) copies the rows that stay in the window and then advances the
//      lengths row.  It comes second because the ring slots it writes may hold rows the first launch reads; inside it every
//      thread has read the lengths row before the barrier that precedes the one thread's write.
// A request whose T + f would pass the page table is left untouched by both launches.
#include <string.h>

#include "common.h"
#include "pq_scan.h"

#pragma clang fp contract(off)

namespace million {

namespace {

constexpr int kWcBlock = 256;
constexpr int kWcSub = 4;           // subspaces per wave (M is a multiple of 4 on every supported shape)
constexpr int kWcMaxRows = 16;      // new rows per request, at most

struct WindowCommitParams {
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
};

// The request's row of layer l and its accepted rows, clamped as sr_load_row (store_ragged.hip) clamps them, and the flush the
// commit implies: f rows (0 or page_size) leave the window's front.  ok = false: T + f would pass the page table.
template <typename IntP>
__device__ __forceinline__ void wc_load_row(IntP row, IntP dev_n, int b, const WindowCommitParams &p, int &T, int &r, int &st,
                                            int &a, int &f, bool &ok) {
    T = row[0]; r = row[1]; st = row[2];
    a = dev_n[b];
    T = T < 0 ? 0 : (T > p.cap_tok ? p.cap_tok : T);
    r = r < 0 ? 0 : (r > p.rcap ? p.rcap : r);
    st = (unsigned)st < (unsigned)p.rcap ? st : 0;
    a = a < 0 ? 0 : (a > p.n_bound ? p.n_bound : a);
    f = r + a > p.rcap ? p.page_size : 0;
    ok = (long long)T + f <= p.cap_tok;
}

template <int DM>
__global__ __launch_bounds__(kWcBlock) void window_commit_encode_kernel(WindowCommitParams p) {
    const int lane = threadIdx.x & 63;
    const int l = blockIdx.y / p.groups_y;
    const int mg = __builtin_amdgcn_readfirstlane((int)((blockIdx.y % p.groups_y) * (kWcBlock / 64) + (threadIdx.x >> 6)));
    const int m0 = mg * kWcSub;
    const bool vside = blockIdx.z & 1;      // workgroup-uniform
    const int bh = blockIdx.z >> 1;
    const int b = bh / p.nh_k, hk = bh % p.nh_k;
    if (m0 >= p.M) return;
    int T, r, st, a, f;
    bool ok;
    {
        // through the constant address space: neither array is written while this kernel runs (the advance is the next launch)
        typedef const __attribute__((address_space(4))) int *const_p;
        wc_load_row((const_p)(p.dev_lengths + l * p.len_ls + 4ll * b), (const_p)p.dev_n, b, p, T, r, st, a, f, ok);
    }
    const int j0 = blockIdx.x * 64;
    if (f == 0 || !ok || j0 >= f) return;      // workgroup-uniform, before the first vector load
    const int j = j0 + lane;
    const bool valid = j < f;
    const int jc = valid ? j : f - 1;
    // source row: the address is selected, the load is one.  jc - r < a: r + a > rcap >= page_size = f
    const f16 *win = vside ? p.v_win : p.k_win;
    const f16 *rows = vside ? p.v_new : p.k_new;
    const long long off_w = l * p.win_ls + (((long long)b * p.nh_k + hk) * p.rcap + (st + jc) % p.rcap) * p.d;
    const long long off_n = l * p.nsl + b * p.nsb + hk * p.nsh + (long long)(jc - r) * p.nsn;
    const f16 *xp = (jc < r ? win + off_w : rows + off_n) + m0 * DM;
    float x[kWcSub][DM];
#pragma unroll
    for (int s = 0; s < kWcSub; ++s)
#pragma unroll
        for (int k = 0; k < DM; ++k) x[s][k] = (float)xp[s * DM + k];
    // destination: token T + jc, inside the page table (T + f <= cap_tok); an id outside the pool drops the store
    const int tok = T + jc;
    const int page = tok >> p.ps_shift;
    const int pid = p.page_ids[l * p.ids_ls + (long long)bh * p.n_pages_cap + page];
    const bool keep = valid && (unsigned)pid < (unsigned)p.n_pool;

    unsigned codes = 0;
    const float *__restrict__ tab = vside ? p.v_cents32 : p.k_cents32;
#pragma unroll
    for (int s = 0; s < kWcSub; ++s) {
        float best = INFINITY;
        int best_c = 0;
        pq_scan_sgpr<DM>(x[s], tab + (long long)(m0 + s) * p.C * DM, p.C, best, best_c);      // wave-uniform rows
        codes |= (unsigned)best_c << (8 * s);
    }
    if (!keep) return;
    const int off = tok & (p.page_size - 1);
    if (!vside) {
        // K page (page_size, M): the token's 4 code bytes are one aligned 32-bit store
        *(unsigned *)(p.k_pool + ((long long)pid * p.page_size + off) * p.M + m0) = codes;
    } else {
        // transposed V page (M, page_size): four lane-contiguous byte rows
        uint8_t *dst = p.v_pool + ((long long)pid * p.M + m0) * p.page_size + off;
#pragma unroll
        for (int s = 0; s < kWcSub; ++s) dst[s * p.page_size] = (uint8_t)(codes >> (8 * s));
    }
}

typedef unsigned wv4 __attribute__((ext_vector_type(4)));

__global__ __launch_bounds__(kWcBlock) void window_commit_append_kernel(WindowCommitParams p) {
    const int l = blockIdx.x / p.bs, b = blockIdx.x % p.bs;
    int *row = p.dev_lengths + l * p.len_ls + 4ll * b;
    int T, r, st, a, f;
    bool ok;
    wc_load_row((const int *)row, p.dev_n, b, p, T, r, st, a, f, ok);
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
        const f16 *src = (vside ? p.v_new : p.k_new) + l * p.nsl + b * p.nsb + hk * p.nsh + (long long)i * p.nsn + 8 * col;
        f16 *dst = (vside ? p.v_win : p.k_win) + l * p.win_ls + (((long long)b * p.nh_k + hk) * p.rcap + slot) * p.d + 8 * col;
        *(wv4 *)dst = *(const wv4 *)src;
    }
    if (threadIdx.x == 0) {
        row[0] = T + f;
        row[1] = r + a - f;
        row[2] = (st + f) % p.rcap;
    }
}

}  // namespace

}  // namespace million

using namespace million;

extern "C" int million_window_commit(const million_window_commit_desc *desc, const void *k_new, const void *v_new, void *k_resid,
                                     void *v_resid, const void *k_cents_prepared, const void *v_cents_prepared, void *k_pool,
                                     void *v_pool, const int32_t *page_ids, int32_t *dev_lengths, const int32_t *dev_n,
                                     million_stream_t stream) {
    if (!desc || desc->struct_size != sizeof(million_window_commit_desc)) { set_error("window_commit: bad desc / struct_size"); return MILLION_ERR_ARG; }
    const million_window_commit_desc &d = *desc;
    if (d.n_layers <= 0 || d.bs <= 0 || d.nh_k <= 0) { set_error("window_commit: n_layers=%d bs=%d nh_k=%d", d.n_layers, d.bs, d.nh_k); return MILLION_ERR_SHAPE; }
    if ((d.d != 128 && d.d != 64) || (d.M != 16 && d.M != 32 && d.M != 64) || d.C < 1 || d.C > 256) {
        set_error("window_commit: d=%d M=%d C=%d (d 64 / 128, M 16 / 32 / 64, C 1 .. 256: uint8 codes)", d.d, d.M, d.C);
        return MILLION_ERR_SHAPE;
    }
    if (d.page_size != 32 && d.page_size != 64 && d.page_size != 128) { set_error("window_commit: page_size=%d (32, 64 or 128)", d.page_size); return MILLION_ERR_SHAPE; }
    if (d.n_bound < 1 || d.n_bound > kWcMaxRows || d.n_bound > d.page_size) {
        set_error("window_commit: n_bound=%d (1 .. %d, at most page_size=%d: one flush per request)", d.n_bound, kWcMaxRows, d.page_size);
        return MILLION_ERR_SHAPE;
    }
    if (d.resid_cap < d.page_size || (long long)d.resid_cap * d.d > 0x7fffffffLL) { set_error("window_commit: resid_cap=%d (at least page_size=%d)", d.resid_cap, d.page_size); return MILLION_ERR_SHAPE; }
    if (d.n_pages_cap <= 0 || d.n_pool <= 0 || (long long)d.n_pages_cap * d.page_size + d.resid_cap + d.n_bound > 0x7fffffffLL ||
        (long long)d.bs * d.nh_k * d.n_pages_cap > 0x7fffffffLL) {
        set_error("window_commit: n_pages_cap=%d n_pool=%d (page table of %lld entries)", d.n_pages_cap, d.n_pool, (long long)d.bs * d.nh_k * d.n_pages_cap);
        return MILLION_ERR_SHAPE;
    }
    const int dm = d.d / d.M;
    const int groups_y = (d.M / kWcSub + kWcBlock / 64 - 1) / (kWcBlock / 64);
    if ((long long)d.bs * d.nh_k * 2 > 65535 || (long long)d.n_layers * groups_y > 65535 || (long long)d.n_layers * d.bs > 0x7fffffffLL) {
        set_error("window_commit: bs * nh_k = %lld (at most 32767), n_layers=%d exceed the grid", (long long)d.bs * d.nh_k, d.n_layers);
        return MILLION_ERR_SHAPE;
    }
    if (dm != 1 && dm != 2 && dm != 4 && dm != 8) { set_error("window_commit: d/M=%d unsupported (1,2,4,8)", dm); return MILLION_ERR_SHAPE; }
    if (d.ids_layer_stride < 0 || d.rows_layer_stride < 0 || d.lengths_layer_stride < 0 ||
        (d.n_layers > 1 && (d.lengths_layer_stride < 4LL * d.bs || d.ids_layer_stride < (long long)d.bs * d.nh_k * d.n_pages_cap ||
                            d.rows_layer_stride < (long long)d.bs * d.nh_k * d.resid_cap * d.d))) {
        set_error("window_commit: layer strides %lld / %lld / %lld shorter than a layer", (long long)d.ids_layer_stride, (long long)d.rows_layer_stride,
                  (long long)d.lengths_layer_stride);
        return MILLION_ERR_ARG;
    }
    if (!dev_n || !dev_lengths) { set_error("window_commit: null dev_n / dev_lengths (every per-request value is read on the device)"); return MILLION_ERR_ARG; }
    if (!k_new || !v_new || !k_resid || !v_resid) { set_error("window_commit: null new rows / windows"); return MILLION_ERR_ARG; }
    if (!k_cents_prepared || !v_cents_prepared) { set_error("window_commit: null prepared codebook (million_prepare_cents: the call needs both)"); return MILLION_ERR_ARG; }
    if (!k_pool || !v_pool || !page_ids) { set_error("window_commit: null pools / page_ids"); return MILLION_ERR_ARG; }
    if (((uintptr_t)k_new | (uintptr_t)v_new | (uintptr_t)k_resid | (uintptr_t)v_resid | (uintptr_t)k_cents_prepared |
         (uintptr_t)v_cents_prepared | (uintptr_t)k_pool | (uintptr_t)v_pool) & 15) {
        set_error("window_commit: rows, windows, prepared codebooks and pools must be 16-byte aligned");
        return MILLION_ERR_ALIGN;
    }
    if (((uintptr_t)page_ids | (uintptr_t)dev_lengths | (uintptr_t)dev_n) & 3) { set_error("window_commit: page_ids / dev_lengths / dev_n must be 4-byte aligned"); return MILLION_ERR_ALIGN; }
    if ((d.new_stride_l | d.new_stride_b | d.new_stride_h | d.new_stride_n | d.rows_layer_stride) & 7) {
        set_error("window_commit: fp16 strides must be multiples of 8 elements (16-byte rows)");
        return MILLION_ERR_ALIGN;
    }
    WindowCommitParams p;
    memset(&p, 0, sizeof(p));
    const size_t tab = (size_t)d.M * d.C * dm;      // prepared blob: two fp16 images, then the fp32 row image
    p.k_new = (const f16 *)k_new; p.v_new = (const f16 *)v_new;
    p.k_win = (f16 *)k_resid; p.v_win = (f16 *)v_resid;
    p.k_cents32 = (const float *)((const f16 *)k_cents_prepared + 2 * tab);
    p.v_cents32 = (const float *)((const f16 *)v_cents_prepared + 2 * tab);
    p.k_pool = (uint8_t *)k_pool; p.v_pool = (uint8_t *)v_pool;
    p.page_ids = page_ids; p.dev_lengths = dev_lengths; p.dev_n = dev_n;
    p.nsl = d.new_stride_l; p.nsb = d.new_stride_b; p.nsh = d.new_stride_h; p.nsn = d.new_stride_n;
    p.ids_ls = d.ids_layer_stride; p.win_ls = d.rows_layer_stride; p.len_ls = d.lengths_layer_stride;
    p.n_layers = d.n_layers; p.bs = d.bs; p.nh_k = d.nh_k; p.d = d.d; p.M = d.M; p.C = d.C;
    p.n_bound = d.n_bound; p.rcap = d.resid_cap;
    p.page_size = d.page_size; p.ps_shift = d.page_size == 32 ? 5 : d.page_size == 64 ? 6 : 7;
    p.n_pages_cap = d.n_pages_cap; p.cap_tok = d.n_pages_cap * d.page_size; p.n_pool = d.n_pool;
    p.groups_y = groups_y;
    const dim3 grid((d.page_size + 63) / 64, d.n_layers * groups_y, d.bs * d.nh_k * 2);
    hipStream_t s = (hipStream_t)stream;
    dispatch_dm(dm, [&](auto w) { hipLaunchKernelGGL((window_commit_encode_kernel<w()>), grid, dim3(kWcBlock), 0, s, p); });
    hipError_t e = hipGetLastError();
    if (e != hipSuccess) { set_error("window_commit encode launch: %s", hipGetErrorString(e)); return MILLION_ERR_LAUNCH; }
    hipLaunchKernelGGL(window_commit_append_kernel, dim3(d.n_layers * d.bs), dim3(kWcBlock), 0, s, p);
    e = hipGetLastError();
    if (e != hipSuccess) { set_error("window_commit append launch: %s", hipGetErrorString(e)); return MILLION_ERR_LAUNCH; }
    return MILLION_OK;
}
