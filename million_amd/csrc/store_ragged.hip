// store_ragged.hip — the store step of a ragged batch in one launch (million_pq_store_ragged), gfx950.
//
// Behind a ragged attention launch (million_pq_chunk_attn with dev_lengths / dev_n_q, million_prefill_attn with dev_spans)
// PagedPQCache._store was a host loop: per slot up to four million_pq_encode launches (K and V of the window in ring order,
// K and V of the new rows) and a host-to-device copy of the slot's lengths row, each with host values baked in.  Here every
// request of the batch is stored by ONE encode launch that reads {T, r, start} and n_b on the device, followed by a
// one-thread-per-request launch that advances the lengths rows: stream order is all the ordering there is (the pattern of
// chunk_merge_kernel: two plain launches, no atomics, tickets or polls).
//
// Per request b (values clamped, see sr_load_row): r + n_b source rows - row j < r is window row (start + j) % resid_cap,
// row j >= r is new row j - r - and source row j becomes token T + j of the request's K pages and transposed V pages.
//
// Arithmetic: the contract and the centroid scan of every encoder kernel, pq_scan_sgpr (pq_scan.h).  pq_encode_kernel's mapping
// (encode.hip) too: lane = token, a wave owns 4 consecutive subspaces, the centroid rows are wave-uniform and come through the
// scalar cache from the fp32 image of the prepared codebook.  The grid is a function of the bounds alone
// (ceil((resid_cap + n_bound) / 64) token blocks x subspace groups x (bs * nh_k) x 2 sides), so a captured launch follows the
// lengths: a block at or past r_b + n_b leaves before its first vector load, a straddling block clamps its dead lanes to the
// last live row and does not store them.  No load sits in a lane-conditional: the source address is selected (window or new
// rows), the page index is clamped to a page that receives a token of the block.  No LDS.
#include <string.h>

#include "common.h"
#include "pq_scan.h"

#pragma clang fp contract(off)

namespace million {

constexpr int kSrBlock = 256;
constexpr int kSrSub = 4;      // subspaces per wave (M is a multiple of 4 on every supported shape)

struct StoreRaggedSide {
    const f16 *new_rows;        // new rows (bs, nh_k, n_bound, d)
    const f16 *win;             // window (bs, nh_k, resid_cap, d); null when resid_cap = 0
    const float *cents32;       // fp32 row image [m][c][dm] of the prepared codebook
    uint8_t *pool;              // K pool (n_pool, page_size, M) / V pool (n_pool, M, page_size)
    long long nsb, nsh, nsn;    // the new rows' strides, fp16 elements
};
struct StoreRaggedParams {
    StoreRaggedSide k, v;
    const int *page_ids;        // (bs, nh_k, n_pages_cap)
    const int *dev_lengths;     // (bs, 4)
    const int *dev_n;           // (bs,)
    long long wsb, wsh;         // window strides (row stride d)
    int bs, nh_k, d, M, C;
    int n_bound, rcap;
    int page_size, ps_shift, n_pages_cap, cap_tok;
};

// The request's row as every kernel of this file reads it.  Device-resident values are not trusted: T into [0, cap_tok],
// r into [0, resid_cap], a start outside [0, resid_cap) reads as 0, n into [0, n_bound]; word 3 is not touched.
template <typename IntP>
__device__ __forceinline__ void sr_load_row(IntP dev_lengths, IntP dev_n, int b, int cap_tok, int rcap, int n_bound,
                                            int &T, int &r, int &st, int &n) {
    T = dev_lengths[4 * b];
    r = dev_lengths[4 * b + 1];
    st = dev_lengths[4 * b + 2];
    n = dev_n[b];
    T = T < 0 ? 0 : (T > cap_tok ? cap_tok : T);
    r = r < 0 ? 0 : (r > rcap ? rcap : r);
    st = (unsigned)st < (unsigned)rcap ? st : 0;
    n = n < 0 ? 0 : (n > n_bound ? n_bound : n);
}

template <int DM>
__global__ __launch_bounds__(kSrBlock) void pq_store_ragged_kernel(StoreRaggedParams p) {
    const int lane = threadIdx.x & 63;
    const int mg = __builtin_amdgcn_readfirstlane((int)(blockIdx.y * (kSrBlock / 64) + (threadIdx.x >> 6)));
    const int m0 = mg * kSrSub;
    const bool vside = blockIdx.z & 1;    // workgroup-uniform
    // field by field: a reference selected between the two kernel-argument structs is read back with vector loads
    StoreRaggedSide sd;
    sd.new_rows = vside ? p.v.new_rows : p.k.new_rows;
    sd.win = vside ? p.v.win : p.k.win;
    sd.cents32 = vside ? p.v.cents32 : p.k.cents32;
    sd.pool = vside ? p.v.pool : p.k.pool;
    sd.nsb = vside ? p.v.nsb : p.k.nsb;
    sd.nsh = vside ? p.v.nsh : p.k.nsh;
    sd.nsn = vside ? p.v.nsn : p.k.nsn;
    const int bh = blockIdx.z >> 1;
    const int b = bh / p.nh_k, hk = bh % p.nh_k;
    if (m0 >= p.M) return;
    int T, r, st, n;
    {
        // through the constant address space: neither array is written while this kernel runs (the advance is the next launch),
        // and only so does hipcc read them with scalar loads (a plain global pointer might alias the pools: vector loads and
        // v_readfirstlane instead)
        typedef const __attribute__((address_space(4))) int *const_p;
        sr_load_row((const_p)p.dev_lengths, (const_p)p.dev_n, b, p.cap_tok, p.rcap, p.n_bound, T, r, st, n);
    }
    if (n == 0) return;                   // the request takes no part: nothing of it is read beyond those words
    const int rows = r + n;
    const int j0 = blockIdx.x * 64;
    // workgroup-uniform exits before the first vector load: a block past the request's rows, a block whose first token lies
    // past the page table (every token of it would drop its store)
    if (j0 >= rows || ((T + j0) >> p.ps_shift) >= p.n_pages_cap) return;
    const int j = j0 + lane;
    const bool valid = j < rows;
    const int jc = valid ? j : rows - 1;
    // source row: the address is selected, the load is one
    const int rmod = p.rcap > 0 ? p.rcap : 1;
    const long long off_w = b * p.wsb + hk * p.wsh + (long long)((st + jc) % rmod) * p.d;
    const long long off_n = b * sd.nsb + hk * sd.nsh + (long long)(jc - r) * sd.nsn;
    const f16 *xp = (jc < r ? sd.win + off_w : sd.new_rows + off_n) + m0 * DM;
    float x[kSrSub][DM];
#pragma unroll
    for (int s = 0; s < kSrSub; ++s)
#pragma unroll
        for (int k = 0; k < DM; ++k) x[s][k] = (float)xp[s * DM + k];
    // destination: token T + j; the page index of a dead or dropped lane is clamped to a page that receives a token of this
    // block (the block's first token lies inside the table, so page n_pages_cap - 1 does whenever a later lane lies past it)
    const int tok = T + jc;
    const int page = tok >> p.ps_shift;
    const bool keep = valid && page < p.n_pages_cap;
    const long long pid = p.page_ids[(long long)bh * p.n_pages_cap + (page < p.n_pages_cap ? page : p.n_pages_cap - 1)];

    unsigned codes = 0;
    const float *__restrict__ tab = sd.cents32;
#pragma unroll
    for (int s = 0; s < kSrSub; ++s) {
        float best = INFINITY;
        int best_c = 0;
        pq_scan_sgpr<DM>(x[s], tab + (long long)(m0 + s) * p.C * DM, p.C, best, best_c);   // wave-uniform rows
        codes |= (unsigned)best_c << (8 * s);
    }
    if (!keep) return;
    const int off = tok & (p.page_size - 1);
    if (!vside) {
        // K page (page_size, M): the token's 4 code bytes are one aligned 32-bit store (M and m0 are multiples of 4)
        *(unsigned *)(sd.pool + (pid * p.page_size + off) * p.M + m0) = codes;
    } else {
        // transposed V page (M, page_size): four lane-contiguous byte rows
        uint8_t *dst = sd.pool + (pid * p.M + m0) * p.page_size + off;
#pragma unroll
        for (int s = 0; s < kSrSub; ++s) dst[s * p.page_size] = (uint8_t)(codes >> (8 * s));
    }
}

// One thread per request, after the encode launch on the same stream: T <- min(T + r + n, cap_tok), r <- 0, start <- 0 from
// the clamped values; word 3 and the rows with n = 0 are not touched.
__global__ void store_ragged_advance_kernel(int *dev_lengths, const int *dev_n, int bs, int cap_tok, int rcap, int n_bound) {
    const int b = blockIdx.x * blockDim.x + threadIdx.x;
    if (b >= bs) return;
    int T, r, st, n;
    sr_load_row((const int *)dev_lengths, dev_n, b, cap_tok, rcap, n_bound, T, r, st, n);
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
    if ((d.d != 128 && d.d != 64) || (d.M != 16 && d.M != 32 && d.M != 64) || d.C < 1 || d.C > 256) {
        set_error("store_ragged: d=%d M=%d C=%d (d 64 / 128, M 16 / 32 / 64, C 1 .. 256: uint8 codes)", d.d, d.M, d.C);
        return MILLION_ERR_SHAPE;
    }
    if (d.page_size != 32 && d.page_size != 64 && d.page_size != 128) { set_error("store_ragged: page_size=%d (32, 64 or 128)", d.page_size); return MILLION_ERR_SHAPE; }
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
    if (((uintptr_t)k_new | (uintptr_t)v_new | (uintptr_t)k_resid | (uintptr_t)v_resid | (uintptr_t)k_cents_prepared |
         (uintptr_t)v_cents_prepared | (uintptr_t)k_pool | (uintptr_t)v_pool) & 15) {
        set_error("store_ragged: rows, windows, prepared codebooks and pools must be 16-byte aligned");
        return MILLION_ERR_ALIGN;
    }
    if (((uintptr_t)page_ids | (uintptr_t)dev_lengths | (uintptr_t)dev_n) & 3) { set_error("store_ragged: page_ids / dev_lengths / dev_n must be 4-byte aligned"); return MILLION_ERR_ALIGN; }
    if ((d.kn_stride_b | d.kn_stride_h | d.kn_stride_n | d.vn_stride_b | d.vn_stride_h | d.vn_stride_n | d.resid_stride_b | d.resid_stride_h) & 7) {
        set_error("store_ragged: fp16 strides must be multiples of 8 elements (16-byte rows)");
        return MILLION_ERR_ALIGN;
    }
    StoreRaggedParams p;
    memset(&p, 0, sizeof(p));
    const int dm = d.d / d.M;
    const size_t tab = (size_t)d.M * d.C * dm;      // prepared blob: two fp16 images, then the fp32 row image
    p.k.new_rows = (const f16 *)k_new; p.v.new_rows = (const f16 *)v_new;
    p.k.win = (const f16 *)k_resid; p.v.win = (const f16 *)v_resid;
    p.k.cents32 = (const float *)((const f16 *)k_cents_prepared + 2 * tab);
    p.v.cents32 = (const float *)((const f16 *)v_cents_prepared + 2 * tab);
    p.k.pool = (uint8_t *)k_pool; p.v.pool = (uint8_t *)v_pool;
    p.page_ids = page_ids; p.dev_lengths = dev_lengths; p.dev_n = dev_n;
    p.k.nsb = d.kn_stride_b; p.k.nsh = d.kn_stride_h; p.k.nsn = d.kn_stride_n;
    p.v.nsb = d.vn_stride_b; p.v.nsh = d.vn_stride_h; p.v.nsn = d.vn_stride_n;
    p.wsb = d.resid_stride_b; p.wsh = d.resid_stride_h;
    p.bs = d.bs; p.nh_k = d.nh_k; p.d = d.d; p.M = d.M; p.C = d.C;
    p.n_bound = d.n_bound; p.rcap = d.resid_cap;
    p.page_size = d.page_size; p.ps_shift = d.page_size == 32 ? 5 : d.page_size == 64 ? 6 : 7;
    p.n_pages_cap = d.n_pages_cap; p.cap_tok = d.n_pages_cap * d.page_size;
    const int groups = d.M / kSrSub;
    const dim3 grid(((long long)d.resid_cap + d.n_bound + 63) / 64, (groups + kSrBlock / 64 - 1) / (kSrBlock / 64), d.bs * d.nh_k * 2);
    hipStream_t s = (hipStream_t)stream;
    if (!dispatch_dm(dm, [&](auto w) { hipLaunchKernelGGL((pq_store_ragged_kernel<w()>), grid, dim3(kSrBlock), 0, s, p); })) {
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
