// cache_fork_wide.hip — million_cache_fork over uint16 or packed code pages (million_cache_fork_wide), gfx950.
//
// cache_fork.hip's call, task list and kernel body with one difference: a page is page_bytes = page_size * M * 2 bytes (uint16
// pools) or page_size * M * (8 + h) / 8 bytes (packed pools: the low plane and the high plane of a page lie behind each other and
// are copied as one byte string).  A packed page is no power of two, so a page starts at id * page_bytes in 64-bit arithmetic and
// a task's vector index is split by division, not by shifts.  It is a kernel of its own so that cache_fork_kernel keeps its code.
// Everything else - SHARE / COPY, the clamps of the source row, the prefix, dropped ids, destinations that take no part, the
// window and meta tasks, no atomics, flags or workspace - is cache_fork.hip's, word for word; the comments there apply.
#include <string.h>

#include "common.h"

namespace million {

constexpr int kForkWBlock = 256;
constexpr int kForkWMaxGrid = 2048;
constexpr int kForkWGroupBytes = 16384;   // per side and page task: G = kForkWGroupBytes / page_bytes pages, 1 <= G <= kForkWMaxG
constexpr int kForkWMaxG = 32;
constexpr int kForkWWinBytes = 16384;     // per side and window task
constexpr int kForkWUnroll = 8;           // 16-byte loads in flight per thread

typedef unsigned fwv4 __attribute__((ext_vector_type(4)));

struct ForkWideParams {
    int *page_ids;              // (layers, bs, nh_k, n_pages_cap)
    uint8_t *k_pool, *v_pool;   // pages of page_bytes bytes
    uint8_t *k_win, *v_win;     // (layers, bs, nh_k, resid_cap, d) fp16, as bytes
    int *dev_lengths;           // (layers, bs, 4)
    const int *dst_slots;       // (n_dst,)
    const int *tail_ids;        // (n_dst, layers, nh_k); SHARE only
    long long ids_ls, win_ls_bytes, len_ls;
    int n_layers, bs, nh_k, n_pages_cap, n_pool;
    int page_bytes, vpp;        // bytes and 16-byte vectors of one page of one side (640 .. 16384 bytes)
    int page_size, ps_shift;
    int win_bytes, rcap;
    int src, n_dst, share;
    int n_pages_bound, cap_tok, prefix;
    int G, n_ptasks, n_wtasks;
    long long n_tasks;
};

__device__ __forceinline__ void forkw_load_row(const ForkWideParams &p, int l, int &T, int &r, int &st) {
    typedef const __attribute__((address_space(4))) int *const_p;
    load_len_row((const_p)(p.dev_lengths + l * p.len_ls + 4ll * p.src), p.cap_tok, p.rcap, p.rcap, T, r, st);
    if (p.prefix >= 0) { T = T < p.prefix ? T : p.prefix; r = 0; st = 0; }
}

__device__ __forceinline__ int forkw_dst(const ForkWideParams &p, int jd) {
    typedef const __attribute__((address_space(4))) int *const_p;
    const_p slots = (const_p)p.dst_slots;
    const int dst = slots[jd];
    if ((unsigned)dst >= (unsigned)p.bs || dst == p.src) return -1;
    for (int i = 0; i < jd; ++i)
        if (slots[i] == dst) return -1;
    return dst;
}

__global__ __launch_bounds__(kForkWBlock) __attribute__((amdgpu_waves_per_eu(4))) void cache_fork_wide_kernel(ForkWideParams p) {
    __shared__ long long s_src[kForkWMaxG], s_dst[kForkWMaxG];      // byte offsets of the task's pages; s_dst < 0: not copied
    const int tid = threadIdx.x;
    const int per_row = p.n_ptasks + p.n_wtasks + 1;
#pragma unroll 1
    for (long long t = blockIdx.x; t < p.n_tasks; t += gridDim.x) {      // workgroup-uniform
        const int sub = (int)(t % per_row);
        const int row = (int)(t / per_row);
        const int h = row % p.nh_k;
        const int jd = (row / p.nh_k) % p.n_dst;
        const int l = row / (p.nh_k * p.n_dst);
        const int dst = forkw_dst(p, jd);
        if (dst < 0) continue;
        int T, r, st;
        forkw_load_row(p, l, T, r, st);
        const int full = T >> p.ps_shift;
        const int n_live = full + ((T & (p.page_size - 1)) ? 1 : 0);      // <= n_pages_bound <= n_pages_cap
        const int *src_ids = p.page_ids + l * p.ids_ls + ((long long)p.src * p.nh_k + h) * p.n_pages_cap;
        int *dst_ids = p.page_ids + l * p.ids_ls + ((long long)dst * p.nh_k + h) * p.n_pages_cap;

        if (sub < p.n_ptasks) {
            // ---- G pages, both sides.  SHARE: the one page task of the row is the tail page, when there is one.
            const int j0 = p.share ? full : sub * p.G;
            const int ng = p.share ? (n_live > full ? 1 : 0) : (n_live - j0 < p.G ? n_live - j0 : p.G);
            if (ng <= 0) continue;
            __syncthreads();      // the previous task's readers of s_src / s_dst are done
            if (tid < ng) {
                const int j = j0 + tid;
                const int sid = src_ids[j];
                const int e = p.share ? p.tail_ids[((long long)jd * p.n_layers + l) * p.nh_k + h] : dst_ids[j];
                const bool copy = e != sid && (unsigned)e < (unsigned)p.n_pool && (unsigned)sid < (unsigned)p.n_pool;
                s_src[tid] = (long long)sid * p.page_bytes;
                s_dst[tid] = copy ? (long long)e * p.page_bytes : -1;
            }
            __syncthreads();
            // vector i of the task: page g = i / (2 * vpp), side (i / vpp) & 1, vector i % vpp of that page.  G * page_bytes <=
            // kForkWGroupBytes or G = 1: nvec <= 2048, one pass of the workgroup
            const unsigned vpp = (unsigned)p.vpp;
            const int nvec = ng * 2 * p.vpp;
#pragma unroll 1
            for (int base = 0; base < nvec; base += kForkWBlock * kForkWUnroll) {
                fwv4 v[kForkWUnroll];
                int g[kForkWUnroll], in_page[kForkWUnroll];      // in_page < 0: the V side
#pragma unroll
                for (int u = 0; u < kForkWUnroll; ++u) {
                    const int i = base + u * kForkWBlock + tid;
                    const unsigned q = (unsigned)(i < nvec ? i : 0) / vpp;      // page and side
                    const int vec = (i < nvec ? i : 0) - (int)(q * vpp);
                    g[u] = (int)(q >> 1);
                    in_page[u] = (q & 1) ? ~(vec << 4) : vec << 4;
                    const bool vside = in_page[u] < 0;
                    if (i < nvec && s_dst[g[u]] >= 0) v[u] = *(const fwv4 *)((vside ? p.v_pool : p.k_pool) + s_src[g[u]] + (vside ? ~in_page[u] : in_page[u]));
                }
#pragma unroll
                for (int u = 0; u < kForkWUnroll; ++u) {
                    const int i = base + u * kForkWBlock + tid;
                    const bool vside = in_page[u] < 0;
                    if (i < nvec && s_dst[g[u]] >= 0) *(fwv4 *)((vside ? p.v_pool : p.k_pool) + s_dst[g[u]] + (vside ? ~in_page[u] : in_page[u])) = v[u];
                }
            }
        } else if (sub < p.n_ptasks + p.n_wtasks) {
            // ---- kForkWWinBytes of each window, byte for byte: ring positions are kept
            const int c0 = (sub - p.n_ptasks) * kForkWWinBytes;
            const int left = p.win_bytes - c0;
            const int nv1 = (left < kForkWWinBytes ? left : kForkWWinBytes) >> 4;      // vectors per side
            const long long so = l * p.win_ls_bytes + ((long long)p.src * p.nh_k + h) * p.win_bytes + c0;
            const long long dof = l * p.win_ls_bytes + ((long long)dst * p.nh_k + h) * p.win_bytes + c0;
#pragma unroll 1
            for (int base = 0; base < 2 * nv1; base += kForkWBlock * kForkWUnroll) {
                fwv4 v[kForkWUnroll];
#pragma unroll
                for (int u = 0; u < kForkWUnroll; ++u) {
                    const int i = base + u * kForkWBlock + tid;
                    const bool vside = i >= nv1;
                    const long long o = (long long)(vside ? i - nv1 : i) << 4;
                    if (i < 2 * nv1) v[u] = *(const fwv4 *)((vside ? p.v_win : p.k_win) + so + o);
                }
#pragma unroll
                for (int u = 0; u < kForkWUnroll; ++u) {
                    const int i = base + u * kForkWBlock + tid;
                    const bool vside = i >= nv1;
                    const long long o = (long long)(vside ? i - nv1 : i) << 4;
                    if (i < 2 * nv1) *(fwv4 *)((vside ? p.v_win : p.k_win) + dof + o) = v[u];
                }
            }
        } else {
            // ---- meta: the table row (SHARE), the lengths row (once per (layer, destination))
            if (p.share) {
                const int tail = p.tail_ids[((long long)jd * p.n_layers + l) * p.nh_k + h];
                for (int j = tid; j < n_live; j += kForkWBlock) dst_ids[j] = j < full ? src_ids[j] : tail;
            }
            if (h == 0 && tid == 0) {
                int *row_d = p.dev_lengths + l * p.len_ls + 4ll * dst;
                row_d[0] = T; row_d[1] = r; row_d[2] = st; row_d[3] = 0;
            }
        }
    }
}

}  // namespace million

using namespace million;

extern "C" int million_cache_fork_wide(const million_fork_desc *desc, int32_t *page_ids, void *k_pool, void *v_pool,
                                       void *k_resid, void *v_resid, int32_t *dev_lengths, const int32_t *dst_slots,
                                       const int32_t *tail_ids, int C, int packed, million_stream_t stream) {
    if (!desc || desc->struct_size != sizeof(million_fork_desc)) { set_error("cache_fork_wide: bad desc / struct_size"); return MILLION_ERR_ARG; }
    const million_fork_desc &d = *desc;
    int ps_shift;
    if (!page_shift("cache_fork_wide", d.page_size, ps_shift)) return MILLION_ERR_SHAPE;
    if (d.M != 16 && d.M != 32 && d.M != 64) { set_error("cache_fork_wide: M=%d (16, 32 or 64)", d.M); return MILLION_ERR_SHAPE; }
    if (C != 512 && C != 1024 && C != 2048 && C != 4096) { set_error("cache_fork_wide: C=%d (512, 1024, 2048 or 4096; C <= 256: million_cache_fork)", C); return MILLION_ERR_SHAPE; }
    if (d.n_layers <= 0 || d.bs <= 0 || d.nh_k <= 0 || d.d <= 0 || (d.d & 7) || d.n_pages_cap <= 0 || d.n_pool <= 0 || d.resid_cap < 0) {
        set_error("cache_fork_wide: n_layers=%d bs=%d nh_k=%d d=%d (a multiple of 8) n_pages_cap=%d n_pool=%d resid_cap=%d", d.n_layers, d.bs,
                  d.nh_k, d.d, d.n_pages_cap, d.n_pool, d.resid_cap);
        return MILLION_ERR_SHAPE;
    }
    if ((long long)d.n_pages_cap * d.page_size > 0x7fffffffLL || (long long)d.bs * d.nh_k * d.n_pages_cap > 0x7fffffffLL ||
        (long long)d.resid_cap * d.d * 2 > 0x7fffffffLL || (long long)d.n_layers * d.bs * d.nh_k > 0x7fffffffLL) {
        set_error("cache_fork_wide: n_pages_cap=%d resid_cap=%d bs=%d nh_k=%d n_layers=%d: a row does not fit 31 bits", d.n_pages_cap, d.resid_cap,
                  d.bs, d.nh_k, d.n_layers);
        return MILLION_ERR_SHAPE;
    }
    if (d.mode != MILLION_FORK_SHARE && d.mode != MILLION_FORK_COPY) { set_error("cache_fork_wide: mode=%d (SHARE 0, COPY 1)", d.mode); return MILLION_ERR_ARG; }
    if (d.src < 0 || d.src >= d.bs) { set_error("cache_fork_wide: src=%d outside [0, %d)", d.src, d.bs); return MILLION_ERR_ARG; }
    if (d.n_dst < 0 || d.n_pages_bound < 0 || d.n_pages_bound > d.n_pages_cap || d.prefix_tokens < -1) {
        set_error("cache_fork_wide: n_dst=%d n_pages_bound=%d (0 .. n_pages_cap=%d) prefix_tokens=%d (>= -1)", d.n_dst, d.n_pages_bound,
                  d.n_pages_cap, d.prefix_tokens);
        return MILLION_ERR_ARG;
    }
    if (d.n_dst == 0) return MILLION_OK;      // no destination: nothing to do, whatever the pointers
    const bool window = d.prefix_tokens < 0 && d.resid_cap > 0;
    if (!page_ids || !k_pool || !v_pool || !dev_lengths || !dst_slots) { set_error("cache_fork_wide: null page_ids / pools / dev_lengths / dst_slots"); return MILLION_ERR_ARG; }
    if (window && (!k_resid || !v_resid)) { set_error("cache_fork_wide: null window with resid_cap=%d and no prefix", d.resid_cap); return MILLION_ERR_ARG; }
    if (d.mode == MILLION_FORK_SHARE && !tail_ids) { set_error("cache_fork_wide: null tail_ids in SHARE mode (the private id of each partial tail page)"); return MILLION_ERR_ARG; }
    if (((uintptr_t)k_pool | (uintptr_t)v_pool | (window ? (uintptr_t)k_resid | (uintptr_t)v_resid : 0)) & 15) {
        set_error("cache_fork_wide: pools and windows must be 16-byte aligned");
        return MILLION_ERR_ALIGN;
    }
    if (((uintptr_t)page_ids | (uintptr_t)dev_lengths | (uintptr_t)dst_slots | (uintptr_t)tail_ids) & 3) { set_error("cache_fork_wide: page_ids / dev_lengths / dst_slots / tail_ids must be 4-byte aligned"); return MILLION_ERR_ALIGN; }
    if (window && (d.rows_layer_stride & 7)) { set_error("cache_fork_wide: the windows' layer stride must be a multiple of 8 elements (16 bytes)"); return MILLION_ERR_ALIGN; }

    ForkWideParams p;
    memset(&p, 0, sizeof(p));
    p.page_ids = page_ids; p.k_pool = (uint8_t *)k_pool; p.v_pool = (uint8_t *)v_pool;
    p.k_win = (uint8_t *)k_resid; p.v_win = (uint8_t *)v_resid;
    p.dev_lengths = dev_lengths; p.dst_slots = dst_slots; p.tail_ids = tail_ids;
    p.ids_ls = d.ids_layer_stride; p.win_ls_bytes = d.rows_layer_stride * 2; p.len_ls = d.lengths_layer_stride;
    p.n_layers = d.n_layers; p.bs = d.bs; p.nh_k = d.nh_k; p.n_pages_cap = d.n_pages_cap; p.n_pool = d.n_pool;
    p.page_size = d.page_size; p.ps_shift = ps_shift;
    p.page_bytes = packed ? d.page_size * d.M * (8 + (C <= 1024 ? 2 : 4)) / 8 : d.page_size * d.M * 2;      // a multiple of 16
    p.vpp = p.page_bytes >> 4;
    p.rcap = d.resid_cap; p.win_bytes = d.resid_cap * d.d * 2;
    p.src = d.src; p.n_dst = d.n_dst; p.share = d.mode == MILLION_FORK_SHARE;
    p.n_pages_bound = d.n_pages_bound; p.cap_tok = d.n_pages_bound * d.page_size; p.prefix = d.prefix_tokens;
    p.G = kForkWGroupBytes / p.page_bytes;
    p.G = p.G < 1 ? 1 : (p.G > kForkWMaxG ? kForkWMaxG : p.G);
    p.n_ptasks = p.share ? 1 : (d.n_pages_bound + p.G - 1) / p.G;
    p.n_wtasks = window ? (p.win_bytes + kForkWWinBytes - 1) / kForkWWinBytes : 0;
    p.n_tasks = (long long)d.n_layers * d.n_dst * d.nh_k * (p.n_ptasks + p.n_wtasks + 1);
    if ((long long)d.n_layers * d.n_dst * d.nh_k > 0x7fffffffLL) { set_error("cache_fork_wide: n_layers * n_dst * nh_k does not fit 31 bits"); return MILLION_ERR_SHAPE; }
    const int grid = (int)(p.n_tasks < kForkWMaxGrid ? p.n_tasks : kForkWMaxGrid);
    hipLaunchKernelGGL(cache_fork_wide_kernel, dim3(grid), dim3(kForkWBlock), 0, (hipStream_t)stream, p);
    hipError_t e = hipGetLastError();
    if (e != hipSuccess) { set_error("cache_fork_wide launch: %s", hipGetErrorString(e)); return MILLION_ERR_LAUNCH; }
    return MILLION_OK;
}
