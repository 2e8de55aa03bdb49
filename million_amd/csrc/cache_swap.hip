// cache_swap.hip — pack requests of a paged cache into contiguous blobs, or restore blobs into a slot's pages, in one launch
// (million_cache_swap), gfx950.
//
// A request that has to give up its batch slot keeps what it has: its code pages (scattered over the global pools behind the
// id table, V pages transposed, the tail page holding dead bytes past T), its residual window (a ring) and its lengths become
// one canonical byte string per (layer, kv head) - blob format 1, include/million_hip.h - that the host copies out, keeps,
// writes to a file, and hands back later to whatever pages the destination slot owns then.  PACK only reads the cache; UNPACK
// writes the pages the slot's table row names, the live ring rows and the lengths row, and nothing else.
//
// The work is cache_fork.hip's: a list of 16-byte-vector copies cut into TASKS, one workgroup per task (a grid-stride loop past
// kSwapMaxGrid tasks).  Per (layer of the call, entry of the slot table, kv head) - a "row":
//   page tasks    ceil(n_pages_bound / G) of them; a task owns G consecutive pages, both sides (8 KiB: G = 1 at 4 KiB pages),
//                 every thread reads the ids of its own vectors and issues its loads before its first store.  PACK zeroes what lies past T on the way:
//                 whole vectors on the K side (a token is M >= 16 bytes), a byte mask inside the vector on the transposed V side;
//   window tasks  kSwapWinBytes of the K window and of the V window in blob (ring) order; the ring row is computed per vector;
//   one meta task UNPACK, kv head 0: the slot's lengths row.
// The task count is a function of the bounds alone; a task past the entry's live pages or rows reads the table and leaves.  No
// task reads what another writes, so there are no atomics, flags or ordering between workgroups, no LDS and no barrier.  Stores are plain 16-byte vector stores.
#include <string.h>

#include "common.h"

namespace million {

constexpr int kSwapBlock = 256;
constexpr int kSwapMaxGrid = 1 << 20;     // workgroups of a launch (2^28 threads); a longer task list is strode over
constexpr int kSwapUnroll = 2;            // 16-byte loads in flight per thread: at 4 KiB pages a page task is one page, K and V side
constexpr int kSwapGroupBytes = kSwapUnroll * kSwapBlock * 16 / 2;      // per side and page task: one pass of the workgroup
constexpr int kSwapWinBytes = 16384;      // per side and window task

typedef unsigned sv4 __attribute__((ext_vector_type(4)));

struct SwapParams {
    const int *page_ids;        // (layers, bs, nh_k, n_pages_cap)
    uint8_t *k_pool, *v_pool;
    uint8_t *k_win, *v_win;     // (layers, bs, nh_k, resid_cap, d) fp16, as bytes
    int *dev_lengths;           // (layers, bs, 4)
    const int *table;           // (n_slots, 4) {slot, T, r, start}
    const long long *offsets;   // (n_slots,)
    uint8_t *blob;
    long long ids_ls, win_ls_bytes, len_ls, blob_bytes;
    int bs, nh_k, n_pages_cap, n_pool;
    int pb_shift, ps_shift, m_shift, page_size;
    int row_b;                  // bytes of a window row: 2 * d
    int rcap, win_bytes;        // rows and bytes of one (layer, slot, kv head) window
    int layer0, n_layers_call, n_slots, cap_tok;
    int G, n_ptasks, n_wtasks;  // per row: page tasks of G pages, window tasks
    long long n_tasks;
};

// Entry js of the slot table as every task reads it, or false when it takes no part.  Its {T, r, start} are a lengths row behind
// the slot word: load_len_row (common.h) with T into [0, cap_tok] (cap_tok = n_pages_bound * page_size) and r into [0, resid_cap];
// the slot must lie in [0, bs) and the entry's rows inside the blob, 16-byte aligned.
__device__ __forceinline__ bool swap_entry(const SwapParams &p, int js, int &slot, int &T, int &r, int &st, int &n_live,
                                           long long &row_bytes, long long &off) {
    // through the constant address space: the table and the offsets are never written while this kernel runs
    typedef const __attribute__((address_space(4))) int *const_p;
    typedef const __attribute__((address_space(4))) long long *const_pl;
    const_p tab = (const_p)p.table;
    slot = tab[4 * js]; T = tab[4 * js + 1]; r = tab[4 * js + 2]; st = tab[4 * js + 3];
    off = ((const_pl)p.offsets)[js];
    if ((unsigned)slot >= (unsigned)p.bs) return false;
    clamp_len_row(p.cap_tok, p.rcap, p.rcap, T, r, st);
    n_live = (int)(((long long)T + p.page_size - 1) >> p.ps_shift);      // <= n_pages_bound <= n_pages_cap
    row_bytes = ((long long)n_live << (p.pb_shift + 1)) + 2ll * r * p.row_b;
    const long long rows = (long long)p.n_layers_call * p.nh_k;      // rows * row_bytes fits 62 bits: validated on the host
    return off >= 0 && !(off & 15) && off <= p.blob_bytes && rows * row_bytes <= p.blob_bytes - off;
}

// The first n bytes (0 <= n <= 16) of a vector, the others zero.
__device__ __forceinline__ sv4 swap_keep_bytes(sv4 v, int n) {
#pragma unroll
    for (int w = 0; w < 4; ++w) {
        const int nb = n - 4 * w;
        const unsigned mask = nb >= 4 ? 0xffffffffu : (nb <= 0 ? 0u : (1u << (8 * nb)) - 1u);
        v[w] &= mask;
    }
    return v;
}

// Small tasks at full occupancy - 8 waves per SIMD (<= 64 registers), one workgroup per task - rather than cache_fork.hip's 32 KiB
// tasks under a grid of 2048: a task's steps depend on each other (table entry, id, data), and what hides that chain is the
// number of tasks in flight.  Measured: DESIGN 4.10, profiles/cache_swap.txt.
template <bool kUnpack>
__global__ __launch_bounds__(kSwapBlock) __attribute__((amdgpu_waves_per_eu(8))) void cache_swap_kernel(SwapParams p) {
    const int tid = threadIdx.x;
    const int per_row = p.n_ptasks + p.n_wtasks + 1;
#pragma unroll 1
    for (unsigned t = blockIdx.x; t < p.n_tasks; t += gridDim.x) {      // workgroup-uniform; n_tasks and the grid fit 31 bits
        const int sub = (int)(t % (unsigned)per_row);
        const int row = (int)(t / (unsigned)per_row);
        const int h = row % p.nh_k;
        const int js = (row / p.nh_k) % p.n_slots;
        const int lc = row / (p.nh_k * p.n_slots);      // layer of the call
        const int l = p.layer0 + lc;
        int slot, T, r, st, n_live;
        long long row_bytes, off;
        if (!swap_entry(p, js, slot, T, r, st, n_live, row_bytes, off)) continue;
        uint8_t *brow = p.blob + off + ((long long)lc * p.nh_k + h) * row_bytes;      // K pages, V pages, K window, V window
        const long long v_pages = (long long)n_live << p.pb_shift;                     // the V pages behind the K pages

        if (sub < p.n_ptasks) {
            // ---- G pages, both sides
            const int j0 = sub * p.G;
            const int ng = n_live - j0 < p.G ? n_live - j0 : p.G;
            if (ng <= 0) continue;
            // every thread reads the ids of its own vectors (the same few words for the whole wave, from the cache): the chain
            // is table entry -> id -> data, with no LDS and no barrier between a task's steps
            const int *ids = p.page_ids + l * p.ids_ls + ((long long)slot * p.nh_k + h) * p.n_pages_cap + j0;
            // vector i of the task: page g = i / (2 * vpp), side (i / vpp) & 1, vector i % vpp of that page
            const int vshift = p.pb_shift - 4;
            const int nvec = ng << (vshift + 1);
#pragma unroll 1
            for (int base = 0; base < nvec; base += kSwapBlock * kSwapUnroll) {
                sv4 v[kSwapUnroll];
                int id[kSwapUnroll];      // outside [0, n_pool): no such page
#pragma unroll
                for (int u = 0; u < kSwapUnroll; ++u) {
                    const int i = base + u * kSwapBlock + tid;
                    id[u] = i < nvec ? ids[i >> (vshift + 1)] : -1;      // page j0 + g < n_live <= n_pages_cap
                }
#pragma unroll
                for (int u = 0; u < kSwapUnroll; ++u) {
                    const int i = base + u * kSwapBlock + tid;
                    const int g = (i < nvec ? i : 0) >> (vshift + 1);
                    const int in_page = (i & ((1 << vshift) - 1)) << 4;
                    const bool vside = (i >> vshift) & 1;
                    const bool page = (unsigned)id[u] < (unsigned)p.n_pool;
                    if (kUnpack) {
                        if (page)
                            v[u] = *(const sv4 *)(brow + (vside ? v_pages : 0) + ((long long)(j0 + g) << p.pb_shift) + in_page);
                    } else {
                        v[u] = sv4{0u, 0u, 0u, 0u};
                        if (page) v[u] = *(const sv4 *)((vside ? p.v_pool : p.k_pool) + ((long long)id[u] << p.pb_shift) + in_page);
                    }
                }
#pragma unroll
                for (int u = 0; u < kSwapUnroll; ++u) {
                    const int i = base + u * kSwapBlock + tid;
                    const int g = (i < nvec ? i : 0) >> (vshift + 1);
                    const int in_page = (i & ((1 << vshift) - 1)) << 4;
                    const bool vside = (i >> vshift) & 1;
                    if (kUnpack) {
                        if ((unsigned)id[u] < (unsigned)p.n_pool) *(sv4 *)((vside ? p.v_pool : p.k_pool) + ((long long)id[u] << p.pb_shift) + in_page) = v[u];
                    } else if (i < nvec) {
                        // live bytes of the vector: K (page_size, M): the vector lies in one token's row; V (M, page_size): 16 columns
                        const int tok0 = ((j0 + g) << p.ps_shift) + (vside ? in_page & (p.page_size - 1) : in_page >> p.m_shift);
                        const int live = vside ? T - tok0 : (tok0 < T ? 16 : 0);
                        *(sv4 *)(brow + (vside ? v_pages : 0) + ((long long)(j0 + g) << p.pb_shift) + in_page) =
                            live >= 16 ? v[u] : swap_keep_bytes(v[u], live);
                    }
                }
            }
        } else if (sub < p.n_ptasks + p.n_wtasks) {
            // ---- kSwapWinBytes of each window in blob order: blob row i is ring row (start + i) % resid_cap
            const int c0 = (sub - p.n_ptasks) * kSwapWinBytes;
            const int left = r * p.row_b - c0;      // r * row_b <= win_bytes < 2^31
            if (left <= 0) continue;
            const int nv1 = (left < kSwapWinBytes ? left : kSwapWinBytes) >> 4;      // vectors per side
            const long long wo = l * p.win_ls_bytes + ((long long)slot * p.nh_k + h) * p.win_bytes;
            uint8_t *bwin = brow + 2 * v_pages + c0;
            const int v_win = r * p.row_b;                                            // the V window behind the K window
#pragma unroll 1
            for (int base = 0; base < 2 * nv1; base += kSwapBlock * kSwapUnroll) {
                sv4 v[kSwapUnroll];
#pragma unroll
                for (int u = 0; u < kSwapUnroll; ++u) {
                    const int i = base + u * kSwapBlock + tid;
                    const bool vside = i >= nv1;
                    const int o = (vside ? i - nv1 : i) << 4;                         // byte in this task's part of the side
                    const int bi = (unsigned)(c0 + o) / (unsigned)p.row_b;            // blob row
                    const int ring = st + bi - (st + bi >= p.rcap ? p.rcap : 0);
                    const long long ro = wo + (long long)ring * p.row_b + (c0 + o - bi * p.row_b);
                    if (i < 2 * nv1) v[u] = kUnpack ? *(const sv4 *)(bwin + (vside ? v_win : 0) + o) : *(const sv4 *)((vside ? p.v_win : p.k_win) + ro);
                }
#pragma unroll
                for (int u = 0; u < kSwapUnroll; ++u) {
                    const int i = base + u * kSwapBlock + tid;
                    const bool vside = i >= nv1;
                    const int o = (vside ? i - nv1 : i) << 4;
                    const int bi = (unsigned)(c0 + o) / (unsigned)p.row_b;
                    const int ring = st + bi - (st + bi >= p.rcap ? p.rcap : 0);
                    const long long ro = wo + (long long)ring * p.row_b + (c0 + o - bi * p.row_b);
                    if (i < 2 * nv1) {
                        if (kUnpack) *(sv4 *)((vside ? p.v_win : p.k_win) + ro) = v[u];
                        else *(sv4 *)(bwin + (vside ? v_win : 0) + o) = v[u];
                    }
                }
            }
        } else if (kUnpack && h == 0 && tid == 0) {
            // ---- meta: the slot's lengths row, once per (layer, entry)
            int *row_d = p.dev_lengths + l * p.len_ls + 4ll * slot;
            row_d[0] = T; row_d[1] = r; row_d[2] = st; row_d[3] = 0;
        }
    }
}

}  // namespace million

using namespace million;

extern "C" int million_cache_swap(const million_swap_desc *desc, const int32_t *page_ids, void *k_pool, void *v_pool, void *k_resid,
                                  void *v_resid, int32_t *dev_lengths, const int32_t *slot_table, const int64_t *blob_offsets,
                                  void *blob, million_stream_t stream) {
    if (!desc || desc->struct_size != sizeof(million_swap_desc)) { set_error("cache_swap: bad desc / struct_size"); return MILLION_ERR_ARG; }
    const million_swap_desc &d = *desc;
    int ps_shift;
    if (!page_shift("cache_swap", d.page_size, ps_shift)) return MILLION_ERR_SHAPE;
    if (d.M != 16 && d.M != 32 && d.M != 64) { set_error("cache_swap: M=%d (16, 32 or 64)", d.M); return MILLION_ERR_SHAPE; }
    if (d.n_layers <= 0 || d.bs <= 0 || d.nh_k <= 0 || d.d <= 0 || (d.d & 7) || d.n_pages_cap <= 0 || d.n_pool <= 0 || d.resid_cap < 0) {
        set_error("cache_swap: n_layers=%d bs=%d nh_k=%d d=%d (a multiple of 8) n_pages_cap=%d n_pool=%d resid_cap=%d", d.n_layers, d.bs,
                  d.nh_k, d.d, d.n_pages_cap, d.n_pool, d.resid_cap);
        return MILLION_ERR_SHAPE;
    }
    if ((long long)d.n_pages_cap * d.page_size > 0x7fffffffLL || (long long)d.bs * d.nh_k * d.n_pages_cap > 0x7fffffffLL ||
        (long long)d.resid_cap * d.d * 2 > 0x7fffffffLL || (long long)d.n_layers * d.bs * d.nh_k > 0x7fffffffLL) {
        set_error("cache_swap: n_pages_cap=%d resid_cap=%d bs=%d nh_k=%d n_layers=%d: a row does not fit 31 bits", d.n_pages_cap, d.resid_cap,
                  d.bs, d.nh_k, d.n_layers);
        return MILLION_ERR_SHAPE;
    }
    if (d.direction != MILLION_SWAP_PACK && d.direction != MILLION_SWAP_UNPACK) { set_error("cache_swap: direction=%d (PACK 0, UNPACK 1)", d.direction); return MILLION_ERR_ARG; }
    if (d.layer0 < 0 || d.n_layers_call <= 0 || d.layer0 > d.n_layers - d.n_layers_call) {
        set_error("cache_swap: layers [%d, %d + %d) not inside [0, %d)", d.layer0, d.layer0, d.n_layers_call, d.n_layers);
        return MILLION_ERR_ARG;
    }
    if (d.n_slots < 0 || d.n_pages_bound < 0 || d.n_pages_bound > d.n_pages_cap || d.blob_bytes < 0) {
        set_error("cache_swap: n_slots=%d n_pages_bound=%d (0 .. n_pages_cap=%d) blob_bytes=%lld (>= 0)", d.n_slots, d.n_pages_bound,
                  d.n_pages_cap, (long long)d.blob_bytes);
        return MILLION_ERR_ARG;
    }
    if (d.n_slots == 0) return MILLION_OK;      // no entry: nothing to do, whatever the pointers
    const bool window = d.resid_cap > 0;
    if (!page_ids || !k_pool || !v_pool || !dev_lengths || !slot_table || !blob_offsets || !blob) {
        set_error("cache_swap: null page_ids / pools / dev_lengths / slot_table / blob_offsets / blob");
        return MILLION_ERR_ARG;
    }
    if (window && (!k_resid || !v_resid)) { set_error("cache_swap: null window with resid_cap=%d", d.resid_cap); return MILLION_ERR_ARG; }
    if (((uintptr_t)k_pool | (uintptr_t)v_pool | (uintptr_t)blob | (window ? (uintptr_t)k_resid | (uintptr_t)v_resid : 0)) & 15) {
        set_error("cache_swap: pools, windows and blob must be 16-byte aligned");
        return MILLION_ERR_ALIGN;
    }
    if ((((uintptr_t)page_ids | (uintptr_t)dev_lengths | (uintptr_t)slot_table) & 3) || ((uintptr_t)blob_offsets & 7)) {
        set_error("cache_swap: page_ids / dev_lengths / slot_table must be 4-byte aligned, blob_offsets 8-byte aligned");
        return MILLION_ERR_ALIGN;
    }
    if (window && (d.rows_layer_stride & 7)) { set_error("cache_swap: the windows' layer stride must be a multiple of 8 elements (16 bytes)"); return MILLION_ERR_ALIGN; }
    if ((long long)d.n_layers_call * d.n_slots * d.nh_k > 0x7fffffffLL) { set_error("cache_swap: n_layers_call * n_slots * nh_k does not fit 31 bits"); return MILLION_ERR_SHAPE; }

    SwapParams p;
    memset(&p, 0, sizeof(p));
    p.page_ids = page_ids; p.k_pool = (uint8_t *)k_pool; p.v_pool = (uint8_t *)v_pool;
    p.k_win = (uint8_t *)k_resid; p.v_win = (uint8_t *)v_resid;
    p.dev_lengths = dev_lengths; p.table = slot_table; p.offsets = (const long long *)blob_offsets; p.blob = (uint8_t *)blob;
    p.ids_ls = d.ids_layer_stride; p.win_ls_bytes = d.rows_layer_stride * 2; p.len_ls = d.lengths_layer_stride;
    p.blob_bytes = d.blob_bytes;
    p.bs = d.bs; p.nh_k = d.nh_k; p.n_pages_cap = d.n_pages_cap; p.n_pool = d.n_pool;
    p.page_size = d.page_size; p.ps_shift = ps_shift;
    p.m_shift = d.M == 16 ? 4 : d.M == 32 ? 5 : 6;
    p.pb_shift = p.ps_shift + p.m_shift;
    p.row_b = d.d * 2; p.rcap = d.resid_cap; p.win_bytes = d.resid_cap * d.d * 2;
    p.layer0 = d.layer0; p.n_layers_call = d.n_layers_call; p.n_slots = d.n_slots;
    p.cap_tok = d.n_pages_bound * d.page_size;
    p.G = kSwapGroupBytes >> p.pb_shift;
    p.G = p.G < 1 ? 1 : p.G;
    p.n_ptasks = (d.n_pages_bound + p.G - 1) / p.G;
    p.n_wtasks = window ? (p.win_bytes + kSwapWinBytes - 1) / kSwapWinBytes : 0;
    p.n_tasks = (long long)d.n_layers_call * d.n_slots * d.nh_k * (p.n_ptasks + p.n_wtasks + 1);
    const long long max_row_bytes = ((long long)d.n_pages_bound << (p.pb_shift + 1)) + 2ll * p.win_bytes;
    if (p.n_tasks > 0x7fffffffLL || max_row_bytes > (1ll << 62) / ((long long)d.n_layers_call * d.nh_k)) {
        set_error("cache_swap: %lld tasks / %lld bytes per row: the call does not fit 31 / 62 bits", p.n_tasks, max_row_bytes);
        return MILLION_ERR_SHAPE;
    }
    const int grid = (int)(p.n_tasks < kSwapMaxGrid ? p.n_tasks : kSwapMaxGrid);
    if (d.direction == MILLION_SWAP_UNPACK)
        hipLaunchKernelGGL(cache_swap_kernel<true>, dim3(grid), dim3(kSwapBlock), 0, (hipStream_t)stream, p);
    else
        hipLaunchKernelGGL(cache_swap_kernel<false>, dim3(grid), dim3(kSwapBlock), 0, (hipStream_t)stream, p);
    hipError_t e = hipGetLastError();
    if (e != hipSuccess) { set_error("cache_swap launch: %s", hipGetErrorString(e)); return MILLION_ERR_LAUNCH; }
    return MILLION_OK;
}
