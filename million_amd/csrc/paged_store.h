// paged_store.h — the ragged page writer: rows of a request's residual window and of its new rows become PQ-coded tokens of the
// request's K pages and transposed V pages, every per-request value read on the device.  gfx950, wave64.
//
// One kernel, paged_store_kernel<DM, P>, instantiated by its three users, each with its own parameter block P (P::kCommit, P::kWide):
//   StoreRaggedParams      million_pq_store_ragged (store_ragged.hip): the r + n source rows of a request become tokens [T, T + r + n);
//   StoreRaggedWideParams  million_pq_store_ragged_wide (store_ragged.hip): the same store with codes of 9 .. 12 bits, into uint16
//                          pages or packed pages (P::kWide);
//   WindowCommitParams     the first launch of million_window_commit (window_commit.hip), every layer: the f rows (0 or page_size) a
//                          commit flushes from the front of the same source sequence become tokens [T, T + f).
// (One merged block for store and commit was built: it regroups the commit's kernel-argument loads, profiles/len_row_refactor.txt A.3.)
// Per request the source sequence is [the r window rows in ring order; the new rows]: row j < r is window row
// (start + j) % resid_cap, row j >= r is new row j - r, and source row j becomes token T + j.  {T, r, start} are the request's
// lengths row, read by load_len_row (common.h), the row count is clamp_count of dev_n[b].
//
// Arithmetic: the contract and the centroid scan of every encoder kernel, pq_scan_sgpr (pq_scan.h).  pq_encode_kernel's mapping
// (encode.hip) too: lane = token, a wave owns 4 consecutive subspaces, the centroid rows are wave-uniform and come through the
// scalar cache from the fp32 image of the prepared codebook (kWide: from the plain fp16 codebook, wide formats have no prepared
// image).  The grid is a function of the bounds alone (token blocks of 64 x
// subspace groups [x layers] x (bs * nh_k) x 2 sides), so a captured launch follows the lengths: a block at or past the request's
// rows leaves before its first vector load, a straddling block clamps its dead lanes to the last live row and does not store
// them.  No load sits in a lane-conditional: the source address is selected (window or new rows).  No LDS.
// Store and commit differ in four things, each under `if constexpr (P::kCommit)` or in P::side(): how many source rows
// become tokens, the layer offsets, what keeps a store from a bad page (the store clamps the page index into the table, the
// commit - whose tokens lie inside the table - tests the page id against the pool), and the row strides (per side / one set,
// dense windows).  P::kWide switches two: the type of the centroid rows the scan reads (P::side() gives const f16 *cents, not
// const float *) and the token store (store_codes4_wide of code_pages.h, not the 4 code bytes below).
// A fourth parameter block, CommitRowsParams (window_commit.hip, million_window_commit_rows), is the commit's with P::kRows: new
// row i of a request is staged row dev_rows[b][i], clamped into [0, n_bound) (ps_new_row below).  kRows is false in WindowCommitParams and
// is not asked of the store's blocks; the instances of the 8-bit store and of both commits are compiled as before.
// WindowCommitWideParams / CommitRowsWideParams (window_commit.hip, million_window_commit_wide / _rows_wide) are the two commit
// blocks with P::kWide: kCommit and kWide are independent switches, so the commit over uint16 / packed pages is these blocks and
// no further line of the kernel.
// A parameter block P has: kCommit (the commit's also kRows), kWide; side(vside); page_ids, dev_lengths, dev_n; bs, nh_k, d, M, C, n_bound, rcap,
// page_size, ps_shift, n_pages_cap, cap_tok (cap_tok = n_pages_cap * page_size); the stores wsb, wsh (window strides, row stride d), the
// wide one packed; the commit nsl, ids_ls, win_ls, len_ls (layer strides), n_pool and groups_y (grid.y per layer).
#pragma once
#include <string.h>

#include "code_pages.h"
#include "pq_scan.h"

namespace million {

constexpr int kPsBlock = 256;
constexpr int kPsSub = 4;      // subspaces per wave (M is a multiple of 4 on every supported shape)

// One side (K or V) of a call as the kernel uses it: P::side(vside) selects it field by field (a reference selected between two
// kernel-argument structs is read back with vector loads)
template <typename CentT>
struct PagedStoreSideT {
    const f16 *new_rows;        // new rows ([layers,] bs, nh_k, n_bound, d)
    const f16 *win;             // window ([layers,] bs, nh_k, resid_cap, d); null when resid_cap = 0
    const CentT *cents;         // float: fp32 row image [m][c][dm] of the prepared codebook; f16 (kWide): the plain (M, C, d_m) codebook
    uint8_t *pool;              // K pool (n_pool, page_size, M) / V pool (n_pool, M, page_size); kWide: uint16 pages as bytes, or packed pages
    long long nsb, nsh, nsn;    // the new rows' strides, fp16 elements
};
typedef PagedStoreSideT<float> PagedStoreSide;

// The request's lengths row and its row count, as every kernel of the store and the commit reads them: T into [0, cap_tok],
// r into [0, resid_cap], n into [0, n_bound]
template <typename IntP, class P>
__device__ __forceinline__ void ps_load_row(IntP row, IntP dev_n, int b, const P &p, int &T, int &r, int &st, int &n) {
    load_len_row(row, p.cap_tok, p.rcap, p.rcap, T, r, st);
    n = clamp_count(dev_n[b], p.n_bound);
}
// The flush a commit of `a` rows implies: f rows (0 or page_size: n_bound <= page_size <= resid_cap) leave the window's front.
// ok = false: T + f would pass the page table, the request is left untouched.
template <class P>
__device__ __forceinline__ void ps_commit_flush(const P &p, int T, int r, int a, int &f, bool &ok) {
    f = r + a > p.rcap ? p.page_size : 0;
    ok = (long long)T + f <= p.cap_tok;
}

// P::kRows: the staged row that new row i of request b is.  i is clamped into [0, n_bound) before the load and the entry after
// it, so no lane reads outside dev_rows (bs, n_bound) or outside the request's n_bound staged rows, whatever either holds.
template <class P>
__device__ __forceinline__ int ps_new_row(const P &p, int b, int i) {
    if constexpr (P::kRows) {
        const int ic = i < 0 ? 0 : (i < p.n_bound ? i : p.n_bound - 1);
        const int x = p.dev_rows[(long long)b * p.n_bound + ic];
        return x < 0 ? 0 : (x < p.n_bound ? x : p.n_bound - 1);
    } else {
        return i;
    }
}

template <int DM, class P>
__global__ __launch_bounds__(kPsBlock) void paged_store_kernel(P p) {
    constexpr bool COMMIT = P::kCommit;
    const int lane = threadIdx.x & 63;
    int l = 0, gy = blockIdx.y;      // layer, subspace-group block
    if constexpr (COMMIT) { l = blockIdx.y / p.groups_y; gy = blockIdx.y % p.groups_y; }
    const int mg = __builtin_amdgcn_readfirstlane((int)(gy * (kPsBlock / 64) + (threadIdx.x >> 6)));
    const int m0 = mg * kPsSub;
    const bool vside = blockIdx.z & 1;    // workgroup-uniform
    const auto sd = p.side(vside);
    const int bh = blockIdx.z >> 1;
    const int b = bh / p.nh_k, hk = bh % p.nh_k;
    if (m0 >= p.M) return;
    int T, r, st, n;
    {
        // through the constant address space: neither array is written while this kernel runs (the advance is the next launch),
        // and only so does hipcc read them with scalar loads (a plain global pointer might alias the pools: vector loads and
        // v_readfirstlane instead)
        typedef const __attribute__((address_space(4))) int *const_p;
        if constexpr (COMMIT) ps_load_row((const_p)(p.dev_lengths + l * p.len_ls + 4ll * b), (const_p)p.dev_n, b, p, T, r, st, n);
        else ps_load_row((const_p)(p.dev_lengths + 4 * b), (const_p)p.dev_n, b, p, T, r, st, n);
    }
    // rows: the source rows that become tokens.  Workgroup-uniform exits before the first vector load.
    int rows;
    const int j0 = blockIdx.x * 64;
    if constexpr (COMMIT) {
        bool ok;
        ps_commit_flush(p, T, r, n, rows, ok);
        if (rows == 0 || !ok || j0 >= rows) return;
    } else {
        if (n == 0) return;               // the request takes no part: nothing of it is read beyond those words
        rows = r + n;
        // a block past the request's rows, a block whose first token lies past the page table (every token of it would drop
        // its store)
        if (j0 >= rows || ((T + j0) >> p.ps_shift) >= p.n_pages_cap) return;
    }
    const int j = j0 + lane;
    const bool valid = j < rows;
    const int jc = valid ? j : rows - 1;
    // source row: the address is selected, the load is one.  (The commit: jc - r < n, as r + n > rcap >= page_size = rows.)
    long long off_w, off_n;
    if constexpr (COMMIT) {
        off_w = l * p.win_ls + (((long long)b * p.nh_k + hk) * p.rcap + (st + jc) % p.rcap) * p.d;
        off_n = l * p.nsl + b * sd.nsb + hk * sd.nsh + (long long)ps_new_row(p, b, jc - r) * sd.nsn;
    } else {
        const int rmod = p.rcap > 0 ? p.rcap : 1;
        off_w = b * p.wsb + hk * p.wsh + (long long)((st + jc) % rmod) * p.d;
        off_n = b * sd.nsb + hk * sd.nsh + (long long)(jc - r) * sd.nsn;
    }
    const f16 *xp = (jc < r ? sd.win + off_w : sd.new_rows + off_n) + m0 * DM;
    float x[kPsSub][DM];
#pragma unroll
    for (int s = 0; s < kPsSub; ++s)
#pragma unroll
        for (int k = 0; k < DM; ++k) x[s][k] = (float)xp[s * DM + k];
    // destination: token T + jc
    const int tok = T + jc;
    const int page = tok >> p.ps_shift;
    long long pid;
    bool keep;
    if constexpr (COMMIT) {
        // inside the page table (T + f <= cap_tok); an id outside the pool drops the store
        const int id = p.page_ids[l * p.ids_ls + (long long)bh * p.n_pages_cap + page];
        keep = valid && (unsigned)id < (unsigned)p.n_pool;
        pid = id;
    } else {
        // the page index of a dead or dropped lane is clamped to a page that receives a token of this block (the block's first
        // token lies inside the table, so page n_pages_cap - 1 does whenever a later lane lies past it)
        keep = valid && page < p.n_pages_cap;
        pid = p.page_ids[(long long)bh * p.n_pages_cap + (page < p.n_pages_cap ? page : p.n_pages_cap - 1)];
    }

    unsigned codes = 0, c4[kPsSub];      // the 4 code bytes of the token; kWide: its 4 codes
    const auto *__restrict__ tab = sd.cents;
#pragma unroll
    for (int s = 0; s < kPsSub; ++s) {
        float best = INFINITY;
        int best_c = 0;
        pq_scan_sgpr<DM>(x[s], tab + (long long)(m0 + s) * p.C * DM, p.C, best, best_c);   // wave-uniform rows
        if constexpr (P::kWide) c4[s] = (unsigned)best_c;
        else codes |= (unsigned)best_c << (8 * s);
    }
    if (!keep) return;
    const int off = tok & (p.page_size - 1);
    if constexpr (P::kWide) {
        store_codes4_wide(sd.pool, pid, off, m0, c4, vside, p.page_size, p.M, p.C, p.packed);
        return;
    }
    if (!vside) {
        // K page (page_size, M): the token's 4 code bytes are one aligned 32-bit store (M and m0 are multiples of 4)
        *(unsigned *)(sd.pool + (pid * p.page_size + off) * p.M + m0) = codes;
    } else {
        // transposed V page (M, page_size): four lane-contiguous byte rows
        uint8_t *dst = sd.pool + (pid * p.M + m0) * p.page_size + off;
#pragma unroll
        for (int s = 0; s < kPsSub; ++s) dst[s * p.page_size] = (uint8_t)(codes >> (8 * s));
    }
}

// Host: the pointer-alignment checks of the entry points and the part of the parameter fill they share.  `who` is the entry
// point's name in the messages; MILLION_OK or the error code with the error text set.  The caller has checked its shape (ps_shift:
// page_shift of common.h) and the null pointers before, and fills in the sides, strides and what else is its own afterwards.
template <class P>
inline int paged_store_fill(const char *who, P &p, int bs, int nh_k, int d, int M, int C, int n_bound, int resid_cap, int page_size,
                            int ps_shift, int n_pages_cap, uintptr_t rows_windows_cents_pools, const int32_t *page_ids,
                            int32_t *dev_lengths, const int32_t *dev_n) {
    if (rows_windows_cents_pools & 15) { set_error("%s: rows, windows, %s and pools must be 16-byte aligned", who, P::kWide ? "codebooks" : "prepared codebooks"); return MILLION_ERR_ALIGN; }
    if (((uintptr_t)page_ids | (uintptr_t)dev_lengths | (uintptr_t)dev_n) & 3) { set_error("%s: page_ids / dev_lengths / dev_n must be 4-byte aligned", who); return MILLION_ERR_ALIGN; }
    memset(&p, 0, sizeof(p));
    p.page_ids = page_ids; p.dev_lengths = dev_lengths; p.dev_n = dev_n;
    p.bs = bs; p.nh_k = nh_k; p.d = d; p.M = M; p.C = C;
    p.n_bound = n_bound; p.rcap = resid_cap;
    p.page_size = page_size; p.ps_shift = ps_shift;
    p.n_pages_cap = n_pages_cap; p.cap_tok = n_pages_cap * page_size;
    return MILLION_OK;
}

}  // namespace million
