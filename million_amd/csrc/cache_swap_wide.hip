// cache_swap_wide.hip — million_cache_swap over uint16 or packed code pages, blob format 2 (million_cache_swap_wide), gfx950.
//
// cache_swap.hip's call and task list - per (layer of the call, entry, kv head) page tasks of G pages, window tasks, one lengths
// task; one workgroup per task, a grid-stride loop past kSwapWMaxGrid; no LDS, no barrier, no atomics; the window and lengths
// tasks are its own, byte for byte - with blob format 2: a page of the blob is a PACKED page (low plane, then high plane,
// include/million_hip.h "Packed code pages") whatever the pool holds, and canonical: bytes of tokens >= T are zero and every field
// is code & (C - 1).  Four instances, direction x pool format:
//   PACK, packed pool    a blob vector is the pool's vector at the same place of the page; what lies past T is cut by a BYTE mask:
//                        a vector of the K high plane spans 16 / (M h / 8) tokens (4 at M 16, h 2), a vector of either V plane 16
//                        columns.  In every plane the live bytes of a vector are its first n, n from T.  At C = 512 / 2048 the top
//                        bit of every field is masked.
//   PACK, uint16 pool    the work is organised by blob vector too: a low-plane vector is the low bytes of 16 consecutive uint16 of
//                        the page (32 contiguous bytes, both sides); a K high-plane vector the fields of 16 * 8/h consecutive codes
//                        (128 or 64 contiguous bytes); a V high-plane vector 16 columns of 8/h rows.  All loads of a vector are
//                        issued before it is stored.
//   UNPACK, packed pool  the blob's bytes, whole pages.
//   UNPACK, uint16 pool  organised by low-plane vector: 16 low bytes and their 16 fields (4 or 8 bytes of the K high plane, a
//                        vector of the V high plane shifted by the subspace's place in its byte) become 16 uint16, two stores;
//                        codes of tokens >= T are written as 0.
#include <string.h>

#include "common.h"

namespace million {

constexpr int kSwapWBlock = 256;
constexpr int kSwapWMaxGrid = 1 << 20;
constexpr int kSwapWGroupBytes = 4096;    // packed bytes per side and page task (G = 1 above that)
constexpr int kSwapWWinBytes = 16384;     // per side and window task
constexpr int kSwapWUnroll = 2;           // window vectors in flight per thread

typedef unsigned swv4 __attribute__((ext_vector_type(4)));

struct SwapWideParams {
    const int *page_ids;        // (layers, bs, nh_k, n_pages_cap)
    uint8_t *k_pool, *v_pool;
    uint8_t *k_win, *v_win;     // (layers, bs, nh_k, resid_cap, d) fp16, as bytes
    int *dev_lengths;           // (layers, bs, 4)
    const int *table;           // (n_slots, 4) {slot, T, r, start}
    const long long *offsets;   // (n_slots,)
    uint8_t *blob;
    long long ids_ls, win_ls_bytes, len_ls, blob_bytes;
    int bs, nh_k, n_pages_cap, n_pool;
    int ps_shift, m_shift, page_size;
    int h;                      // high bits of a packed code: 2 or 4
    int lo_bytes;               // low plane of a page: page_size * M
    int pbp;                    // packed page: lo_bytes * (8 + h) / 8
    int hrow;                   // bytes of a token's row of the K high plane: M * h / 8
    unsigned fmask;             // (C - 1) >> 8: the live bits of a field
    int row_b;                  // bytes of a window row: 2 * d
    int rcap, win_bytes;
    int layer0, n_layers_call, n_slots, cap_tok;
    int G, n_ptasks, n_wtasks;
    long long n_tasks;
};

__device__ __forceinline__ bool swapw_entry(const SwapWideParams &p, int js, int &slot, int &T, int &r, int &st, int &n_live,
                                            long long &row_bytes, long long &off) {
    typedef const __attribute__((address_space(4))) int *const_p;
    typedef const __attribute__((address_space(4))) long long *const_pl;
    const_p tab = (const_p)p.table;
    slot = tab[4 * js]; T = tab[4 * js + 1]; r = tab[4 * js + 2]; st = tab[4 * js + 3];
    off = ((const_pl)p.offsets)[js];
    if ((unsigned)slot >= (unsigned)p.bs) return false;
    clamp_len_row(p.cap_tok, p.rcap, p.rcap, T, r, st);
    n_live = (int)(((long long)T + p.page_size - 1) >> p.ps_shift);      // <= n_pages_bound <= n_pages_cap
    row_bytes = 2ll * n_live * p.pbp + 2ll * r * p.row_b;
    const long long rows = (long long)p.n_layers_call * p.nh_k;      // rows * row_bytes fits 62 bits: validated on the host
    return off >= 0 && !(off & 15) && off <= p.blob_bytes && rows * row_bytes <= p.blob_bytes - off;
}

// The first n bytes (n <= 0: none, n >= 16: all) of a vector, the others zero.
__device__ __forceinline__ swv4 swapw_keep_bytes(swv4 v, int n) {
#pragma unroll
    for (int w = 0; w < 4; ++w) {
        const int nb = n - 4 * w;
        const unsigned mask = nb >= 4 ? 0xffffffffu : (nb <= 0 ? 0u : (1u << (8 * nb)) - 1u);
        v[w] &= mask;
    }
    return v;
}

// Live bytes of the blob vector at byte o of a packed page (Tp live tokens, 0 .. page_size): the planes are token-major on the K
// side (a row of M, or hrow, bytes per token) and 16 columns of one row on the V side.
__device__ __forceinline__ int swapw_live(const SwapWideParams &p, bool vside, int o, int Tp) {
    const bool hi = o >= p.lo_bytes;
    const int oo = hi ? o - p.lo_bytes : o;
    return vside ? Tp - (oo & (p.page_size - 1)) : Tp * (hi ? p.hrow : 1 << p.m_shift) - oo;
}

// 16 consecutive uint16 (two vectors, codes 2q and 2q + 1 in word q) -> their low bytes / their fields (code >> 8) & fm, one byte each
__device__ __forceinline__ swv4 swapw_lo16(swv4 a, swv4 b) {
    swv4 o;
#pragma unroll
    for (int q = 0; q < 4; ++q) {
        const unsigned d0 = q < 2 ? a[2 * q] : b[2 * q - 4], d1 = q < 2 ? a[2 * q + 1] : b[2 * q - 3];
        o[q] = (d0 & 0xffu) | ((d0 >> 8) & 0xff00u) | ((d1 & 0xffu) << 16) | ((d1 << 8) & 0xff000000u);
    }
    return o;
}
__device__ __forceinline__ swv4 swapw_hi16(swv4 a, swv4 b, unsigned fm) {
    swv4 o;
#pragma unroll
    for (int q = 0; q < 4; ++q) {
        const unsigned d0 = q < 2 ? a[2 * q] : b[2 * q - 4], d1 = q < 2 ? a[2 * q + 1] : b[2 * q - 3];
        o[q] = (((d0 >> 8) & 0xffu) | ((d0 >> 16) & 0xff00u) | ((d1 << 8) & 0xff0000u) | (d1 & 0xff000000u)) & (fm * 0x01010101u);
    }
    return o;
}
// 16 low bytes and their 16 fields -> 16 uint16, two vectors
__device__ __forceinline__ void swapw_join16(swv4 lo, swv4 f, swv4 &a, swv4 &b) {
#pragma unroll
    for (int q = 0; q < 4; ++q) {
        const unsigned l = lo[q], g = f[q];
        const unsigned d0 = (l & 0xffu) | ((g & 0xffu) << 8) | ((l & 0xff00u) << 8) | ((g & 0xff00u) << 16);
        const unsigned d1 = ((l >> 16) & 0xffu) | ((g >> 8) & 0xff00u) | ((l >> 8) & 0xff0000u) | (g & 0xff000000u);
        if (q < 2) { a[2 * q] = d0; a[2 * q + 1] = d1; } else { b[2 * q - 4] = d0; b[2 * q - 3] = d1; }
    }
}
// Four fields of h bits in four bytes (each below 2^h) -> h = 2: one byte; h = 4: two bytes.  The first field lowest.
__device__ __forceinline__ unsigned swapw_fold2(unsigned w) { return (w | (w >> 6) | (w >> 12) | (w >> 18)) & 0xffu; }
__device__ __forceinline__ unsigned swapw_fold4(unsigned w) { const unsigned t = w | (w >> 4); return (t & 0xffu) | ((t >> 8) & 0xff00u); }
// ... and back: one byte of four 2-bit fields, two bytes of four 4-bit fields -> four bytes
__device__ __forceinline__ unsigned swapw_spread2(unsigned b) { return (b & 3u) | ((b & 0xcu) << 6) | ((b & 0x30u) << 12) | ((b & 0xc0u) << 18); }
__device__ __forceinline__ unsigned swapw_spread4(unsigned x) { return (x & 0xfu) | ((x & 0xf0u) << 4) | ((x & 0xf00u) << 8) | ((x & 0xf000u) << 12); }

// PACK from a uint16 page (`page`: its first byte, or null: no such page -> zeros): blob vector at byte o of the packed page.
__device__ __forceinline__ swv4 swapw_pack16(const SwapWideParams &p, const uint8_t *page, bool vside, int o) {
    swv4 out = swv4{0u, 0u, 0u, 0u};
    if (!page) return out;
    const unsigned fm = p.fmask;
    if (o < p.lo_bytes) {                       // codes [o, o + 16) of the page, both sides
        const swv4 a = *(const swv4 *)(page + 2ll * o), b = *(const swv4 *)(page + 2ll * o + 16);
        return swapw_lo16(a, b);
    }
    const int oo = o - p.lo_bytes;
    if (!vside) {                               // K: byte b holds the codes [b * 8/h, (b + 1) * 8/h) of the page
        if (p.h == 2) {
            swv4 ld[8];
#pragma unroll
            for (int q = 0; q < 8; ++q) ld[q] = *(const swv4 *)(page + 8ll * oo + 16 * q);
#pragma unroll
            for (int q = 0; q < 4; ++q) {
                const swv4 f = swapw_hi16(ld[2 * q], ld[2 * q + 1], fm);
                out[q] = swapw_fold2(f[0]) | (swapw_fold2(f[1]) << 8) | (swapw_fold2(f[2]) << 16) | (swapw_fold2(f[3]) << 24);
            }
        } else {
            swv4 ld[4];
#pragma unroll
            for (int q = 0; q < 4; ++q) ld[q] = *(const swv4 *)(page + 4ll * oo + 16 * q);
#pragma unroll
            for (int q = 0; q < 2; ++q) {
                const swv4 f = swapw_hi16(ld[2 * q], ld[2 * q + 1], fm);
                out[2 * q] = swapw_fold4(f[0]) | (swapw_fold4(f[1]) << 16);
                out[2 * q + 1] = swapw_fold4(f[2]) | (swapw_fold4(f[3]) << 16);
            }
        }
        return out;
    }
    // V: byte (jb, t) holds token t's fields of the subspaces jb * 8/h + i; the vector is 16 columns of row jb
    const int jb = oo >> p.ps_shift, t0 = oo & (p.page_size - 1);
    if (p.h == 2) {
        swv4 ld[8];
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            const uint8_t *rowp = page + 2ll * (((4 * jb + i) << p.ps_shift) + t0);
            ld[2 * i] = *(const swv4 *)rowp; ld[2 * i + 1] = *(const swv4 *)(rowp + 16);
        }
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            const swv4 f = swapw_hi16(ld[2 * i], ld[2 * i + 1], fm);
#pragma unroll
            for (int q = 0; q < 4; ++q) out[q] |= f[q] << (2 * i);
        }
    } else {
        swv4 ld[4];
#pragma unroll
        for (int i = 0; i < 2; ++i) {
            const uint8_t *rowp = page + 2ll * (((2 * jb + i) << p.ps_shift) + t0);
            ld[2 * i] = *(const swv4 *)rowp; ld[2 * i + 1] = *(const swv4 *)(rowp + 16);
        }
#pragma unroll
        for (int i = 0; i < 2; ++i) {
            const swv4 f = swapw_hi16(ld[2 * i], ld[2 * i + 1], fm);
#pragma unroll
            for (int q = 0; q < 4; ++q) out[q] |= f[q] << (4 * i);
        }
    }
    return out;
}

// kPacked: the pools hold packed pages; else uint16 pages of 2 * lo_bytes bytes.
template <bool kUnpack, bool kPacked>
__global__ __launch_bounds__(kSwapWBlock) void cache_swap_wide_kernel(SwapWideParams p) {
    const int tid = threadIdx.x;
    const int per_row = p.n_ptasks + p.n_wtasks + 1;
    const long long pool_page = kPacked ? p.pbp : 2ll * p.lo_bytes;      // bytes of a page of the pool
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
        if (!swapw_entry(p, js, slot, T, r, st, n_live, row_bytes, off)) continue;
        uint8_t *brow = p.blob + off + ((long long)lc * p.nh_k + h) * row_bytes;      // K pages, V pages, K window, V window
        const long long v_pages = (long long)n_live * p.pbp;                           // the V pages behind the K pages

        if (sub < p.n_ptasks) {
            // ---- G pages, both sides.  A unit is a blob vector; unpacking into uint16 pages, a vector of the low plane
            const int j0 = sub * p.G;
            const int ng = n_live - j0 < p.G ? n_live - j0 : p.G;
            if (ng <= 0) continue;
            const int *ids = p.page_ids + l * p.ids_ls + ((long long)slot * p.nh_k + h) * p.n_pages_cap + j0;
            const unsigned upp = (unsigned)((kUnpack && !kPacked) ? p.lo_bytes : p.pbp) >> 4;      // units per page and side
            const int nunit = ng * 2 * (int)upp;
#pragma unroll 1
            for (int i = tid; i < nunit; i += kSwapWBlock) {
                const unsigned q = (unsigned)i / upp;      // page and side
                const int o = (i - (int)(q * upp)) << 4;   // byte of the (packed) page
                const int g = (int)(q >> 1);
                const bool vside = q & 1;
                const int id = ids[g];                      // page j0 + g < n_live <= n_pages_cap
                const bool page = (unsigned)id < (unsigned)p.n_pool;
                uint8_t *pp = (vside ? p.v_pool : p.k_pool) + (long long)(page ? id : 0) * pool_page;
                uint8_t *bp = brow + (vside ? v_pages : 0) + (long long)(j0 + g) * p.pbp;
                int Tp = T - ((j0 + g) << p.ps_shift);      // live tokens of the page
                Tp = Tp < 0 ? 0 : (Tp > p.page_size ? p.page_size : Tp);
                if (!kUnpack) {
                    swv4 v;
                    if (kPacked) {
                        v = swv4{0u, 0u, 0u, 0u};
                        if (page) v = *(const swv4 *)(pp + o);
                        if (o >= p.lo_bytes) {
                            const unsigned fm = p.fmask | (p.fmask << p.h);      // per byte: 8 / h fields
                            const unsigned bm = (p.h == 2 ? fm | (fm << 4) : fm) * 0x01010101u;
                            v[0] &= bm; v[1] &= bm; v[2] &= bm; v[3] &= bm;
                        }
                    } else {
                        v = swapw_pack16(p, page ? pp : nullptr, vside, o);
                    }
                    *(swv4 *)(bp + o) = swapw_keep_bytes(v, swapw_live(p, vside, o, Tp));
                } else if (kPacked) {
                    if (page) *(swv4 *)(pp + o) = *(const swv4 *)(bp + o);
                } else if (page) {
                    // 16 codes [o, o + 16) of the uint16 page: their low bytes and their fields
                    const swv4 lo = *(const swv4 *)(bp + o);
                    swv4 f;
                    if (!vside) {
                        if (p.h == 2) {
                            const unsigned w = *(const unsigned *)(bp + p.lo_bytes + (o >> 2));
                            f = swv4{swapw_spread2(w & 0xffu), swapw_spread2((w >> 8) & 0xffu), swapw_spread2((w >> 16) & 0xffu), swapw_spread2(w >> 24)};
                        } else {
                            const uint2 w = *(const uint2 *)(bp + p.lo_bytes + (o >> 1));
                            f = swv4{swapw_spread4(w.x & 0xffffu), swapw_spread4(w.x >> 16), swapw_spread4(w.y & 0xffffu), swapw_spread4(w.y >> 16)};
                        }
                    } else {
                        const int m = o >> p.ps_shift, t0 = o & (p.page_size - 1);
                        const int per = 8 / p.h;
                        f = *(const swv4 *)(bp + p.lo_bytes + (((m / per) << p.ps_shift) + t0));
                        const int sh = p.h * (m % per);
                        f[0] >>= sh; f[1] >>= sh; f[2] >>= sh; f[3] >>= sh;
                    }
                    const unsigned bm = p.fmask * 0x01010101u;
                    f[0] &= bm; f[1] &= bm; f[2] &= bm; f[3] &= bm;
                    const int live = swapw_live(p, vside, o, Tp);
                    swv4 a, b;
                    swapw_join16(swapw_keep_bytes(lo, live), swapw_keep_bytes(f, live), a, b);
                    *(swv4 *)(pp + 2ll * o) = a;
                    *(swv4 *)(pp + 2ll * o + 16) = b;
                }
            }
        } else if (sub < p.n_ptasks + p.n_wtasks) {
            // ---- kSwapWWinBytes of each window in blob order: blob row i is ring row (start + i) % resid_cap
            const int c0 = (sub - p.n_ptasks) * kSwapWWinBytes;
            const int left = r * p.row_b - c0;      // r * row_b <= win_bytes < 2^31
            if (left <= 0) continue;
            const int nv1 = (left < kSwapWWinBytes ? left : kSwapWWinBytes) >> 4;      // vectors per side
            const long long wo = l * p.win_ls_bytes + ((long long)slot * p.nh_k + h) * p.win_bytes;
            uint8_t *bwin = brow + 2 * v_pages + c0;
            const int v_win = r * p.row_b;                                            // the V window behind the K window
#pragma unroll 1
            for (int base = 0; base < 2 * nv1; base += kSwapWBlock * kSwapWUnroll) {
                swv4 v[kSwapWUnroll];
#pragma unroll
                for (int u = 0; u < kSwapWUnroll; ++u) {
                    const int i = base + u * kSwapWBlock + tid;
                    const bool vside = i >= nv1;
                    const int o = (vside ? i - nv1 : i) << 4;                         // byte in this task's part of the side
                    const int bi = (unsigned)(c0 + o) / (unsigned)p.row_b;            // blob row
                    const int ring = st + bi - (st + bi >= p.rcap ? p.rcap : 0);
                    const long long ro = wo + (long long)ring * p.row_b + (c0 + o - bi * p.row_b);
                    if (i < 2 * nv1) v[u] = kUnpack ? *(const swv4 *)(bwin + (vside ? v_win : 0) + o) : *(const swv4 *)((vside ? p.v_win : p.k_win) + ro);
                }
#pragma unroll
                for (int u = 0; u < kSwapWUnroll; ++u) {
                    const int i = base + u * kSwapWBlock + tid;
                    const bool vside = i >= nv1;
                    const int o = (vside ? i - nv1 : i) << 4;
                    const int bi = (unsigned)(c0 + o) / (unsigned)p.row_b;
                    const int ring = st + bi - (st + bi >= p.rcap ? p.rcap : 0);
                    const long long ro = wo + (long long)ring * p.row_b + (c0 + o - bi * p.row_b);
                    if (i < 2 * nv1) {
                        if (kUnpack) *(swv4 *)((vside ? p.v_win : p.k_win) + ro) = v[u];
                        else *(swv4 *)(bwin + (vside ? v_win : 0) + o) = v[u];
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

extern "C" int million_cache_swap_wide(const million_swap_desc *desc, const int32_t *page_ids, void *k_pool, void *v_pool, void *k_resid,
                                       void *v_resid, int32_t *dev_lengths, const int32_t *slot_table, const int64_t *blob_offsets,
                                       void *blob, int C, int packed, million_stream_t stream) {
    if (!desc || desc->struct_size != sizeof(million_swap_desc)) { set_error("cache_swap_wide: bad desc / struct_size"); return MILLION_ERR_ARG; }
    const million_swap_desc &d = *desc;
    int ps_shift;
    if (!page_shift("cache_swap_wide", d.page_size, ps_shift)) return MILLION_ERR_SHAPE;
    if (d.M != 16 && d.M != 32 && d.M != 64) { set_error("cache_swap_wide: M=%d (16, 32 or 64)", d.M); return MILLION_ERR_SHAPE; }
    if (C != 512 && C != 1024 && C != 2048 && C != 4096) { set_error("cache_swap_wide: C=%d (512, 1024, 2048 or 4096; C <= 256: million_cache_swap)", C); return MILLION_ERR_SHAPE; }
    if (d.n_layers <= 0 || d.bs <= 0 || d.nh_k <= 0 || d.d <= 0 || (d.d & 7) || d.n_pages_cap <= 0 || d.n_pool <= 0 || d.resid_cap < 0) {
        set_error("cache_swap_wide: n_layers=%d bs=%d nh_k=%d d=%d (a multiple of 8) n_pages_cap=%d n_pool=%d resid_cap=%d", d.n_layers, d.bs,
                  d.nh_k, d.d, d.n_pages_cap, d.n_pool, d.resid_cap);
        return MILLION_ERR_SHAPE;
    }
    if ((long long)d.n_pages_cap * d.page_size > 0x7fffffffLL || (long long)d.bs * d.nh_k * d.n_pages_cap > 0x7fffffffLL ||
        (long long)d.resid_cap * d.d * 2 > 0x7fffffffLL || (long long)d.n_layers * d.bs * d.nh_k > 0x7fffffffLL) {
        set_error("cache_swap_wide: n_pages_cap=%d resid_cap=%d bs=%d nh_k=%d n_layers=%d: a row does not fit 31 bits", d.n_pages_cap, d.resid_cap,
                  d.bs, d.nh_k, d.n_layers);
        return MILLION_ERR_SHAPE;
    }
    if (d.direction != MILLION_SWAP_PACK && d.direction != MILLION_SWAP_UNPACK) { set_error("cache_swap_wide: direction=%d (PACK 0, UNPACK 1)", d.direction); return MILLION_ERR_ARG; }
    if (d.layer0 < 0 || d.n_layers_call <= 0 || d.layer0 > d.n_layers - d.n_layers_call) {
        set_error("cache_swap_wide: layers [%d, %d + %d) not inside [0, %d)", d.layer0, d.layer0, d.n_layers_call, d.n_layers);
        return MILLION_ERR_ARG;
    }
    if (d.n_slots < 0 || d.n_pages_bound < 0 || d.n_pages_bound > d.n_pages_cap || d.blob_bytes < 0) {
        set_error("cache_swap_wide: n_slots=%d n_pages_bound=%d (0 .. n_pages_cap=%d) blob_bytes=%lld (>= 0)", d.n_slots, d.n_pages_bound,
                  d.n_pages_cap, (long long)d.blob_bytes);
        return MILLION_ERR_ARG;
    }
    if (d.n_slots == 0) return MILLION_OK;      // no entry: nothing to do, whatever the pointers
    const bool window = d.resid_cap > 0;
    if (!page_ids || !k_pool || !v_pool || !dev_lengths || !slot_table || !blob_offsets || !blob) {
        set_error("cache_swap_wide: null page_ids / pools / dev_lengths / slot_table / blob_offsets / blob");
        return MILLION_ERR_ARG;
    }
    if (window && (!k_resid || !v_resid)) { set_error("cache_swap_wide: null window with resid_cap=%d", d.resid_cap); return MILLION_ERR_ARG; }
    if (((uintptr_t)k_pool | (uintptr_t)v_pool | (uintptr_t)blob | (window ? (uintptr_t)k_resid | (uintptr_t)v_resid : 0)) & 15) {
        set_error("cache_swap_wide: pools, windows and blob must be 16-byte aligned");
        return MILLION_ERR_ALIGN;
    }
    if ((((uintptr_t)page_ids | (uintptr_t)dev_lengths | (uintptr_t)slot_table) & 3) || ((uintptr_t)blob_offsets & 7)) {
        set_error("cache_swap_wide: page_ids / dev_lengths / slot_table must be 4-byte aligned, blob_offsets 8-byte aligned");
        return MILLION_ERR_ALIGN;
    }
    if (window && (d.rows_layer_stride & 7)) { set_error("cache_swap_wide: the windows' layer stride must be a multiple of 8 elements (16 bytes)"); return MILLION_ERR_ALIGN; }
    if ((long long)d.n_layers_call * d.n_slots * d.nh_k > 0x7fffffffLL) { set_error("cache_swap_wide: n_layers_call * n_slots * nh_k does not fit 31 bits"); return MILLION_ERR_SHAPE; }

    SwapWideParams p;
    memset(&p, 0, sizeof(p));
    p.page_ids = page_ids; p.k_pool = (uint8_t *)k_pool; p.v_pool = (uint8_t *)v_pool;
    p.k_win = (uint8_t *)k_resid; p.v_win = (uint8_t *)v_resid;
    p.dev_lengths = dev_lengths; p.table = slot_table; p.offsets = (const long long *)blob_offsets; p.blob = (uint8_t *)blob;
    p.ids_ls = d.ids_layer_stride; p.win_ls_bytes = d.rows_layer_stride * 2; p.len_ls = d.lengths_layer_stride;
    p.blob_bytes = d.blob_bytes;
    p.bs = d.bs; p.nh_k = d.nh_k; p.n_pages_cap = d.n_pages_cap; p.n_pool = d.n_pool;
    p.page_size = d.page_size; p.ps_shift = ps_shift;
    p.m_shift = d.M == 16 ? 4 : d.M == 32 ? 5 : 6;
    p.h = C <= 1024 ? 2 : 4;
    p.lo_bytes = d.page_size * d.M;
    p.pbp = p.lo_bytes * (8 + p.h) / 8;      // a multiple of 16
    p.hrow = d.M * p.h / 8;
    p.fmask = (unsigned)(C - 1) >> 8;
    p.row_b = d.d * 2; p.rcap = d.resid_cap; p.win_bytes = d.resid_cap * d.d * 2;
    p.layer0 = d.layer0; p.n_layers_call = d.n_layers_call; p.n_slots = d.n_slots;
    p.cap_tok = d.n_pages_bound * d.page_size;
    p.G = kSwapWGroupBytes / p.pbp;
    p.G = p.G < 1 ? 1 : p.G;
    p.n_ptasks = (d.n_pages_bound + p.G - 1) / p.G;
    p.n_wtasks = window ? (p.win_bytes + kSwapWWinBytes - 1) / kSwapWWinBytes : 0;
    p.n_tasks = (long long)d.n_layers_call * d.n_slots * d.nh_k * (p.n_ptasks + p.n_wtasks + 1);
    const long long max_row_bytes = 2ll * d.n_pages_bound * p.pbp + 2ll * p.win_bytes;
    if (p.n_tasks > 0x7fffffffLL || max_row_bytes > (1ll << 62) / ((long long)d.n_layers_call * d.nh_k)) {
        set_error("cache_swap_wide: %lld tasks / %lld bytes per row: the call does not fit 31 / 62 bits", p.n_tasks, max_row_bytes);
        return MILLION_ERR_SHAPE;
    }
    const dim3 grid((unsigned)(p.n_tasks < kSwapWMaxGrid ? p.n_tasks : kSwapWMaxGrid)), block(kSwapWBlock);
    const bool unpack = d.direction == MILLION_SWAP_UNPACK;
    if (unpack && packed) hipLaunchKernelGGL((cache_swap_wide_kernel<true, true>), grid, block, 0, (hipStream_t)stream, p);
    else if (unpack) hipLaunchKernelGGL((cache_swap_wide_kernel<true, false>), grid, block, 0, (hipStream_t)stream, p);
    else if (packed) hipLaunchKernelGGL((cache_swap_wide_kernel<false, true>), grid, block, 0, (hipStream_t)stream, p);
    else hipLaunchKernelGGL((cache_swap_wide_kernel<false, false>), grid, block, 0, (hipStream_t)stream, p);
    hipError_t e = hipGetLastError();
    if (e != hipSuccess) { set_error("cache_swap_wide launch: %s", hipGetErrorString(e)); return MILLION_ERR_LAUNCH; }
    return MILLION_OK;
}
