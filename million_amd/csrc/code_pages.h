// code_pages.h — the token store of wide code pages (codes of 9 .. 12 bits): one token's 4 codes of the subspaces m0 .. m0 + 3
// (m0 and M multiples of 4) go into a uint16 page or into a packed page (million_hip.h, "Packed code pages").  gfx950.
//
// The one place that knows where a code's bits lie inside a page, for every writer: pq_encode_kernel<.., PACKED> and the pack
// half of repack_pages_kernel (encode.hip), pq_flush_wide_kernel (flush_wide.hip) and paged_store_kernel<DM, StoreRaggedWideParams>
// (paged_store.h).  The readers are the attention and gather kernels.  `off` is the token's place inside its page, `vside` selects
// the transposed V page (M, page_size) against the K page (page_size, M).  Every byte written belongs to that token alone and
// all stores are plain vector stores, so any lane = token mapping may call these without ordering between lanes.
#pragma once
#include "common.h"

namespace million {

// uint16 pages: one aligned 64-bit store on a K page, four lane-contiguous 16-bit rows on a transposed V page
__device__ __forceinline__ void store_codes4_u16(uint8_t *pool, long long pid, int off, int m0, const unsigned (&c4)[4], bool vside,
                                                 int page_size, int M) {
    uint16_t *dst = (uint16_t *)pool;
    if (!vside) {
        const unsigned long long codes = (unsigned long long)c4[0] | (unsigned long long)c4[1] << 16 | (unsigned long long)c4[2] << 32 |
                                         (unsigned long long)c4[3] << 48;
        *(unsigned long long *)(dst + (pid * page_size + off) * M + m0) = codes;
    } else {
#pragma unroll
        for (int s = 0; s < 4; ++s) dst[(pid * M + m0 + s) * page_size + off] = (uint16_t)c4[s];
    }
}

// packed pages (`page`: the page's first byte; hb = packed_hi_bits(C)): 4 low bytes - one 32-bit store on a K page, byte rows on
// a V page - and, in the high plane behind them, one whole byte (hb 2: 2 high bits per code) or two (hb 4: one 16-bit store on
// a K page, two byte rows on a V page)
__device__ __forceinline__ void store_codes4_packed(uint8_t *page, int off, int m0, const unsigned (&c4)[4], bool vside, int page_size,
                                                    int M, int hb) {
    uint8_t *hi_plane = page + page_size * M;
    unsigned lo = 0, hi = 0;
#pragma unroll
    for (int s = 0; s < 4; ++s) {
        lo |= (c4[s] & 0xffu) << (8 * s);
        hi |= ((c4[s] >> 8) & ((1u << hb) - 1u)) << (hb * s);
    }
    if (!vside) {
        *(unsigned *)(page + off * M + m0) = lo;
        if (hb == 2) hi_plane[off * (M / 4) + m0 / 4] = (uint8_t)hi;
        else *(unsigned short *)(hi_plane + off * (M / 2) + m0 / 2) = (unsigned short)hi;
    } else {
#pragma unroll
        for (int s = 0; s < 4; ++s) page[(m0 + s) * page_size + off] = (uint8_t)c4[s];
        if (hb == 2) hi_plane[(m0 / 4) * page_size + off] = (uint8_t)hi;
        else {
            hi_plane[(m0 / 2) * page_size + off] = (uint8_t)hi;
            hi_plane[(m0 / 2 + 1) * page_size + off] = (uint8_t)(hi >> 8);
        }
    }
}

// page `pid` of a pool of either format
__device__ __forceinline__ void store_codes4_wide(uint8_t *pool, long long pid, int off, int m0, const unsigned (&c4)[4], bool vside,
                                                  int page_size, int M, int C, bool packed) {
    if (!packed) store_codes4_u16(pool, pid, off, m0, c4, vside, page_size, M);
    else store_codes4_packed(pool + pid * packed_page_bytes(page_size, M, C), off, m0, c4, vside, page_size, M, packed_hi_bits(C));
}

}  // namespace million
