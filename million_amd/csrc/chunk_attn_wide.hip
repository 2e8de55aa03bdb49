// chunk_attn_wide.hip — chunk attention over 16-bit PQ codes (512 .. 4096 centroids per subspace), gfx950.
//
// million_pq_chunk_attn's job, word for word, and its code: chunk_attn_body (chunk_attn.h) with WIDE = true.  The tile step,
// the mask, the per-request cut of the visible tiles into S ranges, the epilogue and chunk_merge_kernel are the uint8 kernel's;
// the descriptor is validated, the split count chosen and the merge launched by chunk_attn.hip.
//
// What is this kernel's own is the code producer.  A table is C * d * 2 bytes = 64 KiB .. 1 MiB, so no codebook is in LDS:
// both are the plain (M, C, d_m) fp16 tensors in global memory (L2 / Infinity Cache resident: every workgroup gathers from the
// same two), as in attn_wide.hip.  A thread owns one (D = 64) or two (D = 128) 16-byte chunks of the [64 keys][D] tile per
// side: 8 / d_m subspaces of one token, whose entries - one global load of 4 (d_m = 2) or 8 (d_m = 4) bytes each - ARE that
// chunk of the dequantised row, so a code tile reaches LDS exactly as a window or chunk tile does: registers, one 16-byte store.
// A tile is dequantised once per workgroup and serves all 8 waves.
//
// Pipeline: while tile t's products run, the gathered entries of tile t + 1 (requested after tile t was stored) and the code
// words of tile t + 2 (requested behind those gathers) are in flight.  At d = 128, d_m = 2: 16 entry dwords and 8 code dwords
// per thread.  LDS is the K + V tile: 32 KiB at d = 128, 16 KiB at d = 64; single-buffered, two barriers per tile.
//
// EVERY gathered index is code & (C - 1).  Code words past T, in page tails, in pages no live entry names and in poisoned
// memory may hold any 16 bits: they are either never loaded (rows past a tile's valid count are written as zeros and masked)
// or, loaded, index inside the table.  Page ids are trusted, as in every other kernel.
//
// Packed pages (million_hip.h, "Packed code pages"): chunk_attn_packed_kernel is this kernel with a third code producer,
// ca_load_codes_packed (chunk_attn.h), which assembles the SAME word of 8 / d_m sixteen-bit fields from a token's low bytes and
// its own high-plane byte(s).  Tile order, split cut, gathers, merge: unchanged, so out and lse are the uint16 launch's bits.
#include "chunk_attn.h"

namespace million {

namespace {

template <int D, int DM, bool RAGGED, bool LSE>
__global__ __launch_bounds__(kThreads, 1) void chunk_attn_wide_kernel(ChunkParams p) {
    chunk_attn_body<D, DM, RAGGED, LSE, true>(p);
}

// Packed pages (million_pq_chunk_attn_packed): the same body with ca_load_codes_packed as the code producer.  The high bits
// per code, h = p.hb, are a wave-uniform field read when the kernel runs, not a template parameter: 16 more instances of this
// body, not 32, for two variable shifts per code word.
template <int D, int DM, bool RAGGED, bool LSE>
__global__ __launch_bounds__(kThreads, 1) void chunk_attn_packed_kernel(ChunkParams p) {
    chunk_attn_body<D, DM, RAGGED, LSE, true, true>(p);
}

template <int D, int DM>
void launch_wide_t(const ChunkParams &p, long long blocks, int lds, hipStream_t s) {
    const bool ragged = p.dev_lengths || p.dev_n_q;
    if (p.hb) {
        if (p.lse) {
            if (ragged) launch_chunk_kernel(chunk_attn_packed_kernel<D, DM, true, true>, p, blocks, lds, s);
            else launch_chunk_kernel(chunk_attn_packed_kernel<D, DM, false, true>, p, blocks, lds, s);
        } else if (ragged) launch_chunk_kernel(chunk_attn_packed_kernel<D, DM, true, false>, p, blocks, lds, s);
        else launch_chunk_kernel(chunk_attn_packed_kernel<D, DM, false, false>, p, blocks, lds, s);
    } else if (p.lse) {
        if (ragged) launch_chunk_kernel(chunk_attn_wide_kernel<D, DM, true, true>, p, blocks, lds, s);
        else launch_chunk_kernel(chunk_attn_wide_kernel<D, DM, false, true>, p, blocks, lds, s);
    } else if (ragged) launch_chunk_kernel(chunk_attn_wide_kernel<D, DM, true, false>, p, blocks, lds, s);
    else launch_chunk_kernel(chunk_attn_wide_kernel<D, DM, false, false>, p, blocks, lds, s);
}

}  // namespace

// d in {128, 64} and d / M in {2, 4}: the caller has checked (chunk_wide_geometry).  lds = the two tiles, below the 64 KiB that
// need no attribute.
void launch_chunk_wide(const ChunkParams &p, int d, long long blocks, int lds, hipStream_t s) {
    const int dm = d / p.M;
    if (d == 128) {
        if (dm == 2) launch_wide_t<128, 2>(p, blocks, lds, s);
        else launch_wide_t<128, 4>(p, blocks, lds, s);
    } else {
        if (dm == 2) launch_wide_t<64, 2>(p, blocks, lds, s);
        else launch_wide_t<64, 4>(p, blocks, lds, s);
    }
}

}  // namespace million
