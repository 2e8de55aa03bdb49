// chunk_attn.hip — a block of new query tokens attended to the PQ-coded cache (chunked prefill, multi-turn, draft
// verification), gfx950.
//
//   out[b,h,i,:] = softmax_j( q[b,h,i,:] . Kall[b,hk,j,:] / sqrt(d) ) Vall[b,hk,j,:],   hk = h / G
//   Kall = [ dequant(K codes, T tokens) ; window rows (r rows of the ring, from resid_start) ; chunk rows 0 .. n_c - 1 ]
//   every row sees the T + r past keys; chunk key j is visible to row i iff j <= i (n_c = n_q) - n_c = 0: past only.
//
// Design
//   * the flash-attention tile step of prefill_attn_kernel, shared through flash_tile.h: S^T = K Q^T with
//     v_mfma_f32_32x32x16_f16, a query row on a lane, in-lane online softmax in the exp2 domain, O^T += V^T P^T with V^T read by
//     ds_read_b64_tr_b16 from the same tile_off LDS image; only the mask is this kernel's own.  The G query heads of a kv head are flattened, rho = i G + g, so a
//     workgroup of 8 waves holds 256 consecutive rows of one (b, kv head) and a wave's 32 rows have a monotone causal limit.
//   * three producers fill ONE [64 keys][D] K and V tile image: (a) 64 tokens of codes, dequantised through both codebooks held
//     in LDS (the row image [m][c][d_m] of million_prepare_cents: the gather of pq_decode, bit for bit); (b) window rows read
//     through the ring; (c) chunk rows.  A tile holds one source; its rows past the source's end are written as zeros and
//     masked, and a code byte is clamped to C - 1 before it indexes the codebook: nothing outside the valid data reaches an
//     MFMA, whatever the pages hold past T (the kernel is total).  Dequantised once per workgroup, the tile serves all 8 waves.
//   * LDS: K + V tile (single-buffered, 2 x 64 x D x 2 B) + the two codebook images (2 x C x D x 2 B): 160 KiB at C = 256,
//     d = 128 - the whole gfx950 CU.  The next tile's code bytes / fp16 rows are loaded into registers while the current tile
//     is computed; two barriers per tile.
//   * the visible tiles of a query block ([codes | window | chunk up to the block's last row]) are cut into S contiguous
//     ranges, one per split (chunk_splits: host logic).  S = 1 writes fp16 out directly; otherwise each split writes
//     unnormalised fp32 O and (m, l) per row to the workspace and chunk_merge_kernel combines them: two plain launches, no
//     atomics, nothing in the workspace has to be initialised.
//   * ragged batches (desc->dev_lengths / dev_n_q): the RAGGED instances read T, r, resid_start and the valid query rows of
//     their request on the device and clamp them; grid, S and workspace are those of the bounds, every request's own tiles
//     are cut into the S ranges (empty ranges write m = -inf, l = 0), rows past a request's n_q are stored as zeros.  The
//     lockstep instances (RAGGED = false) are the kernel without any of it.
//   * linear block id: kv head fastest (a kv head's codes stay on one XCD's L2), then split, then query block, then batch.
//   * the kernel body is chunk_attn.h's chunk_attn_body, shared with chunk_attn_wide.hip (uint16 codes); this file holds the
//     uint8 instances and the host half of both: validation, the split rule, the workspace and the merge.
#include <math.h>
#include <string.h>

#include "chunk_attn.h"

namespace million {

namespace {

// The uint8 kernel: chunk_attn_body (chunk_attn.h) with the LDS codebook producer
template <int D, int DM, bool RAGGED, bool LSE>
__global__ __launch_bounds__(kThreads, 1) void chunk_attn_kernel(ChunkParams p) {
    chunk_attn_body<D, DM, RAGGED, LSE, false>(p);
}

// ---- merge of the splits: one thread per (row, 8 dims) ----
template <int D, bool RAGGED, bool LSE>
__global__ __launch_bounds__(256) void chunk_merge_kernel(ChunkParams p) {
    constexpr int TPR = D / 8;
    const long long gid = (long long)blockIdx.x * 256 + threadIdx.x;
    const long long row = gid / TPR;
    const int part = (int)(gid - row * TPR);
    if (row >= (long long)p.bs * p.nh_k * p.nrows) return;
    const int rho = (int)(row % p.nrows);
    const long long bh = row / p.nrows;
    const int hk = (int)(bh % p.nh_k), b = (int)(bh / p.nh_k);
    typedef f16 h8 __attribute__((ext_vector_type(8)));
    if (RAGGED && p.dev_n_q && rho >= ca_load_n_q(p, b) * p.G) {      // past the request's n_q: no split wrote this row
        const int qz = rho / p.G;
        const h8 z = {(f16)0.f, (f16)0.f, (f16)0.f, (f16)0.f, (f16)0.f, (f16)0.f, (f16)0.f, (f16)0.f};
        *(h8 *)(p.out + b * p.o_sb + (hk * p.G + (rho - qz * p.G)) * p.o_sh + (long long)qz * p.o_sn + 8 * part) = z;
        if constexpr (LSE) if (part == 0) *ca_lse_at(p, b, hk * p.G + (rho - qz * p.G), qz) = -INFINITY;
        return;
    }
    float mx = -INFINITY;
    for (int s = 0; s < p.S; ++s) mx = fmaxf(mx, p.ws_ml[2 * ((bh * p.S + s) * p.nrows + rho)]);
    float L = 0.f, acc[8];
#pragma unroll
    for (int e = 0; e < 8; ++e) acc[e] = 0.f;
    if (mx > -INFINITY) {
        for (int s = 0; s < p.S; ++s) {
            const long long wrow = (bh * p.S + s) * p.nrows + rho;
            const float m = p.ws_ml[2 * wrow], l = p.ws_ml[2 * wrow + 1];
            if (!(m > -INFINITY)) continue;      // a split without a visible key for this row
            const float w = exp2f(m - mx);
            L += w * l;
            const float *o = p.ws_o + wrow * D + 8 * part;
#pragma unroll
            for (int e = 0; e < 8; ++e) acc[e] += w * o[e];
        }
    }
    const float inv = L > 0.f ? 1.0f / L : 0.f;
    const int qi = rho / p.G, head = hk * p.G + (rho - qi * p.G);
    h8 v;
#pragma unroll
    for (int e = 0; e < 8; ++e) v[e] = (f16)(acc[e] * inv);
    *(h8 *)(p.out + b * p.o_sb + head * p.o_sh + (long long)qi * p.o_sn + 8 * part) = v;
    if constexpr (LSE) if (part == 0) *ca_lse_at(p, b, head, qi) = lse_of(mx > -INFINITY ? mx : 0.f, L);
}

constexpr int kChunkTargetWGs = 256;     // one workgroup per MI355X CU (the LDS budget at C = 256 admits one)
constexpr int kChunkMaxSplits = 64;

template <int D, int DM, bool RAGGED, bool LSE>
void launch_chunk_r(const ChunkParams &p, long long blocks, int lds, hipStream_t s) {
    launch_chunk_kernel(chunk_attn_kernel<D, DM, RAGGED, LSE>, p, blocks, lds, s);
}
template <int D, int DM>
void launch_chunk_t(const ChunkParams &p, long long blocks, int lds, hipStream_t s) {
    const bool ragged = p.dev_lengths || p.dev_n_q;
    if (p.lse) { if (ragged) launch_chunk_r<D, DM, true, true>(p, blocks, lds, s); else launch_chunk_r<D, DM, false, true>(p, blocks, lds, s); }
    else if (ragged) launch_chunk_r<D, DM, true, false>(p, blocks, lds, s);
    else launch_chunk_r<D, DM, false, false>(p, blocks, lds, s);
}
template <int D, bool RAGGED>
void launch_chunk_merge(const ChunkParams &p, long long mblocks, hipStream_t s) {
    if (p.lse) hipLaunchKernelGGL((chunk_merge_kernel<D, RAGGED, true>), dim3((unsigned)mblocks), dim3(256), 0, s, p);
    else hipLaunchKernelGGL((chunk_merge_kernel<D, RAGGED, false>), dim3((unsigned)mblocks), dim3(256), 0, s, p);
}

void chunk_attrs_once() {
    if (!device_once(4)) return;
    const int mx = 160 * 1024;
#define CA_ATTR(D, DM)                                                                                                          \
    (void)hipFuncSetAttribute((const void *)chunk_attn_kernel<D, DM, false, false>, hipFuncAttributeMaxDynamicSharedMemorySize, mx); \
    (void)hipFuncSetAttribute((const void *)chunk_attn_kernel<D, DM, true, false>, hipFuncAttributeMaxDynamicSharedMemorySize, mx);  \
    (void)hipFuncSetAttribute((const void *)chunk_attn_kernel<D, DM, false, true>, hipFuncAttributeMaxDynamicSharedMemorySize, mx);  \
    (void)hipFuncSetAttribute((const void *)chunk_attn_kernel<D, DM, true, true>, hipFuncAttributeMaxDynamicSharedMemorySize, mx)
    CA_ATTR(128, 2); CA_ATTR(128, 4); CA_ATTR(128, 8); CA_ATTR(64, 1); CA_ATTR(64, 2); CA_ATTR(64, 4);
#undef CA_ATTR
}

}  // namespace

// Splits of the past: enough workgroups for every CU where the context allows, never more splits than code tiles (every
// split owns >= 1 tile), at most 64.  A pure function of (bs, nh_k, query blocks, T).
int chunk_splits(int bs, int nh_k, int n_qb, int T) {
    const long long blocks = (long long)bs * nh_k * n_qb;
    const long long ntT = ((long long)T + kKeys - 1) / kKeys;
    if (blocks <= 0) return 1;
    long long S = (kChunkTargetWGs + blocks - 1) / blocks;
    if (S > ntT) S = ntT;
    if (S > kChunkMaxSplits) S = kChunkMaxSplits;
    return S < 1 ? 1 : (int)S;
}

static bool chunk_geometry(const million_chunk_attn_desc *d, int &n_qb, int &S, size_t &ws) {
    if (!d || d->struct_size != sizeof(million_chunk_attn_desc) || d->bs <= 0 || d->nh_k <= 0 || d->nh <= 0 || d->nh % d->nh_k ||
        d->n_q < 0 || d->n_tokens < 0 || (d->d != 64 && d->d != 128))
        return false;
    const long long rows = (long long)d->n_q * (d->nh / d->nh_k);
    if (rows > 0x7fffffffLL) return false;
    n_qb = (int)((rows + kRowsWG - 1) / kRowsWG);
    S = chunk_splits(d->bs, d->nh_k, n_qb, d->n_tokens);
    ws = S > 1 ? (size_t)d->bs * d->nh_k * S * rows * (d->d + 2) * sizeof(float) : 0;
    return true;
}

}  // namespace million

using namespace million;

extern "C" size_t million_chunk_attn_workspace_bytes(const million_chunk_attn_desc *desc) {
    int n_qb, S;
    size_t ws;
    return chunk_geometry(desc, n_qb, S, ws) ? ws : 0;
}

// the shapes chunk_attn_wide_kernel is built for: wide_geometry (attn_wide.hip) without a bound on nh / nh_k
static bool chunk_wide_geometry(const char *who, int d, int M, int C) {
    if (wide_geometry(d, M, C, 1)) return true;
    set_error("%s: d=%d M=%d C=%d (d 64 / 128, d / M 2 or 4, C 512 / 1024 / 2048 / 4096: uint16 codes)", who, d, M, C);
    return false;
}

extern "C" size_t million_chunk_attn_wide_workspace_bytes(const million_chunk_attn_desc *desc) {
    int n_qb, S;
    size_t ws;
    if (!chunk_geometry(desc, n_qb, S, ws)) { set_error("chunk_attn_wide: bad desc / struct_size / shape"); return 0; }
    return chunk_wide_geometry("chunk_attn_wide", desc->d, desc->M, desc->C) ? ws : 0;
}

// `wide`: million_pq_chunk_attn_wide - uint16 codes (row-major rows of 2 M bytes) and the plain codebooks; every other check,
// the geometry, the workspace and the merge are the same lines for both widths
// `packed` (with wide): million_pq_chunk_attn_packed - both sides are pools of packed pages (million_hip.h, "Packed code pages")
static int chunk_attn_impl(bool wide, bool packed, const million_chunk_attn_desc *desc, const void *q, const void *k_chunk, const void *v_chunk,
                           const void *k_codes, const void *v_codes, const void *k_page_ids, const void *v_page_ids,
                           const void *k_cents_prepared, const void *v_cents_prepared, const void *k_resid,
                           const void *v_resid, void *out, float *lse, void *workspace, size_t workspace_bytes,
                           million_stream_t stream) {
    if (!desc || desc->struct_size != sizeof(million_chunk_attn_desc)) { set_error("chunk_attn: bad desc / struct_size"); return MILLION_ERR_ARG; }
    const million_chunk_attn_desc &d = *desc;
    if (d.bs <= 0 || d.nh <= 0 || d.nh_k <= 0 || d.nh % d.nh_k) { set_error("chunk_attn: bs=%d nh=%d nh_k=%d", d.bs, d.nh, d.nh_k); return MILLION_ERR_SHAPE; }
    if (wide ? !chunk_wide_geometry(packed ? "chunk_attn_packed" : "chunk_attn_wide", d.d, d.M, d.C) : !u8_geometry("chunk_attn", d.d, d.M, d.C)) return MILLION_ERR_SHAPE;
    if (packed) {      // there is no packed row-major format, and a packed page exists for pages of 32 / 64 / 128 tokens only
        int ps_shift;
        if (d.k_layout != MILLION_KV_PAGED || d.v_layout != MILLION_KV_PAGED) {
            set_error("chunk_attn_packed: k_layout=%d v_layout=%d (both MILLION_KV_PAGED: packed codes live in pages only)", d.k_layout, d.v_layout);
            return MILLION_ERR_SHAPE;
        }
        if (!page_shift("chunk_attn_packed", d.page_size, ps_shift)) return MILLION_ERR_SHAPE;
    }
    if (d.n_q < 0 || (d.n_c != 0 && d.n_c != d.n_q)) { set_error("chunk_attn: n_q=%d n_c=%d (n_c must be 0 or n_q)", d.n_q, d.n_c); return MILLION_ERR_SHAPE; }
    const bool dev_len = d.dev_lengths != nullptr;      // n_tokens is then the bound; r and resid_start are not read
    if (d.n_tokens < 0 || d.resid_cap < 0 ||
        (!dev_len && (d.r < 0 || d.r > d.resid_cap || (d.r > 0 && (d.resid_start < 0 || d.resid_start >= d.resid_cap))))) {
        set_error("chunk_attn: n_tokens=%d r=%d resid_start=%d resid_cap=%d", d.n_tokens, d.r, d.resid_start, d.resid_cap);
        return MILLION_ERR_ARG;
    }
    if ((d.k_layout != MILLION_KV_ROWMAJOR && d.k_layout != MILLION_KV_PAGED) || (d.v_layout != MILLION_KV_ROWMAJOR && d.v_layout != MILLION_KV_PAGED)) {
        set_error("chunk_attn: k_layout=%d v_layout=%d", d.k_layout, d.v_layout);
        return MILLION_ERR_ARG;
    }
    const bool any_paged = d.k_layout == MILLION_KV_PAGED || d.v_layout == MILLION_KV_PAGED;
    if (any_paged && d.n_tokens > 0) {
        int ps_shift;      // the kernel divides by p.ps
        if (!page_shift("chunk_attn", d.page_size, ps_shift)) return MILLION_ERR_SHAPE;
        if ((long long)d.n_pages_cap * d.page_size < d.n_tokens) { set_error("chunk_attn: %d pages of %d tokens hold fewer than n_tokens=%d", d.n_pages_cap, d.page_size, d.n_tokens); return MILLION_ERR_SHAPE; }
    }
    if (d.n_q == 0) return MILLION_OK;
    if (!q || !out) { set_error("chunk_attn: null q / out"); return MILLION_ERR_ARG; }
    if (d.n_c > 0 && (!k_chunk || !v_chunk)) { set_error("chunk_attn: null chunk K / V with n_c=%d", d.n_c); return MILLION_ERR_ARG; }
    if ((dev_len ? d.resid_cap > 0 : d.r > 0) && (!k_resid || !v_resid)) {
        set_error("chunk_attn: null window with r=%d resid_cap=%d", dev_len ? -1 : d.r, d.resid_cap);
        return MILLION_ERR_ARG;
    }
    if (d.n_tokens > 0 && (!k_codes || !v_codes || !k_cents_prepared || !v_cents_prepared ||
                           (d.k_layout == MILLION_KV_PAGED && !k_page_ids) || (d.v_layout == MILLION_KV_PAGED && !v_page_ids))) {
        set_error("chunk_attn: null codes / prepared codebooks / page ids with n_tokens=%d", d.n_tokens);
        return MILLION_ERR_ARG;
    }
    int n_qb, S;
    size_t need;
    if (!chunk_geometry(desc, n_qb, S, need)) { set_error("chunk_attn: %d query rows per kv head", d.n_q); return MILLION_ERR_SHAPE; }
    if (need > 0 && (!workspace || workspace_bytes < need)) { set_error("chunk_attn: workspace %zu < %zu bytes", workspace_bytes, need); return MILLION_ERR_WORKSPACE; }
    if (((uintptr_t)q | (uintptr_t)k_chunk | (uintptr_t)v_chunk | (uintptr_t)k_codes | (uintptr_t)v_codes | (uintptr_t)k_resid |
         (uintptr_t)v_resid | (uintptr_t)out | (uintptr_t)workspace | (uintptr_t)k_cents_prepared | (uintptr_t)v_cents_prepared) & 15) {
        set_error("chunk_attn: every pointer must be 16-byte aligned");
        return MILLION_ERR_ALIGN;
    }
    if ((d.q_stride_b | d.q_stride_h | d.q_stride_n | d.kc_stride_b | d.kc_stride_h | d.kc_stride_n | d.vc_stride_b | d.vc_stride_h |
         d.vc_stride_n | d.o_stride_b | d.o_stride_h | d.o_stride_n | d.resid_stride_b | d.resid_stride_h) & 7) {
        set_error("chunk_attn: fp16 strides must be multiples of 8 elements (16-byte rows)");
        return MILLION_ERR_ALIGN;
    }
    if ((d.k_layout == MILLION_KV_ROWMAJOR && ((d.k_stride_b | d.k_stride_h) & 15)) ||
        (d.v_layout == MILLION_KV_ROWMAJOR && ((d.v_stride_b | d.v_stride_h) & 15))) {
        set_error("chunk_attn: code strides must be multiples of 16 bytes");
        return MILLION_ERR_ALIGN;
    }
    ChunkParams p;
    memset(&p, 0, sizeof(p));
    p.q = (const f16 *)q; p.kc = (const f16 *)k_chunk; p.vc = (const f16 *)v_chunk;
    p.kcodes = (const uint8_t *)k_codes; p.vcodes = (const uint8_t *)v_codes;
    p.kids = k_page_ids; p.vids = v_page_ids;
    p.ktab = (const f16 *)k_cents_prepared; p.vtab = (const f16 *)v_cents_prepared;
    p.kres = (const f16 *)k_resid; p.vres = (const f16 *)v_resid;
    p.out = (f16 *)out;
    p.lse = lse;
    p.bs = d.bs; p.nh = d.nh; p.nh_k = d.nh_k; p.G = d.nh / d.nh_k; p.M = d.M; p.C = d.C;
    p.n_q = d.n_q; p.n_c = d.n_c; p.T = d.n_tokens; p.rcap = d.resid_cap;
    p.r = dev_len ? 0 : d.r;
    p.rs = p.r > 0 ? d.resid_start : 0;
    p.dev_lengths = d.dev_lengths; p.dev_n_q = d.dev_n_q;
    p.res_sb = d.resid_stride_b; p.res_sh = d.resid_stride_h;
    p.k_paged = d.k_layout == MILLION_KV_PAGED; p.v_paged = d.v_layout == MILLION_KV_PAGED;
    p.ps = d.page_size > 0 ? d.page_size : 64; p.n_pages_cap = d.n_pages_cap; p.ids64 = d.page_ids_i64 != 0;
    p.k_sb = d.k_stride_b; p.k_sh = d.k_stride_h; p.v_sb = d.v_stride_b; p.v_sh = d.v_stride_h;
    p.q_sb = d.q_stride_b; p.q_sh = d.q_stride_h; p.q_sn = d.q_stride_n;
    p.kc_sb = d.kc_stride_b; p.kc_sh = d.kc_stride_h; p.kc_sn = d.kc_stride_n;
    p.vc_sb = d.vc_stride_b; p.vc_sh = d.vc_stride_h; p.vc_sn = d.vc_stride_n;
    p.o_sb = d.o_stride_b; p.o_sh = d.o_stride_h; p.o_sn = d.o_stride_n;
    p.nrows = d.n_q * p.G;
    p.n_qb = n_qb;
    p.S = S;
    p.ntT = (d.n_tokens + kKeys - 1) / kKeys;
    p.ntR = (p.r + kKeys - 1) / kKeys;
    p.cb_bytes = d.n_tokens > 0 && !wide ? d.C * d.d * 2 : 0;
    p.hb = packed ? packed_hi_bits(d.C) : 0;
    p.scale_log2e = 1.4426950408889634f / sqrtf((float)d.d);
    if (S > 1) {
        p.ws_o = (float *)workspace;
        p.ws_ml = p.ws_o + (size_t)d.bs * d.nh_k * S * p.nrows * d.d;
    }
    const long long blocks = (long long)d.bs * d.nh_k * n_qb * S;
    if (blocks > 0x7fffffffLL) { set_error("chunk_attn: %lld workgroups", blocks); return MILLION_ERR_SHAPE; }
    const int lds = 2 * kKeys * 2 * d.d + 2 * p.cb_bytes;
    chunk_attrs_once();
    const hipStream_t s = (hipStream_t)stream;
    const int dm = d.d / d.M;
    if (wide) {
        launch_chunk_wide(p, d.d, blocks, lds, s);
    } else if (d.d == 128) {
        if (dm == 2) launch_chunk_t<128, 2>(p, blocks, lds, s);
        else if (dm == 4) launch_chunk_t<128, 4>(p, blocks, lds, s);
        else launch_chunk_t<128, 8>(p, blocks, lds, s);
    } else {
        if (dm == 1) launch_chunk_t<64, 1>(p, blocks, lds, s);
        else if (dm == 2) launch_chunk_t<64, 2>(p, blocks, lds, s);
        else launch_chunk_t<64, 4>(p, blocks, lds, s);
    }
    if (S > 1) {
        const long long threads = (long long)d.bs * d.nh_k * p.nrows * (d.d / 8);
        const long long mblocks = (threads + 255) / 256;
        const bool ragged = p.dev_lengths || p.dev_n_q;
        if (d.d == 128 && ragged) launch_chunk_merge<128, true>(p, mblocks, s);
        else if (d.d == 128) launch_chunk_merge<128, false>(p, mblocks, s);
        else if (ragged) launch_chunk_merge<64, true>(p, mblocks, s);
        else launch_chunk_merge<64, false>(p, mblocks, s);
    }
    const hipError_t e = hipGetLastError();
    if (e != hipSuccess) { set_error("chunk_attn launch: %s", hipGetErrorString(e)); return MILLION_ERR_LAUNCH; }
    return MILLION_OK;
}

extern "C" int million_pq_chunk_attn(const million_chunk_attn_desc *desc, const void *q, const void *k_chunk, const void *v_chunk,
                                     const void *k_codes, const void *v_codes, const void *k_page_ids, const void *v_page_ids,
                                     const void *k_cents_prepared, const void *v_cents_prepared, const void *k_resid,
                                     const void *v_resid, void *out, void *workspace, size_t workspace_bytes,
                                     million_stream_t stream) {
    return chunk_attn_impl(false, false, desc, q, k_chunk, v_chunk, k_codes, v_codes, k_page_ids, v_page_ids, k_cents_prepared, v_cents_prepared,
                           k_resid, v_resid, out, nullptr, workspace, workspace_bytes, stream);
}

extern "C" int million_pq_chunk_attn_lse(const million_chunk_attn_desc *desc, const void *q, const void *k_chunk, const void *v_chunk,
                                         const void *k_codes, const void *v_codes, const void *k_page_ids, const void *v_page_ids,
                                         const void *k_cents_prepared, const void *v_cents_prepared, const void *k_resid,
                                         const void *v_resid, void *out, float *lse, void *workspace, size_t workspace_bytes,
                                         million_stream_t stream) {
    if (!lse) { set_error("chunk_attn_lse: lse null"); return MILLION_ERR_ARG; }
    if ((uintptr_t)lse & 3) { set_error("chunk_attn_lse: lse must be 4-byte aligned"); return MILLION_ERR_ALIGN; }
    return chunk_attn_impl(false, false, desc, q, k_chunk, v_chunk, k_codes, v_codes, k_page_ids, v_page_ids, k_cents_prepared, v_cents_prepared,
                           k_resid, v_resid, out, lse, workspace, workspace_bytes, stream);
}

extern "C" int million_pq_chunk_attn_wide(const million_chunk_attn_desc *desc, const void *q, const void *k_chunk, const void *v_chunk,
                                          const void *k_codes, const void *v_codes, const void *k_page_ids, const void *v_page_ids,
                                          const void *k_cents, const void *v_cents, const void *k_resid, const void *v_resid,
                                          void *out, float *lse, void *workspace, size_t workspace_bytes, million_stream_t stream) {
    if ((uintptr_t)lse & 3) { set_error("chunk_attn_wide: lse must be 4-byte aligned"); return MILLION_ERR_ALIGN; }
    return chunk_attn_impl(true, false, desc, q, k_chunk, v_chunk, k_codes, v_codes, k_page_ids, v_page_ids, k_cents, v_cents, k_resid,
                           v_resid, out, lse, workspace, workspace_bytes, stream);
}

extern "C" int million_pq_chunk_attn_packed(const million_chunk_attn_desc *desc, const void *q, const void *k_chunk, const void *v_chunk,
                                            const void *k_codes, const void *v_codes, const void *k_page_ids, const void *v_page_ids,
                                            const void *k_cents, const void *v_cents, const void *k_resid, const void *v_resid,
                                            void *out, float *lse, void *workspace, size_t workspace_bytes, million_stream_t stream) {
    if ((uintptr_t)lse & 3) { set_error("chunk_attn_packed: lse must be 4-byte aligned"); return MILLION_ERR_ALIGN; }
    return chunk_attn_impl(true, true, desc, q, k_chunk, v_chunk, k_codes, v_codes, k_page_ids, v_page_ids, k_cents, v_cents, k_resid,
                           v_resid, out, lse, workspace, workspace_bytes, stream);
}
