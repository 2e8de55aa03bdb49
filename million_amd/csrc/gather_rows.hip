// gather_rows.hip — million_pq_gather_rows (include/million_hip.h): a token range of every request, dequantised straight from its
// code store, followed by the valid rows of its residual window in ring order, as fp16 rows in a caller's scratch:
//
//   out[b, hk, j, :]            = dequant(codes[b, hk, t0 + j])           j < n_t = t1 - t0     (the gather of million_pq_decode)
//   out[b, hk, n_t + i, :]      = resid[b, hk, (resid_start + i) % resid_cap, :]               i < r
//
// for K and V in ONE launch (side = blockIdx.z, as paged_store_kernel).  Each side's codes are row-major (bs, nh_k, T_cap, M) or
// a page pool behind int32 page ids: K pages (n_pool, page, M), V pages (n_pool, M, page) transposed.
//
// Design
//   * a workgroup of 256 threads owns one tile of 64 output rows of one (b, kv head, side).  The codebook stays in global memory
//     and its entries are gathered through L1 / L2, for both code widths: a C = 4096 table (1 MiB) fits no LDS, and for uint8 codes
//     the form that stages the table (<= 64 KiB) in LDS once per workgroup was built and measured SLOWER - 211 - 232 us against
//     138 us for one 32K block at bs 1 (profiles/chunk_blocks.txt): 64 KiB staged per workgroup against 16 KiB of output per
//     tile, two workgroups per CU at that LDS size, and random 4-byte LDS reads that conflict.
//   * a tile in two phases.  (1) its 64 x M codes go global -> LDS in the order the STORE holds them - subspace fastest for
//     row-major codes and K pages, token fastest for the transposed V pages - so a wave's loads are consecutive bytes either way;
//     the LDS image is [token][M] with a row pitch of M code bytes + 4: an odd number of dwords, so the token-fastest writes of a
//     wave fall into different banks.  (2) thread = (row, 16-byte piece): it reads its 8 / d_m codes from LDS, fetches the
//     entries and stores ONE 16-byte piece; the d / 8 threads of a row store consecutive pieces: token-major rows leave as
//     16-byte stores whatever the layout of the codes.  Window rows are copied in phase 2, 16 bytes per thread.
//   * one body, gather_rows_body<Codes, DM>, for every code format, as chunk_attn_body has a code producer per format: a code
//     source (CodeWords<uint8_t>, CodeWords<uint16_t>, PackedPlanes) says the LDS row pitch, copies a tile's code bytes to LDS
//     (phase 1) and reads the code of a subspace from an LDS row (phase 2); the prologue, the tile bounds, phase 2 and the window
//     copy are shared.
//   * an index is c < C ? c : 0, million_pq_decode's rule, so the result is that call's bit for bit - for every code word.
//   * what is read: code words of tokens t0 <= t < t1 only, page ids of those tokens' pages only, window rows of the ring's
//     valid span only.  Every byte offset is 64-bit.
#include <string.h>

#include "common.h"

namespace million {

namespace {

constexpr int kGatherRows = 64;       // output rows per tile

struct GatherSide {
    const void *codes;                // row-major tensor or page pool
    const int *page_ids;              // paged: (bs, nh_k, n_pages_cap) int32
    const f16 *cents;                 // (M, C, d_m) fp16
    const f16 *resid;                 // (bs, nh_k, resid_cap, d)
    f16 *out;                         // (bs, nh_k, rows_cap, d)
    long long sb, sh;                 // row-major: bytes between batches / kv heads
    int paged;
};

struct GatherParams {
    GatherSide side[2];               // K, V
    int nh_k, d, M, C;
    int t0, n_t, r, rstart, rcap;     // tokens [t0, t0 + n_t), r window rows from rstart in a ring of rcap
    long long res_sb, res_sh, o_sb, o_sh;      // fp16 elements
    int ps_shift, n_pages_cap;
    int hb;                           // packed pages: high bits of a code beside its low byte (2 / 4)
};

// A code source: how a tile's code bytes reach LDS (phase 1) and how a code is read back from its LDS row (phase 2).
//   pitch(M, h)          bytes of a token's LDS row: its code bytes rounded to an odd number of dwords
//   load_tile(...)       the code bytes of tokens [t_first, t_first + n_code) of (b, hk) -> lds [row][pitch], read in the order the
//                        store holds them: a wave's loads are consecutive bytes
//   code(row, m, M, h)   the code of subspace m from an LDS row
template <typename CodeT>
struct CodeWords {      // one word per code: row-major (bs, nh_k, T, M) or K pages (n_pool, page, M) / V pages (n_pool, M, page)
    __host__ __device__ static int pitch(int M, int) { return M * (int)sizeof(CodeT) + 4; }
    __device__ static void load_tile(char *lds, const GatherParams &p, const GatherSide &s, int sidx, int b, int hk, int t_first, int n_code) {
        const int M = p.M, row_pitch = pitch(M, 0);
        const bool v_pages = s.paged && sidx == 1;       // transposed pages: token fastest
        const long long bh = (long long)b * p.nh_k + hk;
        const int *ids = s.paged ? s.page_ids + bh * p.n_pages_cap : nullptr;
        const char *rm_base = (const char *)s.codes + b * s.sb + hk * s.sh;      // row-major
        const int page = 1 << p.ps_shift;
        for (int e = threadIdx.x; e < kGatherRows * M; e += 256) {
            const int row = v_pages ? e % kGatherRows : e / M;
            const int m = v_pages ? e / kGatherRows : e % M;
            if (row < n_code) {
                const int t = t_first + row;             // < t1: the host checked t1 against the store's capacity
                long long off;                           // in code words
                if (s.paged) {
                    const long long pid = ids[t >> p.ps_shift];
                    const int tin = t & (page - 1);
                    off = v_pages ? (pid * M + m) * page + tin : (pid * page + tin) * M + m;
                } else {
                    off = (long long)t * M + m;
                }
                const CodeT c = s.paged ? ((const CodeT *)s.codes)[off] : ((const CodeT *)rm_base)[off];
                *(CodeT *)(lds + row * row_pitch + m * (int)sizeof(CodeT)) = c;
            }
        }
    }
    __device__ static unsigned code(const char *row, int m, int, int) { return ((const CodeT *)row)[m]; }
};

// Packed pages (million_hip.h, "Packed code pages"), pages only: the low plane's bytes, then the high plane's, each plane in the
// order the store holds it (subspace / high byte fastest for K pages, token fastest for the transposed V planes), one byte per
// thread.  The LDS row is [M low bytes | M h / 8 high bytes]; h = GatherParams::hb is a wave-uniform field.
struct PackedPlanes {
    __host__ __device__ static int pitch(int M, int h) { return 4 * (((M * (8 + h)) >> 5) | 1); }      // a token's bytes are a multiple of 4 (16 | M)
    __device__ static void load_tile(char *lds, const GatherParams &p, const GatherSide &s, int sidx, int b, int hk, int t_first, int n_code) {
        const int M = p.M, h = p.hb, row_pitch = pitch(M, h);
        const int HM = (M * h) >> 3;                     // high bytes of a token
        const bool v_pages = sidx == 1;                  // transposed planes: token fastest
        const long long bh = (long long)b * p.nh_k + hk;
        const int *ids = s.page_ids + bh * p.n_pages_cap;
        const int page = 1 << p.ps_shift;
        const long long page_bytes = (long long)page * ((M * (8 + h)) >> 3);      // no power of two
        const uint8_t *pool = (const uint8_t *)s.codes;
        for (int e = threadIdx.x; e < kGatherRows * (M + HM); e += 256) {
            const bool hi = e >= kGatherRows * M;        // wave-uniform: 64 M is a multiple of 256
            const int f = hi ? e - kGatherRows * M : e;
            const int W = hi ? HM : M;                   // bytes of a token in this plane
            const int row = v_pages ? f % kGatherRows : f / W;
            const int m = v_pages ? f / kGatherRows : f % W;
            if (row < n_code) {
                const int t = t_first + row;             // < t1
                const long long pid = ids[t >> p.ps_shift];
                const int tin = t & (page - 1);
                const int off = (hi ? page * M : 0) + (v_pages ? m * page + tin : tin * W + m);
                lds[row * row_pitch + (hi ? M : 0) + m] = (char)pool[pid * page_bytes + off];
            }
        }
    }
    // the raw (8 + h)-bit field of subspace m from its two bytes
    __device__ static unsigned code(const char *row, int m, int M, int h) {
        const uint8_t *r = (const uint8_t *)row;
        return (unsigned)r[m] | ((((unsigned)r[M + ((m * h) >> 3)] >> ((m * h) & 7)) & ((1u << h) - 1u)) << 8);
    }
};

// Codes: CodeWords<uint8_t>, CodeWords<uint16_t> or PackedPlanes.  DM = d / M.
template <typename Codes, int DM>
__global__ __launch_bounds__(256) void gather_rows_body(GatherParams p) {
    constexpr int NM = 8 / DM;                       // subspaces of a 16-byte piece
    typedef struct { f16 v[DM]; } __attribute__((aligned(2 * DM))) Entry;
    typedef f16 h8 __attribute__((ext_vector_type(8)));
    extern __shared__ __attribute__((aligned(16))) char lds_codes[];      // the tile's code bytes: 64 rows of pitch bytes
    const int tid = threadIdx.x;
    const int sidx = blockIdx.z;
    const GatherSide &s = p.side[sidx];
    const int b = blockIdx.y / p.nh_k, hk = blockIdx.y % p.nh_k;
    const int M = p.M, C = p.C, d = p.d, h = p.hb;
    const int pitch = Codes::pitch(M, h);
    const Entry *tab = (const Entry *)s.cents;
    f16 *out = s.out + b * p.o_sb + hk * p.o_sh;
    const f16 *resid = s.resid ? s.resid + b * p.res_sb + hk * p.res_sh : nullptr;
    const int tpr = d / 8;                           // threads (16-byte pieces) per row
    const int j0 = blockIdx.x * kGatherRows;         // this workgroup's tile
    int n_code = p.n_t - j0;                         // coded rows of this tile
    n_code = n_code < 0 ? 0 : (n_code > kGatherRows ? kGatherRows : n_code);
    // ---- phase 1: the tile's code bytes -> LDS [row][pitch] ----
    Codes::load_tile(lds_codes, p, s, sidx, b, hk, p.t0 + j0, n_code);
    __syncthreads();
    // ---- phase 2: thread = (row, 16-byte piece) ----
    for (int it = tid; it < kGatherRows * tpr; it += 256) {
        const int row = it / tpr, ch = it - row * tpr;
        const int j = j0 + row;
        if (row < n_code) {
            Entry en[NM];
#pragma unroll
            for (int i = 0; i < NM; ++i) {
                const int m = ch * NM + i;
                const unsigned c = Codes::code(lds_codes + row * pitch, m, M, h);
                en[i] = tab[(long long)m * C + (c < (unsigned)C ? c : 0u)];
            }
            h8 o;
#pragma unroll
            for (int i = 0; i < NM; ++i)
#pragma unroll
                for (int k = 0; k < DM; ++k) o[i * DM + k] = en[i].v[k];
            *(h8 *)(out + (long long)j * d + 8 * ch) = o;
        } else if (j - p.n_t < p.r) {
            int rr = p.rstart + (j - p.n_t);
            rr = rr >= p.rcap ? rr - p.rcap : rr;
            *(h8 *)(out + (long long)j * d + 8 * ch) = *(const h8 *)(resid + (long long)rr * d + 8 * ch);
        }
    }
}

}  // namespace

}  // namespace million

using namespace million;

// `packed`: million_pq_gather_rows_packed - both sides pools of packed pages, code_bytes = 2 (the logical width of a code)
static int gather_rows_impl(bool packed, const million_gather_rows_desc *desc, const void *k_codes, const void *v_codes,
                            const int32_t *k_page_ids, const int32_t *v_page_ids, const void *k_cents,
                            const void *v_cents, const void *k_resid, const void *v_resid, void *k_out, void *v_out,
                            million_stream_t stream) {
    if (!desc || desc->struct_size != sizeof(million_gather_rows_desc)) { set_error("gather_rows: bad desc / struct_size"); return MILLION_ERR_ARG; }
    const million_gather_rows_desc &d = *desc;
    if (d.bs <= 0 || d.nh_k <= 0 || (long long)d.bs * d.nh_k > 65535) { set_error("gather_rows: bs=%d nh_k=%d (bs * nh_k <= 65535)", d.bs, d.nh_k); return MILLION_ERR_SHAPE; }
    if (d.d != 128 && d.d != 64) { set_error("gather_rows: d=%d (64 or 128)", d.d); return MILLION_ERR_SHAPE; }
    if (d.M <= 0 || d.d % d.M || (d.d / d.M != 1 && d.d / d.M != 2 && d.d / d.M != 4 && d.d / d.M != 8)) {
        set_error("gather_rows: d=%d M=%d (d/M 1, 2, 4 or 8)", d.d, d.M);
        return MILLION_ERR_SHAPE;
    }
    if (d.code_bytes == 1) {
        if (d.C < 1 || d.C > 256) { set_error("gather_rows: C=%d with uint8 codes (1 .. 256)", d.C); return MILLION_ERR_SHAPE; }
    } else if (d.code_bytes == 2) {
        if (d.C != 512 && d.C != 1024 && d.C != 2048 && d.C != 4096) { set_error("gather_rows: C=%d with uint16 codes (512, 1024, 2048 or 4096)", d.C); return MILLION_ERR_SHAPE; }
    } else { set_error("gather_rows: code_bytes=%d (1: uint8, 2: uint16)", d.code_bytes); return MILLION_ERR_SHAPE; }
    if (packed) {
        if (d.code_bytes != 2) { set_error("gather_rows_packed: code_bytes=%d (2: packed pages hold codes of 512 .. 4096 centroids)", d.code_bytes); return MILLION_ERR_SHAPE; }
        if (!wide_geometry(d.d, d.M, d.C, 1)) { set_error("gather_rows_packed: d=%d M=%d C=%d (d 64 / 128, d / M 2 or 4, C 512 / 1024 / 2048 / 4096)", d.d, d.M, d.C); return MILLION_ERR_SHAPE; }
        if (d.k_layout != MILLION_KV_PAGED || d.v_layout != MILLION_KV_PAGED) {
            set_error("gather_rows_packed: k_layout=%d v_layout=%d (both MILLION_KV_PAGED: packed codes live in pages only)", d.k_layout, d.v_layout);
            return MILLION_ERR_SHAPE;
        }
    }
    if (d.t0 < 0 || d.t1 < d.t0 || d.r < 0 || d.resid_cap < 0 || d.r > d.resid_cap || d.resid_start < 0 || (d.resid_cap > 0 && d.resid_start >= d.resid_cap) ||
        (d.resid_cap == 0 && d.resid_start != 0)) {
        set_error("gather_rows: t0=%d t1=%d r=%d resid_start=%d resid_cap=%d", d.t0, d.t1, d.r, d.resid_start, d.resid_cap);
        return MILLION_ERR_ARG;
    }
    const long long n_rows = (long long)(d.t1 - d.t0) + d.r;
    if (d.rows_cap < 0 || n_rows > d.rows_cap) { set_error("gather_rows: %lld rows into rows_cap=%d", n_rows, d.rows_cap); return MILLION_ERR_ARG; }
    const bool kp = d.k_layout == MILLION_KV_PAGED, vp = d.v_layout == MILLION_KV_PAGED;
    if ((!kp && d.k_layout != MILLION_KV_ROWMAJOR) || (!vp && d.v_layout != MILLION_KV_ROWMAJOR)) { set_error("gather_rows: k_layout=%d v_layout=%d", d.k_layout, d.v_layout); return MILLION_ERR_ARG; }
    int ps_shift = 7;
    if (kp || vp) {
        if (!page_shift("gather_rows", d.page_size, ps_shift)) return MILLION_ERR_SHAPE;
        // the table is indexed and its tokens are counted with 32-bit arithmetic (fill_attn_params' limits)
        if (d.n_pages_cap < 0 || (long long)d.bs * d.nh_k * d.n_pages_cap > 0x7fffffffLL || (long long)d.n_pages_cap * d.page_size > 0x7fffffffLL) {
            set_error("gather_rows: page table of %lld entries, %lld tokens per row", (long long)d.bs * d.nh_k * d.n_pages_cap, (long long)d.n_pages_cap * d.page_size);
            return MILLION_ERR_ARG;
        }
        if ((long long)d.n_pages_cap * d.page_size < d.t1) { set_error("gather_rows: n_pages_cap*page_size < t1"); return MILLION_ERR_ARG; }
    }
    if (n_rows == 0) return MILLION_OK;
    if (!k_out || !v_out) { set_error("gather_rows: null pointer (out)"); return MILLION_ERR_ARG; }
    if (d.t1 > d.t0 && (!k_codes || !v_codes || !k_cents || !v_cents || (kp && !k_page_ids) || (vp && !v_page_ids))) {
        set_error("gather_rows: null pointer (codes, codebooks or page ids)");
        return MILLION_ERR_ARG;
    }
    if (d.r > 0 && (!k_resid || !v_resid)) { set_error("gather_rows: null pointer (window)"); return MILLION_ERR_ARG; }
    if (((uintptr_t)k_out | (uintptr_t)v_out | (uintptr_t)k_resid | (uintptr_t)v_resid | (uintptr_t)k_cents | (uintptr_t)v_cents) & 15) {
        set_error("gather_rows: out, window and codebook pointers must be 16-byte aligned");
        return MILLION_ERR_ALIGN;
    }
    if ((d.o_stride_b | d.o_stride_h | d.resid_stride_b | d.resid_stride_h) & 7) { set_error("gather_rows: out and window strides must be multiples of 8 elements (16-byte rows)"); return MILLION_ERR_ALIGN; }
    if (packed && (((uintptr_t)k_codes | (uintptr_t)v_codes) & 15)) { set_error("gather_rows_packed: the pools must be 16-byte aligned"); return MILLION_ERR_ALIGN; }
    if (d.code_bytes == 2 && ((((uintptr_t)k_codes | (uintptr_t)v_codes) & 1) || ((d.k_stride_b | d.k_stride_h | d.v_stride_b | d.v_stride_h) & 1))) {
        set_error("gather_rows: uint16 codes need 2-byte aligned pointers and strides");
        return MILLION_ERR_ALIGN;
    }
    GatherParams p;
    memset(&p, 0, sizeof(p));
    p.side[0] = {k_codes, k_page_ids, (const f16 *)k_cents, (const f16 *)k_resid, (f16 *)k_out, d.k_stride_b, d.k_stride_h, kp ? 1 : 0};
    p.side[1] = {v_codes, v_page_ids, (const f16 *)v_cents, (const f16 *)v_resid, (f16 *)v_out, d.v_stride_b, d.v_stride_h, vp ? 1 : 0};
    p.nh_k = d.nh_k; p.d = d.d; p.M = d.M; p.C = d.C;
    p.t0 = d.t0; p.n_t = d.t1 - d.t0; p.r = d.r; p.rstart = d.resid_start; p.rcap = d.resid_cap;
    p.res_sb = d.resid_stride_b; p.res_sh = d.resid_stride_h; p.o_sb = d.o_stride_b; p.o_sh = d.o_stride_h;
    p.ps_shift = ps_shift; p.n_pages_cap = d.n_pages_cap;
    p.hb = packed ? packed_hi_bits(d.C) : 0;
    const long long n_tiles = (n_rows + kGatherRows - 1) / kGatherRows;      // < 2^26: n_rows fits an int
    const dim3 grid((unsigned)n_tiles, (unsigned)(d.bs * d.nh_k), 2);
    const hipStream_t s = (hipStream_t)stream;
    // the one place an instance is picked: (code source, d / M) - 8 over code words, 2 over packed pages
    const bool ok = dispatch_dm(d.d / d.M, [&](auto w) {
        auto launch = [&](auto codes) {
            typedef decltype(codes) Codes;
            hipLaunchKernelGGL((gather_rows_body<Codes, w()>), grid, dim3(256), kGatherRows * Codes::pitch(d.M, p.hb), s, p);
        };
        if constexpr (w() == 2 || w() == 4) if (packed) return launch(PackedPlanes());
        if (d.code_bytes == 1) launch(CodeWords<uint8_t>());
        else launch(CodeWords<uint16_t>());
    });
    if (!ok) { set_error("gather_rows: d/M=%d unsupported (1, 2, 4, 8)", d.d / d.M); return MILLION_ERR_SHAPE; }
    const hipError_t e = hipGetLastError();
    if (e != hipSuccess) { set_error("gather_rows launch: %s", hipGetErrorString(e)); return MILLION_ERR_LAUNCH; }
    return MILLION_OK;
}

extern "C" int million_pq_gather_rows(const million_gather_rows_desc *desc, const void *k_codes, const void *v_codes,
                                      const int32_t *k_page_ids, const int32_t *v_page_ids, const void *k_cents,
                                      const void *v_cents, const void *k_resid, const void *v_resid, void *k_out, void *v_out,
                                      million_stream_t stream) {
    return gather_rows_impl(false, desc, k_codes, v_codes, k_page_ids, v_page_ids, k_cents, v_cents, k_resid, v_resid, k_out, v_out, stream);
}

extern "C" int million_pq_gather_rows_packed(const million_gather_rows_desc *desc, const void *k_pool, const void *v_pool,
                                             const int32_t *k_page_ids, const int32_t *v_page_ids, const void *k_cents,
                                             const void *v_cents, const void *k_resid, const void *v_resid, void *k_out, void *v_out,
                                             million_stream_t stream) {
    return gather_rows_impl(true, desc, k_pool, v_pool, k_page_ids, v_page_ids, k_cents, v_cents, k_resid, v_resid, k_out, v_out, stream);
}
