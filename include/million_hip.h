/*
 * million_hip.h — C ABI of libmillion_hip.so: MI355X-native (gfx950) PQ-KV attention hot path.
 *
 * This is the drop-in boundary below the reference's Python module `bindings`
 * (reference: scripts/modeldb/bindings/bindings.template.cpp:11-63 declares, and
 * scripts/modeldb/bindings/Interface.template.cu:16-147 defines, one torch-typed C++ symbol per
 * (Ns, Lt, d, M, C) tuple).  Here ONE set of plain-C entry points sits behind all those names:
 * plain pointers and sizes, no torch types.  The Python shim `bindings/` (built by `make bindings`)
 * re-exports the reference's function names on top of these entry points.
 *
 * Conventions
 *   - every pointer is a DEVICE pointer unless the name starts with `host_`;
 *   - fp16 tensors are IEEE binary16 (`_Float16`), codes are uint8 (reference setup.py:10-11);
 *   - `stream` is a hipStream_t passed as void* (NULL = the legacy default stream, which is what the
 *     reference launches on, Interface.template.cu:65,88,109);
 *   - functions return MILLION_OK (0) or a negative error code and NEVER exit the process
 *     (the reference's gpuErrchk calls exit(), Interface.template.cu:3-11); million_last_error()
 *     returns a thread-local description of the last failure;
 *   - no entry point allocates, frees or synchronises: all are legal inside hipGraph capture.
 */
#ifndef MILLION_HIP_H
#define MILLION_HIP_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define MILLION_HIP_VERSION 1

enum {
    MILLION_OK = 0,
    MILLION_ERR_SHAPE = -1,       /* unsupported or inconsistent shape */
    MILLION_ERR_ALIGN = -2,       /* pointer / stride alignment */
    MILLION_ERR_ARG = -3,         /* null pointer, bad enum, r out of range ... */
    MILLION_ERR_WORKSPACE = -4,   /* workspace too small */
    MILLION_ERR_LAUNCH = -5       /* hipGetLastError() after launch */
};

typedef void *million_stream_t;

int million_version(void);
const char *million_last_error(void);

/* ------------------------------------------------------------------------------------------------
 * Codebook preparation.
 * Replaces: the per-call `.contiguous()` / transposes the reference applies to the centroid table
 * (scripts/utils/pq_utils.py:149-159 set_cent; Interface.template.cu:49-50 key_cents.transpose).
 * Input : cents (M, C, d_m) fp16 contiguous — the reference's codebook tensor (main_pq.py:252-260).
 * Output: `prepared`, million_prepared_cents_bytes() bytes, two LDS-ready images back to back:
 *           [0, M*C*d_m*2)            "row image"  [m][c][d_m]   (bank = code: used for K lookups)
 *           [M*C*d_m*2, 2*M*C*d_m*2)  "col image"  [c][m][d_m]   (bank = subspace: used for V lookups)
 * Call once per codebook (set_cent time); the decode entry points take prepared tables. */
size_t million_prepared_cents_bytes(int M, int C, int d_m);
int million_prepare_cents(const void *cents, int M, int C, int d_m, void *prepared,
                          million_stream_t stream);

/* ------------------------------------------------------------------------------------------------
 * PQ encode.
 * Replaces: sa_encode_4d_keops (scripts/utils/pq_utils.py:451-499; call sites :189-190,:235-236,
 * :292-293 and paged_pq_utils.py:161,167,241-242) plus the permute+cat that stores the codes
 * (pq_utils.py:140-147, paged_pq_utils.py:162,173-175).
 * codes[b,hk,t,m] = argmin_c sum_k (x[b,hk,t,m*d_m+k] - cents[m,c,k])^2, fp32 direct form,
 * sequential k, lowest c wins ties; bit-exact with oracle/pq_oracle.c:pq_encode_direct. */
enum {
    MILLION_CODES_ROWMAJOR = 0,   /* dst (bs, nh_k, T_cap, M): reference layout, pq_utils.py:497-499 */
    MILLION_CODES_KPAGES = 1,     /* dst pool (n_pool, page_size, M), via page ids                     */
    MILLION_CODES_VPAGES = 2      /* dst pool (n_pool, M, page_size): transposed pages,                */
                                  /*     paged_pq_utils.py:173-175, MILLION_技术分析文档.md:1330-1340   */
};

typedef struct {
    uint32_t struct_size;         /* = sizeof(million_encode_desc) */
    int32_t bs, nh_k, n;          /* X is (bs, nh_k, n, d) */
    int32_t d, M, C;
    int64_t x_stride_b, x_stride_h, x_stride_n;   /* in fp16 elements; innermost dim contiguous */
    int32_t x_row_start, x_row_mod;   /* row t of X is read at ((x_row_start + t) % x_row_mod) if x_row_mod > 0
                                         (residual ring buffer); else at t */
    int32_t dst_layout;           /* MILLION_CODES_* */
    int32_t dst_token_start;      /* first destination token index t0: tokens [t0, t0+n) are written */
    int64_t dst_stride_b, dst_stride_h;   /* bytes; ROWMAJOR only (row stride is M bytes) */
    int32_t page_size;            /* KPAGES / VPAGES */
    int32_t n_pages_cap;          /* page_ids is (bs, nh_k, n_pages_cap) int32 */
    const int32_t *dev_lengths;   /* optional device array (bs, 4) = {n_tokens, r, resid_start, 0}: when set,
                                     dst_token_start := n_tokens and x_row_start := resid_start are read on the
                                     device (flush of the residual window inside a replayed hipGraph) */
    const void *cents_prepared;   /* optional: the same codebook through million_prepare_cents (its fp32 image
                                     feeds the scalar operands of the distance loop: ~1.6x faster); codes are
                                     identical with or without it */
} million_encode_desc;

int million_pq_encode(const million_encode_desc *desc, const void *x, const void *cents /* (M,C,d_m) fp16 */,
                      void *dst, const int32_t *page_ids, million_stream_t stream);
/* Code width: C <= 256 -> dst holds uint8 codes; 256 < C <= 65536 (nbits 9..16) -> uint16 codes in the same three
 * layouts (reference nbits2dtype, scripts/utils/pq_utils.py:542-552; sa_encode_4d*(target_dtype=...), :449/:499).
 * dst_stride_b / dst_stride_h stay in BYTES.  The decode-attention kernels are uint8-only, as the reference's are
 * (setup.py:10-11); wide codes serve the dequantise-then-attend path (DynamicPQCache.update, pq_utils.py:166-220). */

/* One launch per window flush.
 * Replaces: PagedPQCache.flush_to_pages (scripts/utils/paged_pq_utils.py:130-210): encode of the oldest `desc->n` K
 * rows and V rows of the residual window (two sa_encode_4d_keops calls, :161,:167), the permute + torch.cat that store
 * them (:162,:173-175) and the window shift (:188-204; here: the ring start advances).
 * desc describes the K side: X = k_rows (the K window buffer; the V window must have the same shape and strides),
 * dst_layout = MILLION_CODES_KPAGES into k_pool; the V side is written as MILLION_CODES_VPAGES into v_pool through the
 * same page ids.  dev_lengths (must equal desc->dev_lengths; may be NULL): the destination token and the ring start are
 * read on the device and, once every workgroup has read them, advanced there (n_tokens += n, r -= n, resid_start =
 * (resid_start + n) % resid_cap; the 4th word of each row is the workgroups' ticket and is left at 0).  uint8 codes.
 * min_r (device lengths only; 0 = every batch item): batch items whose window holds fewer than min_r rows are left alone -
 * requests of different lengths share the launch and only those whose window is full flush (pass resid_cap). */
int million_pq_flush(const million_encode_desc *desc, const void *k_rows, const void *v_rows,
                     const void *k_cents, const void *v_cents, void *k_pool, void *v_pool,
                     const int32_t *page_ids, int32_t *dev_lengths, int resid_cap, int min_r, million_stream_t stream);

/* The same for n_layers layers of a cache in ONE launch, and optionally WITHOUT moving the window (encode-ahead).
 * The layers' K / V window buffers, page tables and length rows lie rows_layer_stride fp16 elements, ids_layer_stride
 * int32 and lengths_layer_stride int32 apart (layer 0 at the pointers given); pools and codebooks are shared, as in the
 * reference (one PagedPQCache, one codebook pair for all layers: paged_pq_utils.py:70-80, pq_utils.py:149-159).
 * advance = 0: the rows are encoded into the pages of tokens [n_tokens, n_tokens + n) and nothing else changes - the oldest
 * page of window rows is complete long before the window is full (the reference flushes at r >= extended_residual_size,
 * paged_pq_utils.py:359-361; the rows exist from r >= page_size on), so a cache can encode them during any earlier step,
 * beside that step's attention launches (the kernel runs 4 waves of <= 32 registers per workgroup: it fits on a CU next to
 * an attention workgroup), and commit the flush later with million_lengths_advance alone.  Codes and final state are
 * identical to million_pq_flush at the flush step.  min_r (device lengths) then means "rows present": pass page_size. */
int million_pq_flush_layers(const million_encode_desc *desc, const void *k_rows, const void *v_rows,
                            const void *k_cents, const void *v_cents, void *k_pool, void *v_pool,
                            const int32_t *page_ids, int32_t *dev_lengths, int resid_cap, int min_r,
                            int n_layers, int64_t rows_layer_stride, int64_t ids_layer_stride, int64_t lengths_layer_stride,
                            int advance, million_stream_t stream);

/* The store step of a ragged batch: ONE call for every request, every per-request value read on the device.
 * Replaces, behind a ragged attention launch (million_pq_chunk_attn with dev_lengths / dev_n_q, million_prefill_attn with
 * dev_spans), the host loop of up to four million_pq_encode calls and one lengths copy per request.
 * Request b has the row {T, r, start, word 3} in dev_lengths (bs, 4) and n_b = dev_n[b] new rows.  n_b = 0: the request takes no
 * part - nothing of it is read beyond those words and nothing is written.  Otherwise it has r + n_b source rows: source row
 * j < r is row (start + j) % resid_cap of its window (k_resid / v_resid (bs, nh_k, resid_cap, d), row stride d), source row
 * j >= r is row j - r of k_new / v_new (bs, nh_k, n_bound, d); source row j becomes token T + j: its K codes go to k_pool in the
 * MILLION_CODES_KPAGES layout, its V codes to v_pool in the MILLION_CODES_VPAGES layout, through the same page_ids
 * (bs, nh_k, n_pages_cap) int32.  Codes are those of million_pq_encode, bit for bit (same arithmetic contract).  Then the row is
 * advanced: T <- min(T + r + n_b, n_pages_cap * page_size), r <- 0, start <- 0; word 3 is neither read nor written.
 * The values are not trusted: T is clamped into [0, n_pages_cap * page_size], r into [0, resid_cap], a start outside
 * [0, resid_cap) reads as 0, n_b is clamped into [0, n_bound]; everything above, the advance included, uses the clamped values.
 * A destination token whose page index is >= n_pages_cap drops its store.  Page ids are read only for pages that receive a token.
 * What may hold anything (NaN, garbage, stale ids) and is never read, and what is never written: new rows at or past n_b, window
 * rows outside each request's ring span, every row of a request with n_b = 0 (its lengths row and pages included), page-table
 * entries past the pages written, pool bytes outside the destination tokens.
 * Shapes: d = 128 or 64 with M in {64, 32, 16}, uint8 codes (C <= 256), page_size 32 / 64 / 128, bs * nh_k <= 32767; anything
 * else: MILLION_ERR_SHAPE.  Both codebooks as million_prepare_cents wrote them (required: MILLION_ERR_ARG when null, like null
 * dev_n / dev_lengths / rows / pools / page ids, and null windows with resid_cap > 0).  Rows, windows, codebooks and pools 16-byte
 * aligned, strides multiples of 8 elements: MILLION_ERR_ALIGN otherwise.  n_bound = 0 returns MILLION_OK whatever the pointers.
 * Capture: two launches on `stream` - the encode grid, sized by the bounds alone (ceil((resid_cap + n_bound) / 64) token blocks x
 * subspace groups x bs * nh_k x 2 sides), then one thread per request for the advance; stream order is the only ordering.  The
 * call allocates nothing, synchronises nothing and is a pure function of the descriptor: a captured call follows dev_lengths,
 * dev_n, the rows and the page table as they are when it is replayed. */
typedef struct {
    uint32_t struct_size;         /* = sizeof(million_store_ragged_desc) */
    int32_t bs, nh_k, d, M, C;
    int32_t n_bound;              /* rows of k_new / v_new per (b, hk): the bound of dev_n */
    int64_t kn_stride_b, kn_stride_h, kn_stride_n;   /* k_new, fp16 elements; the d elements of a row are contiguous */
    int64_t vn_stride_b, vn_stride_h, vn_stride_n;   /* v_new */
    int32_t resid_cap;            /* rows of the window buffers; 0: no window (k_resid / v_resid may be NULL) */
    int32_t page_size;            /* 32, 64 or 128 */
    int64_t resid_stride_b, resid_stride_h;          /* both windows, fp16 elements; row stride is d */
    int32_t n_pages_cap;          /* row length of page_ids */
} million_store_ragged_desc;

int million_pq_store_ragged(const million_store_ragged_desc *desc, const void *k_new, const void *v_new,
                            const void *k_resid, const void *v_resid,
                            const void *k_cents_prepared, const void *v_cents_prepared,   /* million_prepare_cents */
                            void *k_pool, void *v_pool, const int32_t *page_ids,
                            int32_t *dev_lengths /* (bs, 4), advanced */, const int32_t *dev_n /* (bs,) */,
                            million_stream_t stream);

/* The window flush of a cache with 9 .. 12-bit codes (C in 512 .. 4096), for uint16 pages and - packed != 0 - packed pages
 * ("Packed code pages" below): million_pq_flush's arguments and meaning, one encode launch for both sides.
 * desc describes the K side as for million_pq_flush (X = k_rows (bs, nh_k, resid_cap, d), the V window of the same shape and
 * strides; dst_layout = MILLION_CODES_KPAGES; x_row_mod = resid_cap; n <= page_size rows).  The oldest n rows of every request's
 * K and V ring window - rows (start + t) % resid_cap, t < n - become tokens [T, T + n) of its K pages (page_size, M) and
 * transposed V pages (M, page_size) through the one page table page_ids (bs, nh_k, n_pages_cap) int32.  k_cents / v_cents are the
 * plain (M, C, d_m) fp16 codebooks (wide formats have no prepared image; desc->cents_prepared is not read).  Codes are those of
 * million_pq_encode / million_pq_encode_packed, bit for bit (same arithmetic contract).
 * dev_lengths NULL (then desc->dev_lengths too): T = desc->dst_token_start and start = desc->x_row_start for every request - the
 * lockstep, host-length form; both are checked against the table and the ring (MILLION_ERR_ARG), min_r is not read, nothing is
 * advanced.  dev_lengths (bs, 4) (must equal desc->dev_lengths): every request's row {T, r, start, word 3} is read on the device
 * and not trusted - T clamped into [0, n_pages_cap * page_size], r into [0, resid_cap], a start outside [0, resid_cap) reads as
 * 0 - and everything below uses the clamped values.  A request with r < min_r takes no part: nothing of it is read beyond the row,
 * nothing of it is written, its row stays as it is (pass resid_cap: only full windows flush; 0: every request).  A destination
 * token whose page index is >= n_pages_cap drops its store; page ids are read only for pages that receive a token.  The rows of
 * the requests that took part then advance: T <- min(T + n, n_pages_cap * page_size), r <- max(r - n, 0), start <- (start + n) %
 * resid_cap; word 3 is neither read nor written (there is no ticket).
 * Never read: window rows outside [start, start + n) of the ring, any row of a request that takes no part, page-table entries of
 * pages that receive no token.  Never written: pool bytes outside the destination tokens (every byte written belongs to one
 * token; all stores are plain vector stores), the windows, the page table.
 * Shapes: d = 128 or 64 with d / M in {2, 4}, C in {512, 1024, 2048, 4096}, page_size 32 / 64 / 128, n <= page_size,
 * bs * nh_k <= 32767 (packed: 4 | M); anything else: MILLION_ERR_SHAPE.  Null rows / codebooks / pools / page ids with n > 0:
 * MILLION_ERR_ARG.  Rows, codebooks and pools 16-byte aligned, strides multiples of 8 elements: MILLION_ERR_ALIGN.  n = 0 returns
 * MILLION_OK whatever the pointers.
 * Capture: one encode launch on `stream` (ceil(n / 64) token blocks x M / 4 subspace groups x bs * nh_k x 2 sides, 16 waves per
 * workgroup, 40 KiB of LDS) and, with dev_lengths, one thread per request for the advance; stream order is the only ordering.
 * The call allocates nothing, synchronises nothing and is a pure function of its arguments: a captured call follows dev_lengths,
 * the rows and the page table as they are when it is replayed. */
int million_pq_flush_wide(const million_encode_desc *desc, const void *k_rows, const void *v_rows,
                          const void *k_cents, const void *v_cents, void *k_pool, void *v_pool,
                          const int32_t *page_ids, int32_t *dev_lengths, int resid_cap, int min_r, int packed,
                          million_stream_t stream);

/* million_pq_flush_wide for n_layers layers of a cache in one call, and optionally WITHOUT moving the window (encode-ahead):
 * million_pq_flush_wide's contract with million_pq_flush_layers' extra arguments.  The layers' K / V windows, page tables and
 * length rows lie rows_layer_stride fp16 elements (a multiple of 8), ids_layer_stride int32 and lengths_layer_stride int32 apart,
 * layer 0 at the pointers given; pools and codebooks are shared.  Everything stated above holds per (layer, request).
 * advance != 0: every (layer, request) is flushed by one encode grid of the 16-wave workgroups above (z = n_layers * bs * nh_k *
 *   2 units), and with dev_lengths ONE more launch, a thread per (layer, request), advances the rows of those that took part.
 * advance == 0 (encode-ahead): the rows become tokens [T, T + n) of the pages and nothing else changes: no advance launch, no
 *   write to dev_lengths, word 3 included.  min_r (device lengths) then means "rows present": pass page_size; a request with
 *   r < min_r takes no part.  The oldest page of window rows is complete resid_cap - page_size steps before it must be flushed,
 *   so a cache encodes it during an earlier step beside that step's attention launches and commits the flush later with
 *   million_lengths_advance alone; codes and final state are those of the flush at the flush step.  Built for that: one launch of
 *   4-wave workgroups (wave = one of the group's 4 subspaces, scanning its whole centroid range; <= 72 registers, <= 9 KiB of LDS:
 *   one fits on a CU beside a wide attention workgroup at d = 128).  Only `pairs_in_flight` (layer, request) pairs are in the grid
 *   (z = pairs_in_flight * nh_k * 2) and the workgroups walk the other pairs; 0: the library's rule (about one workgroup per CU
 *   in flight), a positive value is clamped into [1, n_layers * bs], a negative one is MILLION_ERR_ARG.  pairs_in_flight is not
 *   read when advance != 0.
 * Checks: million_pq_flush_wide's, in the same order with the same codes; n_layers < 0 or n_layers * bs * nh_k > 32767:
 * MILLION_ERR_SHAPE; n = 0 or n_layers = 0: MILLION_OK whatever the pointers.  Capture as million_pq_flush_wide. */
int million_pq_flush_wide_layers(const million_encode_desc *desc, const void *k_rows, const void *v_rows,
                                 const void *k_cents, const void *v_cents, void *k_pool, void *v_pool,
                                 const int32_t *page_ids, int32_t *dev_lengths, int resid_cap, int min_r,
                                 int n_layers, int64_t rows_layer_stride, int64_t ids_layer_stride, int64_t lengths_layer_stride,
                                 int advance, int packed, int pairs_in_flight, million_stream_t stream);

/* million_pq_store_ragged over uint16 pages and - packed != 0 - packed pages: the same descriptor, meaning, clamps, grid rule and
 * two launches (the advance kernel is the same), with plain (M, C, d_m) fp16 codebooks in place of the prepared ones and C in
 * {512, 1024, 2048, 4096}.  What is read, what may hold anything and is never read, and what is never written are as stated there;
 * codes are those of million_pq_encode / million_pq_encode_packed, bit for bit.  Shapes: d = 128 or 64 with d / M in {2, 4}
 * (packed: 4 | M), page_size 32 / 64 / 128, bs * nh_k <= 32767: MILLION_ERR_SHAPE otherwise; nulls MILLION_ERR_ARG, alignment
 * MILLION_ERR_ALIGN, n_bound = 0 MILLION_OK, capture behaviour as million_pq_store_ragged. */
int million_pq_store_ragged_wide(const million_store_ragged_desc *desc, const void *k_new, const void *v_new,
                                 const void *k_resid, const void *v_resid,
                                 const void *k_cents, const void *v_cents,   /* (M, C, d_m) fp16 */
                                 void *k_pool, void *v_pool, const int32_t *page_ids,
                                 int32_t *dev_lengths /* (bs, 4), advanced */, const int32_t *dev_n /* (bs,) */,
                                 int packed, million_stream_t stream);

/* Fork a request of a paged cache: ONE call (one launch) makes n_dst batch slots a copy of slot `src`, for every layer.
 * Serves one long prompt with several questions or sampled continuations: the prompt is encoded once; the other requests
 * share its code pages (SHARE) or get a private copy of them (COPY), and each gets the window and the lengths row.
 * The layout is that of million_pq_flush_layers: page_ids (layers, bs, nh_k, n_pages_cap) int32, k_resid / v_resid
 * (layers, bs, nh_k, resid_cap, d) fp16, dev_lengths (layers, bs, 4) int32, the layers ids_layer_stride int32, rows_layer_stride
 * fp16 elements and lengths_layer_stride int32 apart (inside a layer the arrays are dense); K pool (n_pool, page_size, M) and
 * V pool (n_pool, M, page_size) uint8, shared by all layers.  dst_slots: device (n_dst,) int32; tail_ids: device
 * (n_dst, layers, nh_k) int32, the private page id of each destination's partial tail page (SHARE; may be NULL in COPY mode).
 * Per layer l - every per-request value is read on the device and not trusted:
 *   Source row {T, r, start, word 3} = dev_lengths[l, src]: T is clamped into [0, n_pages_bound * page_size], r into
 *     [0, resid_cap], a start outside [0, resid_cap) reads as 0.  prefix_tokens = p >= 0: T <- min(T, p), r <- 0, start <- 0 and the
 *     window is not copied (the destination becomes the source as it was after its first p tokens, when those were all codes).
 *   full = T / page_size, tail = T % page_size, n_live = full + (tail ? 1 : 0).
 *   Entry e_j of page j < n_live of each destination slot and kv head h - SHARE: the source's id for j < full and
 *     tail_ids[dst index, l, h] for the partial page j = full, and e_j is written into the destination's table row; COPY: the
 *     destination's own entry, the table is not written.  Entries at or past n_live are neither read nor written.
 *   Page j is copied iff e_j differs from the source's id for page j: the whole page on both sides (page_size * M bytes of the K
 *     page, M * page_size bytes of the transposed V page).  Both ids must lie in [0, n_pool): otherwise the copy is dropped - no
 *     fault, no error.
 *   Without a prefix all resid_cap rows of both source windows are copied to each destination, byte for byte, ring position
 *     for ring position.  The destination's lengths row becomes {T, r, start, 0} from the clamped values.
 * Never touched: the source's table row, pages, windows and lengths row, and every slot that is no destination.  A destination
 * equal to src, outside [0, bs), or named by an earlier entry of dst_slots takes no part.  Destination tables (COPY) and tail ids
 * must name pages no other row of the call reads or writes: overlapping ids stay inside the pools but the bytes are then
 * whatever write came last.
 * Errors, all before any launch: null pointers (windows: only when resid_cap > 0 and there is no prefix), src outside [0, bs), a
 * bad struct_size, mode, n_dst < 0 or n_pages_bound outside [0, n_pages_cap]: MILLION_ERR_ARG; page_size not 32 / 64 / 128, M not
 * 16 / 32 / 64, d no positive multiple of 8: MILLION_ERR_SHAPE; pools and windows 16-byte aligned, rows_layer_stride a multiple of
 * 8: MILLION_ERR_ALIGN otherwise.  n_dst = 0 returns MILLION_OK whatever the pointers.
 * One launch on `stream`: 16-byte vector copies, the grid a function of the bounds alone (n_pages_bound pages per (layer,
 * destination, kv head) in COPY mode, one in SHARE mode, the window, one table / lengths task; at most 2048 workgroups that
 * stride over it).  The call allocates nothing, synchronises nothing, uses no atomics, flags or workspace; every destination
 * byte is a function of source bytes and the arguments alone, so a captured call follows the device arrays. */
enum {
    MILLION_FORK_SHARE = 0,       /* destinations name the source's full pages; a private copy of the partial tail page only */
    MILLION_FORK_COPY = 1         /* destinations keep the ids their table rows hold and get a copy of every live page */
};

typedef struct {
    uint32_t struct_size;         /* = sizeof(million_fork_desc) */
    int32_t n_layers, bs, nh_k, d, M, page_size;
    int32_t n_pages_cap;          /* row length of page_ids */
    int32_t n_pool;               /* pages in each pool */
    int32_t resid_cap;            /* rows of the window buffers; 0: no window */
    int64_t ids_layer_stride;     /* int32 between the layers of page_ids */
    int64_t rows_layer_stride;    /* fp16 elements between the layers of k_resid / v_resid */
    int64_t lengths_layer_stride; /* int32 between the layers of dev_lengths */
    int32_t src, n_dst;
    int32_t mode;                 /* MILLION_FORK_* */
    int32_t n_pages_bound;        /* host bound of the pages a request can have, <= n_pages_cap: sizes the COPY grid, clamps T */
    int32_t prefix_tokens;        /* -1: everything, window included; p >= 0: the first min(T, p) tokens */
} million_fork_desc;

int million_cache_fork(const million_fork_desc *desc, int32_t *page_ids, void *k_pool, void *v_pool,
                       void *k_resid, void *v_resid, int32_t *dev_lengths /* (layers, bs, 4) */,
                       const int32_t *dst_slots /* (n_dst,) */, const int32_t *tail_ids /* (n_dst, layers, nh_k) or NULL */,
                       million_stream_t stream);

/* Swap a request of a paged cache out of, or back into, its pages: ONE call (one launch) packs n_slots requests into contiguous
 * blobs (PACK) or restores blobs into the pages the destination slots' table rows name (UNPACK), for the layers
 * [layer0, layer0 + n_layers_call).  The cache arrays are those of the fork call above.  slot_table: device (n_slots, 4) int32
 * {slot, T, r, start}; blob_offsets: device (n_slots,) int64, the byte offset in `blob` of each entry's row (layer0, kv head 0).
 *
 * Blob format, version 1.  T coded tokens, r window rows, ring start `start`; H = nh_k, n_live = ceil(T / page_size).  The rows
 * of (layer, kv head) follow each other layer-major; each row is row_bytes = 2 * n_live * page_size * M + 4 * r * d bytes (a
 * multiple of 16), so the row of (l, h) starts (l * H + h) * row_bytes behind the row of (0, 0) and a range of layers is one
 * contiguous byte range.  A row holds, in this order:
 *   K pages   n_live pages; page j is (page_size, M) uint8 row-major, the codes of tokens [j * page_size, (j + 1) * page_size);
 *             rows of tokens >= T are zero;
 *   V pages   n_live pages; page j is (M, page_size) uint8, transposed as the pool stores it; columns of tokens >= T are zero;
 *   K window  r rows of d fp16 in ring order: blob row i is ring row (start + i) % resid_cap;
 *   V window  the same.
 * The blob is a function of the live data and `start` alone: pool bytes past T, table entries at or past n_live and ring rows
 * outside [start, start + r) never reach it.
 *
 * Per entry - the table values are authoritative (dev_lengths is not read) and, like every device-resident value, not trusted:
 *   T is clamped into [0, n_pages_bound * page_size], r into [0, resid_cap], a start outside [0, resid_cap) reads as 0; row_bytes
 *     follows from the clamped values.
 *   An entry takes no part when its slot lies outside [0, bs), when its offset is negative or no multiple of 16, when its
 *     n_layers_call * H rows do not end at or before blob_bytes.
 *   PACK reads the cache and writes only the blob: exactly the entry's n_layers_call * H * row_bytes bytes.  A page whose table
 *     entry lies outside [0, n_pool) packs as zeros.
 *   UNPACK writes both whole pages (page_size * M bytes) of every page j < n_live into the id the slot's table row holds - an id
 *     outside [0, n_pool) is skipped -, window row i to ring position (start + i) % resid_cap of both windows (other ring rows
 *     are not touched), and dev_lengths[l, slot] = {T, r, start, 0} for the layers of the call.  It never writes the table.
 * No fault and no error for any of these: garbage never becomes an address.  Blob ranges of different entries, and (UNPACK) the
 * ids of different rows and the slots of different entries, must not overlap: the bytes are then whatever write came last.
 * Errors, all before any launch: null pointers (windows: only when resid_cap > 0), a bad struct_size or direction, a layer range
 * not inside [0, n_layers), n_slots < 0, blob_bytes < 0 or n_pages_bound outside [0, n_pages_cap]: MILLION_ERR_ARG; the geometry
 * the fork call refuses, or a task list (below) of 2^31 or more tasks: MILLION_ERR_SHAPE; pools, windows and blob 16-byte aligned, rows_layer_stride a multiple of 8,
 * page_ids / dev_lengths / slot_table 4-byte and blob_offsets 8-byte aligned: MILLION_ERR_ALIGN otherwise.  n_slots = 0 returns
 * MILLION_OK whatever the pointers.
 * One launch on `stream`: 16-byte vector copies, the grid a function of the bounds alone (n_pages_bound pages and resid_cap window
 * rows per (layer of the call, entry, kv head), one lengths task; one workgroup per task, at most 2^20 workgroups that then stride over the list).  The call allocates
 * nothing, synchronises nothing, uses no atomics, flags or workspace. */
enum {
    MILLION_SWAP_PACK = 0,        /* cache -> blob */
    MILLION_SWAP_UNPACK = 1       /* blob -> the pages the slots' table rows name, the windows, the lengths rows */
};

typedef struct {
    uint32_t struct_size;         /* = sizeof(million_swap_desc) */
    int32_t direction;            /* MILLION_SWAP_* */
    int32_t n_layers, bs, nh_k, d, M, page_size;
    int32_t n_pages_cap;          /* row length of page_ids */
    int32_t n_pool;               /* pages in each pool */
    int32_t resid_cap;            /* rows of the window buffers; 0: no window */
    int32_t layer0, n_layers_call;/* the layers this call serves */
    int64_t ids_layer_stride;     /* int32 between the layers of page_ids */
    int64_t rows_layer_stride;    /* fp16 elements between the layers of k_resid / v_resid */
    int64_t lengths_layer_stride; /* int32 between the layers of dev_lengths */
    int64_t blob_bytes;           /* bytes of `blob`: an entry that does not fit takes no part */
    int32_t n_slots;
    int32_t n_pages_bound;        /* host bound of the pages a request can have, <= n_pages_cap: sizes the grid, clamps T */
} million_swap_desc;

int million_cache_swap(const million_swap_desc *desc, const int32_t *page_ids, void *k_pool, void *v_pool,
                       void *k_resid, void *v_resid, int32_t *dev_lengths /* (layers, bs, 4) */,
                       const int32_t *slot_table /* (n_slots, 4) */, const int64_t *blob_offsets /* (n_slots,) */,
                       void *blob, million_stream_t stream);

/* Fork and swap over wide code pages: pools of uint16 pages (packed == 0: K (n_pool, page_size, M), V (n_pool, M, page_size)
 * uint16) or of packed pages (packed != 0: uint8 (n_pool, page_bytes), "Packed code pages" below) that hold codes of C in
 * {512, 1024, 2048, 4096} centroids; h = 2 for C <= 1024, else 4.
 *
 * million_cache_fork_wide: million_cache_fork's contract, word for word - descriptor, SHARE and COPY, the clamps of the source
 * row, prefix_tokens, ids outside [0, n_pool) dropping the copy, duplicate destinations and dst == src taking no part, the errors
 * and their order, one launch whose grid is a function of the bounds alone, no atomics, flags or workspace, capturable - over pages
 * of page_size * M * 2 bytes (uint16) or page_size * M * (8 + h) / 8 bytes (packed: both planes, copied as one byte string).  A
 * page starts at id * page_bytes in 64-bit arithmetic; a page task owns 16384 / page_bytes pages (1 .. 32) of each side.
 * C outside {512, 1024, 2048, 4096}: MILLION_ERR_SHAPE, checked behind M.
 *
 * million_cache_swap_wide: million_cache_swap's contract - entries, clamps, entries that take no part, ids outside the pool
 * packing as zeros and skipped on unpack, the window rows in ring order, the lengths rows, layer ranges, errors (C as above), one
 * launch, the bound-only grid - with blob format 2.
 *
 * Blob format, version 2: format 1 with PACKED pages in place of uint8 pages, whatever the pool's own format.  Each row is
 * row_bytes = 2 * n_live * page_size * M * (8 + h) / 8 + 4 * r * d bytes (a multiple of 16) and holds, in this order:
 *   K pages   n_live pages, each exactly a packed K page: low plane (page_size, M), then high plane (page_size, M * h / 8);
 *   V pages   n_live pages, each a packed V page: low plane (M, page_size), then high plane (M * h / 8, page_size);
 *   K window  r rows of d fp16 in ring order;   V window  the same.
 * The blob is canonical: every byte of both planes that belongs to a token >= T is zero, and every field is code & (C - 1) - at
 * C = 512 / 2048 the top bit of a field is zero, and from a uint16 pool the bits of a code at and above log2 C are dropped.  So
 * PACK writes the same bytes from a uint16 pool and from a packed pool that hold the same codes, and a request packed from one
 * restores into the other.  UNPACK writes both whole pages of every page j < n_live into the id the table row names: a packed
 * pool gets the blob's bytes; a uint16 pool gets (low byte | field << 8) & (C - 1) per code and 0 for the codes of tokens >= T. */
int million_cache_fork_wide(const million_fork_desc *desc, int32_t *page_ids, void *k_pool, void *v_pool,
                            void *k_resid, void *v_resid, int32_t *dev_lengths /* (layers, bs, 4) */,
                            const int32_t *dst_slots /* (n_dst,) */, const int32_t *tail_ids /* (n_dst, layers, nh_k) or NULL */,
                            int C, int packed, million_stream_t stream);

int million_cache_swap_wide(const million_swap_desc *desc, const int32_t *page_ids, void *k_pool, void *v_pool,
                            void *k_resid, void *v_resid, int32_t *dev_lengths /* (layers, bs, 4) */,
                            const int32_t *slot_table /* (n_slots, 4) */, const int64_t *blob_offsets /* (n_slots,) */,
                            void *blob, int C, int packed, million_stream_t stream);

/* ------------------------------------------------------------------------------------------------
 * PQ codebook training.
 * Replaces: train_pq (scripts/utils/pq_utils.py:586-609), which wraps faiss-cpu's IndexPQ.train: ProductQuantizer's default
 * training, one independent Lloyd k-means per subspace - the objective million_pq_encode minimises.  train_opq (:554-584) is
 * not covered.
 *
 * Arithmetic contract (the GPU and tests/kmeans_ref.py agree with it bit for bit):
 *   Inputs.   X (n, d) fp32 or fp16 (fp16 is widened exactly), finite.  d_m = d / M in {1, 2, 4, 8}, 2 <= C <= 4096,
 *             C <= n < 2^24; anything else: MILLION_ERR_SHAPE.
 *   Init.     init_rows: C int32 row indices; centroid c of EVERY subspace is the sub-vector of row init_rows[c] (faiss seeds
 *             all subspaces alike, so one permutation serves them all; indices outside [0, n) are clamped).  Or cents_init: a
 *             caller's (M, C, d_m) fp32 table (warm start).
 *   Assign.   Exactly million_pq_encode's rule on the fp32 table: e = x - c, sq = e * e, acc += sq sequentially in k, each one
 *             IEEE fp32 round-to-nearest operation, no contraction; strict '<' over increasing c: the lowest index wins ties.
 *   Update.   Points are cut into chunks of 4096 consecutive rows (a function of n alone, never of the grid).  Within a chunk
 *             the sum of cluster (m, c) is a sequential fp32 sum in ascending row order starting from +0.0f; the chunk sums are
 *             added sequentially in ascending chunk order.  Counts are int32.  centroid = sum / (float)count, correctly rounded.
 *             No atomic decides any bit.
 *   Empty clusters (faiss's split rule with its random donor made deterministic).  Per subspace, for each c with
 *             count[c] == 0 in ascending order: the donor is the cluster with the largest current count, lowest index on ties;
 *             centroid[c][k] = donor[k] * (1 + eps) and donor[k] *= (1 - eps) on even k, the reverse on odd k (both from the
 *             donor's value before the split; 1 + eps and 1 - eps are formed in fp32); count[c] = count[donor] / 2,
 *             count[donor] -= count[c].  eps = 1/1024 (desc->eps = 0 selects it).
 *   Iterations.  niter >= 1 rounds of assign -> update -> split; the output is the table after the last round.
 *   Outputs.  cents_out (M, C, d_m) fp32; counts_out (M, C) int32: the counts after the last round's split (optional);
 *             objective_out[i] (optional): the sum over all (row, m) of the minimum distance of round i's assignment, each fp32
 *             distance widened and added in fp64, in a fixed order (two runs give the same bits).
 * Parity with faiss is NOT pinned: faiss is on none of this project's machines, and its split draws the donor at random.
 *
 * 3 launches per round (one more for init_rows) on `stream`; no allocation, no synchronisation.  The workspace
 * (million_pq_train_workspace_bytes, 256-byte aligned) needs no initialisation.  x and x_stride_n must be aligned to one
 * sub-vector (d_m elements).  cents_init may alias cents_out. */
typedef struct {
    uint32_t struct_size;         /* = sizeof(million_train_desc) */
    int32_t n, d, M, C;           /* X is (n, d) */
    int32_t niter;
    int32_t x_is_f32;             /* 1: X is fp32, 0: fp16 */
    int64_t x_stride_n;           /* elements between rows of X; the d elements of a row are contiguous */
    float eps;                    /* split perturbation; 0 = 1/1024 (faiss's EPS) */
} million_train_desc;

/* 0 for a descriptor that is not valid. */
size_t million_pq_train_workspace_bytes(const million_train_desc *desc);
int million_pq_train(const million_train_desc *desc, const void *x,
                     const int32_t *init_rows,     /* C row indices, or NULL    } exactly one */
                     const float *cents_init,      /* (M, C, d_m) fp32, or NULL } of the two  */
                     float *cents_out,             /* (M, C, d_m) fp32 */
                     int32_t *counts_out,          /* (M, C), may be NULL */
                     double *objective_out,        /* niter doubles, may be NULL */
                     void *workspace, size_t workspace_bytes, million_stream_t stream);

/* ------------------------------------------------------------------------------------------------
 * PQ decode (reconstruction).
 * Replaces: sa_decode_4d (scripts/utils/pq_utils.py:501-540): out[row, m*d_m + k] = cents[m, codes[row, m], k].
 * codes: (n_rows, M) u8 contiguous (any leading dims flattened); cents: the RAW (M, C, d_m) fp16 codebook;
 * out: (n_rows, d) fp16 contiguous.  Exact (a gather).  Used by the reference only in fallbacks and the
 * perplexity path (pq_utils.py:198-204), so this is a plain bandwidth kernel with the codebook staged in LDS. */
int million_pq_decode(const void *codes /* uint8 for C <= 256, uint16 above */, const void *cents, void *out,
                      int64_t n_rows, int d, int M, int C, million_stream_t stream);

/* ------------------------------------------------------------------------------------------------
 * Fused decode-step attention.
 * Replaces: flash_decoding_allocated_buffer<> (Interface.template.cu:26-120), i.e. the LUT matmul
 * (:49-50), flash_decoding_split_kernel (Kernel.cuh:11-166), flash_decoding_residual_kernel
 * (Kernel.cuh:1038-1209), torch::zeros (:104) and flash_decoding_reduce_kernel (Kernel.cuh:1211-1270)
 * — one launch; and the intended 13-argument flash_decoding_paged_v (call site
 * scripts/utils/paged_pq_utils.py:621-635; spec MILLION_技术分析文档.md:1292-1345) when the codes
 * live in page pools.
 *
 * out[b,h,:] = softmax_j( q[b,h,:] . Kfull[b,hk,j,:] / sqrt(d) ) Vfull[b,hk,j,:],  hk = h / (nh/nh_k),
 * Kfull = [ dequant(k codes, T tokens) ; k_resid valid rows (r rows) ], likewise V.
 * T = 0 and r = 0 (nothing to attend to): out = 0 (the reference divides 0 by 0).
 */
enum {
    MILLION_KV_ROWMAJOR = 0,      /* codes (bs, nh_k, T_cap, M) u8: reference layout (Interface.template.cu:29-30) */
    MILLION_KV_PAGED = 1          /* K: pool (n_pool, page_size, M); V: pool (n_pool, M, page_size) — transposed  */
                                  /* pages (paged_pq_utils.py:173-175); page ids (bs, nh_k, n_pages_cap).          */
                                  /* The reference's 13-arg paged call mixes row-major K with paged V              */
                                  /* (paged_pq_utils.py:621-635): k_layout and v_layout are independent.           */
};

typedef struct {
    uint32_t struct_size;         /* = sizeof(million_attn_desc) */
    int32_t bs, nh, nh_k;         /* any nh / nh_k >= 1: up to 16 query heads per kv head are one launch on the d = 128, M in {64, 32}
                                     shapes (8 on the others); bigger groups run as several launches inside the call */
    int32_t d, M, C;
    int32_t n_tokens;             /* T: quantised tokens per (b, hk); upper bound if dev_lengths != NULL */
    int32_t r;                    /* valid residual rows, 0 <= r <= resid_cap */
    int32_t resid_start;          /* first valid residual row (ring buffer); reference: always 0 */
    int32_t resid_cap;            /* Lt: rows of the residual buffers (reference: Lt == d) */
    int64_t resid_stride_b, resid_stride_h;   /* fp16 elements; row stride is d */
    int32_t k_layout, v_layout;   /* MILLION_KV_* */
    int32_t page_size;            /* PAGED: tokens per page (32, 64 or 128) */
    int32_t n_pages_cap;          /* PAGED: row length of the page-id arrays */
    int32_t page_ids_i64;         /* PAGED: 0 = page ids are int32, 1 = int64 (reference passes int64, paged_pq_utils.py:440) */
    int32_t v_pages_dense;        /* v_layout PAGED only: 1 = the V pool passed to the call is the dense run of transposed
                                     64-token pages million_transpose_v_codes writes (page p of (b, hk) is pool page
                                     (b*nh_k + hk) * n_pages_cap + p): no V page-id array is read (v_page_ids may be NULL) */
    int64_t k_stride_b, k_stride_h;   /* ROWMAJOR: bytes between batches / kv heads of k_codes */
    int64_t v_stride_b, v_stride_h;   /* ROWMAJOR: same for v_codes */
    const int32_t *dev_lengths;   /* optional device array (bs, 4) = {n_tokens, r, resid_start, 0}: when set,
                                     lengths are read on the device (graph replay with changing lengths); every
                                     batch item has its own row, so requests of different lengths can share a
                                     launch - n_tokens above is then only the bound the grid is sized for */
    int32_t k_pool_pages;         /* PAGED: pages in the K / V pools handed to the call; 0 = not given.  Page ids are trusted, */
    int32_t v_pool_pages;         /* as in the reference (paged_pq_utils.py:440-441): only a library built with
                                     -DMILLION_DEBUG_CHECK_IDS (make debug-ids -> libmillion_hip_dbgids.so) reads these,
                                     maps ids outside [0, pool_pages) to page 0 and counts them (million_debug_bad_page_ids) */
} million_attn_desc;

size_t million_attn_workspace_bytes(const million_attn_desc *desc);
/* The workspace must be zeroed once after allocation (million_workspace_init or any memset); every call
 * leaves it ready for the next one.  Calls of DIFFERENT shapes may share a workspace (sized for the largest) as long as
 * bs * nh_k <= 2048; a shape with more (b, kv head) pairs needs a workspace of its own. */
int million_workspace_init(void *workspace, size_t bytes, million_stream_t stream);

/* What the two decode entry points read into a product (tests/test_decode_poison_gpu.py checks it bit for bit, every kernel):
 * code bytes past n_tokens - or past the device length - in the last live page or in a row-major tensor, the pages between the
 * device length and the host bound, pool pages no live entry names, and window rows outside the ring's valid span (the row a
 * fused append writes included) may hold anything, NaN and, at C = 128, bytes >= 128 included: they never reach a product and
 * the output is bitwise the same.  Page-table entries past the live pages (up to n_pages_cap) must still be ids inside the
 * pools: the streaming and lean kernels load the whole row of ids up front, and only in-pool ids are tested.  out needs no
 * initialisation. */
int million_pq_decode_attn(const million_attn_desc *desc,
                           const void *q,              /* (bs, nh, 1, d) fp16 contiguous */
                           const void *k_codes,        /* ROWMAJOR tensor or K page pool */
                           const void *v_codes,        /* ROWMAJOR tensor or V page pool */
                           const void *k_page_ids,     /* k_layout PAGED only: int32 or int64, see page_ids_i64 */
                           const void *v_page_ids,     /* v_layout PAGED only (may alias k_page_ids) */
                           const void *k_cents_prepared, const void *v_cents_prepared,
                           const void *k_resid, const void *v_resid,   /* (bs, nh_k, resid_cap, d) fp16 */
                           void *out,                  /* (bs, nh, 1, d) fp16 */
                           void *workspace, size_t workspace_bytes,
                           million_stream_t stream);

/* Same, fused with the residual-window append of the new token (replaces the two slice-assign copies of
 * DynamicPQCache.decoding, scripts/utils/pq_utils.py:304-312, AND the attention launch that follows them,
 * :314-326): k_new / v_new (bs, nh_k, 1, d) fp16 are attended to as one more window row and stored into
 * row (resid_start + r) % resid_cap of k_resid / v_resid, where r = desc->r is the number of valid rows
 * BEFORE the call (r < resid_cap).  With dev_lengths the row count is read on the device and incremented
 * there once every workgroup has read it.  The contract of million_pq_decode_attn above holds; the row being written may hold
 * anything before the call, and no other window byte is written. */
int million_pq_decode_attn_append(const million_attn_desc *desc, const void *q, const void *k_new, const void *v_new,
                                  const void *k_codes, const void *v_codes, const void *k_page_ids,
                                  const void *v_page_ids, const void *k_cents_prepared,
                                  const void *v_cents_prepared, void *k_resid, void *v_resid, void *out,
                                  void *workspace, size_t workspace_bytes, million_stream_t stream);

/* Log-sum-exp.  The _lse entries below return, beside `out`, the other half of each row's softmax state:
 *   lse = ln sum_j exp(s_j),  s_j = q . k_j / sqrt(d),
 * over exactly the keys the row's `out` is a softmax over: the codes below T, the live window rows, the appended row, the
 * visible rows of the chunk.  Natural log, fp32.  Nothing to attend to: -inf (`out` is 0 there, as ever).  Where a split merge
 * gave up and wrote NaN to `out` (million_debug_tail_faults), lse is NaN too.  lse is indexed like `out` without the d axis:
 * decode (bs, nh), chunk (bs, nh, n_q) contiguous; the rows of a ragged chunk call past the request's dev_n_q get -inf
 * (their `out` is zeros).  The kernels hold the maximum m in the scaled exp2 domain and the denominator l relative to it:
 * lse = (m + log2 l) ln 2, l = 0 -> -inf, stored wherever `out` is stored by the lane or thread that already holds the two;
 * `out` is bitwise what the entry without lse writes.  Two results over DISJOINT key sets combine with million_attn_merge.
 *
 * million_pq_decode_attn_lse: the arguments of million_pq_decode_attn_append plus float *lse (bs, nh) after out.
 * k_new = v_new = NULL: no append (million_pq_decode_attn).  lse = NULL: MILLION_ERR_ARG. */
int million_pq_decode_attn_lse(const million_attn_desc *desc, const void *q, const void *k_new, const void *v_new,
                               const void *k_codes, const void *v_codes, const void *k_page_ids,
                               const void *v_page_ids, const void *k_cents_prepared,
                               const void *v_cents_prepared, void *k_resid, void *v_resid, void *out, float *lse,
                               void *workspace, size_t workspace_bytes, million_stream_t stream);

/* Row-major V codes (bs, nh_k, T, M) u8 (the reference's 10-argument layout, Interface.template.cu:30) -> the dense run
 * of transposed 64-token pages ((bs*nh_k) * ceil(T/64), M, 64) that the fast kernels read with v_pages_dense = 1,
 * page_size = 64, n_pages_cap = ceil(T/64).  Replaces the per-call pad + view + transpose + contiguous of
 * PagedPQCache._call_paged_kernel (scripts/utils/paged_pq_utils.py:464-500).  A caller that passes the same V code
 * tensor on many decode steps (the reference does, between two flushes) transposes once and reuses the pages;
 * million_pq_decode_attn with v_layout = ROWMAJOR does the same transpose into its workspace on EVERY call. */
int million_transpose_v_codes(const void *v_codes, void *v_pages, int bs, int nh_k, int n_tokens, int M,
                              int64_t v_stride_b, int64_t v_stride_h, million_stream_t stream);

/* Which kernel million_pq_decode_attn would pick for a descriptor: 1 = streaming MFMA kernels (d = 128 with M in {64, 32}, and
 * d = 128 / M = 16 with up to 16 query heads per kv head; any batch and any context up to 1M tokens per (b, kv head):
 * calls with more than 64 rounds per wave get more splits; with 256 or 128 centroids, up to 4 query heads per kv head and pages of 64 / 128
 * tokens the "lean" form of it runs - csrc/attn_lean.h - which also takes d = 64 with M in {64, 32, 16} at up to 16
 * query heads per kv head: 5 and more run as ceil(G / 4) virtual kv heads of 3 / 4 query heads, while bs * nh_k * parts <= 2048),
 * 2 = the same after transposing row-major V codes into workspace scratch (one extra launch), 3 = tile MFMA kernel
 * (d = 64 on 32-token pages; d = 64 or d = 128 / M = 16 with more than 2048 virtual (b, kv head) pairs; on the streaming
 * kernel's shapes: no quantised token yet, or more than 1M tokens per (b, kv head)), 4 = the same after the transpose,
 * 0 = scalar fallback (anything else the descriptor allows: C not 128 / 256, paged K with row-major V, ...), -1 = bad descriptor.
 * (5, the grouped MFMA kernel, is retired and not reused.)  Row-major K and V with n_tokens = 0 need no transpose launch: 3 then.
 * The answer is the plan million_pq_decode_attn launches for its first query-head group, under the current
 * million_set_force_generic policy. */
int million_attn_kernel_kind(const million_attn_desc *desc);
/* Kernel choice for A/B measurements and tests: 0 = auto (default), 1 = generic kernel only, 4 = auto, but the helper workgroups of the split merge give up at once (exercises the
 * last arriver's take-over path of the MFMA kernels' tail: every give-up bit is set before the launch's first ticket),
 * 8 = auto, but the helpers have no patience: each gives up through the real path (its atomic on the ticket word) unless
 * every workgroup has already taken its ticket, 16 = auto, but the shapes of the lean kernel (csrc/attn_lean.h) stay on the
 * streaming / tile kernels and no call runs as virtual kv heads (A/B and the tests of those kernels' forms), 64 = auto, but million_prefill_attn runs its plain
 * tile loop at d = 128 instead of the pipelined one (csrc/prefill.hip; A/B and the tests of both forms).  Any other value means auto. */
void million_set_force_generic(int on);

/* The decode step over 16-bit codes (nbits 9 .. 12; the reference stores them as one uint16 each, pq_utils.py:542-552, and has
 * no fused kernel for them: its only route is sa_decode_4d + scaled_dot_product_attention).  One launch (csrc/attn_wide.hip) with
 * the job, the `out`, lse, fused-append and device-length semantics of million_pq_decode_attn_lse above, word for word: nothing
 * to attend to gives zeros and -inf, `out` with lse is bitwise `out` without, the window row an append writes may hold anything.
 *   desc       million_attn_desc as above; C in {512, 1024, 2048, 4096}; d in {128, 64}; d / M in {2, 4}; nh / nh_k <= 16
 *              (one launch; no several-launch form); k_layout = v_layout = MILLION_KV_PAGED, v_pages_dense = 0; resid_cap as
 *              above.  Anything else: MILLION_ERR_SHAPE before any launch.
 *   k_codes    K pool (n_pool, page_size, M) uint16;  v_codes: V pool (n_pool, M, page_size) uint16 (transposed pages).
 *   k_cents    the PLAIN (M, C, d_m) fp16 codebooks, read from global memory (a table is 128 KiB .. 1 MiB: none fits in LDS).
 *   v_cents    Aligned to one entry: 4 bytes at d_m = 2, 8 bytes at d_m = 4.  million_prepare_cents keeps refusing C > 256.
 *   lse        (bs, nh) fp32 or NULL.  k_new = v_new = NULL: no append.
 * Every index the kernel gathers with is code & (C - 1): codes past n_tokens (or the device length) in the last page, pages no
 * live entry names and poisoned memory may hold any 16 bits and change no bit of the output.  Page ids are trusted.
 * The workspace has the layout of million_attn_workspace_bytes' (zeroed once, left at rest by every call; calls of the uint8
 * entries may share it when it is large enough for both).  million_attn_wide_splits: the code splits per (b, kv head) the call
 * would launch (its grid is splits + 1 workgroups per pair), -1 for a descriptor the entry refuses.
 * million_attn_kernel_kind does not know this kernel: it answers for the uint8 entries only. */
size_t million_attn_wide_workspace_bytes(const million_attn_desc *desc);      /* 0 for a descriptor the entry refuses */
int million_attn_wide_splits(const million_attn_desc *desc);
int million_pq_decode_attn_wide(const million_attn_desc *desc, const void *q,
                                const void *k_new, const void *v_new,         /* both NULL: no append */
                                const void *k_codes, const void *v_codes, const void *k_page_ids, const void *v_page_ids,
                                const void *k_cents, const void *v_cents,
                                void *k_resid, void *v_resid, void *out, float *lse /* may be NULL */,
                                void *workspace, size_t workspace_bytes, million_stream_t stream);

/* ------------------------------------------------------------------------------------------------
 * Packed code pages: codes of 512 .. 4096 centroids in 10 or 12 bits instead of a uint16 each.
 *
 * The format.  A code is split into its low byte and h high bits: h = 2 for C in {512, 1024}, h = 4 for C in {2048, 4096} - a
 * function of C alone (no descriptor carries it).  A page of page_size tokens and M subspaces is
 *     page_bytes = page_size * M * (8 + h) / 8
 * bytes: its low plane first, its high plane behind it.  A pool is a contiguous uint8 array (n_pool, page_bytes); one page id
 * names both planes, and page pid starts at byte pid * page_bytes (no power of two: 64-bit arithmetic).
 *   K page  low plane  (page_size, M) uint8: exactly a uint8 K page - byte (t, m) is the low byte of token t's code for subspace m;
 *           high plane (page_size, M * h / 8) uint8: byte j of token t's row holds the subspaces j * 8/h .. j * 8/h + 8/h - 1;
 *           bits [8, 8 + h) of subspace m's code sit at bit h * (m mod 8/h) of byte m / (8/h).
 *   V page  low plane  (M, page_size) uint8: the transposed uint8 page - byte (m, t);
 *           high plane (M * h / 8, page_size) uint8: byte (j, t) holds token t's fields for the subspaces j * 8/h .., in the
 *           same bit order.
 * Every high byte belongs to ONE token on both sides: a store of the tokens [t0, t0 + n) never reads, modifies or zeroes a byte
 * of another token, and the bytes of tokens past the live ones may hold anything.  At C = 512 / 2048 the top bit of a field is
 * not part of a code: the encoder writes it as 0, the readers mask it (code & (C - 1)).
 * page_size in {32, 64, 128} and M in {16, 32, 64} keep every plane a multiple of 16 bytes.  Packed pages are read by decode
 * attention (million_pq_decode_attn_packed), chunk attention (million_pq_chunk_attn_packed) and the row gather
 * (million_pq_gather_rows_packed).  True 9- / 11-bit packing, packed row-major codes and million_pq_decode over packed pages do
 * not exist: million_pq_repack_pages is the way from packed pages to uint16 pages and back.
 *
 * million_pq_encode_packed: million_pq_encode's contract - descriptor, codes bit for bit (the same scan), ring source,
 * dev_lengths, page-table clamps - with dst_layout MILLION_CODES_KPAGES / MILLION_CODES_VPAGES meaning packed pages of the pool
 * dst.  MILLION_CODES_ROWMAJOR, C outside {512, 1024, 2048, 4096}, M no multiple of 4, page_size not 32 / 64 / 128:
 * MILLION_ERR_SHAPE.  dst 16-byte aligned.
 *
 * million_pq_decode_attn_packed: the arguments and every semantic of million_pq_decode_attn_wide - out, lse, fused append,
 * device lengths, code & (C - 1) on every gathered index, the workspace - with k_codes / v_codes the packed pools.  The same
 * launch shape: million_attn_wide_splits and million_attn_wide_workspace_bytes answer for it too.  `out` and lse are bitwise
 * those of million_pq_decode_attn_wide over uint16 pools that hold the same codes.
 *
 * million_pq_repack_pages: n_pages whole pages, page for page, in one launch.  MILLION_REPACK_PACK: src uint16 pages ->
 * dst packed pages (bits of a code above 8 + h are dropped); MILLION_REPACK_UNPACK: src packed pages -> dst uint16 pages.
 * side 0: K pages ((page_size, M) uint16), side 1: V pages ((M, page_size) uint16).  Shapes as above (MILLION_ERR_SHAPE), a
 * bad direction / side or n_pages < 0: MILLION_ERR_ARG; src and dst 16-byte aligned; n_pages = 0: MILLION_OK.  src and dst
 * must not overlap.
 *
 * million_pq_chunk_attn_packed (declared behind million_pq_chunk_attn_wide below): the arguments and every semantic of
 * million_pq_chunk_attn_wide - out, lse (may be NULL), the ragged dev_lengths / dev_n_q, code & (C - 1) on every gathered index
 * - with k_codes / v_codes the packed pools.  The same split count and workspace: million_chunk_attn_wide_workspace_bytes
 * answers for it too.  Both layouts must be MILLION_KV_PAGED (a row-major side: MILLION_ERR_SHAPE before any launch - there is
 * no packed row-major format); page_size 32 / 64 / 128; pools 16-byte aligned.  `out` and lse are bitwise those of
 * million_pq_chunk_attn_wide over uint16 pools that hold the same codes: same tile order, same split cut, same merge.  Bytes of
 * tokens past n_tokens (or the device length), of page tails and of pages no live entry names may hold anything.
 *
 * million_pq_gather_rows_packed (declared behind million_pq_gather_rows below): million_pq_gather_rows' job with the same
 * descriptor - code_bytes = 2, the logical width of a code; both layouts MILLION_KV_PAGED; d / M 2 or 4; anything else is
 * MILLION_ERR_SHAPE before any launch - over the packed K and V pools.  The index rule c < C ? c : 0 is applied to the raw
 * (8 + h)-bit field, so the rows are bit for bit those of million_pq_gather_rows over the MILLION_REPACK_UNPACK image of the same
 * pools.  Only bytes of the tokens t0 <= t < t1 are read. */
enum {
    MILLION_REPACK_PACK = 0,      /* uint16 pages -> packed pages */
    MILLION_REPACK_UNPACK = 1     /* packed pages -> uint16 pages */
};
int million_pq_encode_packed(const million_encode_desc *desc, const void *x, const void *cents /* (M,C,d_m) fp16 */,
                             void *dst, const int32_t *page_ids, million_stream_t stream);
int million_pq_decode_attn_packed(const million_attn_desc *desc, const void *q,
                                  const void *k_new, const void *v_new,       /* both NULL: no append */
                                  const void *k_codes, const void *v_codes, const void *k_page_ids, const void *v_page_ids,
                                  const void *k_cents, const void *v_cents,
                                  void *k_resid, void *v_resid, void *out, float *lse /* may be NULL */,
                                  void *workspace, size_t workspace_bytes, million_stream_t stream);
int million_pq_repack_pages(int direction, const void *src, void *dst, int64_t n_pages, int page_size, int M, int C, int side,
                            million_stream_t stream);

/* ------------------------------------------------------------------------------------------------
 * Prompt (prefill) attention on fp16 K/V.
 * Replaces: scaled_dot_product_attention(q, repeat_kv(k), repeat_kv(v), is_causal=True) of the reference's prompt pass
 * (scripts/utils/pq_utils.py:249-260 DynamicPQCache.prefill, scripts/utils/paged_pq_utils.py:216-320
 * PagedPQCache.prefill; baseline: scripts/modeldb/models/modeling_llama.py:403-443) - GQA without materialising
 * repeat_kv: the nh / nh_k query heads of a kv head share the K/V tiles of one workgroup.
 *   out[b,h,i,:] = softmax_{j <= q_pos0 + i (causal), j < n_kv}( q[b,h,i,:] . k[b,hk,j,:] / sqrt(d) ) v[b,hk,j,:],  hk = h / (nh/nh_k)
 * fp16 in / out, fp32 scores, online softmax and accumulation; d = 128 or 64.  causal = 0: every key (j < n_kv).
 * torch's is_causal=True with q_len == kv_len is q_pos0 = 0; a prompt chunk behind n_past cached fp16 rows is q_pos0 = n_past.
 * Ragged batches (dev_spans, optional; NULL: the host values hold for every request, the launch is the same as without the
 * field - same kernel instance, same grid, same bits):
 *   dev_spans: device (bs, 4) int32 rows {n_q, n_kv, q_pos0, reserved}.  Request b has n_q_b = row[0] query rows and
 *     n_kv_b = row[1] key / value rows, and its query row 0 sits at key position q_pos0_b = row[2], read by the kernel when it
 *     runs (a captured launch follows the array).  desc->n_q and desc->n_kv are then only the BOUNDS the grid and every pointer
 *     range are sized for (padded layout: request b's rows start at b * stride_b, whatever its length); desc->q_pos0 is not
 *     read but still validated (>= 0), and a bound n_kv = 0 with n_q > 0 is still MILLION_ERR_ARG.  The values are not trusted:
 *     n_q_b is clamped into [0, n_q], n_kv_b into [0, n_kv], q_pos0_b into [0, n_kv].  Word 3 is neither read nor written; the
 *     array is never written.  Each request uses the formula above with its own three values (causal: j <= q_pos0_b + i and
 *     j < n_kv_b; otherwise j < n_kv_b).
 *   Rows i >= n_q_b of out[b] (below the bound n_q) are written as zeros; a request with n_kv_b = 0 gets zeros in every row,
 *     with no error; n_q_b = 0: the request takes no part.  Rows at or past the bound are never written.
 *   What may hold anything (NaN, garbage) without reaching a product or the output: q rows at or past n_q_b, K and V rows at
 *   or past n_kv_b, out.
 *   Bit for bit: the live rows of request b equal the call without dev_spans on that request alone (bs = 1) with the host
 *   values (n_q_b, n_kv_b, q_pos0_b); with every row equal to the host values the call equals the call without dev_spans.
 *   Nothing allocates or synchronises and there is no workspace: the call may be captured into a graph. */
typedef struct {
    uint32_t struct_size;         /* = sizeof(million_prefill_desc) */
    int32_t bs, nh, nh_k, d;
    int32_t n_q, n_kv;            /* query rows, key/value rows */
    int32_t q_pos0;               /* position of query row 0 among the keys */
    int32_t causal;
    int64_t q_stride_b, q_stride_h, q_stride_n;   /* fp16 elements; the d elements of a row are contiguous; multiples of 8 */
    int64_t k_stride_b, k_stride_h, k_stride_n;
    int64_t v_stride_b, v_stride_h, v_stride_n;
    int64_t o_stride_b, o_stride_h, o_stride_n;
    const int32_t *dev_spans;     /* NULL, or device (bs, 4) int32 rows {n_q, n_kv, q_pos0, reserved}: n_q / n_kv above are the bounds */
} million_prefill_desc;

int million_prefill_attn(const million_prefill_desc *desc, const void *q /* (bs, nh, n_q, d) */,
                         const void *k /* (bs, nh_k, n_kv, d) */, const void *v, void *out /* (bs, nh, n_q, d) */,
                         million_stream_t stream);
/* The same with the log-sum-exp of every query row ("Log-sum-exp" above): float *lse (bs, nh, n_q) contiguous, after out:
 *   lse[b,h,i] = ln sum_j exp( q[b,h,i,:] . k[b,hk,j,:] / sqrt(d) )  over exactly the keys j of the row's softmax above.
 * -inf (with out = 0) where a row has no key: under dev_spans a request with n_kv_b = 0 and the rows i >= n_q_b below the bound
 * n_q (rows at or past the bound are not written).  lse is required here (NULL: MILLION_ERR_ARG; 4-byte aligned); every other
 * check, the grid and the ragged contract are million_prefill_attn's.  Separate kernel instances: out is bitwise the out of
 * million_prefill_attn on the same arguments, in both forms (pipelined and plain) and with or without dev_spans.  The value
 * comes from the softmax state the output was divided by - in the pipelined kernel the lazy reference in force at the end, not
 * the row maximum.  A prompt pass over K/V held in blocks is then one call per block (non-causal over a past block, causal
 * with q_pos0 counted from the block's first key over the last) and one million_attn_merge of the (out, lse) pairs. */
int million_prefill_attn_lse(const million_prefill_desc *desc, const void *q, const void *k, const void *v, void *out,
                             float *lse /* (bs, nh, n_q) */, million_stream_t stream);

/* ------------------------------------------------------------------------------------------------
 * Chunk attention: a block of n_q new query tokens against the PQ-coded cache (chunked prefill, a second turn on an existing
 * conversation, verification of draft tokens).  The decode entry points take one query token; million_prefill_attn takes fp16
 * K/V only.  For query row i of head h (kv head hk = h / (nh/nh_k)):
 *   out[b,h,i,:] = softmax_j( q[b,h,i,:] . Kall[b,hk,j,:] / sqrt(d) ) Vall[b,hk,j,:]
 *   Kall = [ dequant(K codes, n_tokens) ; window rows (r rows of the ring from resid_start) ; chunk rows 0 .. n_c - 1 ], likewise V.
 * Every row sees all n_tokens + r past keys; chunk key j is visible to row i iff j <= i (causal, the chunk's first row sits at
 * position n_tokens + r).  n_c = n_q: chunked prefill (the caller then stores the chunk's K/V itself); n_c = 0: every row sees
 * the past only (several query tokens of one position set: speculative verification).  Nothing to attend to: out = 0.
 * Dequantisation is the gather of million_pq_decode (bit for bit); fp32 scores, softmax and accumulation; fp16 in and out.
 * Shapes: d = 128 with M in {64, 32, 16}, d = 64 with M in {64, 32, 16}; uint8 codes, any C <= 256; any nh / nh_k >= 1, n_q >= 1;
 * each code side row-major (bs, nh_k, T_cap, M) or paged (K pool (n_pool, page_size, M), V pool (n_pool, M, page_size)
 * transposed) with page_size 32 / 64 / 128 and int32 or int64 ids.  Anything else: MILLION_ERR_SHAPE (no fallback).
 * Code bytes past n_tokens, unused pool pages and window rows outside the ring's valid span are never read into a product.
 * The window and the chunk are read, never written.
 * Ragged batches (both fields optional; both NULL: the host values above hold for every request, the launch is the same as
 * without the fields):
 *   dev_lengths: device (bs, 4) int32 rows {n_tokens, r, resid_start, ticket}, the rows of million_pq_decode_attn.  Request b
 *     attends to T_b = row[0] codes and r_b = row[1] window rows from row[2], read by the kernel when it runs (a captured
 *     launch follows the lengths).  desc->n_tokens is then only the BOUND the grid, the split count and the workspace are sized
 *     for (the capacity check n_pages_cap * page_size >= n_tokens is made against it), desc->r and desc->resid_start are
 *     ignored, the window pointers are required whenever resid_cap > 0 and codes, codebooks and ids whenever the bound is > 0.
 *     The values are not trusted: T_b is clamped into [0, n_tokens], r_b into [0, resid_cap], a start outside [0, resid_cap)
 *     reads as 0.  Word 3 is neither read nor written.  Every request's visible tiles are cut into the call's S ranges (a
 *     range may be empty); page ids are read for tokens < T_b only.
 *   dev_n_q: device (bs,) int32, the valid query rows of each request, clamped into [0, n_q]; with n_c = n_q the chunk of
 *     request b has n_q[b] rows.  Rows i >= n_q[b] of out are written as zeros; n_q[b] = 0: the request takes no part.
 *   What may hold anything (NaN, 0xFF, stale ids) without reaching a product or the output: code bytes at or past T_b (pages
 *   between a request's live pages and the bound included), unused pool pages, page-table entries past a request's live
 *   pages, window rows outside each request's ring span, q rows and chunk K/V rows at or past n_q[b], the workspace, out.
 *   Nothing allocates or synchronises: the call may be captured into a graph. */
typedef struct {
    uint32_t struct_size;         /* = sizeof(million_chunk_attn_desc) */
    int32_t bs, nh, nh_k, d, M, C;
    int32_t n_q;                  /* query rows */
    int32_t n_c;                  /* chunk K/V rows: 0 or n_q */
    int32_t n_tokens;             /* T: quantised tokens per (b, hk) */
    int32_t r;                    /* valid window rows, 0 <= r <= resid_cap */
    int32_t resid_start;          /* first valid window row (ring buffer) */
    int32_t resid_cap;            /* rows of the window buffers */
    int64_t resid_stride_b, resid_stride_h;   /* fp16 elements; row stride is d */
    int32_t k_layout, v_layout;   /* MILLION_KV_* */
    int32_t page_size;            /* PAGED: 32, 64 or 128 */
    int32_t n_pages_cap;          /* PAGED: row length of the page-id arrays (bs, nh_k, n_pages_cap) */
    int32_t page_ids_i64;         /* PAGED: 0 = int32 ids, 1 = int64 */
    int64_t k_stride_b, k_stride_h;   /* ROWMAJOR: bytes between batches / kv heads of k_codes (rows are M bytes) */
    int64_t v_stride_b, v_stride_h;   /* ROWMAJOR: same for v_codes */
    int64_t q_stride_b, q_stride_h, q_stride_n;     /* fp16 elements; the d elements of a row are contiguous; multiples of 8 */
    int64_t kc_stride_b, kc_stride_h, kc_stride_n;  /* k_chunk (bs, nh_k, n_c, d) */
    int64_t vc_stride_b, vc_stride_h, vc_stride_n;  /* v_chunk */
    int64_t o_stride_b, o_stride_h, o_stride_n;     /* out (bs, nh, n_q, d) */
    const int32_t *dev_lengths;   /* NULL, or device (bs, 4) {n_tokens, r, resid_start, ticket}: n_tokens above is the bound */
    const int32_t *dev_n_q;       /* NULL, or device (bs,) valid query rows per request */
} million_chunk_attn_desc;

/* Workspace of a call: 0 when the context is not split (the kernel then writes out directly), else
 * bs * nh_k * S * n_q * (nh/nh_k) * (d + 2) * 4 bytes, S = the split count of the past:
 * min(ceil(256 / (bs * nh_k * ceil(n_q * (nh/nh_k) / 256))), ceil(n_tokens / 64), 64), at least 1.
 * A pure function of the descriptor's host fields (with dev_lengths: of the bound n_tokens; the two device arrays are not read).
 * No initialisation is needed; the workspace holds nothing between calls.  0 for a descriptor that is not valid. */
size_t million_chunk_attn_workspace_bytes(const million_chunk_attn_desc *desc);
int million_pq_chunk_attn(const million_chunk_attn_desc *desc,
                          const void *q,                /* (bs, nh, n_q, d) fp16, strided */
                          const void *k_chunk, const void *v_chunk,   /* (bs, nh_k, n_c, d) fp16, strided; NULL when n_c = 0 */
                          const void *k_codes, const void *v_codes,   /* ROWMAJOR tensors or page pools */
                          const void *k_page_ids, const void *v_page_ids,   /* PAGED sides (may alias) */
                          const void *k_cents_prepared, const void *v_cents_prepared,   /* million_prepare_cents */
                          const void *k_resid, const void *v_resid,   /* (bs, nh_k, resid_cap, d) fp16 */
                          void *out,                    /* (bs, nh, n_q, d) fp16, strided */
                          void *workspace, size_t workspace_bytes,
                          million_stream_t stream);
/* The same with the log-sum-exp of every query row ("Log-sum-exp" above): float *lse (bs, nh, n_q) contiguous, after out. */
int million_pq_chunk_attn_lse(const million_chunk_attn_desc *desc, const void *q, const void *k_chunk, const void *v_chunk,
                              const void *k_codes, const void *v_codes, const void *k_page_ids, const void *v_page_ids,
                              const void *k_cents_prepared, const void *v_cents_prepared, const void *k_resid,
                              const void *v_resid, void *out, float *lse, void *workspace, size_t workspace_bytes,
                              million_stream_t stream);

/* Chunk attention over 16-bit PQ codes (nbits 9 .. 12): million_pq_chunk_attn's job, word for word - the same descriptor, the
 * same Kall, masks, ragged fields (dev_lengths / dev_n_q), split rule, workspace formula and merge - with another code producer.
 *   Codes:     uint16.  Each side row-major (bs, nh_k, T_cap, M) or a page pool (K (n_pool, page_size, M), V (n_pool, M,
 *              page_size) transposed; pages of 32 / 64 / 128 tokens; int32 or int64 ids); the sides may differ.  Row-major
 *              k_stride_* / v_stride_* stay in BYTES; rows are 2 M bytes.
 *   Codebooks: k_cents / v_cents are the plain (M, C, d_m) fp16 tensors in global memory (there is no prepared image and no
 *              codebook in LDS); every entry is one aligned load of 2 d_m bytes, and the dequantised tile is the gather of
 *              million_pq_decode, bit for bit.
 *   Shapes:    C in {512, 1024, 2048, 4096}, d in {128, 64}, d_m = d / M in {2, 4}.  Anything else - C <= 256 (that is
 *              million_pq_chunk_attn's), another C, d_m 1 or 8, another d - is MILLION_ERR_SHAPE before any launch.
 *   Mask:      EVERY gathered index is code & (C - 1); this is part of the contract.  Code words at or past T_b, row-major
 *              padding, page tails, pool pages that no live table entry names and page-table entries past a request's live
 *              pages may hold any bits (with everything the uint8 entry lists: window rows outside the ring span, q and chunk
 *              rows at or past n_q[b], the workspace, out): none of them changes a bit of out or lse, and none sends a load
 *              outside a table.  Page ids of live pages are trusted.
 *   Pointer, alignment, capacity and workspace checks (MILLION_ERR_ARG / _ALIGN / _WORKSPACE) are the uint8 entry's.  lse may
 *   be NULL; out with lse is bitwise out without it.  S and the workspace are million_chunk_attn_workspace_bytes' function of
 *   the descriptor (C is not read by it): with codes < 256 and a table whose first 256 entries per subspace are a C = 256
 *   table, out and lse are bitwise those of million_pq_chunk_attn.  0 from the workspace function: the descriptor is refused. */
size_t million_chunk_attn_wide_workspace_bytes(const million_chunk_attn_desc *desc);
int million_pq_chunk_attn_wide(const million_chunk_attn_desc *desc, const void *q, const void *k_chunk, const void *v_chunk,
                               const void *k_codes, const void *v_codes, const void *k_page_ids, const void *v_page_ids,
                               const void *k_cents, const void *v_cents, const void *k_resid, const void *v_resid,
                               void *out, float *lse /* may be NULL */, void *workspace, size_t workspace_bytes,
                               million_stream_t stream);
/* The same over pools of packed pages ("Packed code pages" above): k_codes / v_codes uint8 (n_pool, page_bytes), both PAGED */
int million_pq_chunk_attn_packed(const million_chunk_attn_desc *desc, const void *q, const void *k_chunk, const void *v_chunk,
                                 const void *k_codes, const void *v_codes, const void *k_page_ids, const void *v_page_ids,
                                 const void *k_cents, const void *v_cents, const void *k_resid, const void *v_resid,
                                 void *out, float *lse /* may be NULL */, void *workspace, size_t workspace_bytes,
                                 million_stream_t stream);

/* ------------------------------------------------------------------------------------------------
 * Gather of rows: a token range of every request dequantised straight from its code store, then its window rows in ring order,
 * as fp16 rows in a caller's buffer - the K/V block a million_prefill_attn_lse call attends to, in memory that does not grow with
 * the context.  For every (b, kv head), for K and for V (one launch does both):
 *   out[b,hk,j,:]              = dequant(codes[b,hk,t0 + j])                         0 <= j < t1 - t0
 *   out[b,hk,(t1 - t0) + i,:]  = resid[b,hk,(resid_start + i) % resid_cap,:]         0 <= i < r
 * Either part may be empty (t1 = t0, r = 0); nothing to write: MILLION_OK without a launch.  Rows of out at or past
 * (t1 - t0) + r are not written.
 * Codes: code_bytes = 1: uint8, any C in 1 .. 256; code_bytes = 2: uint16, C in {512, 1024, 2048, 4096}; a C the code type
 *   cannot hold is MILLION_ERR_SHAPE.  Each side row-major (bs, nh_k, T_cap, M) (k_stride_* / v_stride_* in BYTES, rows of
 *   M * code_bytes bytes) or a page pool (K (n_pool, page_size, M), V (n_pool, M, page_size) transposed; pages of 32 / 64 / 128
 *   tokens) behind int32 page ids (bs, nh_k, n_pages_cap).  d in {128, 64}, d / M in {1, 2, 4, 8}.
 * Codebooks: the plain (M, C, d_m) fp16 tensors (no prepared image).  The dequantised rows are the gather of million_pq_decode,
 *   bit for bit, for EVERY code word: an index is c < C ? c : 0.
 * What is read: code words of tokens t0 <= t < t1, page-table entries of those tokens' pages, window rows of the ring's valid
 *   span.  Code bytes at or past t1, page tails, unused pool pages, page-table entries past ceil(t1 / page_size) and window rows
 *   outside the span may hold anything.  Page ids of the pages read are trusted.
 * Lengths are host values (t0, t1, r, resid_start); there is no device-length form.
 * Validation precedes any HIP call: struct size, d, M, C against code_bytes, the lengths (0 <= t0 <= t1, 0 <= r <= resid_cap,
 *   resid_start inside the ring, (t1 - t0) + r <= rows_cap), layouts, page_size, the table (bs * nh_k * n_pages_cap and
 *   n_pages_cap * page_size within 31 bits - the limits of the attention entries - and n_pages_cap * page_size >= t1:
 *   MILLION_ERR_ARG), null pointers for whatever part is not empty, 16-byte alignment of out, window and codebook pointers and
 *   strides that are multiples of 8 elements (MILLION_ERR_ALIGN).  Every byte offset on the device is 64-bit.
 * One plain launch, no workspace, no atomics: legal inside stream capture. */
typedef struct {
    uint32_t struct_size;         /* = sizeof(million_gather_rows_desc) */
    int32_t bs, nh_k, d, M, C;
    int32_t code_bytes;           /* 1: uint8 codes, 2: uint16 codes */
    int32_t t0, t1;               /* tokens [t0, t1) of every request */
    int32_t r;                    /* valid window rows, 0 <= r <= resid_cap */
    int32_t resid_start;          /* first valid window row (ring buffer) */
    int32_t resid_cap;            /* rows of the window buffers (0: no window) */
    int64_t resid_stride_b, resid_stride_h;   /* fp16 elements; row stride is d */
    int32_t k_layout, v_layout;   /* MILLION_KV_* */
    int32_t page_size;            /* PAGED: 32, 64 or 128 */
    int32_t n_pages_cap;          /* PAGED: row length of the page-id arrays */
    int64_t k_stride_b, k_stride_h;   /* ROWMAJOR: bytes between batches / kv heads of k_codes */
    int64_t v_stride_b, v_stride_h;
    int32_t rows_cap;             /* rows of the out buffers */
    int32_t reserved;             /* 0 */
    int64_t o_stride_b, o_stride_h;   /* out (bs, nh_k, rows_cap, d): fp16 elements; row stride is d */
} million_gather_rows_desc;

int million_pq_gather_rows(const million_gather_rows_desc *desc,
                           const void *k_codes, const void *v_codes,           /* ROWMAJOR tensors or page pools */
                           const int32_t *k_page_ids, const int32_t *v_page_ids, /* PAGED sides (may alias) */
                           const void *k_cents, const void *v_cents,           /* (M, C, d_m) fp16 */
                           const void *k_resid, const void *v_resid,           /* (bs, nh_k, resid_cap, d) fp16; NULL when r = 0 */
                           void *k_out, void *v_out,                           /* (bs, nh_k, rows_cap, d) fp16 */
                           million_stream_t stream);
/* The same over pools of packed pages ("Packed code pages" above): code_bytes = 2, both layouts PAGED, d / M 2 or 4 */
int million_pq_gather_rows_packed(const million_gather_rows_desc *desc,
                                  const void *k_pool, const void *v_pool,             /* uint8 (n_pool, page_bytes) */
                                  const int32_t *k_page_ids, const int32_t *v_page_ids,
                                  const void *k_cents, const void *v_cents, const void *k_resid, const void *v_resid,
                                  void *k_out, void *v_out, million_stream_t stream);

/* ------------------------------------------------------------------------------------------------
 * Merge of partial attentions: n_parts results (out_i, lse_i) of one query over disjoint key sets -> the result over
 * their union.  Per row:  L = max_i lse_i,  w_i = exp(lse_i - L) (0 for -inf),  out = sum w_i out_i / sum w_i in fp32,
 * rounded once to fp16,  lse_out = L + ln sum w_i.  Every part -inf: out = 0, lse_out = -inf.  A NaN lse_i: the row is NaN.
 * Rows are (bs, nh, n_q) with per-tensor element strides (b, h, n), so a part may be a transposed view; a row's d fp16
 * values are contiguous.  One launch, one thread per (row, 8 dims), 16-byte loads and stores: every out stride must be
 * a multiple of 8 elements and every out pointer 16-byte aligned (MILLION_ERR_ALIGN).  `out` may be exactly one of the parts
 * (same pointer and strides): a thread reads its 8 dims of every part before it writes.  Any other overlap is the caller's
 * error; lse_out overlaps no part's lse (a row's lse is read by d / 8 threads).  lse_out may be NULL.  Validation precedes any
 * HIP call. */
#define MILLION_MERGE_MAX_PARTS 8
typedef struct {
    uint32_t struct_size;
    int32_t  n_parts;              /* 1 .. MILLION_MERGE_MAX_PARTS */
    int32_t  bs, nh, n_q;
    int32_t  d;                    /* 64 or 128 */
    int64_t  out_stride[MILLION_MERGE_MAX_PARTS][3];   /* per part: element strides (b, h, n) of its fp16 out rows */
    int64_t  lse_stride[MILLION_MERGE_MAX_PARTS][3];   /* per part: element strides (b, h, n) of its fp32 lse */
    int64_t  res_out_stride[3], res_lse_stride[3];     /* the same for the result */
} million_attn_merge_desc;

int million_attn_merge(const million_attn_merge_desc *desc, const void *const *part_outs, const float *const *part_lses,
                       void *out, float *lse_out /* may be NULL */, million_stream_t stream);

/* ------------------------------------------------------------------------------------------------
 * Draft verification (speculative decoding): n <= 16 draft rows per request at consecutive positions are verified without being
 * stored, and only the accepted ones are appended afterwards.
 *
 * The draft rows see the same past, so their attention over [codes below T; window] is one decode launch with the rows as
 * query heads: q (bs, nh, n, d) contiguous, viewed as (bs, nh * n, 1, d), puts virtual head v = h * n + i under kv head
 * v / (G * n) = h / G (G = nh / nh_k); million_pq_decode_attn_lse without k_new gives (out_a, lse_a) of every row.  (Chunk
 * attention with n_c = 0 gives the same pair.)  million_attn_block_merge then finishes the rows in one launch: the causal
 * attention among the block's own K/V rows, merged with the past part.  Per row (b, h, i) with i < n_b:
 *   s_j = q_i . k_j / sqrt(d) for j <= i, fp32;  L = max(lse_a, max_j s_j);  w = exp(lse_a - L) (0 for -inf);  p_j = exp(s_j - L);
 *   out = (w out_a + sum_j p_j v_j) / (w + sum_j p_j) in fp32, rounded once to fp16;  lse_out = L + ln(w + sum_j p_j).
 * This is million_attn_merge's contract with the second part computed in the kernel.  A NaN lse_a: the row is NaN.
 * dev_n (optional, device (bs,) int32): n_b, clamped into [0, n] on the device; NULL: n_b = n.  Rows i >= n_b get out = 0 and
 * lse_out = -inf (chunk attention's convention); whatever q / k_blk / v_blk / out_a hold at those rows, NaN included, reaches
 * no product and no live row.
 * q, k_blk, v_blk, out_a and out have element strides (b, h, n) and rows of d contiguous fp16; lse_a and lse_out are (bs, nh, n)
 * contiguous fp32; lse_out may be NULL.  `out` may be out_a (same pointer and strides): a lane reads its elements of out_a before
 * it writes them.  k_stage / v_stage (optional, together): the launch copies the n block rows there, bit for bit, as rows of d
 * at b * stage_stride_b + hk * stage_stride_h - the decode launch parks its new row in the same way; million_window_commit
 * reads them.  d = 64 or 128, any nh / nh_k, n in 1 .. 16.  One plain launch of bs * nh single-wave workgroups: no atomics, no
 * workspace, legal inside stream capture.  Validation precedes any HIP call: struct size, n, d, null pointers, 16-byte
 * pointers, strides in multiples of 8 elements. */
typedef struct {
    uint32_t struct_size;          /* = sizeof(million_block_merge_desc) */
    int32_t  bs, nh, nh_k;
    int32_t  n;                    /* draft rows, 1 .. 16 */
    int32_t  d;                    /* 64 or 128 */
    int64_t  q_stride[3], k_stride[3], v_stride[3];   /* element strides (b, h, n); multiples of 8 */
    int64_t  a_stride[3], o_stride[3];                /* out_a, out */
    int64_t  stage_stride_b, stage_stride_h;          /* k_stage / v_stage; their row stride is d */
} million_block_merge_desc;

int million_attn_block_merge(const million_block_merge_desc *desc, const void *q /* (bs, nh, n, d) */,
                             const void *k_blk, const void *v_blk /* (bs, nh_k, n, d) */,
                             const void *out_a /* (bs, nh, n, d) */, const float *lse_a /* (bs, nh, n) */,
                             const int32_t *dev_n /* (bs,), may be NULL */, void *out, float *lse_out /* may be NULL */,
                             void *k_stage, void *v_stage /* may be NULL */, million_stream_t stream);

/* The same launch for a draft that is a tree: n <= 16 nodes in topological order (a parent before its children), several
 * candidates under one parent, several roots allowed.  million_attn_tree_merge takes the desc and the arguments of
 * million_attn_block_merge and dev_mask, device (bs, n) int32, contiguous, 4-byte aligned, not NULL: bit j of word (b, i) says
 * that row i of request b sees block row j - the node's ancestors and itself.  The word is read on the device and never
 * trusted: the kernel uses
 *   m = (mask & ((2u << i) - 1)) | (1u << i)
 * so a row always sees itself and never a later row or a bit at or above n, whatever the word holds.  Everything else is
 * million_attn_block_merge's contract with "j <= i" replaced by "bit j of m": the merge with (out_a, lse_a), NaN and -inf
 * lse_a, dev_n (the live nodes are a prefix; the key loop runs to n_b), the staging of all n block rows, out aliasing out_a.
 * Rows i >= n_b get out = 0 and lse_out = -inf, and neither their q / k / v / out_a nor their mask words reach a live row.  A
 * mask of chains (bits 0 .. i) gives million_attn_block_merge's result bit for bit: a masked key has weight exactly 0 and the
 * kept terms are added in the same ascending order.  The past part (out_a, lse_a) never looks at the order among the rows, so
 * the decode launch (or chunk attention with n_c = 0) before this call is the one of a chain.  One plain launch of bs * nh
 * single-wave workgroups, legal inside stream capture; the mask's contents may change between replays.  Validation precedes
 * any HIP call, as above, plus: dev_mask NULL (MILLION_ERR_ARG) or not 4-byte aligned (MILLION_ERR_ALIGN). */
int million_attn_tree_merge(const million_block_merge_desc *desc, const void *q /* (bs, nh, n, d) */,
                            const void *k_blk, const void *v_blk /* (bs, nh_k, n, d) */,
                            const void *out_a /* (bs, nh, n, d) */, const float *lse_a /* (bs, nh, n) */,
                            const int32_t *dev_n /* (bs,), may be NULL */, const int32_t *dev_mask /* (bs, n) */, void *out,
                            float *lse_out /* may be NULL */, void *k_stage, void *v_stage /* may be NULL */,
                            million_stream_t stream);

/* ------------------------------------------------------------------------------------------------
 * Sink rows: the first tokens of a sequence kept as exact fp16 rows beside the code store (attention sinks: outlier keys that no
 * codebook represents, and a large share of every later row's softmax mass).  n query rows per (b, head) have attended to the
 * cache - a decode, chunk or verify call with its lse: (out_a, lse_a) - and million_attn_sink_merge finishes them in one launch:
 * their attention over the request's s_b live sink rows, merged with the past part.  Every sink row is visible to every query
 * row: the caller guarantees that each query position lies behind the sinks.  Per row (b, h, i) with i < n_b:
 *   s_j = q_i . k_j / sqrt(d) for j < s_b, fp32;  L = max(lse_a, max_j s_j);  w = exp(lse_a - L) (0 for -inf);  p_j = exp(s_j - L);
 *   out = (w out_a + sum_j p_j v_j) / (w + sum_j p_j) in fp32, rounded once to fp16;  lse_out = L + ln(w + sum_j p_j).
 * This is million_attn_merge's contract with the second part computed in the kernel, and the edge cases are
 * million_attn_block_merge's: a NaN lse_a makes the row NaN; lse_a = -inf with s_b = 0 gives out = 0 and lse_out = -inf; rows
 * i >= n_b get out = 0 and lse_out = -inf, and whatever q / out_a hold there, NaN included, reaches no live row.  s_b = 0 is the
 * identity: out is out_a bit for bit (w = 1; fp16 -> fp32 -> fp16) and lse_out is lse_a.
 * k_sink / v_sink are (bs, nh_k, s_cap, d) fp16 with rows of d side by side (row stride d) and element strides sink_stride_b /
 * sink_stride_h.  s_b = dev_s[b] (device (bs,) int32) clamped into [0, s_cap] on the device; dev_s = NULL: s_b = n_sink for every
 * request (n_sink is validated either way).  n_b = dev_n[b] clamped into [0, n]; NULL: n_b = n.  Sink rows at or past s_b may
 * hold anything, NaN included: they reach no product (the key loops run under the wave-uniform bound s_b).
 * q, out_a and out have element strides (b, h, n) and rows of d contiguous fp16; lse_a and lse_out are (bs, nh, n) contiguous
 * fp32; lse_out may be NULL.  `out` may be out_a (same pointer and strides) and lse_out may be lse_a: the one wave that writes a
 * row has read its out_a and lse_a before.  d = 64 or 128, any nh / nh_k, any n >= 1.  One plain launch of single-wave workgroups - n <= 4: bs * nh of them,
 * lane = sink row for the scores and lane = 2 dims for the value sum; n > 4: bs * nh * ceil(n / 16), lane = (row, quarter of d) -
 * no atomics, no workspace, legal inside stream capture; the counts' contents may change between replays.  Validation precedes
 * any HIP call: struct size (MILLION_ERR_ARG); n, d, s_cap, n_sink, nh % nh_k, more than 2^31 - 1 workgroups (MILLION_ERR_SHAPE);
 * null pointers (MILLION_ERR_ARG); 16-byte fp16 pointers, 4-byte int32 / fp32 pointers, strides in multiples of 8 elements
 * (MILLION_ERR_ALIGN). */
typedef struct {
    uint32_t struct_size;          /* = sizeof(million_sink_merge_desc) */
    int32_t  bs, nh, nh_k;
    int32_t  n;                    /* query rows per (b, head), >= 1: 1 for decode, <= 16 for verify, n_q for a chunk */
    int32_t  d;                    /* 64 or 128 */
    int32_t  s_cap;                /* rows of the sink buffers, 1 .. 64 */
    int32_t  n_sink;               /* live sink rows when dev_s is NULL, 0 .. s_cap */
    int64_t  q_stride[3], a_stride[3], o_stride[3];   /* element strides (b, h, n) of q, out_a, out; multiples of 8 */
    int64_t  sink_stride_b, sink_stride_h;            /* k_sink / v_sink (bs, nh_k, s_cap, d): row stride d */
} million_sink_merge_desc;

int million_attn_sink_merge(const million_sink_merge_desc *desc, const void *q /* (bs, nh, n, d) */,
                            const void *k_sink, const void *v_sink /* (bs, nh_k, s_cap, d) */,
                            const void *out_a /* (bs, nh, n, d) */, const float *lse_a /* (bs, nh, n) */,
                            const int32_t *dev_s /* (bs,), may be NULL */, const int32_t *dev_n /* (bs,), may be NULL */,
                            void *out, float *lse_out /* may be NULL */, million_stream_t stream);

/* Append the first a_b = dev_n[b] rows of k_new / v_new (layers, bs, nh_k, n_bound, d) to request b's residual window in every
 * layer of a paged cache, exactly as a_b decode steps would have: a decode step flushes the oldest page_size window rows into
 * the pages when the window is full and then appends.  a_b is clamped into [0, n_bound]; n_bound <= 16 and n_bound <= page_size,
 * so a request flushes at most once.  Per (layer, b), with {T, r, start} of the request's lengths row clamped as
 * million_pq_store_ragged clamps them:
 *   S = [the r window rows in ring order; the a new rows];  f = page_size if r + a > resid_cap, else 0;
 *   rows S[0, f) become tokens [T, T + f) of the K pages and the transposed V pages - the codes million_pq_flush writes, bit
 *   for bit; the new rows with source index >= f go to ring slot (start + r + i) % resid_cap;
 *   then T += f, r += a - f, start = (start + f) % resid_cap.  Word 3 is not touched.
 * Two stream-ordered launches (encode; append and advance), grids sized by the bounds alone, everything per request read on the
 * device: the call may be captured.  A request whose T + f would pass n_pages_cap * page_size is left untouched by both launches
 * (the caller checks before the call); a page id outside [0, n_pool) drops its stores.  The layers of the page tables, windows
 * and lengths lie side by side as for million_pq_flush_layers / million_cache_fork: ids_layer_stride (int32 entries),
 * rows_layer_stride (fp16 elements; each layer's windows contiguous (bs, nh_k, resid_cap, d)), lengths_layer_stride (int32
 * entries); dev_n is one (bs,) array for all layers.  Validation precedes any HIP call. */
typedef struct {
    uint32_t struct_size;          /* = sizeof(million_window_commit_desc) */
    int32_t  n_layers, bs, nh_k, d, M, C;
    int32_t  n_bound;              /* rows of k_new / v_new per request: 1 .. 16, <= page_size */
    int32_t  page_size, n_pages_cap, n_pool, resid_cap;
    int64_t  new_stride_l, new_stride_b, new_stride_h, new_stride_n;   /* k_new and v_new alike, fp16 elements, multiples of 8 */
    int64_t  ids_layer_stride, rows_layer_stride, lengths_layer_stride;
} million_window_commit_desc;

int million_window_commit(const million_window_commit_desc *desc, const void *k_new, const void *v_new, void *k_resid,
                          void *v_resid, const void *k_cents_prepared, const void *v_cents_prepared, void *k_pool,
                          void *v_pool, const int32_t *page_ids, int32_t *dev_lengths, const int32_t *dev_n,
                          million_stream_t stream);

/* million_window_commit for chosen rows (the accepted root-to-node path of a draft tree): the a_b = dev_n[b] new rows of request
 * b are rows dev_rows[b][0 .. a_b) of k_new / v_new, in that order, instead of rows 0 .. a_b.  dev_rows is device (bs, n_bound)
 * int32, contiguous, 4-byte aligned, not NULL, one array for all layers.  The source sequence becomes
 *   S = [the r window rows in ring order; k_new[dev_rows[b][i]] for i < a_b];
 * the flush rule, the ring slots, the lengths advance and every other word of million_window_commit's contract are unchanged,
 * and dev_rows[b] = 0, 1, 2, ... gives its result bit for bit.  An index is clamped into [0, n_bound) on the device; the entries
 * at or past a_b never reach a store, and neither launch reads outside dev_rows or outside the request's n_bound rows of
 * k_new / v_new.  Two stream-ordered launches, as above; validation precedes any HIP call, plus: dev_rows NULL
 * (MILLION_ERR_ARG) or not 4-byte aligned (MILLION_ERR_ALIGN). */
int million_window_commit_rows(const million_window_commit_desc *desc, const void *k_new, const void *v_new, void *k_resid,
                               void *v_resid, const void *k_cents_prepared, const void *v_cents_prepared, void *k_pool,
                               void *v_pool, const int32_t *page_ids, int32_t *dev_lengths, const int32_t *dev_n,
                               const int32_t *dev_rows, million_stream_t stream);

/* million_window_commit / million_window_commit_rows over uint16 pages or packed pages (codes of 512 .. 4096 centroids): the
 * contract above, word for word - the closed form of a_b decode steps, at most one flush per request, n_bound <= 16 and
 * n_bound <= page_size <= resid_cap, a request whose T + f would pass the page table left untouched - with these differences:
 *   k_cents / v_cents   the PLAIN (M, C, d_m) fp16 codebooks (wide codes have no prepared image), 16-byte aligned;
 *   C in {512, 1024, 2048, 4096}; d in {128, 64}; d / M in {2, 4}; page_size in {32, 64, 128};
 *   packed              0: k_pool (n_pool, page_size, M) / v_pool (n_pool, M, page_size) uint16; else packed pages ("Packed code
 *                       pages" above), M a multiple of 4.
 * The codes are million_pq_encode's / million_pq_encode_packed's bit for bit (the scan of million_pq_flush_wide and
 * million_pq_store_ragged_wide).  The first launch is the page writer of million_pq_store_ragged_wide with the commit's rows,
 * the second the append launch of the entries above.  Validation precedes any HIP call and any look at a pointer's value. */
int million_window_commit_wide(const million_window_commit_desc *desc, const void *k_new, const void *v_new, void *k_resid,
                               void *v_resid, const void *k_cents, const void *v_cents, void *k_pool, void *v_pool,
                               const int32_t *page_ids, int32_t *dev_lengths, const int32_t *dev_n, int packed,
                               million_stream_t stream);
int million_window_commit_rows_wide(const million_window_commit_desc *desc, const void *k_new, const void *v_new, void *k_resid,
                                    void *v_resid, const void *k_cents, const void *v_cents, void *k_pool, void *v_pool,
                                    const int32_t *page_ids, int32_t *dev_lengths, const int32_t *dev_n,
                                    const int32_t *dev_rows, int packed, million_stream_t stream);

/* ------------------------------------------------------------------------------------------------
 * Residual-window append.
 * Replaces: the two slice-assign copies of DynamicPQCache.decoding (pq_utils.py:304-312) /
 * PagedPQCache.decoding_with_pages (paged_pq_utils.py:377-380).
 * Writes k_new/v_new (bs, nh_k, 1, d) into row (resid_start + r) % resid_cap of the residual buffers;
 * when dev_lengths != NULL the row comes from the device array and r is incremented there. */
int million_residual_append(const void *k_new, const void *v_new, void *k_resid, void *v_resid,
                            int bs, int nh_k, int d, int resid_cap,
                            int64_t resid_stride_b, int64_t resid_stride_h,
                            int r, int resid_start, int32_t *dev_lengths, million_stream_t stream);

/* After a flush of `n_flushed` residual rows into the code store (reference: flush_to_pages,
 * paged_pq_utils.py:181-208 / DynamicPQCache.decoding, pq_utils.py:297-301) advance the device-resident
 * lengths: n_tokens += n_flushed, r -= n_flushed, resid_start = (resid_start + n_flushed) % resid_cap. */
int million_lengths_advance(int32_t *dev_lengths, int bs, int n_flushed, int resid_cap, million_stream_t stream);

/* Diagnostics only.  -1 in the product build.  In a library built with -DMILLION_DEBUG_CHECK_IDS: waits for the device and
 * returns (and clears) the number of page ids outside [0, k_pool_pages) / [0, v_pool_pages) that the three decode-attention
 * kernels have met since the last call; such ids were read as page 0 instead of as out-of-bounds addresses.  The same build
 * fills the whole LDS allocation of every decode-attention and chunk-attention workgroup with 0xFFFF (fp16 NaN) before the
 * kernel's first LDS write, so that a read of LDS the kernel never wrote gives NaN on every run (tests/lds_poison_child.py). */
int million_debug_bad_page_ids(void);
/* Diagnostics: waits for the device and returns (and clears) the number of (b, kv head) merges of the MFMA decode-attention
 * kernels that gave up waiting for a split's partial (a workgroup of the launch died, or the workspace was not zeroed).  The
 * heads concerned were written as NaN.  0 in every healthy run; after a non-zero answer zero the workspace again
 * (million_workspace_init).  -1: the runtime refused the read. */
int million_debug_tail_faults(void);
/* Diagnostics only: when `buf` is non-NULL the decode-attention kernels store up to 16 x uint64 realtime-counter
 * stamps (100 MHz) per wave at their phase boundaries into buf (grid_size * 8 waves * 32 slots entries).  NULL = off. */
void million_debug_set_stamp_buffer(void *buf);
/* Diagnostics only: runs the kernel's row-swap reductions on one wave: out_max[l] / out_sum[l] = max / sum of
 * in[l % 16 + 16*k], k = 0..3 (device pointers to 64 floats each). */
int million_debug_rows_reduce(const float *in64, float *out_max64, float *out_sum64, million_stream_t stream);

#ifdef __cplusplus
}
#endif
#endif /* MILLION_HIP_H */
