"""Torch-facing wrappers over the C ABI (include/million_hip.h).  PyTorch is plumbing here: device
memory, the current HIP stream and nothing else — all arithmetic runs in libmillion_hip.so.

There is deliberately no CPU/eager fallback: a CPU tensor, a missing library or an unsupported shape
raises.
"""
from __future__ import annotations

import collections
import ctypes
import dataclasses
import weakref
from typing import Callable, Container, Optional

import torch

from . import _lib as L

_ws_cache = {}
_prep_cache = {}


def _stream() -> int:
    # the raw handle of torch's current stream: ~0.2 us (torch.cuda.current_stream().cuda_stream builds a Stream object: ~1.5 us)
    return torch._C._cuda_getCurrentRawStream(torch.cuda.current_device())


def _ptr(t: Optional[torch.Tensor]) -> int:
    return 0 if t is None else t.data_ptr()


def _need_cuda(*ts):
    for t in ts:
        if t is not None and not t.is_cuda:
            raise RuntimeError("million_amd ops need device tensors (no CPU fallback)")


def _check_prepared(who: str, k_prep: torch.Tensor, v_prep: torch.Tensor, M: int, C: int, d: int) -> None:
    if k_prep.dtype != torch.float16 or v_prep.dtype != torch.float16 or k_prep.numel() != v_prep.numel() or k_prep.numel() != 4 * M * C * (d // M):
        raise RuntimeError(f"{who}: k_prep / v_prep must be the prepared codebooks of (M, C, d / M) (prepare_cents)")


def _check_dev_n(who: str, dev_n: torch.Tensor, bs: int) -> None:
    if dev_n.dtype != torch.int32 or tuple(dev_n.shape) != (bs,) or not dev_n.is_contiguous():
        raise RuntimeError(f"{who}: dev_n must be contiguous int32 (bs,)")


def prepare_cents(cents: torch.Tensor, cache: bool = True) -> torch.Tensor:
    """(M, C, d_m) fp16 codebook -> LDS-ready images (row image + column image), see million_prepare_cents.

    Cached per (storage, version): the reference passes the same codebook tensor on every call
    (pq_utils.py:149-159, one table for all layers and heads)."""
    _need_cuda(cents)
    if cents.dtype != torch.float16 or cents.dim() != 3:
        raise RuntimeError(f"codebook must be fp16 (M, C, d_m), got {cents.dtype} {tuple(cents.shape)}")
    # Cache keyed on the tensor OBJECT (weak reference) + its version counter: a data_ptr key would hand a
    # stale table to a new codebook that happens to be allocated where a freed one lived.
    key = id(cents)
    if cache:
        hit = _prep_cache.get(key)
        if hit is not None and hit[0]() is cents and hit[1] == cents._version:
            return hit[2]
    lib = L.load()
    c = cents.contiguous()
    M, C, dm = c.shape
    out = torch.empty(lib.million_prepared_cents_bytes(M, C, dm) // 2, dtype=torch.float16, device=c.device)
    L.check(lib.million_prepare_cents(c.data_ptr(), M, C, dm, out.data_ptr(), _stream()), "million_prepare_cents")
    if cache:
        for k in [k for k, v in _prep_cache.items() if v[0]() is None]:
            del _prep_cache[k]
        _prep_cache[key] = (weakref.ref(cents), cents._version, out)
    return out


def _encode_desc(X, cents, n, layout, token_start, x_row_start, x_row_mod, dev_lengths) -> L.EncodeDesc:
    """What the descriptor of every encode call says, whatever the destination: the rows of X (bs, nh_k, n_rows, d) - n of them,
    default all -, the codebook's geometry, the destination layout and token.  The destination's own fields are the caller's."""
    bs, nhk, n_rows, d = X.shape
    M, C, dm = cents.shape
    desc = L.EncodeDesc()
    desc.struct_size = ctypes.sizeof(L.EncodeDesc)
    desc.bs, desc.nh_k, desc.n, desc.d, desc.M, desc.C = bs, nhk, n_rows if n is None else n, d, M, C
    desc.x_stride_b, desc.x_stride_h, desc.x_stride_n = X.stride(0), X.stride(1), X.stride(2)
    desc.x_row_start, desc.x_row_mod = x_row_start, x_row_mod
    desc.dst_layout, desc.dst_token_start = layout, token_start
    desc.dev_lengths = _ptr(dev_lengths)
    return desc


def pq_encode_into(X: torch.Tensor, cents: torch.Tensor, dst: torch.Tensor, *, layout: int = L.MILLION_CODES_ROWMAJOR,
                   token_start: int = 0, n: Optional[int] = None, page_ids: Optional[torch.Tensor] = None,
                   page_size: int = 0, x_row_start: int = 0, x_row_mod: int = 0,
                   dev_lengths: Optional[torch.Tensor] = None, use_prepared: bool = True,
                   prepared: Optional[torch.Tensor] = None) -> None:
    """Encode rows of X (bs, nh_k, n_rows, d) fp16 and write the codes into `dst` in their final layout.
    use_prepared: hand the kernel the (cached) prepared codebook, whose fp32 image makes the distance loop ~1.6x
    faster; the codes are bit-identical either way.  prepared: that blob, when the caller already holds it (the caches
    do: nothing is allocated or launched on their behalf inside a captured step)."""
    _need_cuda(X, cents, dst, page_ids)
    code_dtype = code_dtype_for(cents.shape[1])
    if X.dtype != torch.float16 or cents.dtype != torch.float16 or dst.dtype != code_dtype:
        raise RuntimeError(f"pq_encode: X and cents must be fp16, dst {code_dtype} for C={cents.shape[1]}")
    if X.dim() != 4 or X.stride(3) != 1:
        raise RuntimeError("pq_encode: X must be (bs, nh_k, n, d) with a contiguous last dim")
    cents = cents.contiguous()
    M, C, dm = cents.shape
    desc = _encode_desc(X, cents, n, layout, token_start, x_row_start, x_row_mod, dev_lengths)
    if layout == L.MILLION_CODES_ROWMAJOR:
        if dst.dim() != 4 or dst.stride(3) != 1 or dst.stride(2) != M or dst.shape[3] != M:
            raise RuntimeError("pq_encode: row-major dst must be (bs, nh_k, T_cap, M) with dense rows")
        if dst.shape[2] < token_start + desc.n:
            raise RuntimeError("pq_encode: dst too short")
        desc.dst_stride_b, desc.dst_stride_h = dst.stride(0) * dst.element_size(), dst.stride(1) * dst.element_size()
    else:
        if page_ids is None or page_ids.dtype != torch.int32 or not page_ids.is_contiguous():
            raise RuntimeError("pq_encode: paged dst needs contiguous int32 page_ids (bs, nh_k, n_pages_cap)")
        if not dst.is_contiguous():
            raise RuntimeError("pq_encode: page pool must be contiguous")
        desc.page_size, desc.n_pages_cap = page_size, page_ids.shape[2]
    if prepared is None and use_prepared and C <= 256:
        prepared = prepare_cents(cents)            # cached per codebook tensor; callers that own one pass it in
    desc.cents_prepared = _ptr(prepared)
    lib = L.load()
    L.check(lib.million_pq_encode(ctypes.byref(desc), X.data_ptr(), cents.data_ptr(), dst.data_ptr(),
                                  _ptr(page_ids), _stream()), "million_pq_encode")
    _vshadow_drop(dst)


def pq_decode(codes: torch.Tensor, cents: torch.Tensor) -> torch.Tensor:
    """Drop-in for sa_decode_4d (reference pq_utils.py:501-540): codes (..., M) u8 (u16 for C > 256) + (M, C, d_m) fp16
    codebook -> (..., d) fp16 reconstruction (exact gather)."""
    _need_cuda(codes, cents)
    if cents.dtype != torch.float16 or cents.dim() != 3:
        raise RuntimeError("pq_decode: cents must be fp16 (M, C, d_m)")
    M, C, dm = cents.shape
    if codes.dtype != code_dtype_for(C):
        raise RuntimeError(f"pq_decode: codes must be {code_dtype_for(C)} for C={C}, got {codes.dtype}")
    if codes.shape[-1] != M:
        raise RuntimeError(f"pq_decode: codes have {codes.shape[-1]} subspaces, codebook {M}")
    codes, cents = codes.contiguous(), cents.contiguous()
    out = torch.empty(*codes.shape[:-1], M * dm, dtype=torch.float16, device=codes.device)
    n_rows = codes.numel() // M
    L.check(L.load().million_pq_decode(codes.data_ptr(), cents.data_ptr(), out.data_ptr(), n_rows, M * dm, M, C,
                                       _stream()), "million_pq_decode")
    return out


def code_dtype_for(C: int):
    """nbits2dtype of the reference (pq_utils.py:542-552) in terms of the codebook size: uint8 up to 256 centroids,
    uint16 up to 65536."""
    if C <= 256:
        return torch.uint8
    if C <= 65536:
        return torch.uint16
    raise RuntimeError(f"codebooks of {C} centroids are not supported (<= 65536)")


# ---- the code formats: what the attention and gather ops and the paged cache need to know of one, in one place ----
WIDE_CENTROIDS = (512, 1024, 2048, 4096)


def packed_hi_bits(C: int) -> int:
    """High bits stored beside the low byte of a packed code: 2 for C in 512 / 1024, 4 for C in 2048 / 4096."""
    if C not in WIDE_CENTROIDS:
        raise RuntimeError(f"packed codes: C={C} (packed pages hold codes of {WIDE_CENTROIDS} centroids; C <= 256 is a uint8 already)")
    return 2 if C <= 1024 else 4


def packed_page_bytes(page_size: int, M: int, C: int) -> int:
    """Bytes of one packed page: page_size * M * (8 + h) / 8, the low plane then the high plane."""
    return page_size * M * (8 + packed_hi_bits(C)) // 8


def _check_packed_pool(who, pool, page_size, M, C):
    if pool.dtype != torch.uint8 or pool.dim() != 2 or pool.shape[1] != packed_page_bytes(page_size, M, C) or not pool.is_contiguous():
        raise RuntimeError(f"{who}: a packed pool must be contiguous uint8 (n_pool, {packed_page_bytes(page_size, M, C)}) "
                           f"for page_size={page_size}, M={M}, C={C}")


def _check_word_store(who, name, codes, paged, page_size, bs, nh_k, M, C, bound):
    """One side's store of code words: a page pool (n_pool, ., .), or row-major (bs, nh_k, T, M) codes that hold the
    bound = (tokens, what the message calls them) the call reads."""
    if paged:
        if not codes.is_contiguous() or codes.dim() != 3:
            raise RuntimeError(f"{who}: {name} page pool must be contiguous (n_pool, ., .)")
        return
    if codes.dim() != 4 or codes.shape[3] != M or codes.shape[:2] != (bs, nh_k):
        raise RuntimeError(f"{who}: {name} must be (bs, nh_k, T, M)")
    if codes.shape[2] and (codes.stride(3) != 1 or codes.stride(2) != M):
        raise RuntimeError(f"{who}: {name} rows must be dense (stride M)")
    if bound[0] > codes.shape[2]:
        raise RuntimeError(f"{who}: {bound[1]} exceeds {name}")


def _check_packed_store(who, name, codes, paged, page_size, bs, nh_k, M, C, bound):
    """One side's pool of packed pages: there is no packed row-major form, and the page size is part of the format."""
    if not paged:
        raise RuntimeError(f"{who}: packed codes live in pages only - k_page_ids and v_page_ids are both needed")
    if page_size not in (32, 64, 128):
        raise RuntimeError(f"{who}: page_size={page_size} (32, 64 or 128)")
    _check_packed_pool(who, codes, page_size, M, C)


def _word_page_shapes(page_size, M, C):
    return (page_size, M), (M, page_size)      # V pages transposed


def _packed_page_shapes(page_size, M, C):
    return ((packed_page_bytes(page_size, M, C),),) * 2


@dataclasses.dataclass(frozen=True)
class CodeFormat:
    """One way PQ codes are held.  FMT_U8, FMT_U16 and FMT_PACKED are all there are; code_format() picks one."""
    name: str
    centroids: Container               # the codebook sizes C it goes with
    dtype: torch.dtype                 # of its stores
    # its stores hold one code per word of `dtype`: a row-major (bs, nh_k, T, M) form exists beside the page pools, pq_encode_into
    # writes both and the dtype selects the format.  False: planes of code bytes, in pages only, written by an op of their own; where
    # an op picks the format from its code tensors, its packed=True says this one
    rowmajor: bool
    code_bytes: int                    # the logical width of a code (million_gather_rows_desc.code_bytes)
    # the attention entries take the prepared blob (prepare_cents), which has no shape: pq_decode_attn is told M and C (and serves
    # row-major sides too: a page table per side).  False: the plain (M, C, d_m) codebook, one table for the two pools
    prepared: bool
    page_shapes: Callable              # (page_size, M, C) -> the shapes of a K page and of a V page in its pools
    check_store: Callable              # (who, name, codes, paged, page_size, bs, nh_k, M, C, bound): one side's store
    # the C entries (include/million_hip.h)
    encode: str
    decode_attn: str
    decode_ws: str
    chunk_attn: str                    # without lse, and
    chunk_attn_lse: str                # with it: one entry with an lse argument that may be null, except for 8-bit codes
    chunk_ws: str
    gather: str
    flush: str                         # the one-launch window flush,
    flush_layers: str                  # the same for several layers in one call, with or without the advance (encode-ahead), and
    store_ragged: str                  # the one-launch ragged store, into its pages
    commit: str                        # draft verification: the one-call commit of the accepted rows, every layer, and
    commit_rows: str                   # ... of chosen rows (the accepted path of a draft tree)
    fork: str                          # a slot becomes a copy of another, and
    swap: str                          # a request leaves its pages for a blob and comes back (blob format 1: uint8, 2: the wide formats)
    # the attention ops of this module over its stores, looked up by name when called (the methods below)
    op_decode_attn: str
    op_chunk_attn: str

    # ---- what a paged cache asks of its format: one call shape per job, whichever the format.  cents, prepared: the (K, V) pairs
    # of the codebooks as they are and of their prepared blobs (None where the format has none); the format takes what its op takes
    def encode_pages(self, X, cent, prepared, pool, **kw):
        """Rows of X into pages of `pool` (pq_encode_into's keywords); pq_encode_into takes the prepared image, the packed encoder has none."""
        if self.rowmajor:
            return pq_encode_into(X, cent, pool, prepared=prepared, **kw)
        return pq_encode_into_packed(X, cent, pool, **kw)

    def decode_workspace(self, q, k_res, *, M, C, page_size):
        """Bytes of the (zeroed) workspace of decode_pages calls of this shape."""
        if self.prepared:
            return decode_workspace_bytes(q, k_res, nh_k=k_res.shape[1], M=M, C=C)
        return decode_wide_workspace_bytes(q, k_res, M=M, C=C, page_size=page_size)

    def decode_pages(self, q, k_pool, v_pool, cents, prepared, k_res, v_res, r, *, M, C, page_ids, **kw):
        """Decode attention over the two pools through one page table; kw: what the three decode ops take alike."""
        op = globals()[self.op_decode_attn]
        if self.prepared:      # pq_decode_attn serves row-major sides too, behind a blob without a shape: a table per side, M and C said
            return op(q, k_pool, v_pool, *prepared, k_res, v_res, r, M=M, C=C, k_page_ids=page_ids, v_page_ids=page_ids, **kw)
        return op(q, k_pool, v_pool, *cents, k_res, v_res, r, page_ids=page_ids, **kw)

    def chunk_op(self, who, route):
        """The chunk attention of an extend call as attend(q, k_chunk, v_chunk, k_codes, v_codes, cents, prepared, k_res, v_res, r, **kw),
        kw pq_chunk_attn's.  route None / "chunk": chunk attention over the codes (pq_chunk_attn, pq_chunk_attn_wide, pq_chunk_attn_packed);
        "blocks": the block route (pq_chunk_attn_blocks: the past dequantised block by block into a bounded scratch and attended by the
        prompt kernel - for long chunks, profiles/chunk_blocks.txt), which picks the format from the code dtype and so is told
        packed=True where that cannot.  A route that does not exist is a ValueError, raised here: before the caller does anything."""
        if route not in (None, "chunk", "blocks"):
            raise ValueError(f"{who}: route={route!r} (None, 'chunk' or 'blocks')")
        name = "pq_chunk_attn_blocks" if route == "blocks" else self.op_chunk_attn
        said = {"packed": True} if route == "blocks" and not self.rowmajor else {}
        return lambda q, k_chunk, v_chunk, k_codes, v_codes, cents, prepared, *window, **kw: globals()[name](
            q, k_chunk, v_chunk, k_codes, v_codes, *(prepared if self.prepared else cents), *window, **said, **kw)

    def commit_pages(self, k_new, v_new, k_res, v_res, cents, prepared, k_pool, v_pool, page_ids, dev_lengths, dev_n, *, M, C, **kw):
        """The accepted rows of a verification into the windows (and, where a window overflows, its oldest rows into the pages) of every
        layer in one call (kw: n_bound, dev_rows): window_commit over the prepared codebooks, window_commit_wide over the codebooks as
        they are."""
        if self.prepared:
            return window_commit(k_new, v_new, k_res, v_res, *prepared, k_pool, v_pool, page_ids, dev_lengths, dev_n, M=M, C=C, **kw)
        return window_commit_wide(k_new, v_new, k_res, v_res, *cents, k_pool, v_pool, page_ids, dev_lengths, dev_n, packed=not self.rowmajor, **kw)

    def fork_pages(self, page_ids, k_pool, v_pool, k_res, v_res, dev_lengths, dst_slots, tail_ids, *, M, C, page_size, **kw):
        """Slots become a copy of another in one launch (kw: cache_fork's src, share, n_pages_bound, prefix_tokens): cache_fork, or
        cache_fork_wide told C, whether the pages are packed and - a packed pool has no such shape - page_size and M."""
        if self.prepared:
            return cache_fork(page_ids, k_pool, v_pool, k_res, v_res, dev_lengths, dst_slots, tail_ids, **kw)
        return cache_fork_wide(page_ids, k_pool, v_pool, k_res, v_res, dev_lengths, dst_slots, tail_ids, C=C, packed=not self.rowmajor,
                               page_size=page_size, M=M, **kw)

    def swap_pages(self, direction, page_ids, k_pool, v_pool, k_res, v_res, dev_lengths, slot_table, blob_offsets, blob, *, M, C, page_size, **kw):
        """Requests into blobs or back in one launch (kw: cache_swap's layer0, n_layers, n_pages_bound): cache_swap (blob format 1) or
        cache_swap_wide (format 2)."""
        if self.prepared:
            return cache_swap(direction, page_ids, k_pool, v_pool, k_res, v_res, dev_lengths, slot_table, blob_offsets, blob, **kw)
        return cache_swap_wide(direction, page_ids, k_pool, v_pool, k_res, v_res, dev_lengths, slot_table, blob_offsets, blob, C=C,
                               packed=not self.rowmajor, page_size=page_size, M=M, **kw)

    def swap_row_bytes(self, T, r, page_size, M, d, C):
        """Bytes of one (layer, kv head) row of a request blob of this format's version."""
        return cache_swap_row_bytes(T, r, page_size, M, d) if self.prepared else cache_swap_row_bytes_wide(T, r, page_size, M, d, C)

    @property
    def blob_version(self):
        """The blob format its swap entry reads and writes (include/million_hip.h): 1 for 8-bit codes, 2 for the wide formats."""
        return 1 if self.prepared else 2

    def flush_pages(self, k_rows, v_rows, cents, k_pool, v_pool, page_ids, **kw):
        """The oldest n rows of the ring windows into pages, one encode launch (kw: pq_flush's n, page_size, token_start, x_row_start,
        dev_lengths, min_r, advance): pq_flush for 8-bit codes, pq_flush_wide - told whether the pages are packed - for the wide
        formats.  Both take the codebooks as they are, and the layers of a cache side by side (5-D windows: the format's
        flush_layers entry); advance=False is encode-ahead."""
        if self.prepared:
            return pq_flush(k_rows, v_rows, *cents, k_pool, v_pool, page_ids, **kw)
        return pq_flush_wide(k_rows, v_rows, *cents, k_pool, v_pool, page_ids, packed=not self.rowmajor, **kw)

    def store_ragged_pages(self, k_new, v_new, k_res, v_res, cents, prepared, k_pool, v_pool, page_ids, dev_lengths, dev_n, **kw):
        """The store step of a ragged batch in one call (kw: M, C, page_size): pq_store_ragged over the prepared codebooks, or
        pq_store_ragged_wide over the codebooks as they are."""
        if self.prepared:
            return pq_store_ragged(k_new, v_new, k_res, v_res, *prepared, k_pool, v_pool, page_ids, dev_lengths, dev_n, **kw)
        return pq_store_ragged_wide(k_new, v_new, k_res, v_res, *cents, k_pool, v_pool, page_ids, dev_lengths, dev_n,
                                    packed=not self.rowmajor, **kw)


FMT_U8 = CodeFormat(
    "uint8", range(1, 257), torch.uint8, rowmajor=True, code_bytes=1, prepared=True, page_shapes=_word_page_shapes,
    check_store=_check_word_store,
    encode="million_pq_encode", decode_attn="million_pq_decode_attn", decode_ws="million_attn_workspace_bytes",
    chunk_attn="million_pq_chunk_attn", chunk_attn_lse="million_pq_chunk_attn_lse", chunk_ws="million_chunk_attn_workspace_bytes",
    gather="million_pq_gather_rows", flush="million_pq_flush_layers", flush_layers="million_pq_flush_layers", store_ragged="million_pq_store_ragged",
    commit="million_window_commit", commit_rows="million_window_commit_rows", fork="million_cache_fork", swap="million_cache_swap",
    op_decode_attn="pq_decode_attn", op_chunk_attn="pq_chunk_attn")
FMT_U16 = CodeFormat(
    "uint16", WIDE_CENTROIDS, torch.uint16, rowmajor=True, code_bytes=2, prepared=False, page_shapes=_word_page_shapes,
    check_store=_check_word_store,
    encode="million_pq_encode", decode_attn="million_pq_decode_attn_wide", decode_ws="million_attn_wide_workspace_bytes",
    chunk_attn="million_pq_chunk_attn_wide", chunk_attn_lse="million_pq_chunk_attn_wide", chunk_ws="million_chunk_attn_wide_workspace_bytes",
    gather="million_pq_gather_rows", flush="million_pq_flush_wide", flush_layers="million_pq_flush_wide_layers",
    store_ragged="million_pq_store_ragged_wide",
    commit="million_window_commit_wide", commit_rows="million_window_commit_rows_wide", fork="million_cache_fork_wide",
    swap="million_cache_swap_wide", op_decode_attn="pq_decode_attn_wide", op_chunk_attn="pq_chunk_attn_wide")
FMT_PACKED = CodeFormat(
    "packed", WIDE_CENTROIDS, torch.uint8, rowmajor=False, code_bytes=2, prepared=False, page_shapes=_packed_page_shapes,
    check_store=_check_packed_store,
    encode="million_pq_encode_packed", decode_attn="million_pq_decode_attn_packed", decode_ws="million_attn_wide_workspace_bytes",
    chunk_attn="million_pq_chunk_attn_packed", chunk_attn_lse="million_pq_chunk_attn_packed", chunk_ws="million_chunk_attn_wide_workspace_bytes",
    gather="million_pq_gather_rows_packed", flush="million_pq_flush_wide", flush_layers="million_pq_flush_wide_layers",
    store_ragged="million_pq_store_ragged_wide",
    commit="million_window_commit_wide", commit_rows="million_window_commit_rows_wide", fork="million_cache_fork_wide",
    swap="million_cache_swap_wide", op_decode_attn="pq_decode_attn_packed", op_chunk_attn="pq_chunk_attn_packed")
CODE_FORMATS = (FMT_U8, FMT_U16, FMT_PACKED)


def code_format(who: str, dtype, C: Optional[int], packed: bool = False) -> CodeFormat:
    """The format of what a caller hands in: the dtype of its code tensors, its codebook size C and its `packed` flag.  Packed pools
    are uint8 and cannot select: the flag does, and without it a uint8 tensor means 8-bit codes.  C = None: the dtype and the flag
    alone (a caller that leaves the check of C to the op it calls)."""
    if packed:
        fmt = FMT_PACKED
        if C is not None:
            packed_hi_bits(C)      # says what packed pages hold
    elif dtype == torch.uint8:
        fmt = FMT_U8
    elif dtype == torch.uint16:
        fmt = FMT_U16
    else:
        raise RuntimeError(f"{who}: codes must be uint8 or uint16, both sides alike")
    if C is not None and C not in fmt.centroids:
        raise RuntimeError(f"{who}: C={C} does not go with {dtype} codes (uint8: C <= 256; uint16: C in {WIDE_CENTROIDS})")
    return fmt


def _check_stores(who, fmt, k_codes, v_codes, k_page_ids, v_page_ids, page_size, M, C, bs=None, nh_k=None, bound=None):
    """The code store of each side of a chunk-attention or gather call, by the format's check.  A side is a page pool when it has
    ids, else row-major.  Pools-only formats need nothing of the batch, and their callers check them first: a wrong M, C or
    page_size is then said by the pool it does not fit, as ever.  bs, nh_k, bound: _check_word_store's."""
    for name, codes, ids in (("k_codes", k_codes, k_page_ids), ("v_codes", v_codes, v_page_ids)):
        fmt.check_store(who, name, codes, ids is not None, page_size, bs, nh_k, M, C, bound)


def _check_page_ids(who, k_page_ids, v_page_ids, page_size, bs, nh_k, ids64_ok):
    """The page ids of a chunk-attention or gather call -> (n_pages_cap, the ids are int64).  ids64_ok: int64 ids are served too."""
    id_types = "int32/int64" if ids64_ok else "int32"
    n_pages_cap, ids64 = 0, False
    for ids in (k_page_ids, v_page_ids):
        if ids is None:
            continue
        if (ids.dtype != torch.int32 and not (ids64_ok and ids.dtype == torch.int64)) or not ids.is_contiguous() or ids.dim() != 3 or ids.shape[:2] != (bs, nh_k):
            raise RuntimeError(f"{who}: page ids must be contiguous {id_types} (bs, nh_k, n_pages)")
        if n_pages_cap and (ids.shape[2] != n_pages_cap or (ids.dtype == torch.int64) != ids64):
            raise RuntimeError(f"{who}: K and V page ids must agree in {'dtype and ' if ids64_ok else ''}length")
        n_pages_cap, ids64 = ids.shape[2], ids.dtype == torch.int64
    if (k_page_ids is not None or v_page_ids is not None) and page_size is None:
        raise RuntimeError(f"{who}: paged codes need page_size")
    return n_pages_cap, ids64


def pq_encode(X: torch.Tensor, cents: torch.Tensor) -> torch.Tensor:
    """Drop-in for sa_encode_4d_keops (reference pq_utils.py:451-499): (bs, nh_k, n, d) -> (bs, nh_k, n, M) u8 (u16 for
    nbits 9..16, as sa_encode_4d_keops(target_dtype=nbits2dtype(nbits)) returns)."""
    bs, nhk, n, d = X.shape
    codes = torch.empty(bs, nhk, n, cents.shape[0], dtype=code_dtype_for(cents.shape[1]), device=X.device)
    if n:
        pq_encode_into(X, cents, codes)
    return codes


def _check_flush_windows(who, k_rows, v_rows):
    """The K and V ring windows of a flush -> (bs, nh_k, cap, d)."""
    if k_rows.shape != v_rows.shape or k_rows.stride() != v_rows.stride() or k_rows.dtype != torch.float16 or v_rows.dtype != torch.float16:
        raise RuntimeError(f"{who}: K and V windows must be fp16 with the same shape and strides")
    if k_rows.dim() != 4 or k_rows.stride(3) != 1:
        raise RuntimeError(f"{who}: windows must be (bs, nh_k, cap, d) with a contiguous last dim")
    return k_rows.shape


def _check_table(who, page_ids, bs, nh_k):
    """The one page table of a flush or ragged store (pq_flush words its own, together with its pools)."""
    if page_ids.dtype != torch.int32 or not page_ids.is_contiguous() or page_ids.dim() != 3 or page_ids.shape[:2] != (bs, nh_k):
        raise RuntimeError(f"{who}: contiguous int32 page_ids (bs, nh_k, n_pages_cap) expected")


def _check_dev_lengths(who, dev_lengths, bs):
    if dev_lengths.dtype != torch.int32 or dev_lengths.shape != (bs, 4) or not dev_lengths.is_contiguous():
        raise RuntimeError(f"{who}: dev_lengths must be contiguous int32 (bs, 4)")


def pq_flush(k_rows: torch.Tensor, v_rows: torch.Tensor, k_cents: torch.Tensor, v_cents: torch.Tensor,
             k_pool: torch.Tensor, v_pool: torch.Tensor, page_ids: torch.Tensor, *, n: int, page_size: int,
             token_start: int = 0, x_row_start: int = 0, dev_lengths: Optional[torch.Tensor] = None, min_r: int = 0,
             advance: bool = True) -> None:
    """One launch per window flush (reference PagedPQCache.flush_to_pages, paged_pq_utils.py:130-210): encode the oldest n
    rows of the K and V windows (rings of k_rows.shape[2] rows) into a K page and a transposed V page; with dev_lengths
    the destination token and the ring start are read on the device and advanced there; min_r > 0 then skips the batch
    items whose window holds fewer rows (ragged batches: only the full windows flush).

    Several layers in one launch: k_rows / v_rows (layers, bs, nh_k, cap, d), page_ids (layers, bs, nh_k, n_pages_cap),
    dev_lengths (layers, bs, 4) - the layers of one cache allocated side by side.  advance=False: encode only (encode-ahead;
    the window moves later: lengths_advance)."""
    _need_cuda(k_rows, v_rows, k_cents, v_cents, k_pool, v_pool, page_ids, dev_lengths)
    n_layers, x_ls, ids_ls, len_ls = 1, 0, 0, 0
    if k_rows.dim() == 5:
        if page_ids.dim() != 4 or page_ids.shape[0] != k_rows.shape[0] or (dev_lengths is not None and (dev_lengths.dim() != 3 or dev_lengths.shape[0] != k_rows.shape[0])):
            raise RuntimeError("pq_flush: layered windows need layered page_ids (and dev_lengths)")
        if k_rows.stride(0) != v_rows.stride(0) or not page_ids.is_contiguous() or (dev_lengths is not None and not dev_lengths.is_contiguous()):
            raise RuntimeError("pq_flush: layered windows must share the layer stride; contiguous page_ids / dev_lengths")
        n_layers, x_ls, ids_ls = k_rows.shape[0], k_rows.stride(0), page_ids.stride(0)
        len_ls = dev_lengths.stride(0) if dev_lengths is not None else 0
        k_rows, v_rows, page_ids = k_rows[0], v_rows[0], page_ids[0]
    bs, nhk, cap, d = _check_flush_windows("pq_flush", k_rows, v_rows)
    if page_ids.dtype != torch.int32 or not page_ids.is_contiguous() or not k_pool.is_contiguous() or not v_pool.is_contiguous():
        raise RuntimeError("pq_flush: contiguous pools and contiguous int32 page_ids (bs, nh_k, n_pages_cap) expected")
    k_cents, v_cents = k_cents.contiguous(), v_cents.contiguous()
    M, C, dm = k_cents.shape
    if v_cents.shape != k_cents.shape or C > 256 or k_pool.dtype != torch.uint8 or v_pool.dtype != torch.uint8:
        raise RuntimeError("pq_flush: uint8 codes, equal codebook shapes")
    desc = L.EncodeDesc()
    desc.struct_size = ctypes.sizeof(L.EncodeDesc)
    desc.bs, desc.nh_k, desc.n, desc.d, desc.M, desc.C = bs, nhk, n, d, M, C
    desc.x_stride_b, desc.x_stride_h, desc.x_stride_n = k_rows.stride(0), k_rows.stride(1), k_rows.stride(2)
    desc.x_row_start, desc.x_row_mod = x_row_start, cap
    desc.dst_layout, desc.dst_token_start = L.MILLION_CODES_KPAGES, token_start
    desc.page_size, desc.n_pages_cap = page_size, page_ids.shape[2]
    desc.dev_lengths = _ptr(dev_lengths)
    L.check(L.load().million_pq_flush_layers(ctypes.byref(desc), k_rows.data_ptr(), v_rows.data_ptr(), k_cents.data_ptr(),
                                             v_cents.data_ptr(), k_pool.data_ptr(), v_pool.data_ptr(), page_ids.data_ptr(),
                                             _ptr(dev_lengths), cap, min_r if dev_lengths is not None else 0,
                                             n_layers, x_ls, ids_ls, len_ls, int(bool(advance)), _stream()), "million_pq_flush_layers")


def _store_ragged(who, k_new, v_new, k_res, v_res, k_pool, v_pool, page_ids, dev_lengths, dev_n, M, C, page_size, n_bound, books,
                  pools_behind_table=None):
    """The body of pq_store_ragged and pq_store_ragged_wide: the checks of the new rows, the windows, n_bound, the page table, dev_lengths
    and dev_n, the descriptor and the call.  What is an op's own is handed in and runs where it always ran: books(bs, nh_k, d) ->
    (entry, k_cents, v_cents, extra arguments) checks the codebooks (the wide op: and the pools) behind the windows,
    pools_behind_table() checks pools behind the page table."""
    if k_new.dim() != 4 or k_new.stride(3) != 1 or v_new.shape != k_new.shape or v_new.stride(3) != 1:
        raise RuntimeError(f"{who}: k_new / v_new must be (bs, nh_k, n, d) of one shape with a contiguous last dim")
    bs, nhk, n_rows, d = k_new.shape
    n_bound = n_rows if n_bound is None else int(n_bound)
    if n_bound < 0 or n_bound > n_rows:
        raise RuntimeError(f"{who}: n_bound={n_bound} outside [0, {n_rows}]")
    if (k_res is None) != (v_res is None):
        raise RuntimeError(f"{who}: K and V windows go together")
    cap = 0
    if k_res is not None:
        if (k_res.dtype != torch.float16 or v_res.dtype != torch.float16 or k_res.dim() != 4 or k_res.shape != v_res.shape
                or k_res.stride() != v_res.stride() or k_res.shape[:2] != (bs, nhk) or k_res.shape[3] != d
                or k_res.stride(3) != 1 or k_res.stride(2) != d):
            raise RuntimeError(f"{who}: windows must be fp16 (bs, nh_k, cap, d) with dense rows, K and V alike")
        cap = k_res.shape[2]
    entry, k_cents, v_cents, extra = books(bs, nhk, d)
    _check_table(who, page_ids, bs, nhk)
    if pools_behind_table is not None:
        pools_behind_table()
    _check_dev_lengths(who, dev_lengths, bs)
    _check_dev_n(who, dev_n, bs)
    desc = L.StoreRaggedDesc()
    desc.struct_size = ctypes.sizeof(L.StoreRaggedDesc)
    desc.bs, desc.nh_k, desc.d, desc.M, desc.C, desc.n_bound = bs, nhk, d, M, C, n_bound
    desc.kn_stride_b, desc.kn_stride_h, desc.kn_stride_n = k_new.stride(0), k_new.stride(1), k_new.stride(2)
    desc.vn_stride_b, desc.vn_stride_h, desc.vn_stride_n = v_new.stride(0), v_new.stride(1), v_new.stride(2)
    desc.resid_cap, desc.page_size, desc.n_pages_cap = cap, page_size, page_ids.shape[2]
    if k_res is not None:
        desc.resid_stride_b, desc.resid_stride_h = k_res.stride(0), k_res.stride(1)
    L.check(getattr(L.load(), entry)(ctypes.byref(desc), k_new.data_ptr(), v_new.data_ptr(), _ptr(k_res), _ptr(v_res), k_cents.data_ptr(),
                                     v_cents.data_ptr(), k_pool.data_ptr(), v_pool.data_ptr(), page_ids.data_ptr(), dev_lengths.data_ptr(),
                                     dev_n.data_ptr(), *extra, _stream()), entry)


def pq_store_ragged(k_new: torch.Tensor, v_new: torch.Tensor, k_res: Optional[torch.Tensor], v_res: Optional[torch.Tensor],
                    k_prep: torch.Tensor, v_prep: torch.Tensor, k_pool: torch.Tensor, v_pool: torch.Tensor,
                    page_ids: torch.Tensor, dev_lengths: torch.Tensor, dev_n: torch.Tensor, *, M: int, C: int, page_size: int,
                    n_bound: Optional[int] = None) -> None:
    """The store step of a ragged batch in one call (million_pq_store_ragged): for every request b with dev_n[b] > 0 the
    r_b window rows of k_res / v_res (bs, nh_k, cap, d) in ring order and then the first dev_n[b] rows of k_new / v_new
    (bs, nh_k, n, d) are encoded behind the request's T_b tokens - K pages in k_pool, transposed V pages in v_pool, through
    page_ids (bs, nh_k, n_pages_cap) int32 - and the request's row of dev_lengths (bs, 4) int32 is advanced on the device
    (T += r + n, r = start = 0).  Every per-request value is read on the device, so the call can be captured and replayed
    while dev_lengths, dev_n and the rows change.  k_prep / v_prep: the prepared codebooks (prepare_cents).  n_bound: the rows of
    k_new / v_new the grid is sized for (default: all of them); dev_n is clamped into [0, n_bound].  k_res = v_res = None: no
    window (every r reads as 0)."""
    who = "pq_store_ragged"
    _need_cuda(k_new, v_new, k_res, v_res, k_prep, v_prep, k_pool, v_pool, page_ids, dev_lengths, dev_n)
    if k_new.dtype != torch.float16 or v_new.dtype != torch.float16 or k_pool.dtype != torch.uint8 or v_pool.dtype != torch.uint8:
        raise RuntimeError(f"{who}: new rows must be fp16, pools uint8")

    def books(bs, nh_k, d):
        _check_prepared(who, k_prep, v_prep, M, C, d)
        return FMT_U8.store_ragged, k_prep, v_prep, ()

    def pools_behind_table():
        if not k_pool.is_contiguous() or not v_pool.is_contiguous():
            raise RuntimeError(f"{who}: page pools must be contiguous")

    _store_ragged(who, k_new, v_new, k_res, v_res, k_pool, v_pool, page_ids, dev_lengths, dev_n, M, C, page_size, n_bound, books,
                  pools_behind_table)
    _vshadow_drop(v_pool)


def _check_wide_pools(who, k_cents, v_cents, k_pool, v_pool, page_size, bs, nh_k, d, packed):
    """The codebooks and the two pools of a wide flush or ragged store -> (fmt, M, C): the format by code_format (the pools' dtype,
    C, the packed flag), each pool by the format's check_store and its page shape."""
    if k_cents.dtype != torch.float16 or v_cents.dtype != torch.float16 or k_cents.dim() != 3 or v_cents.shape != k_cents.shape:
        raise RuntimeError(f"{who}: k_cents / v_cents must be fp16 (M, C, d_m) of one shape (the codebooks as they are: wide codes have no prepared image)")
    M, C, dm = k_cents.shape
    if M * dm != d:
        raise RuntimeError(f"{who}: codebooks of M={M}, d_m={dm} do not go with rows of d={d}")
    if C not in WIDE_CENTROIDS:
        raise RuntimeError(f"{who}: C={C} (codes of {WIDE_CENTROIDS} centroids; C <= 256 takes {who.replace('_wide', '')})")
    if k_pool.dtype != v_pool.dtype:
        raise RuntimeError(f"{who}: codes must be uint8 or uint16, both sides alike")
    if not packed and k_pool.dtype == torch.uint8:
        raise RuntimeError(f"{who}: uint8 pools hold 8-bit codes, which take {who.replace('_wide', '')} (packed pools: packed=True)")
    fmt = code_format(who, k_pool.dtype, C, packed)
    shapes = fmt.page_shapes(page_size, M, C)
    for name, pool, shape in (("k_pool", k_pool, shapes[0]), ("v_pool", v_pool, shapes[1])):
        fmt.check_store(who, name, pool, True, page_size, bs, nh_k, M, C, None)
        if tuple(pool.shape[1:]) != tuple(shape):
            raise RuntimeError(f"{who}: {name} must be (n_pool, {', '.join(map(str, shape))}) for page_size={page_size}, M={M}")
    return fmt, M, C


def pq_flush_wide(k_rows: torch.Tensor, v_rows: torch.Tensor, k_cents: torch.Tensor, v_cents: torch.Tensor,
                  k_pool: torch.Tensor, v_pool: torch.Tensor, page_ids: torch.Tensor, *, n: int, page_size: int,
                  token_start: int = 0, x_row_start: int = 0, dev_lengths: Optional[torch.Tensor] = None, min_r: int = 0,
                  packed: bool = False, advance: bool = True, pairs_in_flight: Optional[int] = None) -> None:
    """pq_flush for codes of 512 .. 4096 centroids (million_pq_flush_wide): the oldest n <= page_size rows of the K and V windows
    (bs, nh_k, cap, d) become tokens [T, T + n) of uint16 pages - K (n_pool, page_size, M), V (n_pool, M, page_size) - or, packed=True,
    of packed pages (uint8 (n_pool, packed_page_bytes)), in one encode launch; the codes are pq_encode_into's / pq_encode_into_packed's
    bit for bit.  dev_lengths (bs, 4) int32: every request's {T, r, start} is read on the device (clamped), requests with r < min_r
    take no part, the rows of the others advance there (a second, one-thread-per-request launch; word 3 untouched).  None:
    token_start / x_row_start for every request, nothing advances.

    Several layers in one call (million_pq_flush_wide_layers), as pq_flush takes them: k_rows / v_rows (layers, bs, nh_k, cap, d),
    page_ids (layers, bs, nh_k, n_pages_cap), dev_lengths (layers, bs, 4) - the layers of one cache allocated side by side; one
    encode launch and one advance launch for all of them.  advance=False: encode only (encode-ahead; nothing of dev_lengths is
    written, min_r means "rows present", the window moves later: lengths_advance) - a launch of small workgroups built to run
    beside a step's attention launches, `pairs_in_flight` (layer, request) pairs in its grid and the others walked (None: the
    library's rule, about one workgroup per CU in flight)."""
    who = "pq_flush_wide"
    _need_cuda(k_rows, v_rows, k_cents, v_cents, k_pool, v_pool, page_ids, dev_lengths)
    layered = k_rows.dim() == 5
    n_layers, x_ls, ids_ls, len_ls = 1, 0, 0, 0
    if layered:
        if (v_rows.dim() != 5 or v_rows.shape[0] != k_rows.shape[0] or page_ids.dim() != 4 or page_ids.shape[0] != k_rows.shape[0]
                or (dev_lengths is not None and (dev_lengths.dim() != 3 or dev_lengths.shape[0] != k_rows.shape[0]))):
            raise RuntimeError(f"{who}: layered windows need layered page_ids (and dev_lengths) of as many layers")
        if k_rows.stride(0) != v_rows.stride(0) or not page_ids.is_contiguous() or (dev_lengths is not None and not dev_lengths.is_contiguous()):
            raise RuntimeError(f"{who}: layered windows must share the layer stride; contiguous page_ids / dev_lengths")
        if k_rows.stride(0) % 8:
            raise RuntimeError(f"{who}: the layer stride of the windows must be a multiple of 8 elements")
        n_layers = k_rows.shape[0]
        if n_layers:
            x_ls, ids_ls = k_rows.stride(0), page_ids.stride(0)
            len_ls = dev_lengths.stride(0) if dev_lengths is not None else 0
            k_rows, v_rows, page_ids = k_rows[0], v_rows[0], page_ids[0]
            lengths0 = dev_lengths[0] if dev_lengths is not None else None
        else:
            return
    else:
        lengths0 = dev_lengths
    if pairs_in_flight is not None and (advance or int(pairs_in_flight) < 1):
        raise RuntimeError(f"{who}: pairs_in_flight={pairs_in_flight} (a positive count, with advance=False only)")
    bs, nhk, cap, d = _check_flush_windows(who, k_rows, v_rows)
    k_cents, v_cents = k_cents.contiguous(), v_cents.contiguous()
    fmt, M, C = _check_wide_pools(who, k_cents, v_cents, k_pool, v_pool, page_size, bs, nhk, d, packed)
    _check_table(who, page_ids, bs, nhk)
    if lengths0 is not None:
        _check_dev_lengths(who, lengths0, bs)
    if not 0 <= n <= page_size:
        raise RuntimeError(f"{who}: n={n} outside [0, page_size={page_size}]")
    desc = _encode_desc(k_rows, k_cents, n, L.MILLION_CODES_KPAGES, token_start, x_row_start, cap, lengths0)
    desc.page_size, desc.n_pages_cap = page_size, page_ids.shape[2]
    if not layered and advance:
        L.check(getattr(L.load(), fmt.flush)(ctypes.byref(desc), k_rows.data_ptr(), v_rows.data_ptr(), k_cents.data_ptr(), v_cents.data_ptr(),
                                             k_pool.data_ptr(), v_pool.data_ptr(), page_ids.data_ptr(), _ptr(dev_lengths), cap,
                                             min_r if dev_lengths is not None else 0, int(bool(packed)), _stream()), fmt.flush)
        return
    L.check(getattr(L.load(), fmt.flush_layers)(ctypes.byref(desc), k_rows.data_ptr(), v_rows.data_ptr(), k_cents.data_ptr(), v_cents.data_ptr(),
                                                k_pool.data_ptr(), v_pool.data_ptr(), page_ids.data_ptr(), _ptr(lengths0), cap,
                                                min_r if lengths0 is not None else 0, n_layers, x_ls, ids_ls, len_ls, int(bool(advance)),
                                                int(bool(packed)), int(pairs_in_flight or 0), _stream()), fmt.flush_layers)


def pq_store_ragged_wide(k_new: torch.Tensor, v_new: torch.Tensor, k_res: Optional[torch.Tensor], v_res: Optional[torch.Tensor],
                         k_cents: torch.Tensor, v_cents: torch.Tensor, k_pool: torch.Tensor, v_pool: torch.Tensor,
                         page_ids: torch.Tensor, dev_lengths: torch.Tensor, dev_n: torch.Tensor, *, M: int, C: int, page_size: int,
                         packed: bool = False, n_bound: Optional[int] = None) -> None:
    """pq_store_ragged for codes of 512 .. 4096 centroids (million_pq_store_ragged_wide): the same call - every request's window
    rows in ring order and then its first dev_n[b] new rows behind its T_b tokens, its row of dev_lengths advanced on the device -
    into uint16 pages or, packed=True, packed pages, with the codebooks as they are (fp16 (M, C, d_m)) in place of the prepared
    ones.  Codes are pq_encode_into's / pq_encode_into_packed's bit for bit."""
    who = "pq_store_ragged_wide"
    _need_cuda(k_new, v_new, k_res, v_res, k_cents, v_cents, k_pool, v_pool, page_ids, dev_lengths, dev_n)
    if k_new.dtype != torch.float16 or v_new.dtype != torch.float16:
        raise RuntimeError(f"{who}: new rows must be fp16")

    def books(bs, nh_k, d):
        kc, vc = k_cents.contiguous(), v_cents.contiguous()
        fmt, M_c, C_c = _check_wide_pools(who, kc, vc, k_pool, v_pool, page_size, bs, nh_k, d, packed)
        if (M_c, C_c) != (M, C):
            raise RuntimeError(f"{who}: M={M}, C={C} said, codebooks of M={M_c}, C={C_c}")
        return fmt.store_ragged, kc, vc, (int(bool(packed)),)

    _store_ragged(who, k_new, v_new, k_res, v_res, k_pool, v_pool, page_ids, dev_lengths, dev_n, M, C, page_size, n_bound, books)


def _u8_cache_pools(who, k_pool, v_pool):
    """The two uint8 pools of a fork or swap call -> (n_pool, page_size, M)."""
    if (k_pool.dtype != torch.uint8 or v_pool.dtype != torch.uint8 or k_pool.dim() != 3 or not k_pool.is_contiguous() or not v_pool.is_contiguous()
            or v_pool.shape != (k_pool.shape[0], k_pool.shape[2], k_pool.shape[1])):
        raise RuntimeError(f"{who}: contiguous uint8 pools (n_pool, page_size, M) and (n_pool, M, page_size) expected")
    return tuple(k_pool.shape)


def _wide_cache_pools(who, k_pool, v_pool, C, packed, page_size, M):
    """The two pools of a wide fork or swap call -> (n_pool, page_size, M), by _check_wide_pools' rules without the codebooks (the
    calls move codes and never look one up): C, the pools' dtype and the packed flag pick the format, the format checks each pool
    and its page shape.  uint16 pools say page_size and M by their shape; packed pools (n_pool, page_bytes) cannot, so both are said."""
    if C not in WIDE_CENTROIDS:
        raise RuntimeError(f"{who}: C={C} (codes of {WIDE_CENTROIDS} centroids; C <= 256 takes {who.replace('_wide', '')})")
    if k_pool.dtype != v_pool.dtype:
        raise RuntimeError(f"{who}: codes must be uint8 or uint16, both sides alike")
    if not packed and k_pool.dtype == torch.uint8:
        raise RuntimeError(f"{who}: uint8 pools hold 8-bit codes, which take {who.replace('_wide', '')} (packed pools: packed=True)")
    fmt = code_format(who, k_pool.dtype, C, packed)
    if packed and (page_size is None or M is None):
        raise RuntimeError(f"{who}: packed pools are (n_pool, page_bytes): page_size= and M= must be said")
    if not packed:
        if k_pool.dim() != 3:
            raise RuntimeError(f"{who}: k_pool page pool must be contiguous (n_pool, page_size, M)")
        if (page_size is not None and page_size != k_pool.shape[1]) or (M is not None and M != k_pool.shape[2]):
            raise RuntimeError(f"{who}: page_size={page_size}, M={M} said, k_pool of pages {tuple(k_pool.shape[1:])}")
        page_size, M = k_pool.shape[1:]
    if page_size not in (32, 64, 128) or M not in (16, 32, 64):
        raise RuntimeError(f"{who}: page_size={page_size} (32, 64 or 128), M={M} (16, 32 or 64)")
    shapes = fmt.page_shapes(page_size, M, C)
    for name, pool, shape in (("k_pool", k_pool, shapes[0]), ("v_pool", v_pool, shapes[1])):
        fmt.check_store(who, name, pool, True, page_size, None, None, M, C, None)
        if tuple(pool.shape[1:]) != tuple(shape):
            raise RuntimeError(f"{who}: {name} must be (n_pool, {', '.join(map(str, shape))}) for page_size={page_size}, M={M}")
    if k_pool.shape[0] != v_pool.shape[0]:
        raise RuntimeError(f"{who}: k_pool and v_pool must hold the same number of pages")
    return k_pool.shape[0], page_size, M


def _cache_fork(who, entry, pools, extra, page_ids, k_pool, v_pool, k_res, v_res, dev_lengths, dst_slots, tail_ids, src, share,
                n_pages_bound, prefix_tokens):
    """cache_fork and cache_fork_wide: the checks of the cache arrays, the descriptor, the launch of `entry`.  pools():
    (n_pool, page_size, M) of the two pools or the format's refusal; extra: the entry's arguments between tail_ids and the stream."""
    _need_cuda(page_ids, k_pool, v_pool, k_res, v_res, dev_lengths, dst_slots, tail_ids)
    if page_ids.dtype != torch.int32 or page_ids.dim() != 4 or page_ids[0].numel() and not page_ids[0].is_contiguous():
        raise RuntimeError(f"{who}: int32 page_ids (layers, bs, nh_k, n_pages_cap), each layer contiguous, expected")
    n_layers, bs, nhk, cap_pages = page_ids.shape
    n_pool, page_size, M = pools()
    if (k_res.dtype != torch.float16 or v_res.dtype != torch.float16 or k_res.dim() != 5 or k_res.shape != v_res.shape or k_res.stride() != v_res.stride()
            or k_res.shape[:3] != (n_layers, bs, nhk) or not k_res[0].is_contiguous()):
        raise RuntimeError(f"{who}: fp16 windows (layers, bs, nh_k, cap, d), each layer contiguous, K and V alike, expected")
    cap, d = k_res.shape[3], k_res.shape[4]
    if dev_lengths.dtype != torch.int32 or dev_lengths.shape != (n_layers, bs, 4) or not dev_lengths[0].is_contiguous():
        raise RuntimeError(f"{who}: int32 dev_lengths (layers, bs, 4) expected")
    if dst_slots.dtype != torch.int32 or dst_slots.dim() != 1 or not dst_slots.is_contiguous():
        raise RuntimeError(f"{who}: dst_slots must be contiguous int32 (n_dst,)")
    n_dst = dst_slots.numel()
    if tail_ids is not None and (tail_ids.dtype != torch.int32 or tail_ids.shape != (n_dst, n_layers, nhk) or not tail_ids.is_contiguous()):
        raise RuntimeError(f"{who}: tail_ids must be contiguous int32 (n_dst, layers, nh_k)")
    if share and tail_ids is None:
        raise RuntimeError(f"{who}: share=True needs tail_ids")
    desc = L.ForkDesc()
    desc.struct_size = ctypes.sizeof(L.ForkDesc)
    desc.n_layers, desc.bs, desc.nh_k, desc.d, desc.M, desc.page_size = n_layers, bs, nhk, d, M, page_size
    desc.n_pages_cap, desc.n_pool, desc.resid_cap = cap_pages, n_pool, cap
    desc.ids_layer_stride, desc.rows_layer_stride, desc.lengths_layer_stride = page_ids.stride(0), k_res.stride(0), dev_lengths.stride(0)
    desc.src, desc.n_dst, desc.mode = int(src), n_dst, L.MILLION_FORK_SHARE if share else L.MILLION_FORK_COPY
    desc.n_pages_bound = cap_pages if n_pages_bound is None else int(n_pages_bound)
    desc.prefix_tokens = int(prefix_tokens)
    L.check(getattr(L.load(), entry)(ctypes.byref(desc), page_ids.data_ptr(), k_pool.data_ptr(), v_pool.data_ptr(), k_res.data_ptr(),
                                     v_res.data_ptr(), dev_lengths.data_ptr(), dst_slots.data_ptr(), _ptr(tail_ids), *extra, _stream()), entry)
    _vshadow_drop(v_pool)


def cache_fork(page_ids: torch.Tensor, k_pool: torch.Tensor, v_pool: torch.Tensor, k_res: torch.Tensor, v_res: torch.Tensor,
               dev_lengths: torch.Tensor, dst_slots: torch.Tensor, tail_ids: Optional[torch.Tensor], *, src: int, share: bool,
               n_pages_bound: Optional[int] = None, prefix_tokens: int = -1) -> None:
    """Make the batch slots dst_slots (device int32 (n_dst,)) a copy of slot `src` in every layer, in one launch
    (million_cache_fork): page_ids (layers, bs, nh_k, n_pages_cap) int32, k_pool (n_pool, page_size, M) / v_pool
    (n_pool, M, page_size) uint8, k_res / v_res (layers, bs, nh_k, cap, d) fp16, dev_lengths (layers, bs, 4) int32 - the layers
    of one cache side by side.  share=True: the destinations' table rows get the source's ids and tail_ids (device int32
    (n_dst, layers, nh_k)) for the partial tail page, which alone is copied; share=False: every live page is copied into the
    ids the destinations' rows hold.  The window and the lengths row follow; prefix_tokens >= 0 copies the first tokens only and
    no window.  n_pages_bound (default: the table's row length) bounds the source's pages: it sizes the grid."""
    _cache_fork("cache_fork", "million_cache_fork", lambda: _u8_cache_pools("cache_fork", k_pool, v_pool), (), page_ids, k_pool, v_pool,
                k_res, v_res, dev_lengths, dst_slots, tail_ids, src, share, n_pages_bound, prefix_tokens)


def cache_fork_wide(page_ids: torch.Tensor, k_pool: torch.Tensor, v_pool: torch.Tensor, k_res: torch.Tensor, v_res: torch.Tensor,
                    dev_lengths: torch.Tensor, dst_slots: torch.Tensor, tail_ids: Optional[torch.Tensor], *, src: int, share: bool,
                    n_pages_bound: Optional[int] = None, prefix_tokens: int = -1, C: int, packed: bool = False,
                    page_size: Optional[int] = None, M: Optional[int] = None) -> None:
    """cache_fork over the pools of a wide cache (million_cache_fork_wide): uint16 pools (n_pool, page_size, M) / (n_pool, M,
    page_size) or, packed=True, packed pools uint8 (n_pool, packed_page_bytes(page_size, M, C)) - then page_size= and M= are said,
    the pools' shape cannot.  Every argument and every rule is cache_fork's; a packed page is copied whole, both planes."""
    who = "cache_fork_wide"
    _cache_fork(who, "million_cache_fork_wide", lambda: _wide_cache_pools(who, k_pool, v_pool, C, packed, page_size, M),
                (int(C), int(bool(packed))), page_ids, k_pool, v_pool, k_res, v_res, dev_lengths, dst_slots, tail_ids, src, share,
                n_pages_bound, prefix_tokens)


def cache_swap_row_bytes(T: int, r: int, page_size: int, M: int, d: int) -> int:
    """Bytes of one (layer, kv head) row of a request blob, format 1 (million_cache_swap): the K pages and the V pages of
    ceil(T / page_size) pages, r window rows of d fp16 per side.  Always a multiple of 16."""
    n_live = (int(T) + page_size - 1) // page_size
    return 2 * n_live * page_size * M + 4 * int(r) * d


def cache_swap_row_bytes_wide(T: int, r: int, page_size: int, M: int, d: int, C: int) -> int:
    """Bytes of one (layer, kv head) row of a request blob, format 2 (million_cache_swap_wide): format 1's row with packed pages -
    packed_page_bytes(page_size, M, C) each - whatever the pool holds.  Always a multiple of 16."""
    n_live = (int(T) + page_size - 1) // page_size
    return 2 * n_live * packed_page_bytes(page_size, M, C) + 4 * int(r) * d


def _cache_swap(who, entry, pools, extra, direction, page_ids, k_pool, v_pool, k_res, v_res, dev_lengths, slot_table, blob_offsets, blob,
                layer0, n_layers, n_pages_bound):
    """cache_swap and cache_swap_wide: the checks of the cache arrays, the descriptor, the launch of `entry` (pools, extra:
    _cache_fork's)."""
    _need_cuda(page_ids, k_pool, v_pool, k_res, v_res, dev_lengths, slot_table, blob_offsets, blob)
    if direction not in (L.MILLION_SWAP_PACK, L.MILLION_SWAP_UNPACK):
        raise RuntimeError(f"{who}: direction must be MILLION_SWAP_PACK or MILLION_SWAP_UNPACK")
    if page_ids.dtype != torch.int32 or page_ids.dim() != 4 or page_ids[0].numel() and not page_ids[0].is_contiguous():
        raise RuntimeError(f"{who}: int32 page_ids (layers, bs, nh_k, n_pages_cap), each layer contiguous, expected")
    n_all, bs, nhk, cap_pages = page_ids.shape
    n_pool, page_size, M = pools()
    if (k_res.dtype != torch.float16 or v_res.dtype != torch.float16 or k_res.dim() != 5 or k_res.shape != v_res.shape or k_res.stride() != v_res.stride()
            or k_res.shape[:3] != (n_all, bs, nhk) or not k_res[0].is_contiguous()):
        raise RuntimeError(f"{who}: fp16 windows (layers, bs, nh_k, cap, d), each layer contiguous, K and V alike, expected")
    cap, d = k_res.shape[3], k_res.shape[4]
    if dev_lengths.dtype != torch.int32 or dev_lengths.shape != (n_all, bs, 4) or not dev_lengths[0].is_contiguous():
        raise RuntimeError(f"{who}: int32 dev_lengths (layers, bs, 4) expected")
    if slot_table.dtype != torch.int32 or slot_table.dim() != 2 or slot_table.shape[1] != 4 or not slot_table.is_contiguous():
        raise RuntimeError(f"{who}: slot_table must be contiguous int32 (n_slots, 4)")
    n_slots = slot_table.shape[0]
    if blob_offsets.dtype != torch.int64 or blob_offsets.shape != (n_slots,) or not blob_offsets.is_contiguous():
        raise RuntimeError(f"{who}: blob_offsets must be contiguous int64 (n_slots,)")
    if blob.dtype != torch.uint8 or blob.dim() != 1 or not blob.is_contiguous():
        raise RuntimeError(f"{who}: blob must be a contiguous 1-D uint8 tensor")
    desc = L.SwapDesc()
    desc.struct_size = ctypes.sizeof(L.SwapDesc)
    desc.direction = int(direction)
    desc.n_layers, desc.bs, desc.nh_k, desc.d, desc.M, desc.page_size = n_all, bs, nhk, d, M, page_size
    desc.n_pages_cap, desc.n_pool, desc.resid_cap = cap_pages, n_pool, cap
    desc.layer0, desc.n_layers_call = int(layer0), n_all - int(layer0) if n_layers is None else int(n_layers)
    desc.ids_layer_stride, desc.rows_layer_stride, desc.lengths_layer_stride = page_ids.stride(0), k_res.stride(0), dev_lengths.stride(0)
    desc.blob_bytes = blob.numel()
    desc.n_slots = n_slots
    desc.n_pages_bound = cap_pages if n_pages_bound is None else int(n_pages_bound)
    L.check(getattr(L.load(), entry)(ctypes.byref(desc), page_ids.data_ptr(), k_pool.data_ptr(), v_pool.data_ptr(), k_res.data_ptr(),
                                     v_res.data_ptr(), dev_lengths.data_ptr(), slot_table.data_ptr(), blob_offsets.data_ptr(),
                                     blob.data_ptr(), *extra, _stream()), entry)
    if direction == L.MILLION_SWAP_UNPACK:
        _vshadow_drop(v_pool)


def cache_swap(direction: int, page_ids: torch.Tensor, k_pool: torch.Tensor, v_pool: torch.Tensor, k_res: torch.Tensor,
               v_res: torch.Tensor, dev_lengths: torch.Tensor, slot_table: torch.Tensor, blob_offsets: torch.Tensor,
               blob: torch.Tensor, *, layer0: int = 0, n_layers: Optional[int] = None, n_pages_bound: Optional[int] = None) -> None:
    """Pack requests into blobs (direction = L.MILLION_SWAP_PACK) or restore blobs into the pages the slots' table rows name
    (L.MILLION_SWAP_UNPACK), for the layers [layer0, layer0 + n_layers) (default: from layer0 on), in one launch
    (million_cache_swap).  The cache arrays are those of cache_fork; slot_table: device int32 (n_slots, 4) {slot, T, r, start};
    blob_offsets: device int64 (n_slots,), the byte offset in `blob` (device uint8, 1-D) of each entry's first row of layer0.
    n_pages_bound (default: the table's row length) bounds a request's pages: it sizes the grid and clamps T."""
    _cache_swap("cache_swap", "million_cache_swap", lambda: _u8_cache_pools("cache_swap", k_pool, v_pool), (), direction, page_ids, k_pool,
                v_pool, k_res, v_res, dev_lengths, slot_table, blob_offsets, blob, layer0, n_layers, n_pages_bound)


def cache_swap_wide(direction: int, page_ids: torch.Tensor, k_pool: torch.Tensor, v_pool: torch.Tensor, k_res: torch.Tensor,
                    v_res: torch.Tensor, dev_lengths: torch.Tensor, slot_table: torch.Tensor, blob_offsets: torch.Tensor,
                    blob: torch.Tensor, *, layer0: int = 0, n_layers: Optional[int] = None, n_pages_bound: Optional[int] = None,
                    C: int, packed: bool = False, page_size: Optional[int] = None, M: Optional[int] = None) -> None:
    """cache_swap over the pools of a wide cache (million_cache_swap_wide; the pools: cache_fork_wide's) with blob format 2: the
    pages of the blob are packed pages whatever the pools hold, dead bytes zero and every field code & (C - 1), so a uint16 pool
    and a packed pool that hold the same codes pack to the same bytes, and a blob restores into either."""
    who = "cache_swap_wide"
    _cache_swap(who, "million_cache_swap_wide", lambda: _wide_cache_pools(who, k_pool, v_pool, C, packed, page_size, M),
                (int(C), int(bool(packed))), direction, page_ids, k_pool, v_pool, k_res, v_res, dev_lengths, slot_table, blob_offsets, blob,
                layer0, n_layers, n_pages_bound)


def transpose_v_codes(v_codes: torch.Tensor, n_tokens: Optional[int] = None) -> torch.Tensor:
    """Row-major V codes (bs, nh_k, T, M) u8 -> dense transposed 64-token pages ((bs*nh_k)*ceil(T/64), M, 64)."""
    _need_cuda(v_codes)
    if v_codes.dtype != torch.uint8 or v_codes.dim() != 4:
        raise RuntimeError("transpose_v_codes: (bs, nh_k, T, M) uint8 expected")
    bs, nhk, T, M = v_codes.shape
    T = T if n_tokens is None else n_tokens
    if T <= 0 or v_codes.stride(3) != 1 or v_codes.stride(2) != M:
        raise RuntimeError("transpose_v_codes: dense rows and T > 0 expected")
    pages = torch.empty(bs * nhk * ((T + 63) // 64), M, 64, dtype=torch.uint8, device=v_codes.device)
    L.check(L.load().million_transpose_v_codes(v_codes.data_ptr(), pages.data_ptr(), bs, nhk, T, M, v_codes.stride(0),
                                               v_codes.stride(1), _stream()), "million_transpose_v_codes")
    return pages


# Transposed shadow of row-major V code tensors.  The reference's production call (Interface.template.cu:26-38) hands the
# SAME value_codes tensor to the kernel on every decode step between two flushes (DynamicPQCache.value_cache[layer] is
# replaced by torch.cat only when the window is flushed, pq_utils.py:140-147).  The fast kernels want transposed pages, so
# the first call on a tensor transposes it once and later calls reuse the pages.  Keyed on the tensor OBJECT (weak
# reference, so a new tensor at a recycled address never hits) + its version counter (in-place writes through torch
# invalidate) + geometry; bounded (least recently used) so abandoned tensors do not pin memory.
_vshadow: "dict[int, tuple]" = {}
_VSHADOW_MAX = 128


def _base_of(t: torch.Tensor) -> torch.Tensor:
    b = t._base
    return t if b is None else b


def _v_pages_of(v_codes: torch.Tensor, n_tokens: int) -> torch.Tensor:
    """Keyed on the BASE tensor of v_codes (weak reference: a new tensor at a recycled address never hits) + the shared
    version counter + the view's geometry: `store[:, :, :T]` taken afresh on every call (what DynamicPQCache.decoding(
    fused=False) and the reference's PagedPQCache pass) finds the pages made for the previous view of the same store."""
    base = _base_of(v_codes)
    key = id(base)
    sig = (v_codes._version, n_tokens, v_codes.shape, v_codes.stride(), v_codes.data_ptr())
    hit = _vshadow.get(key)
    if hit is not None and hit[0]() is base and hit[1] == sig:
        return hit[2]
    pages = transpose_v_codes(v_codes, n_tokens)
    for k in [k for k, v in _vshadow.items() if v[0]() is None]:
        del _vshadow[k]
    while len(_vshadow) >= _VSHADOW_MAX:
        del _vshadow[next(iter(_vshadow))]
    _vshadow.pop(key, None)
    _vshadow[key] = (weakref.ref(base), sig, pages)
    return pages


def _vshadow_drop(dst: torch.Tensor) -> None:
    """dst was written behind torch's back (a kernel of this library: no version bump): forget a transposed shadow of it."""
    _vshadow.pop(id(_base_of(dst)), None)


def attn_workspace(desc: L.AttnDesc, device: torch.device) -> torch.Tensor:
    lib = L.load()
    need = lib.million_attn_workspace_bytes(ctypes.byref(desc))
    # one workspace per (device, stream) serves every shape (its head does not move with the shape, million_hip.h);
    # shapes with more than 2048 (b, kv head) pairs get one of their own
    pairs = desc.bs * desc.nh_k
    key = (device.index, torch.cuda.current_stream().cuda_stream, pairs if pairs > 2048 else 0)
    ws = _ws_cache.get(key)
    if ws is None or ws.numel() < need:
        # zeroed once; every call leaves it ready.  Grown with headroom: the row-major path keeps a
        # transposed copy of the V codes here, which grows with the context.
        ws = torch.zeros(need + need // 2, dtype=torch.uint8, device=device)
        _ws_cache[key] = ws
    return ws


def make_attn_desc(q, k_res, *, nh_k, M, C, n_tokens, r, resid_start=0, k_paged=False, v_paged=False,
                   page_size=0, n_pages_cap=0, page_ids_i64=False, k_codes=None, v_codes=None,
                   dev_lengths=None, v_pages_dense=False) -> L.AttnDesc:
    bs, nh, _, d = q.shape
    desc = L.AttnDesc()
    desc.struct_size = ctypes.sizeof(L.AttnDesc)
    desc.bs, desc.nh, desc.nh_k, desc.d, desc.M, desc.C = bs, nh, nh_k, d, M, C
    desc.n_tokens, desc.r, desc.resid_start, desc.resid_cap = n_tokens, r, resid_start, k_res.shape[2]
    desc.resid_stride_b, desc.resid_stride_h = k_res.stride(0), k_res.stride(1)
    desc.k_layout = L.MILLION_KV_PAGED if k_paged else L.MILLION_KV_ROWMAJOR
    desc.v_layout = L.MILLION_KV_PAGED if v_paged else L.MILLION_KV_ROWMAJOR
    desc.page_size, desc.n_pages_cap, desc.page_ids_i64 = page_size, n_pages_cap, int(page_ids_i64)
    desc.v_pages_dense = int(v_pages_dense)
    if not k_paged and k_codes is not None:
        desc.k_stride_b, desc.k_stride_h = k_codes.stride(0), k_codes.stride(1)
    if not v_paged and v_codes is not None:
        desc.v_stride_b, desc.v_stride_h = v_codes.stride(0), v_codes.stride(1)
    desc.dev_lengths = _ptr(dev_lengths)
    # pool sizes: read only by the MILLION_DEBUG_CHECK_IDS build of the library (page ids are trusted otherwise)
    if k_paged and k_codes is not None:
        desc.k_pool_pages = k_codes.shape[0]
    if v_paged and not v_pages_dense and v_codes is not None:
        desc.v_pool_pages = v_codes.shape[0]
    return desc


def decode_workspace_bytes(q, k_res, *, nh_k, M, C, n_tokens=0, k_codes=None, v_codes=None) -> int:
    """million_attn_workspace_bytes of a decode call of this shape: what a cache allocates (zeroed) once and hands to every
    pq_decode_attn(workspace=).  Row-major stores (k_codes / v_codes) add the transposed-V scratch of n_tokens tokens."""
    desc = make_attn_desc(q, k_res, nh_k=nh_k, M=M, C=C, n_tokens=n_tokens, r=0, k_codes=k_codes, v_codes=v_codes)
    return int(L.load().million_attn_workspace_bytes(ctypes.byref(desc)))


def _check_rowmajor(name, codes, M, n_tokens):
    if codes.dim() != 4 or codes.shape[3] != M:
        raise RuntimeError(f"pq_decode_attn: {name} must be (bs, nh_k, T, M)")
    if codes.shape[2] and (codes.stride(3) != 1 or codes.stride(2) != M):
        raise RuntimeError(f"pq_decode_attn: {name} rows must be dense (stride M)")
    if n_tokens > codes.shape[2]:
        raise RuntimeError(f"pq_decode_attn: n_tokens exceeds {name}")


# ---- the checks every decode front makes (pq_decode_attn; pq_decode_attn_wide and _packed), each called where the front always made it ----
def _check_fp16_q_window(who, q, k_res, v_res):
    if q.dtype != torch.float16 or k_res.dtype != torch.float16 or v_res.dtype != torch.float16:
        raise RuntimeError(f"{who}: q and residuals must be fp16")


def _check_q_window(who, q, k_res, v_res, window_4d=False):
    """window_4d: a window that is not 4-D is refused here too (the wide fronts; pq_decode_attn has no such check)."""
    if q.dim() != 4 or q.shape[2] != 1 or not q.is_contiguous():
        raise RuntimeError(f"{who}: q must be contiguous (bs, nh, 1, d)")
    if ((window_4d and k_res.dim() != 4) or k_res.shape != v_res.shape or k_res.stride() != v_res.stride() or k_res.stride(3) != 1
            or k_res.stride(2) != k_res.shape[3]):
        raise RuntimeError(f"{who}: residual buffers must share shape/strides with dense rows")


def _new_rows(who, q, nh_k, k_new, v_new):
    """The rows of a fused append, checked and contiguous: r counts the valid rows BEFORE the call, the new row becomes row r."""
    if k_new is None or v_new is None or tuple(k_new.shape) != (q.shape[0], nh_k, 1, q.shape[3]) or v_new.shape != k_new.shape:
        raise RuntimeError(f"{who}: k_new / v_new must be (bs, nh_k, 1, d)")
    if k_new.dtype != torch.float16 or v_new.dtype != torch.float16:
        raise RuntimeError(f"{who}: k_new / v_new must be fp16")
    return k_new.contiguous(), v_new.contiguous()


def _lse_buffer(who, q, lse):
    if lse is None:
        return torch.empty(q.shape[0], q.shape[1], 1, dtype=torch.float32, device=q.device)
    if lse.dtype != torch.float32 or tuple(lse.shape) != (q.shape[0], q.shape[1], 1) or not lse.is_contiguous():
        raise RuntimeError(f"{who}: lse must be contiguous fp32 (bs, nh, 1)")
    return lse


def pq_decode_attn(q: torch.Tensor, k_codes: torch.Tensor, v_codes: torch.Tensor, k_prep: torch.Tensor,
                   v_prep: torch.Tensor, k_res: torch.Tensor, v_res: torch.Tensor, r: int, *, M: int, C: int,
                   n_tokens: Optional[int] = None, resid_start: int = 0,
                   k_page_ids: Optional[torch.Tensor] = None, v_page_ids: Optional[torch.Tensor] = None,
                   page_size: int = 0, out: Optional[torch.Tensor] = None,
                   dev_lengths: Optional[torch.Tensor] = None, workspace: Optional[torch.Tensor] = None,
                   k_new: Optional[torch.Tensor] = None, v_new: Optional[torch.Tensor] = None,
                   return_lse: bool = False, lse: Optional[torch.Tensor] = None):
    """One fused launch: score/softmax/value-reconstruct over the code store + residual window + merge.

    A side is row-major when its page ids are None: codes (bs, nh_k, T_cap, M) u8 — the reference's
    10-arg call (Interface.template.cu:26-38).  Paged: K pool (n_pool, page_size, M), V pool
    (n_pool, M, page_size), page ids (bs, nh_k, n_pages_cap) int32/int64 (paged_pq_utils.py:621-635 passes
    row-major K with paged V).

    return_lse=True (or an lse= buffer): returns (out, lse), lse fp32 (bs, nh, 1) - the natural-log sum of exp of every head's
    scaled scores over exactly the keys `out` is a softmax over (million_pq_decode_attn_lse; -inf where there is none).  Two
    results over disjoint key sets combine with attn_merge.
    """
    _need_cuda(q, k_codes, v_codes, k_prep, v_prep, k_res, v_res, k_page_ids, v_page_ids, out, dev_lengths, lse)
    _check_fp16_q_window("pq_decode_attn", q, k_res, v_res)
    if k_codes.dtype != torch.uint8 or v_codes.dtype != torch.uint8:
        raise RuntimeError("pq_decode_attn: codes must be uint8")
    _check_q_window("pq_decode_attn", q, k_res, v_res)
    nh_k = k_res.shape[1]
    k_paged, v_paged = k_page_ids is not None, v_page_ids is not None
    n_pages_cap, ids64 = 0, False
    for ids in (k_page_ids, v_page_ids):
        if ids is None:
            continue
        if ids.dtype not in (torch.int32, torch.int64) or not ids.is_contiguous() or ids.dim() != 3:
            raise RuntimeError("pq_decode_attn: page ids must be contiguous int32/int64 (bs, nh_k, n_pages)")
        if n_pages_cap and (ids.shape[2] != n_pages_cap or (ids.dtype == torch.int64) != ids64):
            raise RuntimeError("pq_decode_attn: K and V page ids must agree in dtype and length")
        n_pages_cap, ids64 = ids.shape[2], ids.dtype == torch.int64
    if n_tokens is None:
        if k_paged and v_paged:
            raise RuntimeError("pq_decode_attn: fully paged mode needs n_tokens")
        n_tokens = (v_codes if k_paged else k_codes).shape[2]
    if k_paged:
        if not k_codes.is_contiguous():
            raise RuntimeError("pq_decode_attn: K page pool must be contiguous")
    else:
        _check_rowmajor("key_codes", k_codes, M, n_tokens)
    if v_paged:
        if not v_codes.is_contiguous():
            raise RuntimeError("pq_decode_attn: V page pool must be contiguous")
    else:
        _check_rowmajor("value_codes", v_codes, M, n_tokens)
    v_dense = False
    if (not v_paged and not k_paged and n_tokens > 0 and C in (128, 256) and q.shape[3] in (64, 128) and M in (16, 32, 64)
            and dev_lengths is None):
        # the reference's 10-argument layout on the MFMA shapes (streaming and tile kernels: the whole binding surface):
        # transposed pages of V, made once per code tensor
        v_codes = _v_pages_of(v_codes, n_tokens)
        v_paged, v_dense, page_size, n_pages_cap = True, True, 64, (n_tokens + 63) // 64
    desc = make_attn_desc(q, k_res, nh_k=nh_k, M=M, C=C, n_tokens=n_tokens, r=r, resid_start=resid_start,
                          k_paged=k_paged, v_paged=v_paged, page_size=page_size, n_pages_cap=n_pages_cap,
                          page_ids_i64=ids64, k_codes=k_codes, v_codes=None if v_dense else v_codes,
                          dev_lengths=dev_lengths, v_pages_dense=v_dense)
    if out is None:
        out = torch.empty_like(q)
    ws = workspace if workspace is not None else attn_workspace(desc, q.device)
    lib = L.load()
    if k_new is not None:      # a v_new without k_new is the library's to refuse or ignore, as ever
        _need_cuda(k_new, v_new)
        k_new, v_new = _new_rows("pq_decode_attn", q, nh_k, k_new, v_new)
    if return_lse or lse is not None:
        lse = _lse_buffer("pq_decode_attn", q, lse)
        L.check(lib.million_pq_decode_attn_lse(ctypes.byref(desc), q.data_ptr(), _ptr(k_new), _ptr(v_new), _ptr(k_codes),
                                               _ptr(v_codes), _ptr(k_page_ids), _ptr(v_page_ids), k_prep.data_ptr(),
                                               v_prep.data_ptr(), k_res.data_ptr(), v_res.data_ptr(), out.data_ptr(),
                                               lse.data_ptr(), ws.data_ptr(), ws.numel(), _stream()), "million_pq_decode_attn_lse")
        return out, lse
    if k_new is not None:
        L.check(lib.million_pq_decode_attn_append(ctypes.byref(desc), q.data_ptr(), k_new.data_ptr(), v_new.data_ptr(),
                                                  _ptr(k_codes), _ptr(v_codes), _ptr(k_page_ids), _ptr(v_page_ids),
                                                  k_prep.data_ptr(), v_prep.data_ptr(), k_res.data_ptr(),
                                                  v_res.data_ptr(), out.data_ptr(), ws.data_ptr(), ws.numel(),
                                                  _stream()), "million_pq_decode_attn_append")
        return out
    L.check(lib.million_pq_decode_attn(ctypes.byref(desc), q.data_ptr(), _ptr(k_codes), _ptr(v_codes),
                                       _ptr(k_page_ids), _ptr(v_page_ids),
                                       k_prep.data_ptr(), v_prep.data_ptr(), k_res.data_ptr(), v_res.data_ptr(),
                                       out.data_ptr(), ws.data_ptr(), ws.numel(), _stream()),
            "million_pq_decode_attn")
    return out


def wide_attn_desc(who, q, k_pool, v_pool, k_cents, v_cents, k_res, v_res, r, n_tokens, page_ids, page_size, resid_start,
               dev_lengths, packed=False) -> L.AttnDesc:
    """Every check of a wide decode call that needs no library, and its descriptor.  packed: the pools hold packed pages
    (uint8 (n_pool, packed_page_bytes)); every other check is the same."""
    _need_cuda(q, k_pool, v_pool, k_cents, v_cents, k_res, v_res, page_ids, dev_lengths)
    _check_fp16_q_window(who, q, k_res, v_res)
    if packed:
        if k_pool.dtype != torch.uint8 or v_pool.dtype != torch.uint8:
            raise RuntimeError(f"{who}: packed pools must be uint8 (uint16 codes: pq_decode_attn_wide)")
    elif k_pool.dtype != torch.uint16 or v_pool.dtype != torch.uint16:
        raise RuntimeError(f"{who}: codes must be uint16 (uint8 codes: pq_decode_attn)")
    if k_cents.dtype != torch.float16 or v_cents.dtype != torch.float16 or k_cents.dim() != 3 or k_cents.shape != v_cents.shape:
        raise RuntimeError(f"{who}: k_cents / v_cents must be the plain fp16 (M, C, d_m) codebooks of one shape")
    if not k_cents.is_contiguous() or not v_cents.is_contiguous():
        raise RuntimeError(f"{who}: codebooks must be contiguous")
    _check_q_window(who, q, k_res, v_res, window_4d=True)
    M, C, dm = k_cents.shape
    if M * dm != q.shape[3]:
        raise RuntimeError(f"{who}: codebooks of {M} x {dm} dims for d={q.shape[3]}")
    if page_ids is None or page_ids.dtype not in (torch.int32, torch.int64) or not page_ids.is_contiguous() or page_ids.dim() != 3:
        raise RuntimeError(f"{who}: page_ids must be contiguous int32/int64 (bs, nh_k, n_pages)")
    if not k_pool.is_contiguous() or not v_pool.is_contiguous():
        raise RuntimeError(f"{who}: page pools must be contiguous")
    if packed:
        _check_packed_pool(who, k_pool, page_size, M, C)
        _check_packed_pool(who, v_pool, page_size, M, C)
    elif k_pool.dim() != 3 or tuple(k_pool.shape[1:]) != (page_size, M) or v_pool.dim() != 3 or tuple(v_pool.shape[1:]) != (M, page_size):
        raise RuntimeError(f"{who}: pools must be K (n_pool, page_size, M) and V (n_pool, M, page_size)")
    if dev_lengths is not None and (dev_lengths.dtype != torch.int32 or tuple(dev_lengths.shape) != (q.shape[0], 4)
                                    or not dev_lengths.is_contiguous()):
        raise RuntimeError(f"{who}: dev_lengths must be contiguous int32 (bs, 4)")
    return make_attn_desc(q, k_res, nh_k=k_res.shape[1], M=M, C=C, n_tokens=n_tokens, r=r, resid_start=resid_start, k_paged=True,
                          v_paged=True, page_size=page_size, n_pages_cap=page_ids.shape[2],
                          page_ids_i64=page_ids.dtype == torch.int64, k_codes=k_pool, v_codes=v_pool, dev_lengths=dev_lengths)


def decode_wide_workspace_bytes(q, k_res, *, M, C, page_size=64) -> int:
    """million_attn_wide_workspace_bytes of a wide decode call of this shape: what a cache allocates (zeroed) once and hands to
    every pq_decode_attn_wide(workspace=)."""
    desc = make_attn_desc(q, k_res, nh_k=k_res.shape[1], M=M, C=C, n_tokens=0, r=0, k_paged=True, v_paged=True,
                          page_size=page_size, n_pages_cap=1)
    lib = L.load()
    need = int(lib.million_attn_wide_workspace_bytes(ctypes.byref(desc)))
    if not need:      # 0: the entry refuses the shape, and has said why
        raise RuntimeError(f"decode_wide_workspace_bytes: {lib.million_last_error().decode(errors='replace')}")
    return need


def attn_wide_splits(desc: L.AttnDesc) -> int:
    """Code splits per (b, kv head) a wide decode call of this descriptor launches; -1: the entry refuses it."""
    return int(L.load().million_attn_wide_splits(ctypes.byref(desc)))


def pq_decode_attn_wide(q: torch.Tensor, k_pool: torch.Tensor, v_pool: torch.Tensor, k_cents: torch.Tensor,
                        v_cents: torch.Tensor, k_res: torch.Tensor, v_res: torch.Tensor, r: int, *, n_tokens: int,
                        page_ids: torch.Tensor, page_size: int, resid_start: int = 0, out: Optional[torch.Tensor] = None,
                        dev_lengths: Optional[torch.Tensor] = None, workspace: Optional[torch.Tensor] = None,
                        k_new: Optional[torch.Tensor] = None, v_new: Optional[torch.Tensor] = None,
                        return_lse: bool = False, lse: Optional[torch.Tensor] = None):
    """pq_decode_attn over uint16 codes (512 .. 4096 centroids): one fused launch (million_pq_decode_attn_wide) over the paged
    code store + residual window + merge, the fused append and the lse included, with pq_decode_attn's semantics.

    K pool (n_pool, page_size, M) u16, V pool (n_pool, M, page_size) u16, one page-id table (bs, nh_k, n_pages_cap) int32/int64
    for both sides; k_cents / v_cents are the plain (M, C, d_m) fp16 codebooks (there is no prepared image)."""
    return _decode_attn_wide_call("pq_decode_attn_wide", FMT_U16, q, k_pool, v_pool, k_cents, v_cents, k_res, v_res, r, n_tokens, page_ids,
                                  page_size, resid_start, out, dev_lengths, workspace, k_new, v_new, return_lse, lse)


def _decode_attn_wide_call(who, fmt, q, k_pool, v_pool, k_cents, v_cents, k_res, v_res, r, n_tokens, page_ids, page_size, resid_start,
                           out, dev_lengths, workspace, k_new, v_new, return_lse, lse):
    """pq_decode_attn_wide (FMT_U16) and pq_decode_attn_packed (FMT_PACKED): one set of checks, one workspace, the format's entry."""
    _need_cuda(out, lse, k_new, v_new, workspace)
    desc = wide_attn_desc(who, q, k_pool, v_pool, k_cents, v_cents, k_res, v_res, r, n_tokens, page_ids, page_size,
                      resid_start, dev_lengths, fmt is FMT_PACKED)
    if out is None:
        out = torch.empty_like(q)
    elif out.dtype != torch.float16 or out.numel() != q.numel() or not out.is_contiguous():
        raise RuntimeError(f"{who}: out must be contiguous fp16 of q's size")
    if k_new is not None or v_new is not None:
        k_new, v_new = _new_rows(who, q, k_res.shape[1], k_new, v_new)
    want_lse = return_lse or lse is not None
    if want_lse:
        lse = _lse_buffer(who, q, lse)
    lib = L.load()
    if workspace is None:
        need = int(getattr(lib, fmt.decode_ws)(ctypes.byref(desc)))
        key = (q.device.index, torch.cuda.current_stream().cuda_stream, "wide")
        workspace = _ws_cache.get(key)
        if workspace is None or workspace.numel() < need:      # zeroed once; every call leaves it ready (need = 0: the call is refused below)
            workspace = _ws_cache[key] = torch.zeros(max(need, 256), dtype=torch.uint8, device=q.device)
    L.check(getattr(lib, fmt.decode_attn)(ctypes.byref(desc), q.data_ptr(), _ptr(k_new), _ptr(v_new), k_pool.data_ptr(),
                                          v_pool.data_ptr(), page_ids.data_ptr(), page_ids.data_ptr(), k_cents.data_ptr(),
                                          v_cents.data_ptr(), k_res.data_ptr(), v_res.data_ptr(), out.data_ptr(), _ptr(lse),
                                          workspace.data_ptr(), workspace.numel(), _stream()), fmt.decode_attn)
    return (out, lse) if want_lse else out


# ---- packed code pages (include/million_hip.h, "Packed code pages") ----
def pq_encode_into_packed(X: torch.Tensor, cents: torch.Tensor, dst: torch.Tensor, *, layout: int, token_start: int = 0,
                          n: Optional[int] = None, page_ids: torch.Tensor = None, page_size: int = 0, x_row_start: int = 0,
                          x_row_mod: int = 0, dev_lengths: Optional[torch.Tensor] = None) -> None:
    """pq_encode_into with a packed pool as destination (million_pq_encode_packed): layout MILLION_CODES_KPAGES / VPAGES, the
    same codes bit for bit; the plain codebook (C in 512 .. 4096 has no prepared image)."""
    who = "pq_encode_into_packed"
    _need_cuda(X, cents, dst, page_ids, dev_lengths)
    if X.dtype != torch.float16 or cents.dtype != torch.float16 or cents.dim() != 3:
        raise RuntimeError(f"{who}: X and cents must be fp16, cents (M, C, d_m)")
    if X.dim() != 4 or X.stride(3) != 1:
        raise RuntimeError(f"{who}: X must be (bs, nh_k, n, d) with a contiguous last dim")
    if layout not in (L.MILLION_CODES_KPAGES, L.MILLION_CODES_VPAGES):
        raise RuntimeError(f"{who}: layout must be MILLION_CODES_KPAGES or MILLION_CODES_VPAGES (there are no packed row-major codes)")
    cents = cents.contiguous()
    M, C, dm = cents.shape
    _check_packed_pool(who, dst, page_size, M, C)
    if page_ids is None or page_ids.dtype != torch.int32 or not page_ids.is_contiguous() or page_ids.dim() != 3:
        raise RuntimeError(f"{who}: contiguous int32 page_ids (bs, nh_k, n_pages_cap) needed")
    desc = _encode_desc(X, cents, n, layout, token_start, x_row_start, x_row_mod, dev_lengths)
    desc.page_size, desc.n_pages_cap = page_size, page_ids.shape[2]
    L.check(L.load().million_pq_encode_packed(ctypes.byref(desc), X.data_ptr(), cents.data_ptr(), dst.data_ptr(), page_ids.data_ptr(),
                                              _stream()), "million_pq_encode_packed")


def pq_decode_attn_packed(q: torch.Tensor, k_pool: torch.Tensor, v_pool: torch.Tensor, k_cents: torch.Tensor,
                          v_cents: torch.Tensor, k_res: torch.Tensor, v_res: torch.Tensor, r: int, *, n_tokens: int,
                          page_ids: torch.Tensor, page_size: int, resid_start: int = 0, out: Optional[torch.Tensor] = None,
                          dev_lengths: Optional[torch.Tensor] = None, workspace: Optional[torch.Tensor] = None,
                          k_new: Optional[torch.Tensor] = None, v_new: Optional[torch.Tensor] = None,
                          return_lse: bool = False, lse: Optional[torch.Tensor] = None):
    """pq_decode_attn_wide over packed pools (million_pq_decode_attn_packed): K and V pool uint8 (n_pool, packed_page_bytes),
    everything else - arguments, checks, workspace (decode_wide_workspace_bytes), results bit for bit - as pq_decode_attn_wide."""
    return _decode_attn_wide_call("pq_decode_attn_packed", FMT_PACKED, q, k_pool, v_pool, k_cents, v_cents, k_res, v_res, r, n_tokens, page_ids,
                                  page_size, resid_start, out, dev_lengths, workspace, k_new, v_new, return_lse, lse)


def _repack(who, direction, src, side, page_size, M, C, out):
    _need_cuda(src, out)
    if side not in ("k", "v"):
        raise RuntimeError(f"{who}: side must be 'k' or 'v'")
    pb = packed_page_bytes(page_size, M, C)
    u16_shape = (page_size, M) if side == "k" else (M, page_size)
    if direction == L.MILLION_REPACK_PACK:
        if src.dtype != torch.uint16 or src.dim() != 3 or tuple(src.shape[1:]) != u16_shape or not src.is_contiguous():
            raise RuntimeError(f"{who}: pages must be contiguous uint16 (n_pages, {u16_shape[0]}, {u16_shape[1]})")
        want = (torch.uint8, (src.shape[0], pb))
    else:
        _check_packed_pool(who, src, page_size, M, C)
        want = (torch.uint16, (src.shape[0],) + u16_shape)
    if out is None:
        out = torch.empty(want[1], dtype=want[0], device=src.device)
    elif out.dtype != want[0] or tuple(out.shape) != want[1] or not out.is_contiguous():
        raise RuntimeError(f"{who}: out must be contiguous {want[0]} {want[1]}")
    L.check(L.load().million_pq_repack_pages(direction, src.data_ptr(), out.data_ptr(), src.shape[0], page_size, M, C,
                                             0 if side == "k" else 1, _stream()), "million_pq_repack_pages")
    return out


def pq_pack_pages(pages: torch.Tensor, *, side: str, C: int, out: Optional[torch.Tensor] = None) -> torch.Tensor:
    """uint16 pages -> packed pages, page for page (million_pq_repack_pages): K pages (n, page_size, M) with side="k", transposed
    V pages (n, M, page_size) with side="v" -> uint8 (n, packed_page_bytes)."""
    if pages.dim() != 3:
        raise RuntimeError("pq_pack_pages: pages must be contiguous uint16 (n_pages, page_size, M) or (n_pages, M, page_size)")
    page_size, M = (pages.shape[1], pages.shape[2]) if side == "k" else (pages.shape[2], pages.shape[1])
    return _repack("pq_pack_pages", L.MILLION_REPACK_PACK, pages, side, page_size, M, C, out)


def pq_unpack_pages(packed: torch.Tensor, *, side: str, page_size: int, M: int, C: int, out: Optional[torch.Tensor] = None) -> torch.Tensor:
    """Packed pages uint8 (n, packed_page_bytes) -> uint16 K pages (n, page_size, M) or V pages (n, M, page_size): the way of
    what reads uint16 pages only (pq_decode) to codes held in packed pages; chunk attention and pq_gather_rows read packed pages
    themselves (pq_chunk_attn_packed, pq_gather_rows(packed=True))."""
    return _repack("pq_unpack_pages", L.MILLION_REPACK_UNPACK, packed, side, page_size, M, C, out)


def prefill_attn(q: torch.Tensor, k: torch.Tensor, v: torch.Tensor, *, causal: bool = True, q_pos0: int = 0,
                 out: Optional[torch.Tensor] = None, dev_spans: Optional[torch.Tensor] = None, return_lse: bool = False,
                 lse: Optional[torch.Tensor] = None):
    """Prompt attention on fp16 K/V (million_prefill_attn): q (bs, nh, n_q, d), k / v (bs, nh_k, n_kv, d) -> (bs, nh, n_q, d).
    Replaces scaled_dot_product_attention(q, repeat_kv(k), repeat_kv(v), is_causal=True) of the reference's prompt pass
    (pq_utils.py:249-260) without materialising repeat_kv.  Row strides are free (transposed (bs, n, h, d) projections are
    fine), the d elements of a row must be contiguous.
    dev_spans: a ragged batch - int32 (bs, 4) rows {n_q, n_kv, q_pos0, reserved} on q's device, read by the kernel when it runs
    (a captured call follows them).  The tensors' n_q and n_kv are then the bounds of the padded layout, `q_pos0` is not used,
    each request attends with its own three values (clamped into the bounds); rows past a request's n_q come back as zeros, a
    request without keys as zeros, and q rows past n_q[b], K / V rows past n_kv[b] and `out` may hold anything before the call.
    return_lse (or lse=, contiguous fp32 (bs, nh, n_q)): returns (out, lse) through million_prefill_attn_lse - lse = ln sum_j
    exp(q . k_j / sqrt(d)) over the keys of the row's softmax, -inf where a row has none; `out` is bitwise the call without it.
    Parts over disjoint key ranges (non-causal over a past block, causal with q_pos0 counted from the block's first key over
    the last one) combine exactly with attn_merge."""
    if dev_spans is not None:      # first: what is wrong with the rows is said before anything about the tensors beside them
        if not isinstance(dev_spans, torch.Tensor) or dev_spans.dtype != torch.int32:
            raise RuntimeError("prefill_attn: dev_spans must be an int32 tensor")
        if q.dim() != 4 or tuple(dev_spans.shape) != (q.shape[0], 4) or not dev_spans.is_contiguous():
            raise RuntimeError(f"prefill_attn: dev_spans must be contiguous, of shape (bs, 4) = ({q.shape[0] if q.dim() == 4 else '?'}, 4)")
        if not dev_spans.is_cuda or dev_spans.device != q.device:
            raise RuntimeError("prefill_attn: dev_spans must live on the device of q (the kernel reads it there)")
    _need_cuda(q, k, v, out, lse)
    if q.dtype != torch.float16 or k.dtype != torch.float16 or v.dtype != torch.float16:
        raise RuntimeError("prefill_attn: q, k, v must be fp16")
    if q.dim() != 4 or k.dim() != 4 or k.shape != v.shape or q.shape[0] != k.shape[0] or q.shape[3] != k.shape[3]:
        raise RuntimeError(f"prefill_attn: q (bs, nh, n_q, d) and k, v (bs, nh_k, n_kv, d) expected, got {tuple(q.shape)} {tuple(k.shape)} {tuple(v.shape)}")
    bs, nh, n_q, d = q.shape
    nh_k, n_kv = k.shape[1], k.shape[2]
    if nh % nh_k:
        raise RuntimeError(f"prefill_attn: nh={nh} is not a multiple of nh_k={nh_k}")
    fix = lambda t: t if (t.stride(3) == 1 and all(s_ % 8 == 0 for s_ in t.stride()[:3])) else t.contiguous()
    q, k, v = fix(q), fix(k), fix(v)
    if out is None:
        # token-major memory under the (bs, nh, n_q, d) shape: the o_proj of a prompt pass wants (bs, n, nh * d), and
        # out.transpose(1, 2).reshape(bs, n, nh * d) is then a view instead of a copy of the whole output
        out = torch.empty(bs, n_q, nh, d, dtype=torch.float16, device=q.device).transpose(1, 2)
    elif out.shape != (bs, nh, n_q, d) or out.dtype != torch.float16 or out.stride(3) != 1:
        raise RuntimeError("prefill_attn: out must be fp16 (bs, nh, n_q, d) with contiguous rows")
    desc = L.PrefillDesc()
    desc.struct_size = ctypes.sizeof(L.PrefillDesc)
    desc.bs, desc.nh, desc.nh_k, desc.d = bs, nh, nh_k, d
    desc.n_q, desc.n_kv, desc.q_pos0, desc.causal = n_q, n_kv, q_pos0, int(causal)
    desc.q_stride_b, desc.q_stride_h, desc.q_stride_n = q.stride(0), q.stride(1), q.stride(2)
    desc.k_stride_b, desc.k_stride_h, desc.k_stride_n = k.stride(0), k.stride(1), k.stride(2)
    desc.v_stride_b, desc.v_stride_h, desc.v_stride_n = v.stride(0), v.stride(1), v.stride(2)
    desc.o_stride_b, desc.o_stride_h, desc.o_stride_n = out.stride(0), out.stride(1), out.stride(2)
    desc.dev_spans = _ptr(dev_spans)
    if return_lse or lse is not None:
        if lse is None:
            lse = torch.empty(bs, nh, n_q, dtype=torch.float32, device=q.device)
        elif lse.dtype != torch.float32 or tuple(lse.shape) != (bs, nh, n_q) or not lse.is_contiguous():
            raise RuntimeError("prefill_attn: lse must be contiguous fp32 (bs, nh, n_q)")
        L.check(L.load().million_prefill_attn_lse(ctypes.byref(desc), q.data_ptr(), k.data_ptr(), v.data_ptr(), out.data_ptr(),
                                                  lse.data_ptr(), _stream()), "million_prefill_attn_lse")
        return out, lse
    L.check(L.load().million_prefill_attn(ctypes.byref(desc), q.data_ptr(), k.data_ptr(), v.data_ptr(), out.data_ptr(), _stream()),
            "million_prefill_attn")
    return out


# ---- the reference's 10- / 13-argument calls, steady state ----------------------------------------------------------
# An unchanged reference harness calls `bindings.*` eagerly, 32 times per token (pq_utils.py:61-94); its boundary is a
# compiled pybind11 module (bindings.template.cpp:11-63).  pq_decode_attn above validates everything and rebuilds the
# descriptor on every call (~21 us of Python per call for a ~8 us kernel).  decode_attn_planned keeps, per call signature
# (shapes, strides, dtypes, device), the validated descriptor and workspace of the first call: a steady-state call is a
# signature tuple, a dict lookup, two descriptor fields, the data pointers and ONE ctypes call.
class _Plan:
    __slots__ = ("desc", "desc_ref", "ws", "ws_ptr", "ws_bytes", "v_dense", "kc", "kver", "kprep", "vc", "vver", "vprep")


_plans: "collections.OrderedDict[tuple, _Plan]" = collections.OrderedDict()      # least recently used first
_MAX_PLANS = 256


def _plan_cents(plan: _Plan, key_cents, value_cents, check):
    if plan.kc() is not key_cents or plan.kver != key_cents._version:
        if check is not None:
            check()                      # a codebook the plan has not seen: the caller's shape / dtype checks again
        plan.kprep, plan.kc, plan.kver = prepare_cents(key_cents), weakref.ref(key_cents), key_cents._version
    if value_cents is key_cents:
        return plan.kprep, plan.kprep
    if plan.vc is None or plan.vc() is not value_cents or plan.vver != value_cents._version:
        if check is not None:
            check()
        plan.vprep, plan.vc, plan.vver = prepare_cents(value_cents), weakref.ref(value_cents), value_cents._version
    return plan.kprep, plan.vprep


def _plan_signature(stream, query, key_codes, value_codes, key_residuals, value_residuals, v_page_ids, page_size, M, C):
    """Only what does NOT change from one decode step to the next is in the signature: the reference's contiguous
    (bs, nh_k, T, M) stores change their length and their batch / head strides at every flush, so those are written into the
    descriptor per call (round 3 keyed on them: every new T added a plan, and after 256 plans nothing was cached any more).
    What the signature leaves out is checked per call by _check_stores_per_call."""
    paged = v_page_ids is not None
    return (stream, query.shape, query.dtype, query.is_contiguous(), key_codes.shape[1], key_codes.stride()[2:], key_codes.dtype,
            value_codes.shape if paged else value_codes.stride()[2:], value_codes.dtype,
            key_residuals.shape, key_residuals.stride(), key_residuals.dtype, value_residuals.shape, value_residuals.stride(),
            value_residuals.dtype,
            (v_page_ids.shape, v_page_ids.dtype, v_page_ids.is_contiguous(), page_size) if paged else None,
            query.device.index, M, C)


def _check_stores_per_call(query, key_codes, value_codes, T, M, paged):
    """The T-dependent facts a cached plan cannot vouch for (the signature holds neither the stores' lengths nor their batch /
    head extents): the key store belongs to this query batch, and a row-major value store is at least as long as the key store
    it is read beside (million_transpose_v_codes reads T rows of it: a shorter store would be read out of bounds)."""
    if key_codes.dim() != 4 or key_codes.shape[0] != query.shape[0] or key_codes.shape[3] != M:
        raise RuntimeError(f"pq_decode_attn: key_codes {tuple(key_codes.shape)} do not match query batch {query.shape[0]} / M={M}")
    if not paged:
        if (value_codes.dim() != 4 or value_codes.shape[:2] != key_codes.shape[:2] or value_codes.shape[3] != M
                or value_codes.shape[2] < T):
            raise RuntimeError(f"pq_decode_attn: n_tokens exceeds value_codes (value_codes {tuple(value_codes.shape)} beside "
                               f"key_codes {tuple(key_codes.shape)})")


def decode_attn_planned(query, key_codes, value_codes, key_cents, value_cents, key_residuals, value_residuals, r, *, M, C,
                        v_page_ids=None, page_size=0, check=None):
    """The reference's production call (row-major K codes; V row-major, or a transposed page pool with page ids) with the
    per-call host work cut to the minimum.  Falls to pq_decode_attn (full validation) on the first call of a signature and
    for anything unusual (non-contiguous query, shapes off the MFMA kernels, empty store).  check: the caller's own argument
    checks, run on those slow-path calls only (a signature that passed them once passes them again: dtypes, the T-independent
    shapes and strides of every tensor are in the signature, the codebooks are identified by object and version; the stores'
    lengths and extents, which change at every flush, are checked on every call: _check_stores_per_call).
    Threads: a signature (the stream is part of it) must be driven from ONE thread at a time - the plan's descriptor is written
    per call; different streams have different plans and may be driven concurrently."""
    kshape = key_codes.shape
    T = kshape[2]
    paged = v_page_ids is not None
    stream = _stream()      # part of the signature: the workspace of a plan belongs to one (device, stream)
    # (the tuple of _plan_signature, spelled out: this is the per-call path of an eager harness - a Python call costs ~0.2 us)
    sig = (stream, query.shape, query.dtype, query.is_contiguous(), kshape[1], key_codes.stride()[2:], key_codes.dtype,
           value_codes.shape if paged else value_codes.stride()[2:], value_codes.dtype,
           key_residuals.shape, key_residuals.stride(), key_residuals.dtype, value_residuals.shape, value_residuals.stride(),
           value_residuals.dtype,
           (v_page_ids.shape, v_page_ids.dtype, v_page_ids.is_contiguous(), page_size) if paged else None,
           query.device.index, M, C)
    plan = _plans.get(sig)
    if plan is None:
        if check is not None:
            check()
        kp = prepare_cents(key_cents)
        vp = kp if value_cents is key_cents else prepare_cents(value_cents)
        out = pq_decode_attn(query.contiguous(), key_codes, value_codes, kp, vp, key_residuals, value_residuals, int(r), M=M, C=C,
                             **(dict(n_tokens=T, v_page_ids=v_page_ids.contiguous(), page_size=int(page_size)) if paged else {}))
        d = query.shape[3]
        fast_shape = (C in (128, 256) and d in (64, 128) and M in (16, 32, 64) and T > 0 and query.is_contiguous()
                      and key_codes.is_cuda and (not paged or v_page_ids.is_contiguous()))
        if fast_shape:                             # the call above has validated this signature
            while len(_plans) >= _MAX_PLANS:       # least recently used plan (and its workspace) goes
                _plans.popitem(last=False)
            plan = _Plan()
            if paged:
                plan.desc = make_attn_desc(query, key_residuals, nh_k=key_residuals.shape[1], M=M, C=C, n_tokens=T, r=int(r),
                                           k_paged=False, v_paged=True, page_size=int(page_size), n_pages_cap=v_page_ids.shape[2],
                                           page_ids_i64=v_page_ids.dtype == torch.int64, k_codes=key_codes, v_codes=value_codes)
            else:
                plan.desc = make_attn_desc(query, key_residuals, nh_k=key_residuals.shape[1], M=M, C=C, n_tokens=T, r=int(r),
                                           k_paged=False, v_paged=True, page_size=64, n_pages_cap=(T + 63) // 64,
                                           k_codes=key_codes, v_pages_dense=True)
            plan.desc_ref = ctypes.byref(plan.desc)
            plan.ws = attn_workspace(plan.desc, query.device)
            plan.ws_ptr, plan.ws_bytes = plan.ws.data_ptr(), plan.ws.numel()
            plan.v_dense = not paged
            plan.kc, plan.kver, plan.kprep = weakref.ref(key_cents), key_cents._version, kp
            plan.vc, plan.vver, plan.vprep = (None, 0, kp) if value_cents is key_cents else (weakref.ref(value_cents), value_cents._version, vp)
            _plans[sig] = plan
        return out
    try:
        _plans.move_to_end(sig)
    except KeyError:      # another thread's miss path evicted this signature between the lookup and here: the plan in hand is still valid
        pass
    # what the signature cannot vouch for (_check_stores_per_call, inlined): extents of the stores, which change at every flush
    if len(kshape) != 4 or kshape[0] != query.shape[0] or kshape[3] != M:
        _check_stores_per_call(query, key_codes, value_codes, T, M, paged)
    if not paged:
        vshape = value_codes.shape
        if len(vshape) != 4 or vshape[0] != kshape[0] or vshape[1] != kshape[1] or vshape[3] != M or vshape[2] < T:
            _check_stores_per_call(query, key_codes, value_codes, T, M, paged)
    if T <= 0:
        raise RuntimeError("decode_attn_planned: empty code store")      # (never cached: fast_shape needs T > 0)
    r = int(r)
    if not 0 <= r <= key_residuals.shape[2]:
        raise RuntimeError(f"pq_decode_attn: r={r} outside [0, {key_residuals.shape[2]}]")
    kp, vp = _plan_cents(plan, key_cents, value_cents, check)
    desc = plan.desc
    desc.n_tokens, desc.r = T, r
    desc.k_stride_b, desc.k_stride_h = key_codes.stride(0), key_codes.stride(1)      # (16-byte alignment: checked by the C entry)
    if plan.v_dense:
        desc.n_pages_cap = (T + 63) // 64
        v_ptr, ids_ptr = _v_pages_of(value_codes, T).data_ptr(), 0
    else:
        if v_page_ids.shape[2] * page_size < T:
            raise RuntimeError("pq_decode_attn: page table shorter than the key codes")
        v_ptr, ids_ptr = value_codes.data_ptr(), v_page_ids.data_ptr()
    ws_ptr, ws_bytes = plan.ws_ptr, plan.ws_bytes
    out = torch.empty_like(query)
    rc = L.load().million_pq_decode_attn(plan.desc_ref, query.data_ptr(), key_codes.data_ptr(), v_ptr, 0, ids_ptr, kp.data_ptr(),
                                         vp.data_ptr(), key_residuals.data_ptr(), value_residuals.data_ptr(), out.data_ptr(),
                                         ws_ptr, ws_bytes, stream)
    if rc:
        L.check(rc, "million_pq_decode_attn")
    return out


def residual_append(k_new: torch.Tensor, v_new: torch.Tensor, k_res: torch.Tensor, v_res: torch.Tensor, r: int,
                    resid_start: int = 0, dev_lengths: Optional[torch.Tensor] = None) -> None:
    """Write the new token's K/V rows into the residual window (replaces pq_utils.py:304-312)."""
    _need_cuda(k_new, v_new, k_res, v_res, dev_lengths)
    bs, nhk, cap, d = k_res.shape
    if k_new.shape != (bs, nhk, 1, d) or v_new.shape != (bs, nhk, 1, d):
        raise RuntimeError("residual_append: new rows must be (bs, nh_k, 1, d)")
    k_new, v_new = k_new.contiguous(), v_new.contiguous()
    lib = L.load()
    L.check(lib.million_residual_append(k_new.data_ptr(), v_new.data_ptr(), k_res.data_ptr(), v_res.data_ptr(),
                                        bs, nhk, d, cap, k_res.stride(0), k_res.stride(1), r, resid_start,
                                        _ptr(dev_lengths), _stream()), "million_residual_append")


def lengths_advance(dev_lengths: torch.Tensor, n_flushed: int, resid_cap: int) -> None:
    _need_cuda(dev_lengths)
    L.check(L.load().million_lengths_advance(dev_lengths.data_ptr(), dev_lengths.shape[0], n_flushed, resid_cap,
                                             _stream()), "million_lengths_advance")


def set_force_generic(on) -> None:
    """0 / False = auto, 1 / True = scalar fallback kernel only, 4 = auto with the merge helpers giving up at once (every give-up
    bit preset), 8 = auto with helpers that have no patience (each gives up through the real atomic path), 16 = auto, but the
    lean kernel's shapes stay on the streaming / tile kernels and nothing runs as virtual kv heads, 64 = auto, but prompt
    attention runs its plain tile loop at d = 128; any other value = auto - million_hip.h: million_set_force_generic."""
    L.load().million_set_force_generic(int(on))


def tail_faults() -> int:
    """million_debug_tail_faults: waits for the device and returns (and clears) the number of split merges that gave up waiting
    for a partial since the last call (their heads were written as NaN).  0 in every healthy run; bench.py and smoke() read it
    after their timed regions and fail on anything else.  After a non-zero answer zero the workspace again."""
    return int(L.load().million_debug_tail_faults())


def attn_kernel_kind(desc: L.AttnDesc) -> int:
    return L.load().million_attn_kernel_kind(ctypes.byref(desc))


def chunk_attn_desc(q, k_res, *, nh_k, M, C, n_tokens, r, n_c, resid_start=0, k_paged=False, v_paged=False, page_size=0,
                    n_pages_cap=0, page_ids_i64=False, k_codes=None, v_codes=None, k_chunk=None, v_chunk=None,
                    out=None, dev_lengths=None, dev_n_q=None) -> L.ChunkAttnDesc:
    bs, nh, n_q, d = q.shape
    desc = L.ChunkAttnDesc()
    desc.struct_size = ctypes.sizeof(L.ChunkAttnDesc)
    desc.bs, desc.nh, desc.nh_k, desc.d, desc.M, desc.C = bs, nh, nh_k, d, M, C
    desc.n_q, desc.n_c, desc.n_tokens, desc.r = n_q, n_c, n_tokens, r
    desc.resid_start, desc.resid_cap = resid_start, k_res.shape[2]
    desc.resid_stride_b, desc.resid_stride_h = k_res.stride(0), k_res.stride(1)
    desc.k_layout = L.MILLION_KV_PAGED if k_paged else L.MILLION_KV_ROWMAJOR
    desc.v_layout = L.MILLION_KV_PAGED if v_paged else L.MILLION_KV_ROWMAJOR
    desc.page_size, desc.n_pages_cap, desc.page_ids_i64 = page_size, n_pages_cap, int(page_ids_i64)
    if not k_paged and k_codes is not None:
        desc.k_stride_b, desc.k_stride_h = (k_codes.stride(i) * k_codes.element_size() for i in (0, 1))      # bytes
    if not v_paged and v_codes is not None:
        desc.v_stride_b, desc.v_stride_h = (v_codes.stride(i) * v_codes.element_size() for i in (0, 1))
    desc.q_stride_b, desc.q_stride_h, desc.q_stride_n = q.stride(0), q.stride(1), q.stride(2)
    if k_chunk is not None:
        desc.kc_stride_b, desc.kc_stride_h, desc.kc_stride_n = k_chunk.stride(0), k_chunk.stride(1), k_chunk.stride(2)
        desc.vc_stride_b, desc.vc_stride_h, desc.vc_stride_n = v_chunk.stride(0), v_chunk.stride(1), v_chunk.stride(2)
    if out is not None:
        desc.o_stride_b, desc.o_stride_h, desc.o_stride_n = out.stride(0), out.stride(1), out.stride(2)
    if dev_lengths is not None:
        desc.dev_lengths = dev_lengths.data_ptr()
    if dev_n_q is not None:
        desc.dev_n_q = dev_n_q.data_ptr()
    return desc


def chunk_attn_workspace_bytes(desc: L.ChunkAttnDesc) -> int:
    return int(L.load().million_chunk_attn_workspace_bytes(ctypes.byref(desc)))


def chunk_attn_wide_workspace_bytes(desc: L.ChunkAttnDesc) -> int:
    """Workspace of a pq_chunk_attn_wide call of this descriptor (chunk_attn_desc): chunk_attn_workspace_bytes' function of the
    same shape; 0 also for a descriptor the wide entry refuses."""
    return int(L.load().million_chunk_attn_wide_workspace_bytes(ctypes.byref(desc)))


def _chunk_attn_call(who, fmt, q, k_chunk, v_chunk, k_codes, v_codes, k_prep, v_prep, k_res, v_res, r, M, C, n_tokens, resid_start,
                     k_page_ids, v_page_ids, page_size, out, workspace, dev_lengths, dev_n_q, return_lse, lse):
    """pq_chunk_attn (FMT_U8: prepared codebooks), pq_chunk_attn_wide (FMT_U16: the plain codebooks in k_prep / v_prep) and
    pq_chunk_attn_packed (FMT_PACKED: pools of packed pages, plain codebooks): one set of checks, one descriptor, the entry
    point of the format."""
    _need_cuda(q, k_chunk, v_chunk, k_codes, v_codes, k_prep, v_prep, k_res, v_res, k_page_ids, v_page_ids, out, workspace,
               dev_lengths, dev_n_q, lse)
    if q.dtype != torch.float16 or k_res.dtype != torch.float16 or v_res.dtype != torch.float16:
        raise RuntimeError(f"{who}: q and window buffers must be fp16")
    if not fmt.rowmajor:
        _check_stores(who, fmt, k_codes, v_codes, k_page_ids, v_page_ids, page_size, M, C)
    elif k_codes.dtype != fmt.dtype or v_codes.dtype != fmt.dtype:
        raise RuntimeError(f"{who}: codes must be {fmt.name}" + ("" if fmt.prepared else " (uint8 codes: pq_chunk_attn)"))
    if not fmt.prepared:
        for t in (k_prep, v_prep):
            if t.dtype != torch.float16 or t.dim() != 3 or not t.is_contiguous():
                raise RuntimeError(f"{who}: k_cents / v_cents must be the plain contiguous fp16 (M, C, d_m) codebooks")
        if C not in fmt.centroids:
            raise RuntimeError(f"{who}: C={C} (one of {fmt.centroids})")
    if q.dim() != 4:
        raise RuntimeError(f"{who}: q must be (bs, nh, n_q, d)")
    bs, nh, n_q, d = q.shape
    if (k_res.dim() != 4 or k_res.shape != v_res.shape or k_res.stride() != v_res.stride() or k_res.stride(3) != 1
            or k_res.stride(2) != d or k_res.shape[0] != bs or k_res.shape[3] != d):
        raise RuntimeError(f"{who}: window buffers must be (bs, nh_k, cap, d), share shape / strides, dense rows")
    nh_k = k_res.shape[1]
    if not fmt.prepared and (M <= 0 or d % M or tuple(k_prep.shape) != (M, C, d // M) or v_prep.shape != k_prep.shape):
        raise RuntimeError(f"{who}: codebooks {tuple(k_prep.shape)} {tuple(v_prep.shape)} are not (M, C, d / M) for M={M} C={C} d={d}")
    fix = lambda t: t if (t.stride(3) == 1 and all(s_ % 8 == 0 for s_ in t.stride()[:3])) else t.contiguous()
    q = fix(q)
    n_c = 0
    if k_chunk is not None or v_chunk is not None:
        if k_chunk is None or v_chunk is None:
            raise RuntimeError(f"{who}: k_chunk and v_chunk go together")
        if k_chunk.dtype != torch.float16 or v_chunk.dtype != torch.float16:
            raise RuntimeError(f"{who}: chunk K/V must be fp16")
        if k_chunk.shape != (bs, nh_k, n_q, d) or v_chunk.shape != k_chunk.shape:
            raise RuntimeError(f"{who}: chunk K/V must be (bs, nh_k, n_q, d) = {(bs, nh_k, n_q, d)}, got "
                               f"{tuple(k_chunk.shape)} {tuple(v_chunk.shape)}")
        k_chunk, v_chunk = fix(k_chunk), fix(v_chunk)
        n_c = n_q
    n_pages_cap, ids64 = _check_page_ids(who, k_page_ids, v_page_ids, page_size, bs, nh_k, ids64_ok=True)
    if fmt.rowmajor:
        _check_stores(who, fmt, k_codes, v_codes, k_page_ids, v_page_ids, page_size, M, C, bs, nh_k, (n_tokens, "n_tokens"))
    if dev_lengths is None and not 0 <= r <= k_res.shape[2]:
        raise RuntimeError(f"{who}: r={r} outside [0, {k_res.shape[2]}]")
    for name, t, shape in (("dev_lengths", dev_lengths, (bs, 4)), ("dev_n_q", dev_n_q, (bs,))):
        if t is not None and (t.dtype != torch.int32 or not t.is_contiguous() or tuple(t.shape) != shape):
            raise RuntimeError(f"{who}: {name} must be contiguous int32 {shape}")
    if out is None:
        out = torch.empty(bs, n_q, nh, d, dtype=torch.float16, device=q.device).transpose(1, 2)
    elif out.shape != (bs, nh, n_q, d) or out.dtype != torch.float16 or out.stride(3) != 1:
        raise RuntimeError(f"{who}: out must be fp16 (bs, nh, n_q, d) with contiguous rows")
    desc = chunk_attn_desc(q, k_res, nh_k=nh_k, M=M, C=C, n_tokens=int(n_tokens), r=0 if dev_lengths is not None else int(r),
                           n_c=n_c, resid_start=int(resid_start), k_paged=k_page_ids is not None, v_paged=v_page_ids is not None,
                           page_size=int(page_size or 0), n_pages_cap=n_pages_cap, page_ids_i64=ids64, k_codes=k_codes, v_codes=v_codes,
                           k_chunk=k_chunk, v_chunk=v_chunk, out=out, dev_lengths=dev_lengths, dev_n_q=dev_n_q)
    lib = L.load()
    need = getattr(lib, fmt.chunk_ws)(ctypes.byref(desc))
    if workspace is None or workspace.numel() < need:
        workspace = torch.empty(max(need, 1), dtype=torch.uint8, device=q.device) if need else None
    want_lse = return_lse or lse is not None
    if want_lse:
        if lse is None:
            lse = torch.empty(bs, nh, n_q, dtype=torch.float32, device=q.device)
        elif lse.dtype != torch.float32 or tuple(lse.shape) != (bs, nh, n_q) or not lse.is_contiguous():
            raise RuntimeError(f"{who}: lse must be contiguous fp32 (bs, nh, n_q)")
    # one entry with an lse argument (None: no lse) - except that 8-bit codes have an entry without the argument, too
    entry = fmt.chunk_attn_lse if want_lse else fmt.chunk_attn
    lse_arg = (lse.data_ptr() if want_lse else None,) if entry == fmt.chunk_attn_lse else ()
    L.check(getattr(lib, entry)(ctypes.byref(desc), q.data_ptr(), _ptr(k_chunk), _ptr(v_chunk), k_codes.data_ptr(), v_codes.data_ptr(),
                                _ptr(k_page_ids), _ptr(v_page_ids), k_prep.data_ptr(), v_prep.data_ptr(), k_res.data_ptr(),
                                v_res.data_ptr(), out.data_ptr(), *lse_arg, _ptr(workspace),
                                0 if workspace is None else workspace.numel(), _stream()), entry)
    return (out, lse) if want_lse else out


def pq_chunk_attn(q: torch.Tensor, k_chunk: Optional[torch.Tensor], v_chunk: Optional[torch.Tensor], k_codes: torch.Tensor,
                  v_codes: torch.Tensor, k_prep: torch.Tensor, v_prep: torch.Tensor, k_res: torch.Tensor, v_res: torch.Tensor,
                  r: int, *, M: int, C: int, n_tokens: int, resid_start: int = 0, k_page_ids: Optional[torch.Tensor] = None,
                  v_page_ids: Optional[torch.Tensor] = None, page_size: Optional[int] = None, out: Optional[torch.Tensor] = None,
                  workspace: Optional[torch.Tensor] = None, dev_lengths: Optional[torch.Tensor] = None,
                  dev_n_q: Optional[torch.Tensor] = None, return_lse: bool = False, lse: Optional[torch.Tensor] = None):
    """n_q query tokens against [the PQ codes of n_tokens tokens; r window rows of the ring from resid_start; the chunk]
    (million_pq_chunk_attn): q (bs, nh, n_q, d) -> (bs, nh, n_q, d).  k_chunk / v_chunk (bs, nh_k, n_q, d): the chunk's own
    K/V, attended causally (chunked prefill, a later turn of a conversation); None: every row sees the past only (draft
    verification).  A code side is row-major (bs, nh_k, T_cap, M) when its page ids are None, else a page pool (K
    (n_pool, page_size, M), V (n_pool, M, page_size)).  q, k_chunk, v_chunk and out may be strided (rows of d contiguous
    elements); the default out is token-major under the (bs, nh, n_q, d) shape, as prefill_attn's.  Nothing is written
    but `out`: storing the chunk in the cache is the caller's (DynamicPQCache.extend / PagedPQCache.extend).
    Ragged batches: dev_lengths, device int32 (bs, 4) rows {T, r, resid_start, ticket} (a cache's `lengths[l]`), gives every
    request its own lengths, read on the device when the kernel runs: n_tokens is then only the bound the launch is sized
    for, r and resid_start are ignored; with a caller's workspace= (chunk_attn_workspace_bytes) and out= the call allocates
    nothing and can be captured into a graph.  dev_n_q, device int32 (bs,): the valid query (and chunk) rows of each
    request; the rows past them are returned as zeros and their q / chunk rows are never read into a product.
    return_lse=True (or an lse= buffer): returns (out, lse), lse fp32 (bs, nh, n_q) contiguous - the natural-log sum of exp of
    every row's scaled scores over the keys it sees (million_pq_chunk_attn_lse); -inf for a row that sees none and for the rows
    past a request's dev_n_q."""
    return _chunk_attn_call("pq_chunk_attn", FMT_U8, q, k_chunk, v_chunk, k_codes, v_codes, k_prep, v_prep, k_res, v_res, r, M, C, n_tokens, resid_start,
                            k_page_ids, v_page_ids, page_size, out, workspace, dev_lengths, dev_n_q, return_lse, lse)


def pq_chunk_attn_wide(q: torch.Tensor, k_chunk: Optional[torch.Tensor], v_chunk: Optional[torch.Tensor], k_codes: torch.Tensor,
                  v_codes: torch.Tensor, k_cents: torch.Tensor, v_cents: torch.Tensor, k_res: torch.Tensor, v_res: torch.Tensor,
                  r: int, *, M: int, C: int, n_tokens: int, resid_start: int = 0, k_page_ids: Optional[torch.Tensor] = None,
                  v_page_ids: Optional[torch.Tensor] = None, page_size: Optional[int] = None, out: Optional[torch.Tensor] = None,
                  workspace: Optional[torch.Tensor] = None, dev_lengths: Optional[torch.Tensor] = None,
                  dev_n_q: Optional[torch.Tensor] = None, return_lse: bool = False, lse: Optional[torch.Tensor] = None):
    """pq_chunk_attn over uint16 codes (C in 512 / 1024 / 2048 / 4096, d / M in {2, 4}): million_pq_chunk_attn_wide.  The same
    arguments, checks, defaults, ragged fields and lse as pq_chunk_attn, with torch.uint16 code tensors (row-major
    (bs, nh_k, T_cap, M) or page pools, per side) and k_cents / v_cents the plain contiguous fp16 (M, C, d_m) codebooks: there
    is no prepared image.  Every gathered index is code & (C - 1), so code words past n_tokens, page tails and pages no live
    entry names may hold anything.  With out=, workspace= (chunk_attn_wide_workspace_bytes) and, when asked for, lse= the call
    allocates nothing and can be captured into a graph."""
    return _chunk_attn_call("pq_chunk_attn_wide", FMT_U16, q, k_chunk, v_chunk, k_codes, v_codes, k_cents, v_cents, k_res, v_res, r, M, C, n_tokens, resid_start,
                            k_page_ids, v_page_ids, page_size, out, workspace, dev_lengths, dev_n_q, return_lse, lse)


def pq_chunk_attn_packed(q: torch.Tensor, k_chunk: Optional[torch.Tensor], v_chunk: Optional[torch.Tensor], k_codes: torch.Tensor,
                  v_codes: torch.Tensor, k_cents: torch.Tensor, v_cents: torch.Tensor, k_res: torch.Tensor, v_res: torch.Tensor,
                  r: int, *, M: int, C: int, n_tokens: int, resid_start: int = 0, k_page_ids: Optional[torch.Tensor] = None,
                  v_page_ids: Optional[torch.Tensor] = None, page_size: Optional[int] = None, out: Optional[torch.Tensor] = None,
                  workspace: Optional[torch.Tensor] = None, dev_lengths: Optional[torch.Tensor] = None,
                  dev_n_q: Optional[torch.Tensor] = None, return_lse: bool = False, lse: Optional[torch.Tensor] = None):
    """pq_chunk_attn_wide over pools of packed pages (million_pq_chunk_attn_packed): k_codes / v_codes contiguous uint8
    (n_pool, packed_page_bytes(page_size, M, C)), both page-id tensors required (there is no packed row-major format), page_size
    32 / 64 / 128.  Everything else - arguments, checks, ragged fields, lse, workspace (chunk_attn_wide_workspace_bytes) - as
    pq_chunk_attn_wide, and the result is that call's over uint16 pools holding the same codes, bit for bit."""
    return _chunk_attn_call("pq_chunk_attn_packed", FMT_PACKED, q, k_chunk, v_chunk, k_codes, v_codes, k_cents, v_cents, k_res, v_res, r, M, C, n_tokens, resid_start,
                            k_page_ids, v_page_ids, page_size, out, workspace, dev_lengths, dev_n_q, return_lse, lse)


def attn_merge(outs, lses, out: Optional[torch.Tensor] = None, lse_out: Optional[torch.Tensor] = None, return_lse: bool = False):
    """Merge of partial attentions (million_attn_merge): outs[i] fp16 (bs, nh, n_q, d) and lses[i] fp32 (bs, nh, n_q) are the
    results of one query over DISJOINT key sets (pq_decode_attn / pq_chunk_attn with return_lse); returns their softmax over
    the union - with return_lse (or an lse_out buffer) (out, lse_out).  Up to 8 parts, d 64 or 128.  The tensors may be any
    views whose rows of d are contiguous and 16-byte aligned (every other out stride a multiple of 8 elements): a transposed
    view costs no copy.  `out` may be one of the parts (same tensor view); lse_out overlaps no part's lse.  A part whose lse
    is -inf has weight 0; all of them: out 0, lse -inf; a NaN lse: the row is NaN."""
    outs, lses = list(outs), list(lses)
    P = len(outs)
    if not 1 <= P <= L.MILLION_MERGE_MAX_PARTS or len(lses) != P:
        raise RuntimeError(f"attn_merge: 1 .. {L.MILLION_MERGE_MAX_PARTS} parts, one lse per out")
    _need_cuda(*outs, *lses, out, lse_out)
    bs, nh, n_q, d = outs[0].shape
    for o, l in zip(outs, lses):
        if o.dtype != torch.float16 or tuple(o.shape) != (bs, nh, n_q, d) or (n_q and o.stride(3) != 1):
            raise RuntimeError(f"attn_merge: every out must be fp16 {(bs, nh, n_q, d)} with contiguous rows")
        if l.dtype != torch.float32 or tuple(l.shape) != (bs, nh, n_q):
            raise RuntimeError(f"attn_merge: every lse must be fp32 {(bs, nh, n_q)}")
    if out is None:
        out = torch.empty(bs, nh, n_q, d, dtype=torch.float16, device=outs[0].device)
    elif out.dtype != torch.float16 or tuple(out.shape) != (bs, nh, n_q, d) or (n_q and out.stride(3) != 1):
        raise RuntimeError("attn_merge: out must be fp16 (bs, nh, n_q, d) with contiguous rows")
    if lse_out is None and return_lse:
        lse_out = torch.empty(bs, nh, n_q, dtype=torch.float32, device=outs[0].device)
    if lse_out is not None and (lse_out.dtype != torch.float32 or tuple(lse_out.shape) != (bs, nh, n_q)):
        raise RuntimeError("attn_merge: lse_out must be fp32 (bs, nh, n_q)")
    desc = L.AttnMergeDesc()
    desc.struct_size = ctypes.sizeof(L.AttnMergeDesc)
    desc.n_parts, desc.bs, desc.nh, desc.n_q, desc.d = P, bs, nh, n_q, d
    for i, (o, l) in enumerate(zip(outs, lses)):
        for k in range(3):
            desc.out_stride[i][k], desc.lse_stride[i][k] = o.stride(k), l.stride(k)
    for k in range(3):
        desc.res_out_stride[k] = out.stride(k)
        desc.res_lse_stride[k] = lse_out.stride(k) if lse_out is not None else 0
    po = (L.c_vp * P)(*[o.data_ptr() for o in outs])
    pl = (L.c_vp * P)(*[l.data_ptr() for l in lses])
    L.check(L.load().million_attn_merge(ctypes.byref(desc), po, pl, out.data_ptr(), _ptr(lse_out), _stream()), "million_attn_merge")
    return (out, lse_out) if (return_lse or lse_out is not None) else out


def pq_gather_rows(k_codes: torch.Tensor, v_codes: torch.Tensor, k_cents: torch.Tensor, v_cents: torch.Tensor,
                   k_out: torch.Tensor, v_out: torch.Tensor, *, t0: int, t1: int, k_res: Optional[torch.Tensor] = None,
                   v_res: Optional[torch.Tensor] = None, r: int = 0, resid_start: int = 0,
                   k_page_ids: Optional[torch.Tensor] = None, v_page_ids: Optional[torch.Tensor] = None,
                   page_size: Optional[int] = None, packed: bool = False) -> int:
    """Tokens [t0, t1) of every request dequantised from its code store, then its r window rows in ring order from resid_start, as
    fp16 rows from row 0 of k_out / v_out (bs, nh_k, rows_cap, d) (million_pq_gather_rows; one launch does K and V).  Returns the
    rows written, (t1 - t0) + r; the rows behind them are not touched.  A code side is row-major (bs, nh_k, T_cap, M) when its
    page ids are None, else a page pool (K (n_pool, page_size, M), V (n_pool, M, page_size)) behind int32 ids (bs, nh_k, n_pages).
    uint8 codes with any C <= 256, uint16 codes with C in 512 / 1024 / 2048 / 4096; k_cents / v_cents are the plain contiguous
    fp16 (M, C, d_m) codebooks.  The coded rows are pq_decode's, bit for bit.  Host lengths only.  Nothing is allocated.
    packed=True (million_pq_gather_rows_packed): k_codes / v_codes are pools of packed pages, contiguous uint8
    (n_pool, packed_page_bytes(page_size, M, C)), C in 512 / 1024 / 2048 / 4096, d / M 2 or 4, both page-id tensors required; the
    rows are those of the call over the pq_unpack_pages image of the pools, bit for bit.  Without the flag a uint8 pool means
    8-bit codes, as ever."""
    _need_cuda(k_codes, v_codes, k_cents, v_cents, k_out, v_out, k_res, v_res, k_page_ids, v_page_ids)
    who = "pq_gather_rows"
    for t in (k_cents, v_cents):
        if t.dtype != torch.float16 or t.dim() != 3 or not t.is_contiguous() or t.shape != k_cents.shape:
            raise RuntimeError(f"{who}: k_cents / v_cents must be the plain contiguous fp16 (M, C, d_m) codebooks, alike")
    M, C, dm = k_cents.shape
    d = M * dm
    if not packed and k_codes.dtype != v_codes.dtype:
        raise RuntimeError(f"{who}: codes must be uint8 or uint16, both sides alike")
    fmt = code_format(who, k_codes.dtype, None if packed else C, packed)      # (packed: the pool check says a C it does not hold)
    if not fmt.rowmajor:      # the gather over packed pages is built for d / M 2 and 4
        _check_stores(who, fmt, k_codes, v_codes, k_page_ids, v_page_ids, page_size, M, C)
        if dm not in (2, 4):
            raise RuntimeError(f"{who}: d / M = {dm} over packed pages (2 or 4)")
    for t in (k_out, v_out):
        if (t.dtype != torch.float16 or t.dim() != 4 or t.shape[3] != d or t.stride(3) != 1 or t.stride(2) != d
                or t.shape != k_out.shape or t.stride() != k_out.stride()):
            raise RuntimeError(f"{who}: k_out / v_out must be fp16 (bs, nh_k, rows_cap, d = {d}) with dense rows, alike")
    bs, nh_k, rows_cap = k_out.shape[:3]
    resid_cap = 0
    if k_res is not None or v_res is not None:
        if (k_res is None or v_res is None or k_res.dtype != torch.float16 or v_res.dtype != torch.float16 or k_res.dim() != 4
                or k_res.shape != v_res.shape or k_res.stride() != v_res.stride() or k_res.stride(3) != 1 or k_res.stride(2) != d
                or k_res.shape[:2] != (bs, nh_k) or k_res.shape[3] != d):
            raise RuntimeError(f"{who}: window buffers must be fp16 (bs, nh_k, cap, d), share shape / strides, dense rows")
        resid_cap = k_res.shape[2]
    if not 0 <= r <= resid_cap:
        raise RuntimeError(f"{who}: r={r} outside [0, {resid_cap}]")
    n_pages_cap, _ = _check_page_ids(who, k_page_ids, v_page_ids, page_size, bs, nh_k, ids64_ok=False)
    if fmt.rowmajor:
        _check_stores(who, fmt, k_codes, v_codes, k_page_ids, v_page_ids, page_size, M, C, bs, nh_k, (t1, f"t1={t1}"))
    k_paged, v_paged = k_page_ids is not None, v_page_ids is not None
    desc = L.GatherRowsDesc()
    desc.struct_size = ctypes.sizeof(L.GatherRowsDesc)
    desc.bs, desc.nh_k, desc.d, desc.M, desc.C, desc.code_bytes = bs, nh_k, d, M, C, fmt.code_bytes
    desc.t0, desc.t1, desc.r, desc.resid_start, desc.resid_cap = int(t0), int(t1), int(r), int(resid_start), resid_cap
    if resid_cap:
        desc.resid_stride_b, desc.resid_stride_h = k_res.stride(0), k_res.stride(1)
    desc.k_layout = L.MILLION_KV_PAGED if k_paged else L.MILLION_KV_ROWMAJOR
    desc.v_layout = L.MILLION_KV_PAGED if v_paged else L.MILLION_KV_ROWMAJOR
    desc.page_size, desc.n_pages_cap = int(page_size or 0), n_pages_cap
    if not k_paged:
        desc.k_stride_b, desc.k_stride_h = (k_codes.stride(i) * fmt.code_bytes for i in (0, 1))      # bytes
    if not v_paged:
        desc.v_stride_b, desc.v_stride_h = (v_codes.stride(i) * fmt.code_bytes for i in (0, 1))
    desc.rows_cap, desc.o_stride_b, desc.o_stride_h = rows_cap, k_out.stride(0), k_out.stride(1)
    L.check(getattr(L.load(), fmt.gather)(ctypes.byref(desc), k_codes.data_ptr(), v_codes.data_ptr(), _ptr(k_page_ids), _ptr(v_page_ids),
                                          k_cents.data_ptr(), v_cents.data_ptr(), _ptr(k_res), _ptr(v_res), k_out.data_ptr(),
                                          v_out.data_ptr(), _stream()), fmt.gather)
    return int(t1) - int(t0) + int(r)


# ---- the block route of chunk attention: a long chunk at the prompt kernel's rate, in memory that does not grow with T ----------
# ceil(128 Ki / 7) rounded up to a multiple of 64: seven blocks and the chunk are eight parts - one merge - up to T = 128 Ki
CHUNK_BLOCK_TOKENS = 18752
CHUNK_BLOCKS_MAX_PARTS = L.MILLION_MERGE_MAX_PARTS ** 2      # two merge levels


def chunk_blocks_plan(n_tokens: int, r: int, has_chunk: bool, block_tokens: Optional[int] = None) -> dict:
    """The plan of pq_chunk_attn_blocks, a pure function of host ints.  The past [0, n_tokens) is cut into blocks of block_tokens
    (the last may be shorter); the r window rows ride behind the LAST block's rows in the scratch (alone when n_tokens = 0); the
    chunk is a part of its own.  -> {"parts": [("block", t0, t1, r_here) | ("chunk",)], "groups": [[part indices]]}: one group
    when there are at most MILLION_MERGE_MAX_PARTS (8) parts - one attn_merge into the result - else groups of up to 8 in order,
    each merged into an intermediate pair, and one more merge of those.  No part: out = 0, lse = -inf.  More than 64 parts are
    refused (RuntimeError): raise block_tokens."""
    bt = CHUNK_BLOCK_TOKENS if block_tokens is None else int(block_tokens)
    if bt < 1 or n_tokens < 0 or r < 0:
        raise RuntimeError(f"chunk_blocks_plan: n_tokens={n_tokens} r={r} block_tokens={bt}")
    parts = [("block", t0, min(t0 + bt, n_tokens), 0) for t0 in range(0, n_tokens, bt)]
    if r:
        if parts:
            parts[-1] = parts[-1][:3] + (r,)
        else:
            parts.append(("block", 0, 0, r))
    if has_chunk:
        parts.append(("chunk",))
    P = L.MILLION_MERGE_MAX_PARTS
    if len(parts) > CHUNK_BLOCKS_MAX_PARTS:
        raise RuntimeError(f"chunk_blocks_plan: {len(parts)} parts (n_tokens={n_tokens}, block_tokens={bt}) exceed {CHUNK_BLOCKS_MAX_PARTS}: "
                           "raise block_tokens")
    idx = list(range(len(parts)))
    return {"parts": parts, "groups": [idx[i:i + P] for i in range(0, len(idx), P)]}


def _chunk_blocks_layout(bs, nh, nh_k, n_q, d, resid_cap, block_tokens):
    """(total bytes, offsets) of the workspace: K scratch, V scratch, then 2 x 8 (out, lse) pairs - the parts of one group and the
    groups' results - every segment on a 256-byte boundary."""
    bt = CHUNK_BLOCK_TOKENS if block_tokens is None else int(block_tokens)
    if d not in (64, 128):
        raise RuntimeError(f"chunk_blocks_workspace_bytes: d={d} (64 or 128)")
    if min(bs, nh, nh_k) <= 0 or nh % nh_k or n_q < 0 or resid_cap < 0 or bt < 1:
        raise RuntimeError(f"chunk_blocks_workspace_bytes: bs={bs} nh={nh} nh_k={nh_k} n_q={n_q} resid_cap={resid_cap} block_tokens={bt}")
    if bt + resid_cap > 0x7fffffff or bs * nh * n_q > 0x7fffffff:
        raise RuntimeError(f"chunk_blocks_workspace_bytes: block_tokens + resid_cap = {bt + resid_cap}, bs * nh * n_q = {bs * nh * n_q} "
                           "do not fit 31 bits")
    up = lambda x: (x + 255) // 256 * 256
    P = L.MILLION_MERGE_MAX_PARTS
    scratch = up(bs * nh_k * (bt + resid_cap) * d * 2)
    o, l = up(bs * nh * n_q * d * 2), up(bs * nh * n_q * 4)
    off = {"k": 0, "v": scratch, "out": 2 * scratch, "lse": 2 * scratch + 2 * P * o, "o": o, "l": l, "rows": bt + resid_cap}
    return 2 * scratch + 2 * P * (o + l), off


def chunk_blocks_workspace_bytes(bs: int, nh: int, nh_k: int, n_q: int, d: int, resid_cap: int, block_tokens: Optional[int] = None) -> int:
    """Bytes of the workspace= of pq_chunk_attn_blocks: the fp16 K and V scratch of ONE block plus the window,
    2 * bs * nh_k * (block_tokens + resid_cap) * d * 2, and sixteen partial (out, lse) pairs of (bs, nh, n_q, d) fp16 +
    (bs, nh, n_q) fp32 (the parts of one merge group and the groups' results), each segment rounded up to 256 bytes.  A function
    of the shapes and block_tokens - never of the context length.  No initialisation is needed."""
    return _chunk_blocks_layout(bs, nh, nh_k, n_q, d, resid_cap, block_tokens)[0]


def pq_chunk_attn_blocks(q: torch.Tensor, k_chunk: Optional[torch.Tensor], v_chunk: Optional[torch.Tensor], k_codes: torch.Tensor,
                         v_codes: torch.Tensor, k_prep: torch.Tensor, v_prep: torch.Tensor, k_res: torch.Tensor, v_res: torch.Tensor,
                         r: int, *, M: int, C: int, n_tokens: int, resid_start: int = 0, k_page_ids: Optional[torch.Tensor] = None,
                         v_page_ids: Optional[torch.Tensor] = None, page_size: Optional[int] = None, out: Optional[torch.Tensor] = None,
                         workspace: Optional[torch.Tensor] = None, dev_lengths: Optional[torch.Tensor] = None,
                         dev_n_q: Optional[torch.Tensor] = None, return_lse: bool = False, lse: Optional[torch.Tensor] = None,
                         block_tokens: Optional[int] = None, packed: bool = False):
    """Chunk attention by blocks - pq_chunk_attn's meaning (n_q rows against [the codes of n_tokens tokens; r window rows; the chunk,
    causally]) and arguments, uint8 codes with prepared codebooks as pq_chunk_attn or uint16 codes with the plain codebooks as
    pq_chunk_attn_wide (the code dtype selects), served by the prompt kernel: per block of block_tokens past tokens one
    pq_gather_rows into a bounded fp16 scratch (the window behind the last block's rows) and one non-causal
    prefill_attn(return_lse=True) over it, one causal prefill_attn over k_chunk / v_chunk themselves, and attn_merge of the parts
    (chunk_blocks_plan).  For long chunks this runs at the prompt kernel's rate where the chunk kernel does not
    (profiles/chunk_blocks.txt); its transient memory, chunk_blocks_workspace_bytes, does not grow with n_tokens.
    Host lengths only: dev_lengths / dev_n_q raise.  With out=, workspace= and, when asked for, lse= the call allocates nothing
    and is a chain of launches on the current stream: it can be captured into a graph.  Each part's out is rounded to fp16
    before the merge: the result is within the attention bar of pq_chunk_attn's, not bitwise equal to it.
    packed=True: k_codes / v_codes are pools of packed pages (uint8 there cannot select: it already means prepared codebooks) and
    k_prep / v_prep the plain codebooks; the flag goes to pq_gather_rows and nothing else in the route changes, so the result is
    bitwise the uint16 route's over the same codes."""
    who = "pq_chunk_attn_blocks"
    if dev_lengths is not None or dev_n_q is not None:
        raise RuntimeError(f"{who}: host lengths only - dev_lengths / dev_n_q are pq_chunk_attn's (the chunk route)")
    _need_cuda(q, k_chunk, v_chunk, k_codes, v_codes, k_prep, v_prep, k_res, v_res, k_page_ids, v_page_ids, out, workspace, lse)
    if q.dim() != 4 or q.dtype != torch.float16:
        raise RuntimeError(f"{who}: q must be fp16 (bs, nh, n_q, d)")
    bs, nh, n_q, d = q.shape
    if k_res.dim() != 4 or k_res.shape[0] != bs or k_res.shape[3] != d or nh % k_res.shape[1]:
        raise RuntimeError(f"{who}: window buffers must be (bs, nh_k, cap, d), nh a multiple of nh_k")
    nh_k, cap = k_res.shape[1], k_res.shape[2]
    if M <= 0 or d % M:
        raise RuntimeError(f"{who}: d={d} M={M}")
    dm = d // M
    if not packed and k_codes.dtype not in (torch.uint8, torch.uint16):
        raise RuntimeError(f"{who}: codes must be uint8 (prepared codebooks) or uint16 (plain codebooks)")
    if code_format(who, k_codes.dtype, None, packed).prepared:      # prepared codebooks, as pq_chunk_attn takes them: their first image is the plain [m][c][d_m] table
        _check_prepared(who, k_prep, v_prep, M, C, d)
        k_cents, v_cents = (t.reshape(-1)[:M * C * dm].view(M, C, dm) for t in (k_prep, v_prep))
    else:      # the plain codebooks, as pq_chunk_attn_wide / pq_chunk_attn_packed take them
        k_cents, v_cents = k_prep, v_prep
    if (k_chunk is None) != (v_chunk is None):
        raise RuntimeError(f"{who}: k_chunk and v_chunk go together")
    if k_chunk is not None and (k_chunk.shape != (bs, nh_k, n_q, d) or v_chunk.shape != k_chunk.shape):
        raise RuntimeError(f"{who}: chunk K/V must be (bs, nh_k, n_q, d) = {(bs, nh_k, n_q, d)}, got {tuple(k_chunk.shape)} {tuple(v_chunk.shape)}")
    n_tokens, r = int(n_tokens), int(r)
    if not 0 <= r <= cap:
        raise RuntimeError(f"{who}: r={r} outside [0, {cap}]")
    plan = chunk_blocks_plan(n_tokens, r, k_chunk is not None, block_tokens)
    need, off = _chunk_blocks_layout(bs, nh, nh_k, n_q, d, cap, block_tokens)
    if out is None:
        out = torch.empty(bs, n_q, nh, d, dtype=torch.float16, device=q.device).transpose(1, 2)
    elif out.shape != (bs, nh, n_q, d) or out.dtype != torch.float16 or out.stride(3) != 1:
        raise RuntimeError(f"{who}: out must be fp16 (bs, nh, n_q, d) with contiguous rows")
    want_lse = return_lse or lse is not None
    if lse is not None and (lse.dtype != torch.float32 or tuple(lse.shape) != (bs, nh, n_q) or not lse.is_contiguous()):
        raise RuntimeError(f"{who}: lse must be contiguous fp32 (bs, nh, n_q)")
    if workspace is None:
        workspace = torch.empty(need, dtype=torch.uint8, device=q.device)
    elif workspace.dtype != torch.uint8 or workspace.dim() != 1 or workspace.numel() < need or workspace.data_ptr() % 256:
        raise RuntimeError(f"{who}: workspace must be a 256-byte aligned uint8 tensor of at least {need} bytes (chunk_blocks_workspace_bytes)")
    parts, groups = plan["parts"], plan["groups"]
    if n_q == 0:
        return (out, lse if lse is not None else torch.empty(bs, nh, 0, dtype=torch.float32, device=q.device)) if want_lse else out
    if lse is None and want_lse:
        lse = torch.empty(bs, nh, n_q, dtype=torch.float32, device=q.device)
    if not parts:
        out.zero_()
        if want_lse:
            lse.fill_(float("-inf"))
        return (out, lse) if want_lse else out
    P = L.MILLION_MERGE_MAX_PARTS
    kscr = workspace[off["k"]:off["k"] + bs * nh_k * off["rows"] * d * 2].view(torch.float16).view(bs, nh_k, off["rows"], d)
    vscr = workspace[off["v"]:off["v"] + bs * nh_k * off["rows"] * d * 2].view(torch.float16).view(bs, nh_k, off["rows"], d)
    slot_o = lambda i: workspace[off["out"] + i * off["o"]:off["out"] + i * off["o"] + bs * nh * n_q * d * 2].view(torch.float16).view(bs, nh, n_q, d)
    slot_l = lambda i: workspace[off["lse"] + i * off["l"]:off["lse"] + i * off["l"] + bs * nh * n_q * 4].view(torch.float32).view(bs, nh, n_q)

    def run_part(part, o, l):
        if part[0] == "chunk":
            prefill_attn(q, k_chunk, v_chunk, causal=True, out=o, lse=l)
            return
        _, t0, t1, r_here = part
        n = pq_gather_rows(k_codes, v_codes, k_cents, v_cents, kscr, vscr, t0=t0, t1=t1, k_res=k_res, v_res=v_res, r=r_here,
                           resid_start=resid_start if r_here else 0, k_page_ids=k_page_ids, v_page_ids=v_page_ids, page_size=page_size,
                           **({"packed": True} if packed else {}))
        prefill_attn(q, kscr[:, :, :n], vscr[:, :, :n], causal=False, out=o, lse=l)

    if len(parts) == 1:      # one part is the result
        l = lse if lse is not None else slot_l(0)
        run_part(parts[0], out, l)
        return (out, lse) if want_lse else out
    tops_o, tops_l = [], []
    for g, group in enumerate(groups):
        res_o, res_l = (out, lse) if len(groups) == 1 else (slot_o(P + g), slot_l(P + g))
        if len(group) == 1:      # a last group of one part is its own result
            run_part(parts[group[0]], res_o, res_l)
        else:
            for j, i in enumerate(group):
                run_part(parts[i], slot_o(j), slot_l(j))
            attn_merge([slot_o(j) for j in range(len(group))], [slot_l(j) for j in range(len(group))], out=res_o, lse_out=res_l)
        if len(groups) == 1:
            return (out, lse) if want_lse else out
        tops_o.append(res_o)
        tops_l.append(res_l)
    attn_merge(tops_o, tops_l, out=out, lse_out=lse)
    return (out, lse) if want_lse else out


def attn_block_merge(q: torch.Tensor, k_blk: torch.Tensor, v_blk: torch.Tensor, out_a: torch.Tensor, lse_a: torch.Tensor,
                     dev_n: Optional[torch.Tensor] = None, out: Optional[torch.Tensor] = None, lse_out: Optional[torch.Tensor] = None,
                     return_lse: bool = False, k_stage: Optional[torch.Tensor] = None, v_stage: Optional[torch.Tensor] = None,
                     dev_mask: Optional[torch.Tensor] = None):
    """Finish the attention of n <= 16 draft rows per request in one launch (million_attn_block_merge): (out_a, lse_a), fp16
    (bs, nh, n, d) and fp32 (bs, nh, n) contiguous, is every row's attention over the past (pq_decode_attn over the rows as query
    heads, or pq_chunk_attn without a chunk, with return_lse); row i then attends causally to the block's own rows j <= i of
    k_blk / v_blk (bs, nh_k, n, d) and the two parts are merged as attn_merge merges them.  q, k_blk, v_blk, out_a and out may be
    any views with contiguous rows of d and the other strides multiples of 8 elements; `out` may be out_a itself.  dev_n, device
    int32 (bs,): the live rows of each request, clamped into [0, n]; the rows past them get out = 0 and lse = -inf and their q /
    k / v never reach a live row.  k_stage / v_stage, fp16 (bs, nh_k, >= n, d) with dense rows: the launch copies the block rows
    there (window_commit reads them).  dev_mask, device int32 (bs, n) contiguous: the draft is a tree in topological order and
    bit j of word (b, i) says that row i sees block row j (million_attn_tree_merge); the kernel keeps bits 0 .. i and sets bit i,
    whatever the word holds.  None: the chain, million_attn_block_merge.  Returns out, or (out, lse_out) with return_lse (or an
    lse_out buffer)."""
    _need_cuda(q, k_blk, v_blk, out_a, lse_a, dev_n, out, lse_out, k_stage, v_stage, dev_mask)
    if q.dim() != 4 or any(t.dtype != torch.float16 for t in (q, k_blk, v_blk, out_a)):
        raise RuntimeError("attn_block_merge: q, k_blk, v_blk and out_a must be fp16 (bs, nh | nh_k, n, d)")
    bs, nh, n, d = q.shape
    if k_blk.dim() != 4 or k_blk.shape[0] != bs or k_blk.shape[2:] != (n, d) or v_blk.shape != k_blk.shape or nh % k_blk.shape[1]:
        raise RuntimeError(f"attn_block_merge: k_blk / v_blk must be (bs, nh_k, n, d) = ({bs}, nh_k, {n}, {d}), nh a multiple of nh_k")
    nh_k = k_blk.shape[1]
    fix = lambda t: t if (t.stride(3) == 1 and all(s_ % 8 == 0 for s_ in t.stride()[:3])) else t.contiguous()
    q, k_blk, v_blk = fix(q), fix(k_blk), fix(v_blk)
    if tuple(out_a.shape) != (bs, nh, n, d) or out_a.stride(3) != 1:
        raise RuntimeError("attn_block_merge: out_a must be (bs, nh, n, d) with contiguous rows")
    if lse_a.dtype != torch.float32 or tuple(lse_a.shape) != (bs, nh, n) or not lse_a.is_contiguous():
        raise RuntimeError("attn_block_merge: lse_a must be contiguous fp32 (bs, nh, n)")
    if dev_n is not None:
        _check_dev_n("attn_block_merge", dev_n, bs)
    if out is None:
        out = torch.empty(bs, nh, n, d, dtype=torch.float16, device=q.device)
    elif out.dtype != torch.float16 or tuple(out.shape) != (bs, nh, n, d) or out.stride(3) != 1:
        raise RuntimeError("attn_block_merge: out must be fp16 (bs, nh, n, d) with contiguous rows")
    if lse_out is None and return_lse:
        lse_out = torch.empty(bs, nh, n, dtype=torch.float32, device=q.device)
    if lse_out is not None and (lse_out.dtype != torch.float32 or tuple(lse_out.shape) != (bs, nh, n) or not lse_out.is_contiguous()):
        raise RuntimeError("attn_block_merge: lse_out must be contiguous fp32 (bs, nh, n)")
    if (k_stage is None) != (v_stage is None):
        raise RuntimeError("attn_block_merge: k_stage and v_stage go together")
    desc = L.BlockMergeDesc()
    desc.struct_size = ctypes.sizeof(L.BlockMergeDesc)
    desc.bs, desc.nh, desc.nh_k, desc.n, desc.d = bs, nh, nh_k, n, d
    for k in range(3):
        desc.q_stride[k], desc.k_stride[k], desc.v_stride[k] = q.stride(k), k_blk.stride(k), v_blk.stride(k)
        desc.a_stride[k], desc.o_stride[k] = out_a.stride(k), out.stride(k)
    if k_stage is not None:
        for t in (k_stage, v_stage):
            if (t.dtype != torch.float16 or t.dim() != 4 or t.shape[:2] != (bs, nh_k) or t.shape[2] < n or t.shape[3] != d
                    or t.stride(3) != 1 or t.stride(2) != d or t.stride() != k_stage.stride()):
                raise RuntimeError("attn_block_merge: k_stage / v_stage must be fp16 (bs, nh_k, >= n, d) with dense rows, alike")
        desc.stage_stride_b, desc.stage_stride_h = k_stage.stride(0), k_stage.stride(1)
    if dev_mask is not None:
        if dev_mask.dtype != torch.int32 or tuple(dev_mask.shape) != (bs, n) or not dev_mask.is_contiguous() or dev_mask.device != q.device:
            raise RuntimeError(f"attn_block_merge: dev_mask must be contiguous int32 (bs, n) = ({bs}, {n}) on the device of q")
        L.check(L.load().million_attn_tree_merge(ctypes.byref(desc), q.data_ptr(), k_blk.data_ptr(), v_blk.data_ptr(), out_a.data_ptr(),
                                                 lse_a.data_ptr(), _ptr(dev_n), dev_mask.data_ptr(), out.data_ptr(), _ptr(lse_out),
                                                 _ptr(k_stage), _ptr(v_stage), _stream()), "million_attn_tree_merge")
        return (out, lse_out) if (return_lse or lse_out is not None) else out
    L.check(L.load().million_attn_block_merge(ctypes.byref(desc), q.data_ptr(), k_blk.data_ptr(), v_blk.data_ptr(), out_a.data_ptr(),
                                              lse_a.data_ptr(), _ptr(dev_n), out.data_ptr(), _ptr(lse_out), _ptr(k_stage),
                                              _ptr(v_stage), _stream()), "million_attn_block_merge")
    return (out, lse_out) if (return_lse or lse_out is not None) else out


SINK_MAX_ROWS = 64


def attn_sink_merge(q: torch.Tensor, k_sink: torch.Tensor, v_sink: torch.Tensor, out_a: torch.Tensor, lse_a: torch.Tensor, *,
                    n_sink: Optional[int] = None, dev_s: Optional[torch.Tensor] = None, dev_n: Optional[torch.Tensor] = None,
                    out: Optional[torch.Tensor] = None, lse_out: Optional[torch.Tensor] = None, return_lse: bool = False):
    """Attend n query rows per (b, head) to the exact fp16 sink rows of their request and merge that with their attention over
    the past, in one launch (million_attn_sink_merge): (out_a, lse_a), fp16 (bs, nh, n, d) and contiguous fp32 (bs, nh, n), is a
    decode / chunk / verify result with its lse; k_sink / v_sink are fp16 (bs, nh_k, s_cap <= 64, d) with dense rows.  Every
    live sink row is visible to every query row.  The live rows of request b: dev_s[b] (device int32 (bs,), clamped into
    [0, s_cap] on the device), or n_sink for all (a host int; default s_cap); not both.  dev_n, device int32 (bs,): the live
    query rows, clamped into [0, n]; the rows past them get out = 0 and lse = -inf.  Zero sink rows are the identity on
    (out_a, lse_a), bit for bit.  q, out_a and out may be any views with contiguous rows of d and the other strides multiples
    of 8 elements; `out` may be out_a itself.  Returns out, or (out, lse_out) with return_lse (or an lse_out buffer)."""
    _need_cuda(q, k_sink, v_sink, out_a, lse_a, dev_s, dev_n, out, lse_out)
    if q.dim() != 4 or any(t.dtype != torch.float16 for t in (q, k_sink, v_sink, out_a)):
        raise RuntimeError("attn_sink_merge: q, k_sink, v_sink and out_a must be fp16 (bs, nh | nh_k, n | s_cap, d)")
    bs, nh, n, d = q.shape
    if (k_sink.dim() != 4 or k_sink.shape[0] != bs or k_sink.shape[3] != d or v_sink.shape != k_sink.shape or nh % k_sink.shape[1]
            or not 1 <= k_sink.shape[2] <= SINK_MAX_ROWS):
        raise RuntimeError(f"attn_sink_merge: k_sink / v_sink must be (bs, nh_k, s_cap, d) = ({bs}, nh_k, 1 .. {SINK_MAX_ROWS}, {d}), "
                           "nh a multiple of nh_k")
    nh_k, s_cap = k_sink.shape[1], k_sink.shape[2]
    for t in (k_sink, v_sink):
        if t.stride(3) != 1 or t.stride(2) != d or t.stride() != k_sink.stride():
            raise RuntimeError("attn_sink_merge: k_sink / v_sink must have dense rows (row stride d), alike")
    if dev_s is not None and n_sink is not None:
        raise RuntimeError("attn_sink_merge: n_sink (host) or dev_s (device), not both")
    if dev_s is not None:
        _check_dev_n("attn_sink_merge", dev_s, bs)
    n_sink = (0 if dev_s is not None else s_cap) if n_sink is None else int(n_sink)
    if not 0 <= n_sink <= s_cap:
        raise RuntimeError(f"attn_sink_merge: n_sink={n_sink} outside [0, {s_cap}]")
    fix = lambda t: t if (t.stride(3) == 1 and all(s_ % 8 == 0 for s_ in t.stride()[:3])) else t.contiguous()
    q = fix(q)
    if tuple(out_a.shape) != (bs, nh, n, d) or out_a.stride(3) != 1:
        raise RuntimeError("attn_sink_merge: out_a must be (bs, nh, n, d) with contiguous rows")
    if lse_a.dtype != torch.float32 or tuple(lse_a.shape) != (bs, nh, n) or not lse_a.is_contiguous():
        raise RuntimeError("attn_sink_merge: lse_a must be contiguous fp32 (bs, nh, n)")
    if dev_n is not None:
        _check_dev_n("attn_sink_merge", dev_n, bs)
    if out is None:
        out = torch.empty(bs, nh, n, d, dtype=torch.float16, device=q.device)
    elif out.dtype != torch.float16 or tuple(out.shape) != (bs, nh, n, d) or out.stride(3) != 1:
        raise RuntimeError("attn_sink_merge: out must be fp16 (bs, nh, n, d) with contiguous rows")
    if lse_out is None and return_lse:
        lse_out = torch.empty(bs, nh, n, dtype=torch.float32, device=q.device)
    if lse_out is not None and (lse_out.dtype != torch.float32 or tuple(lse_out.shape) != (bs, nh, n) or not lse_out.is_contiguous()):
        raise RuntimeError("attn_sink_merge: lse_out must be contiguous fp32 (bs, nh, n)")
    desc = L.SinkMergeDesc()
    desc.struct_size = ctypes.sizeof(L.SinkMergeDesc)
    desc.bs, desc.nh, desc.nh_k, desc.n, desc.d, desc.s_cap, desc.n_sink = bs, nh, nh_k, n, d, s_cap, n_sink
    for k in range(3):
        desc.q_stride[k], desc.a_stride[k], desc.o_stride[k] = q.stride(k), out_a.stride(k), out.stride(k)
    desc.sink_stride_b, desc.sink_stride_h = k_sink.stride(0), k_sink.stride(1)
    L.check(L.load().million_attn_sink_merge(ctypes.byref(desc), q.data_ptr(), k_sink.data_ptr(), v_sink.data_ptr(), out_a.data_ptr(),
                                             lse_a.data_ptr(), _ptr(dev_s), _ptr(dev_n), out.data_ptr(), _ptr(lse_out), _stream()),
            "million_attn_sink_merge")
    return (out, lse_out) if (return_lse or lse_out is not None) else out


def window_commit(k_new: torch.Tensor, v_new: torch.Tensor, k_res: torch.Tensor, v_res: torch.Tensor, k_prep: torch.Tensor,
                  v_prep: torch.Tensor, k_pool: torch.Tensor, v_pool: torch.Tensor, page_ids: torch.Tensor,
                  dev_lengths: torch.Tensor, dev_n: torch.Tensor, *, M: int, C: int, n_bound: Optional[int] = None,
                  dev_rows: Optional[torch.Tensor] = None) -> None:
    """Append the first dev_n[b] rows of k_new / v_new (layers, bs, nh_k, n, d) to request b's window in every layer, exactly as
    that many decode steps would have (million_window_commit): a request whose window would overflow first has its oldest
    page_size rows - window rows in ring order, then new rows - encoded behind its T tokens (the codes pq_flush writes), the
    rest of the new rows go to the ring, and the rows of dev_lengths (layers, bs, 4) advance on the device.  k_res / v_res
    (layers, bs, nh_k, cap, d), page_ids (layers, bs, nh_k, n_pages_cap): the layers of one cache side by side, as cache_fork
    takes them; dev_n int32 (bs,) serves every layer.  n_bound (default n): the rows the grids are sized for, at most 16 and at
    most page_size; dev_n is clamped into [0, n_bound].  dev_rows, device int32 (bs, n_bound) contiguous: the dev_n[b] new rows
    of request b are rows dev_rows[b][0 .. dev_n[b]) of k_new / v_new, in that order (million_window_commit_rows: the accepted
    path of a draft tree); an index is clamped into [0, n_bound).  None: the first dev_n[b] rows, million_window_commit."""
    _need_cuda(k_new, v_new, k_res, v_res, k_prep, v_prep, k_pool, v_pool, page_ids, dev_lengths, dev_n, dev_rows)
    if k_new.dtype != torch.float16 or v_new.dtype != torch.float16 or k_new.dim() != 5 or v_new.shape != k_new.shape or \
            k_new.stride() != v_new.stride() or k_new.stride(4) != 1:
        raise RuntimeError("window_commit: k_new / v_new must be fp16 (layers, bs, nh_k, n, d) of one shape and strides, contiguous rows")
    n_layers, bs, nhk, n_rows, d = k_new.shape
    n_bound = n_rows if n_bound is None else int(n_bound)
    if n_bound > n_rows:
        raise RuntimeError(f"window_commit: n_bound={n_bound} exceeds the {n_rows} rows of k_new")
    if page_ids.dtype != torch.int32 or page_ids.dim() != 4 or page_ids.shape[:3] != (n_layers, bs, nhk) or not page_ids[0].is_contiguous():
        raise RuntimeError("window_commit: int32 page_ids (layers, bs, nh_k, n_pages_cap), each layer contiguous, expected")
    if (k_pool.dtype != torch.uint8 or v_pool.dtype != torch.uint8 or k_pool.dim() != 3 or not k_pool.is_contiguous() or not v_pool.is_contiguous()
            or v_pool.shape != (k_pool.shape[0], k_pool.shape[2], k_pool.shape[1]) or k_pool.shape[2] != M):
        raise RuntimeError("window_commit: contiguous uint8 pools (n_pool, page_size, M) and (n_pool, M, page_size) expected")
    n_pool, page_size, _ = k_pool.shape
    if (k_res.dtype != torch.float16 or v_res.dtype != torch.float16 or k_res.dim() != 5 or k_res.shape != v_res.shape or k_res.stride() != v_res.stride()
            or k_res.shape[:3] != (n_layers, bs, nhk) or k_res.shape[4] != d or not k_res[0].is_contiguous()):
        raise RuntimeError("window_commit: fp16 windows (layers, bs, nh_k, cap, d), each layer contiguous, K and V alike, expected")
    if dev_lengths.dtype != torch.int32 or dev_lengths.shape != (n_layers, bs, 4) or not dev_lengths[0].is_contiguous():
        raise RuntimeError("window_commit: int32 dev_lengths (layers, bs, 4) expected")
    _check_dev_n("window_commit", dev_n, bs)
    _check_prepared("window_commit", k_prep, v_prep, M, C, d)
    desc = L.WindowCommitDesc()
    desc.struct_size = ctypes.sizeof(L.WindowCommitDesc)
    desc.n_layers, desc.bs, desc.nh_k, desc.d, desc.M, desc.C, desc.n_bound = n_layers, bs, nhk, d, M, C, n_bound
    desc.page_size, desc.n_pages_cap, desc.n_pool, desc.resid_cap = page_size, page_ids.shape[3], n_pool, k_res.shape[3]
    desc.new_stride_l, desc.new_stride_b, desc.new_stride_h, desc.new_stride_n = k_new.stride()[:4]
    desc.ids_layer_stride, desc.rows_layer_stride, desc.lengths_layer_stride = page_ids.stride(0), k_res.stride(0), dev_lengths.stride(0)
    if dev_rows is not None:
        if dev_rows.dtype != torch.int32 or tuple(dev_rows.shape) != (bs, n_bound) or not dev_rows.is_contiguous() or dev_rows.device != k_new.device:
            raise RuntimeError(f"window_commit: dev_rows must be contiguous int32 (bs, n_bound) = ({bs}, {n_bound}) on the device of k_new")
        L.check(getattr(L.load(), FMT_U8.commit_rows)(ctypes.byref(desc), k_new.data_ptr(), v_new.data_ptr(), k_res.data_ptr(), v_res.data_ptr(),
                                                      k_prep.data_ptr(), v_prep.data_ptr(), k_pool.data_ptr(), v_pool.data_ptr(),
                                                      page_ids.data_ptr(), dev_lengths.data_ptr(), dev_n.data_ptr(), dev_rows.data_ptr(),
                                                      _stream()), FMT_U8.commit_rows)
        _vshadow_drop(v_pool)
        return
    L.check(getattr(L.load(), FMT_U8.commit)(ctypes.byref(desc), k_new.data_ptr(), v_new.data_ptr(), k_res.data_ptr(), v_res.data_ptr(),
                                             k_prep.data_ptr(), v_prep.data_ptr(), k_pool.data_ptr(), v_pool.data_ptr(),
                                             page_ids.data_ptr(), dev_lengths.data_ptr(), dev_n.data_ptr(), _stream()),
            FMT_U8.commit)
    _vshadow_drop(v_pool)


def window_commit_wide(k_new: torch.Tensor, v_new: torch.Tensor, k_res: torch.Tensor, v_res: torch.Tensor, k_cents: torch.Tensor,
                       v_cents: torch.Tensor, k_pool: torch.Tensor, v_pool: torch.Tensor, page_ids: torch.Tensor,
                       dev_lengths: torch.Tensor, dev_n: torch.Tensor, *, n_bound: Optional[int] = None, packed: bool = False,
                       dev_rows: Optional[torch.Tensor] = None) -> None:
    """window_commit for codes of 512 .. 4096 centroids (million_window_commit_wide / million_window_commit_rows_wide): the same
    call with the same meaning - the first dev_n[b] rows (dev_rows: the chosen rows) of k_new / v_new (layers, bs, nh_k, n, d) join
    request b's window in every layer as that many decode steps would have, a window they overflow flushing its oldest page_size
    rows first - into uint16 pages (K (n_pool, page_size, M), V (n_pool, M, page_size)) or, packed=True, packed pages (uint8
    (n_pool, packed_page_bytes)), with the codebooks as they are (fp16 (M, C, d_m)) in place of the prepared ones.  The codes are
    pq_encode_into's / pq_encode_into_packed's bit for bit."""
    who = "window_commit_wide"
    _need_cuda(k_new, v_new, k_res, v_res, k_cents, v_cents, k_pool, v_pool, page_ids, dev_lengths, dev_n, dev_rows)
    if k_new.dtype != torch.float16 or v_new.dtype != torch.float16 or k_new.dim() != 5 or v_new.shape != k_new.shape or \
            k_new.stride() != v_new.stride() or k_new.stride(4) != 1:
        raise RuntimeError(f"{who}: k_new / v_new must be fp16 (layers, bs, nh_k, n, d) of one shape and strides, contiguous rows")
    n_layers, bs, nhk, n_rows, d = k_new.shape
    n_bound = n_rows if n_bound is None else int(n_bound)
    if n_bound > n_rows:
        raise RuntimeError(f"{who}: n_bound={n_bound} exceeds the {n_rows} rows of k_new")
    if page_ids.dtype != torch.int32 or page_ids.dim() != 4 or page_ids.shape[:3] != (n_layers, bs, nhk) or not page_ids[0].is_contiguous():
        raise RuntimeError(f"{who}: int32 page_ids (layers, bs, nh_k, n_pages_cap), each layer contiguous, expected")
    if (k_res.dtype != torch.float16 or v_res.dtype != torch.float16 or k_res.dim() != 5 or k_res.shape != v_res.shape or k_res.stride() != v_res.stride()
            or k_res.shape[:3] != (n_layers, bs, nhk) or k_res.shape[4] != d or not k_res[0].is_contiguous()):
        raise RuntimeError(f"{who}: fp16 windows (layers, bs, nh_k, cap, d), each layer contiguous, K and V alike, expected")
    k_cents, v_cents = k_cents.contiguous(), v_cents.contiguous()
    if packed:      # a packed pool has no page_size axis: the one size whose page has the pool's bytes (page bytes grow with the size)
        sizes = [ps for ps in (32, 64, 128) if k_pool.dim() == 2 and k_cents.dim() == 3 and k_cents.shape[1] in WIDE_CENTROIDS
                 and k_pool.shape[1] == packed_page_bytes(ps, k_cents.shape[0], k_cents.shape[1])]
        if not sizes:
            raise RuntimeError(f"{who}: a packed pool must be contiguous uint8 (n_pool, packed_page_bytes) for page_size 32, 64 or 128")
        page_size = sizes[0]
    else:
        if k_pool.dim() != 3:
            raise RuntimeError(f"{who}: pools must be K (n_pool, page_size, M) and V (n_pool, M, page_size)")
        page_size = k_pool.shape[1]
    fmt, M, C = _check_wide_pools(who, k_cents, v_cents, k_pool, v_pool, page_size, bs, nhk, d, packed)      # the format names the entries
    if k_pool.shape[0] != v_pool.shape[0]:
        raise RuntimeError(f"{who}: K and V pools of one page count expected")
    if dev_lengths.dtype != torch.int32 or dev_lengths.shape != (n_layers, bs, 4) or not dev_lengths[0].is_contiguous():
        raise RuntimeError(f"{who}: int32 dev_lengths (layers, bs, 4) expected")
    _check_dev_n(who, dev_n, bs)
    desc = L.WindowCommitDesc()
    desc.struct_size = ctypes.sizeof(L.WindowCommitDesc)
    desc.n_layers, desc.bs, desc.nh_k, desc.d, desc.M, desc.C, desc.n_bound = n_layers, bs, nhk, d, M, C, n_bound
    desc.page_size, desc.n_pages_cap, desc.n_pool, desc.resid_cap = page_size, page_ids.shape[3], k_pool.shape[0], k_res.shape[3]
    desc.new_stride_l, desc.new_stride_b, desc.new_stride_h, desc.new_stride_n = k_new.stride()[:4]
    desc.ids_layer_stride, desc.rows_layer_stride, desc.lengths_layer_stride = page_ids.stride(0), k_res.stride(0), dev_lengths.stride(0)
    args = (ctypes.byref(desc), k_new.data_ptr(), v_new.data_ptr(), k_res.data_ptr(), v_res.data_ptr(), k_cents.data_ptr(), v_cents.data_ptr(),
            k_pool.data_ptr(), v_pool.data_ptr(), page_ids.data_ptr(), dev_lengths.data_ptr(), dev_n.data_ptr())
    if dev_rows is not None:
        if dev_rows.dtype != torch.int32 or tuple(dev_rows.shape) != (bs, n_bound) or not dev_rows.is_contiguous() or dev_rows.device != k_new.device:
            raise RuntimeError(f"{who}: dev_rows must be contiguous int32 (bs, n_bound) = ({bs}, {n_bound}) on the device of k_new")
        L.check(getattr(L.load(), fmt.commit_rows)(*args, dev_rows.data_ptr(), int(bool(packed)), _stream()), fmt.commit_rows)
        return
    L.check(getattr(L.load(), fmt.commit)(*args, int(bool(packed)), _stream()), fmt.commit)
