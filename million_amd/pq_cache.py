"""Host-side mirror of the reference's KV-cache objects for the PQ-KV hot path.

Same names, constructor arguments and method meaning as the reference (scripts/utils/pq_utils.py:98-408
DynamicPQCache, scripts/utils/paged_pq_utils.py:10-397 PagedPQCache, scripts/utils/
dynamic_paged_pq_utils.py:10-321 PageManager, pq_utils.py:8-96 l2Ns / KernelRegistry), re-designed for
MI355X:

  * storage is PREALLOCATED (288 GB HBM): no torch.cat growth (pq_utils.py:145-146 reallocates O(T) per
    flush), no per-step pad/transpose of all V codes (paged_pq_utils.py:464-486);
  * the encode kernel writes codes straight into their final place (row-major store, K pages,
    transposed V pages);
  * the residual window is a ring buffer: a flush advances `resid_start`, nothing is shifted
    (paged_pq_utils.py:188-204 clones and copies the survivors);
  * lengths live on the device as well (int32 (bs, 4) = {n_tokens, r, resid_start, 0}) so a whole decode
    step can be captured in one hipGraph and replayed while the lengths change;
  * no global singletons (reference: metaclass Singleton), no exit(), no silent fallbacks: errors raise.

[QUIRK]s of the reference that are NOT reproduced: seen_tokens double counting on flush
(paged_pq_utils.py:208), page pool built from batch 0 / head 0 only (:457), causal mask with one query
row in the fallback (:888), the nested try/except fallbacks.
"""
from __future__ import annotations

import heapq
from typing import Dict, List, Optional, Set

import numpy as np
import torch

from . import _lib as L
from . import ops
from . import spec_tree


def l2Ns(l: int) -> int:
    """Split-count heuristic of the reference (pq_utils.py:8-22).  Only selects the binding NAME here:
    the HIP kernel sizes its own split count from the CU count."""
    if l > 2048:
        return 32
    if l > 256:
        return 16
    if l > 128:
        return 4
    if l > 64:
        return 2
    return 1


def scalarTypeToStr(scalar_t) -> str:
    if scalar_t == torch.float16:
        return "f16"
    if scalar_t == torch.float32:
        return "f32"
    raise ValueError(f"Unknown scalar type: {scalar_t}")


def nbits2dtype(nbits: int):
    """pq_utils.py:542-552."""
    if nbits <= 8:
        return torch.uint8
    if nbits <= 16:
        return torch.uint16
    if nbits <= 32:
        return torch.uint32
    if nbits <= 64:
        return torch.uint64
    raise ValueError("nbits must be <= 64")


class KernelRegistry:
    """pq_utils.py:32-96: resolves `bindings.flash_decoding_allocated_buffer_{T}u8_Ns{Ns}Lt{d}d{d}M{M}C{C}`
    by name and owns the (unused by the HIP path, but part of the signature) partial buffers."""

    def __init__(self, *, M=64, d=128, nbits=8, nh=32, scalar_t=torch.float16, device="cuda"):
        self.kernels, self.partial_out_buffers, self.partial_lse_buffers = {}, {}, {}
        self.M, self.d, self.nbits, self.nh, self.scalar_t, self.device = M, d, nbits, nh, scalar_t, device

    def get_kernel(self, l=4096):
        Ns = l2Ns(l)
        if Ns not in self.kernels:
            self.kernels[Ns] = self.get_custom_kernel_with_allocated_buffer(l)
        return self.kernels[Ns]

    def get_custom_kernel_with_allocated_buffer(self, l=4096):
        if self.nbits != 8:
            raise NotImplementedError("Only uint8 code type is supported for now")
        Ns = l2Ns(l)
        fname = (f"flash_decoding_allocated_buffer_{scalarTypeToStr(self.scalar_t)}u8_"
                 f"Ns{Ns}Lt{self.d}d{self.d}M{self.M}C{2 ** self.nbits}")
        func = getattr(__import__("bindings"), fname)
        po = torch.empty(1, self.nh, Ns + 1, self.d, dtype=self.scalar_t, device=self.device)
        pl = torch.empty(1, self.nh, Ns + 1, dtype=self.scalar_t, device=self.device)
        self.partial_out_buffers[Ns], self.partial_lse_buffers[Ns] = po, pl

        def flash_decoding(query, key_codes, value_codes, key_cents, value_cents, key_residuals, value_residuals, r):
            return func(query, key_codes, value_codes, key_cents, value_cents, key_residuals, value_residuals, r, po, pl)

        return flash_decoding


class PageManager:
    """Free-list page allocator with the semantics of dynamic_paged_pq_utils.py:10-321 (allocate_page,
    allocate_pages, free_page, growth by 1.5x capped by max_pages, stats) over ids only — the pools
    themselves are preallocated tensors owned by the cache, so growth never copies pool memory here."""

    def __init__(self, page_size: int = 64, initial_pages: int = 100, max_pages: Optional[int] = None, M: int = 64):
        if max_pages is not None and initial_pages > max_pages:
            initial_pages = max_pages
        self.page_size, self.M = page_size, M
        self.initial_pages, self.max_pages = initial_pages, max_pages
        self.current_active_pages = initial_pages
        self.free_pages: Set[int] = set(range(initial_pages))
        self._heap: List[int] = list(range(initial_pages))     # min-heap over free ids: lowest id first
        self.allocated_pages: Dict[int, Dict] = {}
        self.total_allocations = self.page_reuse_count = self.total_expansions = 0
        self._ever_used: Set[int] = set()
        self._extra_refs: Dict[int, int] = {}      # references beyond the first, shared pages only (share_page)

    def _expand_page_pool(self, additional_pages: Optional[int] = None):
        if additional_pages is None:
            additional_pages = max(self.current_active_pages // 2, 50)      # :80
        if self.max_pages is not None:
            room = self.max_pages - self.current_active_pages
            if room <= 0:
                raise RuntimeError(f"Cannot expand page pool: reached max_pages limit {self.max_pages}")
            additional_pages = min(additional_pages, room)
        new = self.current_active_pages + additional_pages
        self.free_pages.update(range(self.current_active_pages, new))
        for i in range(self.current_active_pages, new):
            heapq.heappush(self._heap, i)
        self.current_active_pages = new
        self.total_expansions += 1

    def allocate_page(self) -> int:
        if not self.free_pages:
            try:
                self._expand_page_pool()
            except RuntimeError as e:
                raise RuntimeError(f"No free pages available and cannot expand: {e}")
        pid = heapq.heappop(self._heap)     # deterministic (the reference pops an arbitrary set element)
        self.free_pages.remove(pid)
        if pid in self._ever_used:
            self.page_reuse_count += 1
        self._ever_used.add(pid)
        self.allocated_pages[pid] = {"allocation_count": 1}
        self.total_allocations += 1
        return pid

    def allocate_pages(self, n: int) -> List[int]:
        if n <= 0:
            return []
        if len(self.free_pages) < n:
            self._expand_page_pool(additional_pages=n - len(self.free_pages))
            if len(self.free_pages) < n:
                raise RuntimeError(f"Cannot bulk-allocate {n} pages: max_pages={self.max_pages}")
        return [self.allocate_page() for _ in range(n)]

    def share_page(self, page_id: int) -> int:
        """One more owner of an allocated page (PagedPQCache.fork: requests that share a prompt's code pages); each owner
        gives its reference back with free_page.  Returns the page's reference count."""
        if page_id not in self.allocated_pages:
            raise RuntimeError(f"share_page: page {page_id} is not allocated")
        self._extra_refs[page_id] = self._extra_refs.get(page_id, 0) + 1
        return 1 + self._extra_refs[page_id]

    def share_pages(self, page_ids) -> None:
        """share_page for every id of a list (a fork shares hundreds of pages per table row); all or nothing."""
        alloc, extra = self.allocated_pages, self._extra_refs
        for pid in page_ids:
            if pid not in alloc:
                raise RuntimeError(f"share_page: page {pid} is not allocated")
        for pid in page_ids:
            extra[pid] = extra.get(pid, 0) + 1

    def ref_count(self, page_id: int) -> int:
        """Owners of a page: 0 for a free (or unknown) id, 1 for a page never shared."""
        return 1 + self._extra_refs.get(page_id, 0) if page_id in self.allocated_pages else 0

    def free_page(self, page_id: int):
        """Drops one reference; the id returns to the free list with the last one."""
        if page_id not in self.allocated_pages:
            return
        extra = self._extra_refs.get(page_id, 0)
        if extra:
            if extra == 1:
                del self._extra_refs[page_id]
            else:
                self._extra_refs[page_id] = extra - 1
            return
        del self.allocated_pages[page_id]
        self.free_pages.add(page_id)
        heapq.heappush(self._heap, page_id)

    def get_stats(self) -> Dict:
        return {"initial_pages": self.initial_pages, "current_active_pages": self.current_active_pages,
                "max_pages": self.max_pages, "allocated_pages": len(self.allocated_pages),
                "free_pages": len(self.free_pages),
                "utilization": len(self.allocated_pages) / max(self.current_active_pages, 1),
                "page_reuse_count": self.page_reuse_count, "total_allocations": self.total_allocations,
                "total_expansions": self.total_expansions}

    def sharing_stats(self) -> Dict:
        """shared_pages: allocated pages with more than one owner; extra_references: owners beyond the first, over all pages
        (the pages a cache without sharing would hold in addition)."""
        return {"shared_pages": len(self._extra_refs), "extra_references": sum(self._extra_refs.values())}


class _CacheBase:
    def set_cent(self, key_cent: torch.Tensor, value_cent: torch.Tensor):
        """cent is (M, C, d//M) — one table shared by all layers and heads (pq_utils.py:149-159)."""
        self.key_cent = key_cent.to(self.device, self.scalar_t).contiguous()
        self.value_cent = self.key_cent if value_cent is key_cent else value_cent.to(self.device, self.scalar_t).contiguous()
        if self.key_cent.shape[1] != self.C or self.value_cent.shape[1] != self.C:
            raise ValueError(f"codebooks must have 2**nbits = {self.C} centroids per subspace")
        if self._fmt.prepared:      # LDS-ready images for the fused decode kernels and the fp32 image for the encoder
            self._kprep = ops.prepare_cents(self.key_cent, cache=False)
            self._vprep = self._kprep if self.value_cent is self.key_cent else ops.prepare_cents(self.value_cent, cache=False)
        else:
            self._kprep = self._vprep = None

    def _prefill_attention(self, q, k, v, dev_spans=None, return_lse=False):
        """Causal attention of the prompt on its own fp16 K/V (reference: repeat_kv + torch SDPA, pq_utils.py:249-260):
        the MFMA flash kernel of this library (csrc/prefill.hip), the G query heads of a kv head sharing its K/V tiles.
        dev_spans: the per-request lengths of a ragged batch (ops.prefill_attn).  return_lse: (out, lse), lse fp32 (bs, nh, n) -
        every row's log-sum-exp over the keys it saw (million_prefill_attn_lse; `out` is bitwise the call without it)."""
        if return_lse:
            return ops.prefill_attn(q, k, v, causal=True, dev_spans=dev_spans, return_lse=True)
        return ops.prefill_attn(q, k, v, causal=True, dev_spans=dev_spans)

    # self._fmt: the ops.CodeFormat of the cache's code stores, picked once by __init__.  Its jobs (encode_pages,
    # decode_workspace, decode_pages, chunk_op) take both forms of the codebooks and use the one their op takes
    def _cents(self):
        return (self.key_cent, self.value_cent), (self._kprep, self._vprep)


class DynamicPQCache(_CacheBase):
    """Row-major code store + residual window of Lt=d rows; flush ALL Lt rows when full
    (reference pq_utils.py:98-328).  `max_tokens` bounds the preallocated store."""

    def __init__(self, *, bs, nh, num_key_value_heads, M, layer_num, dtype=None, nbits=8, d=128,
                 scalar_t=torch.float16, max_tokens=32768 + 1024, device="cuda", sink_tokens=0):
        if sink_tokens:
            raise NotImplementedError("DynamicPQCache: sink_tokens is a property of PagedPQCache (DESIGN.md 4.13)")
        # nbits <= 8: uint8 codes, every path.  nbits 9..16: uint16 codes (nbits2dtype, pq_utils.py:542-552) on the
        # dequantise-then-attend paths (update, prefill) and, at nbits 9..12, extend (million_pq_chunk_attn_wide); the fused
        # decode kernels of this cache are uint8-only, as the reference's are (KernelRegistry raises NotImplementedError,
        # pq_utils.py:50-52).
        if not 1 <= nbits <= 16:
            raise NotImplementedError("nbits must be in 1..16")
        dtype = nbits2dtype(nbits) if dtype is None else dtype
        if dtype != nbits2dtype(nbits):
            raise ValueError(f"dtype {dtype} does not match nbits={nbits} ({nbits2dtype(nbits)})")
        self.bs, self.nh, self.num_key_value_heads, self.M, self.layer_num = bs, nh, num_key_value_heads, M, layer_num
        self.dtype, self.nbits, self.d, self.scalar_t, self.device = dtype, nbits, d, scalar_t, torch.device(device)
        self.C = 2 ** nbits
        self._fmt = ops.code_format("DynamicPQCache", dtype, None)      # (nbits 13 .. 16: uint16 codes that no attention op reads)
        self.max_residual_length = d          # "Lt = d", pq_utils.py:110
        self.max_tokens = (max_tokens + d - 1) // d * d
        self.registery = KernelRegistry(M=M, d=d, nbits=nbits, nh=nh, scalar_t=scalar_t, device=device)
        self.init_cache()

    def init_cache(self):
        z = lambda *s, dt: torch.zeros(*s, dtype=dt, device=self.device)
        nk, Lt = self.num_key_value_heads, self.max_residual_length
        self._k_store = [z(self.bs, nk, self.max_tokens, self.M, dt=self.dtype) for _ in range(self.layer_num)]
        self._v_store = [z(self.bs, nk, self.max_tokens, self.M, dt=self.dtype) for _ in range(self.layer_num)]
        self.key_residual_cache = [z(self.bs, nk, Lt, self.d, dt=self.scalar_t) for _ in range(self.layer_num)]
        self.value_residual_cache = [z(self.bs, nk, Lt, self.d, dt=self.scalar_t) for _ in range(self.layer_num)]
        self.seen_tokens = [0] * self.layer_num
        self.residualed_tokens = [0] * self.layer_num
        self._T = [0] * self.layer_num
        self._ws = None

    # views with the reference's shapes
    @property
    def key_cache(self):
        return [s[:, :, :t] for s, t in zip(self._k_store, self._T)]

    @property
    def value_cache(self):
        return [s[:, :, :t] for s, t in zip(self._v_store, self._T)]

    def _append_codes(self, X, layer_idx, n):
        T = self._T[layer_idx]
        if T + n > self.max_tokens:
            raise RuntimeError(f"DynamicPQCache: {T + n} tokens exceed max_tokens={self.max_tokens}")
        ops.pq_encode_into(X[0], self.key_cent, self._k_store[layer_idx], token_start=T, n=n, prepared=self._kprep)
        ops.pq_encode_into(X[1], self.value_cent, self._v_store[layer_idx], token_start=T, n=n, prepared=self._vprep)
        self._T[layer_idx] = T + n

    def prefill(self, query_states, key_states, value_states, layer_idx, distort_recent=False, return_lse=False):
        """distort_recent=True attends to the DEQUANTISED prompt (perplexity-style evaluation of the quantiser,
        pq_utils.py:222-260 docstring); leave it False when serving.  The attention sees the prompt only: on a cache that
        already holds tokens use extend().  return_lse: (out, lse) (_prefill_attention)."""
        n = key_states.size(2)
        T0 = self._T[layer_idx]
        self._append_codes((key_states, value_states), layer_idx, n)       # pq_utils.py:235-240
        self.seen_tokens[layer_idx] += n
        if distort_recent:                                                 # :242-246
            key_states = ops.pq_decode(self._k_store[layer_idx][:, :, T0:T0 + n], self.key_cent)
            value_states = ops.pq_decode(self._v_store[layer_idx][:, :, T0:T0 + n], self.value_cent)
        return self._prefill_attention(query_states, key_states, value_states, **({"return_lse": True} if return_lse else {}))

    def update(self, key_states, value_states, layer_idx, distort_recent=False):
        """The reference's non-kernel path (pq_utils.py:166-220), DynamicCache-compatible: encode and store the new
        K/V, return the full-length fp16 K/V for a dense attention — the dequantised past followed by the new rows
        as they are (or dequantised too with distort_recent).  No residual window on this path (as in the reference).
        A block of new tokens on a cache that is not empty is served without the fp16 past by extend()."""
        n = key_states.size(2)
        T0 = self._T[layer_idx]
        self._append_codes((key_states, value_states), layer_idx, n)
        self.seen_tokens[layer_idx] += n
        upto = T0 + n if distort_recent else T0
        past_k = ops.pq_decode(self._k_store[layer_idx][:, :, :upto], self.key_cent) if upto else None
        past_v = ops.pq_decode(self._v_store[layer_idx][:, :, :upto], self.value_cent) if upto else None
        if distort_recent:
            return past_k, past_v
        if past_k is None:
            return key_states, value_states
        return torch.cat([past_k, key_states.to(past_k.dtype)], dim=2), torch.cat([past_v, value_states.to(past_v.dtype)], dim=2)

    def decoding(self, query_states, key_states, value_states, layer_idx, fused=True):
        """One decode step of one layer (pq_utils.py:281-328).  fused=True (default): append + attention in ONE launch.
        fused=False: the reference's own call sequence - copy the new row into the window (:304-312), then the kernel
        `registery.get_kernel(l=seen_tokens)` resolves by name from `bindings` (:315-325)."""
        if self.nbits > 8:
            raise NotImplementedError("Only uint8 code type is supported by the fused decode kernels (use update())")
        Lt = self.max_residual_length
        if self.residualed_tokens[layer_idx] == Lt:                        # pq_utils.py:288-302
            self._append_codes((self.key_residual_cache[layer_idx], self.value_residual_cache[layer_idx]), layer_idx, Lt)
            self.residualed_tokens[layer_idx] = 0
        r = self.residualed_tokens[layer_idx]
        self.residualed_tokens[layer_idx] = r + 1
        self.seen_tokens[layer_idx] += 1
        if not fused:
            ops.residual_append(key_states, value_states, self.key_residual_cache[layer_idx],
                                self.value_residual_cache[layer_idx], r)
            kernel = self.registery.get_kernel(l=self.seen_tokens[layer_idx])
            T = self._T[layer_idx]
            return kernel(query_states, self._k_store[layer_idx][:, :, :T], self._v_store[layer_idx][:, :, :T],
                          self.key_cent, self.value_cent, self.key_residual_cache[layer_idx],
                          self.value_residual_cache[layer_idx], r + 1)
        if self._ws is None:      # sized once for max_tokens (partials + transposed-V scratch of the row-major path)
            need = ops.decode_workspace_bytes(query_states, self.key_residual_cache[layer_idx], nh_k=self.num_key_value_heads,
                                              M=self.M, C=self.C, n_tokens=self.max_tokens,
                                              k_codes=self._k_store[layer_idx], v_codes=self._v_store[layer_idx])
            self._ws = torch.zeros(need, dtype=torch.uint8, device=self.device)
        # append (:304-312) + attention (:314-326) in ONE launch
        return ops.pq_decode_attn(query_states, self._k_store[layer_idx], self._v_store[layer_idx], self._kprep,
                                  self._vprep, self.key_residual_cache[layer_idx], self.value_residual_cache[layer_idx],
                                  r, M=self.M, C=self.C, n_tokens=self._T[layer_idx], k_new=key_states,
                                  v_new=value_states, workspace=self._ws)

    def extend(self, query_states, key_states, value_states, layer_idx, route=None):
        """n new tokens of one layer on a cache that may already hold tokens (a later turn of a conversation, the next chunk
        of a prompt): returns their attention over [the PQ codes; the residual window; the new rows, causally]
        (million_pq_chunk_attn: the past is read as codes, never as fp16), then leaves the cache as prefill() of the
        whole sequence would have - the window rows and then the new rows are encoded behind T, the window is empty.
        On an empty cache this is prefill().  nbits 9 .. 12: the same over the uint16 store and the codebooks as they are
        (million_pq_chunk_attn_wide); nbits 13 .. 16 have no chunk kernel.  route="blocks": the attention by
        blocks through the prompt kernel (CodeFormat.chunk_op) - at nbits 9 .. 12 too - followed by the same store."""
        attend = self._fmt.chunk_op("extend", route)
        if self.nbits > 12:
            raise NotImplementedError(f"extend: nbits={self.nbits}: the chunk-attention kernels read uint8 codes (nbits <= 8) or "
                                      "uint16 codes of nbits 9 .. 12")
        T, r = self._T[layer_idx], self.residualed_tokens[layer_idx]
        if T == 0 and r == 0:
            return self.prefill(query_states, key_states, value_states, layer_idx)
        n = key_states.size(2)
        kres, vres = self.key_residual_cache[layer_idx], self.value_residual_cache[layer_idx]
        out = attend(query_states, key_states, value_states, self._k_store[layer_idx], self._v_store[layer_idx],
                     *self._cents(), kres, vres, r, M=self.M, C=self.C, n_tokens=T)
        if T + r + n > self.max_tokens:
            raise RuntimeError(f"DynamicPQCache: {T + r + n} tokens exceed max_tokens={self.max_tokens}")
        if r:
            self._append_codes((kres, vres), layer_idx, r)
        self._append_codes((key_states, value_states), layer_idx, n)
        self.residualed_tokens[layer_idx] = 0
        self.seen_tokens[layer_idx] += n
        return out

    @property
    def pq_cache_size(self):
        return sum(2 * self.bs * self.num_key_value_heads * t * self.M * self._k_store[0].element_size() for t in self._T)

    @property
    def residual_cache_size(self):
        return sum(c.numel() * c.element_size() for c in self.key_residual_cache + self.value_residual_cache)


SNAPSHOT_VERSION = 1      # of an 8-bit cache's snapshots; a wide cache writes and reads version 2 (ops.CodeFormat.blob_version)
_SNAPSHOT_GEOMETRY = ("layer_num", "nh_k", "d", "M", "nbits", "page_size", "resid_cap")


class RequestSnapshot:
    """One request of a PagedPQCache outside its pages (swap_out / swap_in, formats.save_request): `blob`, a 1-D uint8 host
    tensor in blob format 1 (include/million_hip.h, million_cache_swap; pinned when it comes from swap_out) - format 2
    (million_cache_swap_wide) when it comes from a cache with nbits 9 .. 12 through paged_turns.swap_out -, and `meta`, a dict
    of plain ints and strings: "version", the geometry (layer_num, nh_k, d, M, nbits, page_size, resid_cap), the request (T
    coded tokens, r window rows, ring start `start`, `seen` tokens) and the sha256 of the key and value codebook bytes."""

    def __init__(self, blob: torch.Tensor, meta: Dict):
        self.blob, self.meta = blob, dict(meta)


class _PerLayer:
    """`cache._T[l]`-style access to a (layers, requests) host array: reading gives request 0's value (all requests move in
    lockstep unless slots are recycled, see PagedPQCache.release), writing sets every request of the layer."""

    def __init__(self, arr):
        self._a = arr

    def __getitem__(self, l):
        return int(self._a[l, 0])

    def __setitem__(self, l, v):
        self._a[l, :] = v

    def __len__(self):
        return self._a.shape[0]

    def __iter__(self):
        return (int(x) for x in self._a[:, 0])

    def __eq__(self, other):
        return list(self) == list(other)


class PagedPQCache(_CacheBase):
    """Paged code store: K pages (page_size, M) row-major, V pages (M, page_size) transposed, a residual
    ring of `extended_residual_size` rows; when r reaches it the OLDEST page_size rows are flushed
    (reference paged_pq_utils.py:10-397; policy :141-153, :359-361).

    One global pool per side serves all layers; page ids are handed out by a PageManager.  With
    `preallocate=True` (default) the page table of every (layer, b, hk) is filled for `max_tokens` at
    init, so decode steps touch no host state and are hipGraph-capturable.

    Lengths are kept per (layer, request) - on the host (numpy, (layers, bs)) and on the device (`lengths[l]`, int32
    (bs, 4)) - so that a batch slot can finish and be recycled while the others keep decoding: `release(b)` returns the
    slot's pages and zeroes its lengths, `prefill_request(b, ...)` encodes a new prompt into it (`prefill_ragged`: several
    slots' prompts of different lengths, one attention launch).  Requests of different
    lengths share every launch through the device-resident lengths (`use_dev_lengths=True`).

    `sink_tokens=S` (0 .. 64; 0: nothing is allocated and every call launches what it always did): the first min(S, n) rows of
    a request's first store step (prefill*, extend*) stay exact fp16 rows beside the pages - the attention sinks - and only the
    rows behind them are encoded; decoding_with_pages, the extend forms and verify merge them into their result with one more
    launch (ops.attn_sink_merge), the live count read on the device.  `seen` counts them, T does not.  DESIGN.md 4.13.

    `nbits` 9 .. 12 with `dtype=torch.uint16` (uint16 pools, codebooks of 2**nbits centroids): the core life - prefill,
    prefill_request, decoding_with_pages (ops.pq_decode_attn_wide), the in-line flush of requests in lockstep, release, cleanup -
    and NotImplementedError naming nbits for the rest (extend*, prefill_ragged, fork, swap, verify / commit, update, sinks;
    fork and swap of such a cache: million_amd.paged_turns).
    DESIGN.md 4.14.  extend / extend_request of such a cache, packed or not: million_amd.paged_turns.  Requests at
    different lengths - a flush that reads every request's lengths on the device, prefill_ragged, extend_ragged -: million_amd.paged_turns
    too (flush, decode, prefill_ragged, extend_ragged); the methods here keep the lockstep flush and the refusals.

    `packed=True` (nbits 9 .. 12 only; nbits = 8: ValueError): the same cache over packed pools - uint8 (n_pool,
    ops.packed_page_bytes), 10 bits per code at nbits 9 / 10 and 12 at nbits 11 / 12 instead of 16 (include/million_hip.h,
    "Packed code pages") - through ops.pq_encode_into_packed and ops.pq_decode_attn_packed: the same codes, the same outputs bit
    for bit, the same refusals, (8 + h) / 16 of the pool bytes.  DESIGN.md 4.17."""

    def __init__(self, *, bs, nh, num_key_value_heads, M, layer_num, dtype=torch.uint8, nbits=8, d=128,
                 scalar_t=torch.float16, page_size=64, extended_residual_size=128, max_pages_per_layer=None,
                 max_tokens=32768 + 1024, preallocate=True, device="cuda", sink_tokens=0, packed=False):
        if nbits not in (8, 9, 10, 11, 12) or dtype != nbits2dtype(nbits):
            raise NotImplementedError(f"PagedPQCache: nbits=8 with dtype=torch.uint8, or nbits 9 .. 12 with dtype=torch.uint16 "
                                      f"(DESIGN.md 4.14), are the code types that exist; got nbits={nbits}, dtype={dtype}")
        if packed and nbits == 8:
            raise ValueError("PagedPQCache: packed=True needs nbits 9 .. 12 (a code of nbits=8 is one byte already)")
        if isinstance(sink_tokens, bool) or int(sink_tokens) != sink_tokens or not 0 <= sink_tokens <= ops.SINK_MAX_ROWS:
            raise ValueError(f"sink_tokens must be an integer in 0 .. {ops.SINK_MAX_ROWS}")
        if nbits > 8 and sink_tokens:
            raise NotImplementedError(f"PagedPQCache: sink_tokens > 0 on a cache with nbits={nbits} (uint16 codes) is not built yet "
                                      "(DESIGN.md 4.14)")
        if page_size not in (32, 64, 128):
            raise ValueError("page_size must be 32, 64 or 128")
        if extended_residual_size < page_size:
            raise ValueError("extended_residual_size must be >= page_size")
        self.bs, self.nh, self.num_key_value_heads, self.M, self.layer_num = bs, nh, num_key_value_heads, M, layer_num
        self.dtype, self.nbits, self.d, self.scalar_t, self.device = dtype, nbits, d, scalar_t, torch.device(device)
        self.C = 2 ** nbits
        self.page_size, self.extended_residual_size = page_size, extended_residual_size
        self.max_residual_length = extended_residual_size
        self.n_pages_cap = (max_tokens + page_size - 1) // page_size
        if max_pages_per_layer is not None:
            self.n_pages_cap = min(self.n_pages_cap, max_pages_per_layer // max(bs * num_key_value_heads, 1))
        self.max_tokens = self.n_pages_cap * page_size
        self.preallocate = preallocate
        self.sink_tokens = int(sink_tokens)
        self.packed = bool(packed)
        self._fmt = ops.code_format("PagedPQCache", dtype, self.C, self.packed)      # every later "which format?" reads this
        self.registery = KernelRegistry(M=M, d=d, nbits=nbits, nh=nh, scalar_t=scalar_t, device=device)
        self.init_cache()

    def init_cache(self):
        nk, cap = self.num_key_value_heads, self.extended_residual_size
        total = self.layer_num * self.bs * nk * self.n_pages_cap
        z = lambda *s, dt: torch.zeros(*s, dtype=dt, device=self.device)
        # K pages (page_size, M), V pages (M, page_size), uint8 or uint16 at nbits 9 .. 12; packed: a low-byte plane and a plane of
        # 2 / 4 high bits per code in one uint8 page, one page id for both
        k_page, v_page = self._fmt.page_shapes(self.page_size, self.M, self.C)
        self.key_page_pool = z(total, *k_page, dt=self._fmt.dtype)
        self.value_page_pool = z(total, *v_page, dt=self._fmt.dtype)
        self.page_manager = PageManager(self.page_size, initial_pages=total, max_pages=total, M=self.M)
        # the layers' page tables, windows and length rows lie side by side (one allocation each; the per-layer lists are
        # views): one launch can then serve every layer (begin_step: encode-ahead, commit)
        self._page_ids_all = z(self.layer_num, self.bs, nk, self.n_pages_cap, dt=torch.int32)
        self._kres_all = z(self.layer_num, self.bs, nk, cap, self.d, dt=self.scalar_t)
        self._vres_all = z(self.layer_num, self.bs, nk, cap, self.d, dt=self.scalar_t)
        self._lengths_all = z(self.layer_num, self.bs, 4, dt=torch.int32)
        self.page_ids = [self._page_ids_all[l] for l in range(self.layer_num)]
        self.key_residual_cache = [self._kres_all[l] for l in range(self.layer_num)]
        self.value_residual_cache = [self._vres_all[l] for l in range(self.layer_num)]
        self.lengths = [self._lengths_all[l] for l in range(self.layer_num)]     # device mirror
        # host mirrors, (layers, requests)
        zi = lambda: np.zeros((self.layer_num, self.bs), dtype=np.int64)
        self._seen_a, self._r_a, self._T_a, self._rs_a, self._pages_a = zi(), zi(), zi(), zi(), zi()
        # sink rows (sink_tokens = S > 0): the first min(S, prompt) tokens of every request as exact fp16 rows beside the pages, the
        # live count per (layer, request) on the device (every attention call reads it there) and in a host mirror (_note_sinks)
        S = self.sink_tokens
        self._ksink_all = z(self.layer_num, self.bs, nk, S, self.d, dt=self.scalar_t) if S else None
        self._vsink_all = z(self.layer_num, self.bs, nk, S, self.d, dt=self.scalar_t) if S else None
        self._sink_all = z(self.layer_num, self.bs, dt=torch.int32) if S else None
        self._sink_a, self._sink_lse = zi(), None
        self._sink_views = [(self._ksink_all[l], self._vsink_all[l], self._sink_all[l]) for l in range(self.layer_num)] if S else None
        self._pre_a = zi()      # 1: the oldest page_size window rows are already encoded at tokens [T, T + page_size) (begin_step)
        self._pre_join = False
        self._dev_rows_stale = False      # a host-length step moved the mirror and not the device rows (_refresh_device_rows)
        self._host_pids = [[[[] for _ in range(nk)] for _ in range(self.bs)] for _ in range(self.layer_num)]
        self._ws = None
        # draft verification (verify / commit): the record of the running verify, the staged rows, one decode workspace per n
        self._verify_rec, self._kstage, self._vstage, self._ws_verify = None, None, None, {}
        self._side, self._flush_events, self._ahead = None, {}, None
        # knobs of begin_step (None: the defaults of _ea_groups / begin_step): steps an encode-ahead is spread over, launches per step
        self.encode_ahead_steps = self.encode_ahead_launches = None
        if self.preallocate:
            for l in range(self.layer_num):
                for b in range(self.bs):
                    self._assign_pages(l, self.n_pages_cap, b)

    # per-layer views with the reference's names (request 0's value; assignment sets every request)
    seen_tokens = property(lambda self: _PerLayer(self._seen_a), lambda self, v: self._set_rows(self._seen_a, v))
    residualed_tokens = property(lambda self: _PerLayer(self._r_a), lambda self, v: self._set_rows(self._r_a, v))
    _T = property(lambda self: _PerLayer(self._T_a), lambda self, v: self._set_rows(self._T_a, v))
    _rstart = property(lambda self: _PerLayer(self._rs_a), lambda self, v: self._set_rows(self._rs_a, v))
    _pages_assigned = property(lambda self: _PerLayer(self._pages_a))

    @staticmethod
    def _set_rows(arr, v):
        v = np.asarray([list(x) if hasattr(x, "__len__") else x for x in v] if not isinstance(v, np.ndarray) else v)
        arr[...] = v if v.ndim == 2 else v[:, None]

    def _lockstep(self, layer_idx) -> bool:
        a = (self._T_a[layer_idx], self._r_a[layer_idx], self._rs_a[layer_idx])
        return all((x == x[0]).all() for x in a)

    def _assign_pages(self, layer_idx, upto_pages, b=None):
        """Page ids for pages [have, upto_pages) of every kv head of request b (None: every request)."""
        for bb in (range(self.bs) if b is None else (b,)):
            have = int(self._pages_a[layer_idx, bb])
            if upto_pages <= have:
                continue
            if upto_pages > self.n_pages_cap:
                raise RuntimeError(f"PagedPQCache: {upto_pages} pages exceed capacity {self.n_pages_cap} (max_tokens)")
            n_new = upto_pages - have
            nk = self.num_key_value_heads
            ids = self.page_manager.allocate_pages(n_new * nk)
            for h in range(nk):
                self._host_pids[layer_idx][bb][h].extend(ids[h * n_new:(h + 1) * n_new])
            t = torch.tensor(ids, dtype=torch.int32).reshape(nk, n_new)
            self.page_ids[layer_idx][bb, :, have:upto_pages] = t.to(self.device)
            self._pages_a[layer_idx, bb] = upto_pages

    # ---- the mirror transitions: every rule that moves _T_a, _r_a, _rs_a, _seen_a, _pre_a (and the device rows) is written
    # here, once.  `sel` / `b` index the (layers, requests) arrays: a layer, (layer, request mask), a mask of both, ...
    def _note_flushed(self, sel):
        """A flush moved the window of the entries `sel`: its oldest page_size rows are codes behind T now."""
        ps = self.page_size
        self._T_a[sel] += ps
        self._r_a[sel] -= ps
        self._rs_a[sel] = (self._rs_a[sel] + ps) % self.extended_residual_size
        self._pre_a[sel] = 0      # (rows encoded ahead are in their pages: flushed in line they were encoded again, same codes)

    def _note_appended(self, layer_idx=slice(None)):
        """A decode step appended one row to the window of every request of a layer (of every layer)."""
        self._r_a[layer_idx] += 1
        self._seen_a[layer_idx] += 1

    def _note_stored(self, layer_idx, n, b=slice(None)):
        """n new rows of request b (every request) were encoded behind T."""
        self._T_a[layer_idx, b] += n
        self._seen_a[layer_idx, b] += n

    def _note_window_emptied(self, layer_idx, b=slice(None)):
        """The r window rows of request b (every request) were encoded behind T, in ring order: they are seen already."""
        self._T_a[layer_idx, b] += self._r_a[layer_idx, b]
        self._r_a[layer_idx, b] = 0
        self._rs_a[layer_idx, b] = 0

    def _note_sinks(self, layer_idx, b, s):
        """Request(s) b of a layer (slice(None): of every layer) keep s sink rows from now on - s an int, or an array that
        broadcasts over the entries: the host count and the device count the attention calls read move here, together, and
        nowhere else.  Sink rows are tokens the request has seen and the pages do not hold."""
        if not self.sink_tokens:
            return
        self._seen_a[layer_idx, b] += s - self._sink_a[layer_idx, b]
        self._sink_a[layer_idx, b] = s
        self._sink_all[layer_idx, b] = s if np.isscalar(s) else torch.from_numpy(np.asarray(s, np.int32)).to(self.device)

    def _sink_merge(self, layer_idx, q, out, lse, sel=slice(None), dev_n=None):
        """The sink part of an attention call, in place on its (out, lse): ops.attn_sink_merge over the sink rows of the layer
        (of the requests `sel`), the live counts read on the device."""
        ks, vs, cnt = self._sink_views[layer_idx]
        if sel != slice(None):
            ks, vs, cnt = ks[sel], vs[sel], cnt[sel]
        ops.attn_sink_merge(q, ks, vs, out, lse, dev_s=cnt, dev_n=dev_n, out=out, lse_out=lse)

    def _no_sinks(self, what):
        if self.sink_tokens:
            raise NotImplementedError(f"PagedPQCache: {what} of a cache with sink_tokens > 0 is not built yet (DESIGN.md 4.13)")

    def _no_wide(self, what):
        """nbits 9 .. 12 (uint16 codes): the core life is built - prefill, prefill_request, decoding_with_pages, the in-line
        flush, release - and the rest refused by name, before any state changes."""
        if self.nbits > 8:
            raise NotImplementedError(f"PagedPQCache: {what} of a cache with nbits={self.nbits} (uint16 codes) is not built yet "
                                      "(DESIGN.md 4.14)")

    def _sync_lengths(self, layer_idx, b=None):
        """The device rows of a layer - of request b alone: the others' are not touched - written from the mirror."""
        sel = slice(None) if b is None else slice(b, b + 1)
        T = self._T_a[layer_idx, sel]
        rows = np.stack([T, self._r_a[layer_idx, sel], self._rs_a[layer_idx, sel], np.zeros_like(T)], axis=1)
        self.lengths[layer_idx][sel].copy_(torch.from_numpy(rows.astype(np.int32)))

    def _refresh_device_rows(self):
        """Steps with use_dev_lengths=False (decoding_with_pages, flush_to_pages, begin_step) move the host mirror only.  The
        calls whose kernels read the device rows whatever the mode (fork: the source's row; commit: every slot's) write the
        rows from the mirror first; after steps with device lengths there is nothing to do."""
        if self._dev_rows_stale:
            for l in range(self.layer_num):
                self._sync_lengths(l)
            self._dev_rows_stale = False

    def _reserve(self, layer_idx, n, b=None, ask=False) -> bool:
        """Room for n more tokens behind T of request b (None: every request, in lockstep).  A preallocated table is checked
        against max_tokens, an on-demand one gets its pages now (_assign_pages raises past the capacity).  ask=True only
        answers whether a preallocated table has the room and assigns nothing: pages on demand are begin_step's to take."""
        T = int(self._T_a[layer_idx, 0 if b is None else b])
        if self.preallocate:
            if T + n > self.max_tokens:
                if ask:
                    return False
                raise RuntimeError(f"PagedPQCache: {T + n} tokens exceed max_tokens={self.max_tokens}")
        elif not ask:
            self._assign_pages(layer_idx, (T + n + self.page_size - 1) // self.page_size, b)
        return True

    def _encode_to_pages(self, K, V, layer_idx, n, *, b=None, x_row_start=0, x_row_mod=0):
        """Encode n rows of K, V (bs or 1, nh_k, n, d) behind the T quantised tokens of every request (b = None: requests
        in lockstep) or of request b.  x_row_mod > 0: K, V are rings of x_row_mod rows read from x_row_start on."""
        sel = slice(None) if b is None else slice(b, b + 1)
        T = int(self._T_a[layer_idx, 0 if b is None else b])
        self._reserve(layer_idx, n, b)
        kw = dict(token_start=T, n=n, page_ids=self.page_ids[layer_idx][sel], page_size=self.page_size,
                  x_row_start=x_row_start, x_row_mod=x_row_mod)
        self._fmt.encode_pages(K, self.key_cent, self._kprep, self.key_page_pool, layout=L.MILLION_CODES_KPAGES, **kw)
        self._fmt.encode_pages(V, self.value_cent, self._vprep, self.value_page_pool, layout=L.MILLION_CODES_VPAGES, **kw)

    def _store(self, K, V, layer_idx, n, b=None, all_rows=False):
        """The store step under every prefill / extend form, for request b (None: every request, in lockstep): the window
        into codes when it holds rows (ring order, behind T), the n new rows behind those, the mirror, the device row of
        request b (all_rows, or b = None: every row of the layer).  Leaves what prefill of the whole sequence would."""
        i, sel = (0, slice(None)) if b is None else (b, slice(b, b + 1))
        r = int(self._r_a[layer_idx, i])
        if r:
            self._encode_to_pages(self.key_residual_cache[layer_idx][sel], self.value_residual_cache[layer_idx][sel], layer_idx, r,
                                  b=b, x_row_start=int(self._rs_a[layer_idx, i]), x_row_mod=self.extended_residual_size)
            self._note_window_emptied(layer_idx, sel)
        s = 0
        if self.sink_tokens and not self._seen_a[layer_idx, sel].any():      # the request's first rows: its sinks stay fp16
            s = min(self.sink_tokens, n)
            self._ksink_all[layer_idx][sel, :, :s].copy_(K[:, :, :s])
            self._vsink_all[layer_idx][sel, :, :s].copy_(V[:, :, :s])
            self._note_sinks(layer_idx, sel, s)
            K, V = K[:, :, s:], V[:, :, s:]
        if n - s:
            self._encode_to_pages(K, V, layer_idx, n - s, b=b)
        self._note_stored(layer_idx, n - s, sel)
        self._sync_lengths(layer_idx, None if all_rows else b)

    def _reserve_ragged(self, layer_idx, n_new):
        """Room for the window rows and the n_new[b] new rows of every slot that takes part, before anything is launched
        (paging on demand: the page table is complete when the one store call reads it)."""
        for b in range(self.bs):
            if n_new[b] > 0:
                self._reserve(layer_idx, int(self._r_a[layer_idx, b]) + n_new[b], b)

    def _store_ragged(self, K, V, layer_idx, n_new, dev_n):
        """_store() for every slot with n_new[b] > 0 in ONE call (the ragged store of the cache's format: ops.pq_store_ragged,
        ops.pq_store_ragged_wide): the windows in ring order and the
        first n_new[b] rows of K, V (bs, nh_k, n, d) behind each T_b, every per-slot value read from `lengths[layer_idx]` and
        dev_n on the device, the device rows advanced there - no _sync_lengths.  The slots' pages were reserved before the
        attention launch (_reserve_ragged); the mirror moves through the same owners as _store."""
        who = [b for b in range(self.bs) if n_new[b] > 0]
        self._fmt.store_ragged_pages(K, V, self.key_residual_cache[layer_idx], self.value_residual_cache[layer_idx], *self._cents(),
                                     self.key_page_pool, self.value_page_pool, self.page_ids[layer_idx], self.lengths[layer_idx], dev_n,
                                     M=self.M, C=self.C, page_size=self.page_size)
        for b in who:
            sel = slice(b, b + 1)
            self._note_window_emptied(layer_idx, sel)
            self._note_stored(layer_idx, n_new[b], sel)

    def prefill(self, query_states, key_states, value_states, layer_idx, distort_recent=False, return_lse=False):
        """Bulk encode of the prompt straight into pages (reference paged_pq_utils.py:216-320: encode,
        torch.cat, per-page permute+contiguous); the residual window stays empty.  The attention sees the
        prompt only: on a cache that already holds tokens use extend().  return_lse: (out, lse), lse fp32 (bs, nh, n) over the
        whole prompt - with sinks too: they lie inside the prompt."""
        if not self._lockstep(layer_idx):
            raise RuntimeError("PagedPQCache.prefill: requests are at different lengths; use prefill_request(b, ...)")
        self._store(key_states, value_states, layer_idx, key_states.size(2))
        return self._prefill_attention(query_states, key_states, value_states, **({"return_lse": True} if return_lse else {}))

    def prefill_request(self, b, query_states, key_states, value_states, layer_idx, return_lse=False):
        """The prompt of ONE request (tensors of batch 1) into batch slot b, the other slots untouched - a recycled slot
        (release) starts its next request while the rest of the batch keeps decoding.  return_lse: (out, lse) as prefill()."""
        if key_states.size(0) != 1 or self._T_a[layer_idx, b] or self._r_a[layer_idx, b] or self._sink_a[layer_idx, b]:
            raise RuntimeError("prefill_request: tensors of batch 1 into an empty slot (release it first)")
        self._store(key_states, value_states, layer_idx, key_states.size(2), b, all_rows=True)      # (every device row: as ever)
        return self._prefill_attention(query_states, key_states, value_states, **({"return_lse": True} if return_lse else {}))

    def prefill_ragged(self, query_states, key_states, value_states, layer_idx, n_new, device_store=False, return_lse=False):
        """prefill_request() for every slot in ONE attention launch - the counterpart of extend_ragged for empty slots, at
        the prompt kernel's rate: tensors of batch bs padded to n = max(n_new) rows, slot b owns the first n_new[b] of them
        (n_new: bs host ints in [0, n]).  A slot with n_new[b] > 0 must be empty (T = r = 0; a slot that holds tokens takes
        extend_ragged).  The launch reads the rows {n_b, n_b, 0, 0} from a small device tensor; the rows past n_new[b] - q, K
        and V - may hold anything and their output rows are zeros.  The encodes stay host-driven per slot; slot b is then left
        exactly as prefill_request(b, ...) with its own rows leaves it (pages, host lengths, its device row).  A slot with
        n_new[b] = 0 takes no part: host and device lengths, pages and window stay as they are (it may be mid-decode).
        device_store=True: the per-slot encodes and length copies are ONE ops.pq_store_ragged call behind the attention launch
        (an int32 device copy of n_new beside `lengths[layer_idx]`): same pages, same codes, same host and device lengths.
        return_lse: (out, lse), lse fp32 (bs, nh, n); -inf in the rows past n_new[b]."""
        self._no_wide("prefill_ragged")
        return self._prefill_ragged("prefill_ragged", query_states, key_states, value_states, layer_idx, n_new, device_store, return_lse)

    def _prefill_ragged(self, who_, query_states, key_states, value_states, layer_idx, n_new, device_store, return_lse):
        """prefill_ragged() for a cache of any format, as _extend: the public method refuses the wide ones first,
        million_amd.paged_turns serves them from here (who_: the caller's name in the messages).  The prompt kernel never sees
        codes; the store is the format's (_store: encode_pages; _store_ragged: store_ragged_pages)."""
        n_new = [int(x) for x in n_new]
        n = query_states.size(2)
        if (len(n_new) != self.bs or query_states.size(0) != self.bs or key_states.size(0) != self.bs or key_states.size(2) != n
                or value_states.shape != key_states.shape):
            raise RuntimeError(f"{who_}: tensors of batch {self.bs}, padded to the same rows, and one n_new per slot")
        if any(x < 0 or x > n for x in n_new):
            raise RuntimeError(f"{who_}: n_new outside [0, {n}]")
        who = [b for b in range(self.bs) if n_new[b] > 0]
        if device_store:
            self._no_sinks(f"{who_}(device_store=True)")
        for b in who:      # every slot's precondition and capacity before anything is launched
            if self._T_a[layer_idx, b] or self._r_a[layer_idx, b] or self._sink_a[layer_idx, b]:
                raise RuntimeError(f"{who_}: slot {b} holds tokens (release it first, or use extend_ragged)")
            if n_new[b] > self.max_tokens:
                raise RuntimeError(f"PagedPQCache: {n_new[b]} tokens exceed max_tokens={self.max_tokens}")
        if device_store:
            self._reserve_ragged(layer_idx, n_new)
        spans = torch.tensor([[x, x, 0, 0] for x in n_new], dtype=torch.int32).to(self.device)
        out = self._prefill_attention(query_states, key_states, value_states, dev_spans=spans, **({"return_lse": True} if return_lse else {}))
        if device_store:
            self._store_ragged(key_states, value_states, layer_idx, n_new, torch.tensor(n_new, dtype=torch.int32).to(self.device))
            return out
        for b in who:      # the encodes stay host-driven per slot, as prefill_request does them
            self._store(key_states[b:b + 1, :, :n_new[b]], value_states[b:b + 1, :, :n_new[b]], layer_idx, n_new[b], b)
        return out

    # ---- extend: a block of new tokens behind the cached ones ------------------------------------------------------------
    def _join_flush(self, layer_idx) -> bool:
        """The side-stream flush of a layer (flush_ahead): what is pending is issued up to this layer (keeping the side stream
        `depth` layers ahead), the layer's own flush event is waited for.  False: the layer has no flush on the side stream."""
        if self._ahead is not None:
            self._ahead_issue(upto_layer=layer_idx)
        ev = self._flush_events.pop(layer_idx, None)
        if ev is None:
            return False
        torch.cuda.current_stream().wait_event(ev)
        return True

    def _join_side(self, layer_idx, b=None):
        """Before extend touches a layer: its pending side-stream flush (flush_ahead) is issued and waited for, and window rows
        encoded ahead (begin_step) are complete.  extend encodes every window row again - rows encoded ahead get the same codes
        in the same pages - so the encoded-ahead flag of the layer (of request b) is cleared."""
        self._join_flush(layer_idx)
        if self._pre_join:
            torch.cuda.current_stream().wait_stream(self._side)
        self._pre_a[layer_idx, slice(None) if b is None else b] = 0

    def _extend_slot(self, attend, query_states, key_states, value_states, layer_idx, b, return_lse=False, all_rows=False):
        """b = None: every request (lockstep); else request b with batch-1 tensors.  attend: the attention op of the cache's
        format and the call's route (ops.CodeFormat.chunk_op); its (out, lse) goes into the sink merge and the store follows, whichever it is.
        return_lse: (out, lse) of that op; all_rows: every device row of the layer is rewritten, as prefill_request does.  The
        callers checked the capacity."""
        i, sel = (0, slice(None)) if b is None else (b, slice(b, b + 1))
        T, r, rs = int(self._T_a[layer_idx, i]), int(self._r_a[layer_idx, i]), int(self._rs_a[layer_idx, i])
        ids = self.page_ids[layer_idx][sel]
        sinks = bool(self.sink_tokens)
        out = attend(query_states, key_states, value_states, self.key_page_pool, self.value_page_pool, *self._cents(),
                     self.key_residual_cache[layer_idx][sel], self.value_residual_cache[layer_idx][sel], r,
                     M=self.M, C=self.C, n_tokens=T, resid_start=rs, k_page_ids=ids, v_page_ids=ids,
                     page_size=self.page_size, **({"return_lse": True} if return_lse or sinks else {}))
        if sinks:      # before the store: a request's first chunk has its sinks among the chunk rows, and none kept yet
            self._sink_merge(layer_idx, query_states, out[0], out[1], sel)
            out = out if return_lse else out[0]
        self._store(key_states, value_states, layer_idx, key_states.size(2), b, all_rows=all_rows)      # the window in ring order, then the new rows
        return out

    def _extend_room(self, layer_idx, i, n, to_prefill):
        """Refuses n new tokens of request i (0: every request, in lockstep) that the pages cannot take behind its T coded and r
        window tokens - before anything is joined or launched.  to_prefill: the rows go to prefill(), which keeps a request's
        first sink_tokens rows outside the pages."""
        need = int(self._T_a[layer_idx, i]) + int(self._r_a[layer_idx, i]) + n - (min(self.sink_tokens, n) if to_prefill else 0)
        if need > self.max_tokens:
            raise RuntimeError(f"PagedPQCache: {need} tokens exceed max_tokens={self.max_tokens}")

    def _extend(self, who, out_of_step, query_states, key_states, value_states, layer_idx, route):
        """extend() for a cache of any format: the public method refuses the wide ones first, million_amd.paged_turns serves them
        from here.  Order: a route that does not exist, requests out of lockstep (out_of_step: the caller's words for it, which
        name its own call for one request), the capacity, then the join and the launches."""
        attend = self._fmt.chunk_op(who, route)
        if not self._lockstep(layer_idx):
            raise RuntimeError(out_of_step)
        empty = self._T_a[layer_idx, 0] == 0 and self._r_a[layer_idx, 0] == 0 and not self._sink_a[layer_idx].any()
        self._extend_room(layer_idx, 0, key_states.size(2), empty)
        self._join_side(layer_idx)
        if empty:
            return self.prefill(query_states, key_states, value_states, layer_idx)
        return self._extend_slot(attend, query_states, key_states, value_states, layer_idx, None)

    def _extend_request(self, who, b, query_states, key_states, value_states, layer_idx, return_lse, route):
        """extend_request() for a cache of any format, as _extend.  An empty slot is prefill_request() - with return_lse, which the
        prompt kernel has not, chunk attention over the chunk alone (every device row rewritten, as prefill_request does) -
        whatever `route` says."""
        attend = self._fmt.chunk_op(who, route)
        if key_states.size(0) != 1 or query_states.size(0) != 1:
            raise RuntimeError(f"{who}: tensors of batch 1")
        empty = self._T_a[layer_idx, b] == 0 and self._r_a[layer_idx, b] == 0 and not self._sink_a[layer_idx, b]
        self._extend_room(layer_idx, b, key_states.size(2), empty and not return_lse)
        self._join_side(layer_idx, b)
        if empty and not return_lse:
            return self.prefill_request(b, query_states, key_states, value_states, layer_idx)
        if empty:
            return self._extend_slot(self._fmt.chunk_op(who, None), query_states, key_states, value_states, layer_idx, b, return_lse=True, all_rows=True)
        return self._extend_slot(attend, query_states, key_states, value_states, layer_idx, b, return_lse=return_lse)

    def extend(self, query_states, key_states, value_states, layer_idx, route=None):
        """n new tokens of one layer, every request in lockstep (a later turn of the conversations, the next chunk of their
        prompts): returns their attention over [the PQ codes in the pages; the residual window; the new rows, causally]
        (million_pq_chunk_attn: the past is read as codes, never as fp16), then leaves the cache exactly as prefill() of
        the whole sequence would have - the window rows (in ring order) and then the new rows are encoded into the pages
        behind T, the window is emptied (r = 0, resid_start = 0), host and device lengths advance.  Pending encode-ahead
        work of the layer (begin_step, flush_ahead) is joined first and its flags cleared: rows encoded ahead are encoded
        again into the same pages with the same codes.  On an empty cache this is prefill().
        route: None / "chunk": chunk attention as above; "blocks": the same attention by blocks through the prompt kernel
        (ops.pq_chunk_attn_blocks, DESIGN.md 4.16: for long chunks), followed by the same store."""
        self._no_wide("extend")
        return self._extend("extend", "PagedPQCache.extend: requests are at different lengths; use extend_request(b, ...)", query_states, key_states, value_states, layer_idx, route)

    def extend_request(self, b, query_states, key_states, value_states, layer_idx, return_lse=False, route=None):
        """extend() for ONE request (tensors of batch 1) in slot b; the other slots, their host and device lengths, are not
        touched (they may keep decoding with use_dev_lengths=True).  On an empty slot this is prefill_request().
        return_lse=True: returns (out, lse), lse fp32 (1, nh, n) - every row's log-sum-exp over the keys it saw
        (ops.pq_chunk_attn).  The prompt kernel has none, so an empty slot is then served by chunk attention over the chunk
        alone, followed by the same store: the slot, the pages and every length are left as prefill_request leaves them.
        route: as extend(); an empty slot keeps its present routes whatever it says."""
        self._no_wide("extend_request")
        return self._extend_request("extend_request", b, query_states, key_states, value_states, layer_idx, return_lse, route)

    def extend_ragged(self, query_states, key_states, value_states, layer_idx, n_new, device_store=False):
        """extend_request() for every slot in ONE attention launch: tensors of batch bs padded to n_q = max(n_new) rows,
        slot b owns the first n_new[b] of them (n_new: bs host ints in [0, n_q]).  The launch reads each slot's lengths from
        `lengths[layer_idx]` on the device and n_new from a small device copy; the rows past n_new[b] - q, K and V - may
        hold anything and their output rows are zeros.  A slot with n_new[b] > 0 is then left exactly as
        extend_request(b, ...) with its own rows leaves it (pending encode-ahead joined, window rows encoded in ring order
        behind T_b, the chunk rows behind those, T_b += r_b + n_b, r_b = resid_start_b = 0, its device row rewritten); an
        empty slot is served by the same launch (the chunk only).  A slot with n_new[b] = 0 takes no part: host and device
        lengths, pages and window stay as they are.  device_store=True: the per-slot encodes and length copies are ONE
        ops.pq_store_ragged call behind the attention launch, on the same `lengths[layer_idx]` and device copy of n_new - same
        pages, same codes, same host and device lengths; the device rows are advanced by the call, not written from the host."""
        self._no_wide("extend_ragged")
        return self._extend_ragged("extend_ragged", query_states, key_states, value_states, layer_idx, n_new, device_store)

    def _extend_ragged(self, who_, query_states, key_states, value_states, layer_idx, n_new, device_store):
        """extend_ragged() for a cache of any format, as _extend: the public method refuses the wide ones first,
        million_amd.paged_turns serves them from here (who_: the caller's name in the messages).  The attention is the chunk op
        of the cache's format (ops.CodeFormat.chunk_op) with dev_lengths / dev_n_q, the store the format's."""
        attend = self._fmt.chunk_op(who_, None)
        n_new = [int(x) for x in n_new]
        n_q = query_states.size(2)
        if len(n_new) != self.bs or query_states.size(0) != self.bs or key_states.size(0) != self.bs or key_states.size(2) != n_q:
            raise RuntimeError(f"{who_}: tensors of batch {self.bs} and one n_new per slot")
        if any(n < 0 or n > n_q for n in n_new):
            raise RuntimeError(f"{who_}: n_new outside [0, {n_q}]")
        if device_store:
            self._no_sinks(f"{who_}(device_store=True)")
        who = [b for b in range(self.bs) if n_new[b] > 0]
        for b in who:      # capacity of every slot before anything is launched
            tot = int(self._T_a[layer_idx, b] + self._r_a[layer_idx, b]) + n_new[b]
            if tot > self.max_tokens:
                raise RuntimeError(f"PagedPQCache: {tot} tokens exceed max_tokens={self.max_tokens}")
        for b in who:
            self._join_side(layer_idx, b)
        if device_store:
            self._reserve_ragged(layer_idx, n_new)
        ids = self.page_ids[layer_idx]
        kres, vres = self.key_residual_cache[layer_idx], self.value_residual_cache[layer_idx]
        dev_n = torch.tensor(n_new, dtype=torch.int32).to(self.device)
        bound = int(self._T_a[layer_idx].max())
        out = attend(query_states, key_states, value_states, self.key_page_pool, self.value_page_pool, *self._cents(),
                     kres, vres, 0, M=self.M, C=self.C, n_tokens=bound, k_page_ids=ids, v_page_ids=ids,
                     page_size=self.page_size, dev_lengths=self.lengths[layer_idx], dev_n_q=dev_n,
                     **({"return_lse": True} if self.sink_tokens else {}))
        if self.sink_tokens:      # before the stores, as _extend_slot
            out, lse = out
            self._sink_merge(layer_idx, query_states, out, lse, dev_n=dev_n)
        if device_store:
            self._store_ragged(key_states, value_states, layer_idx, n_new, dev_n)
            return out
        for b in who:      # the encodes stay host-driven per slot, as extend_request does them
            self._store(key_states[b:b + 1, :, :n_new[b]], value_states[b:b + 1, :, :n_new[b]], layer_idx, n_new[b], b)
        return out

    # ---- fork: a slot becomes a copy of another -------------------------------------------------------------------------
    def _note_forked(self, src, dsts, n_tokens=None):
        """The slots dsts became a copy of slot src in every layer (fork) - of its first n_tokens tokens, all of them codes,
        when n_tokens is given.  Nothing of them is encoded ahead: their next flush is an in-line one."""
        for arr in (self._T_a, self._r_a, self._rs_a, self._seen_a):
            arr[:, dsts] = arr[:, [src]]
        if n_tokens is not None:
            self._T_a[:, dsts] = self._seen_a[:, dsts] = n_tokens
            self._r_a[:, dsts] = self._rs_a[:, dsts] = 0
        self._pre_a[:, dsts] = 0
        if self.sink_tokens:      # the source's sink rows, all of them whatever n_tokens says: they precede every coded token
            self._sink_a[:, dsts] = 0
            if n_tokens is None:
                self._seen_a[:, dsts] -= self._sink_a[:, [src]]      # (_note_sinks counts them as seen)
            self._ksink_all[:, dsts] = self._ksink_all[:, src:src + 1]
            self._vsink_all[:, dsts] = self._vsink_all[:, src:src + 1]
            self._note_sinks(slice(None), dsts, self._sink_a[:, [src]])

    def _note_restored(self, b, meta):
        """Slot b holds, in every layer, the request a snapshot describes (swap_in): T coded tokens, r window rows from ring
        row `start` on, `seen` tokens in all.  Nothing of it is encoded ahead."""
        self._T_a[:, b], self._r_a[:, b], self._rs_a[:, b], self._seen_a[:, b] = meta["T"], meta["r"], meta["start"], meta["seen"]
        self._pre_a[:, b] = 0

    def fork(self, src, dst, n_tokens=None):
        """Slot(s) dst (one slot or a list) become a copy of slot src, in every layer and in ONE launch (ops.cache_fork): the
        codes, the residual window and the lengths - what prefill_request of the same prompt and the same decode steps would
        have left there, bit for bit, without the prompt pass.  n_tokens (0 .. T of the source): only the first n_tokens coded
        tokens and no window - the slot a prompt of those tokens would have filled.
        Paging on demand (preallocate=False) SHARES the code pages: the destinations' table rows name the source's full pages
        (PageManager.share_page: a page returns to the free list when its last owner releases it) and only a partial tail
        page is copied, into one fresh id per (layer, kv head, destination).  Nothing ever writes a token below a request's
        T, so a shared page never changes under its owners.  A preallocated table keeps its fixed ids and gets a copy of
        every live page.  Call it between steps: the source must be at the same lengths in every layer (its pending
        encode-ahead work is joined, as extend does); every destination must be empty (release it first)."""
        self._no_wide("fork")
        return self._fork(src, dst, n_tokens)

    def _fork(self, src, dst, n_tokens):
        """fork() behind its refusal of wide caches: the launch is the format's (ops.CodeFormat.fork_pages; paged_turns.fork)."""
        dsts = [int(dst)] if np.isscalar(dst) else [int(x) for x in dst]
        src = int(src)
        nk, ps, nl = self.num_key_value_heads, self.page_size, self.layer_num
        if not 0 <= src < self.bs or not dsts or any(not 0 <= b < self.bs for b in dsts):
            raise RuntimeError(f"fork: slots outside [0, {self.bs})")
        if src in dsts or len(set(dsts)) != len(dsts):
            raise RuntimeError("fork: destinations must differ from the source and from each other")
        for b in dsts:
            if self._T_a[:, b].any() or self._r_a[:, b].any():
                raise RuntimeError(f"fork: slot {b} holds tokens (release it first)")
        cols = (self._T_a[:, src], self._r_a[:, src], self._rs_a[:, src])
        if self._ahead is not None or any((c != c[0]).any() for c in cols):
            raise RuntimeError("fork: the source is mid-step (its layers are at different lengths); fork between steps")
        T_src = int(self._T_a[0, src])
        if n_tokens is not None and not 0 <= int(n_tokens) <= T_src:
            raise RuntimeError(f"fork: n_tokens={n_tokens} outside [0, {T_src}] (the coded tokens of slot {src})")
        T = T_src if n_tokens is None else int(n_tokens)
        full, tail = divmod(T, ps)
        n_live = full + (1 if tail else 0)
        share = not self.preallocate
        if share and tail:
            need = nl * nk * len(dsts)
            returned = sum(len(self._host_pids[l][b][h]) for l in range(nl) for b in dsts for h in range(nk))
            if len(self.page_manager.free_pages) + returned < need:
                raise RuntimeError(f"fork: {need} free pages needed for the partial tail pages, "
                                   f"{len(self.page_manager.free_pages) + returned} left")
        for l in range(nl):
            self._join_side(l, src)
        buf = list(dsts)      # one host-to-device copy: the destination slots, then the tail ids (n_dst, layers, nh_k)
        if share:
            pm = self.page_manager
            for b in dsts:
                for l in range(nl):
                    for h in range(nk):
                        for pid in self._host_pids[l][b][h]:      # pages of an empty slot hold no token
                            pm.free_page(pid)
                        mine = self._host_pids[l][src][h][:full]
                        pm.share_pages(mine)
                        tid = pm.allocate_page() if tail else -1
                        if tail:
                            mine.append(tid)
                        buf.append(tid)
                        self._host_pids[l][b][h] = mine
                    self._pages_a[l, b] = n_live
        self._refresh_device_rows()      # the kernel reads the source's T, r, start from its device rows
        dev = torch.tensor(buf, dtype=torch.int32).to(self.device)
        tail_ids = dev[len(dsts):].view(len(dsts), nl, nk) if share else None
        self._fmt.fork_pages(self._page_ids_all, self.key_page_pool, self.value_page_pool, self._kres_all, self._vres_all,
                             self._lengths_all, dev[:len(dsts)], tail_ids, M=self.M, C=self.C, page_size=self.page_size, src=src,
                             share=share, n_pages_bound=n_live, prefix_tokens=-1 if n_tokens is None else T)
        self._note_forked(src, dsts, None if n_tokens is None else T)

    def sharing_stats(self) -> Dict:
        """PageManager.sharing_stats: pages with more than one owner, and the owners beyond the first."""
        return self.page_manager.sharing_stats()

    def release(self, b):
        """Request b has finished: its pages go back to the PageManager (on-demand paging; a preallocated table keeps its
        fixed ids for the slot's next request; a page shared through fork goes back with its last owner), its host and device
        lengths return to zero.  The other slots, and any captured graph (lengths are read on the device), are not touched."""
        for l in range(self.layer_num):
            if not self.preallocate:
                for h in range(self.num_key_value_heads):
                    for pid in self._host_pids[l][b][h]:
                        self.page_manager.free_page(pid)
                    self._host_pids[l][b][h] = []
                self._pages_a[l, b] = 0
            self._note_sinks(l, b, 0)
            self._T_a[l, b] = self._r_a[l, b] = self._rs_a[l, b] = self._seen_a[l, b] = self._pre_a[l, b] = 0
            self.lengths[l][b].zero_()

    reset_request = release

    # ---- swap: a request leaves its pages for host memory and comes back ---------------------------------------------------
    def _cent_digests(self):
        """sha256 of the key and of the value codebook bytes; computed on first use, once per pair of codebook tensors."""
        hit = getattr(self, "_cent_sha", None)
        if hit is None or hit[0] is not self.key_cent or hit[1] is not self.value_cent:
            import hashlib
            sha = lambda t: hashlib.sha256(t.detach().cpu().contiguous().view(torch.uint8).numpy().tobytes()).hexdigest()
            k = sha(self.key_cent)
            hit = self._cent_sha = (self.key_cent, self.value_cent, k, k if self.value_cent is self.key_cent else sha(self.value_cent))
        return hit[2], hit[3]

    def _swap_geometry(self) -> Dict:
        return dict(layer_num=self.layer_num, nh_k=self.num_key_value_heads, d=self.d, M=self.M, nbits=self.nbits,
                    page_size=self.page_size, resid_cap=self.extended_residual_size)

    def _swap_ranges(self, layer_bytes, staging_bytes):
        """[(layer0, n)]: the layers in ranges of at most staging_bytes, at least one layer each."""
        per = max(1, int(staging_bytes) // max(layer_bytes, 1))
        return [(l0, min(per, self.layer_num - l0)) for l0 in range(0, self.layer_num, per)]

    def swap_out(self, b, release=True, staging_bytes=64 << 20):
        """Slot(s) b (one slot or a list) as RequestSnapshot(s) in host memory: the codes, the residual window and the lengths
        of every layer, packed by ONE launch per range of layers (ops.cache_swap) into a device staging buffer of at most
        staging_bytes (at least one layer) and copied from there into a pinned blob, everything on the current stream.  The call
        synchronises before it returns; release=True then releases the slot(s) - pages shared through fork stay with their
        other owners.  swap_in() of the snapshot - into any empty slot of any cache of the same geometry and codebooks, on any
        GPU, in any process (formats.save_request) - decodes on with the bits this slot would have produced.  Call it between
        steps, as fork: the slot must be at the same lengths in every layer (its pending encode-ahead work is joined)."""
        self._no_sinks("swap_out / snapshot_request")
        self._no_wide("swap_out / snapshot_request")
        return self._swap_out(b, release, staging_bytes)

    def _swap_out(self, b, release, staging_bytes):
        """swap_out() behind its refusals: the launch, the row bytes and the snapshot version are the format's
        (ops.CodeFormat.swap_pages, swap_row_bytes, blob_version; paged_turns.swap_out)."""
        one = np.isscalar(b)
        slots = [int(b)] if one else [int(x) for x in b]
        nk, nl = self.num_key_value_heads, self.layer_num
        if not slots or any(not 0 <= s < self.bs for s in slots) or len(set(slots)) != len(slots):
            raise RuntimeError(f"swap_out: distinct slots inside [0, {self.bs}) expected")
        for s in slots:
            cols = (self._T_a[:, s], self._r_a[:, s], self._rs_a[:, s], self._seen_a[:, s])
            if self._ahead is not None or any((c != c[0]).any() for c in cols):
                raise RuntimeError(f"swap_out: slot {s} is mid-step (its layers are at different lengths); swap between steps")
        for l in range(nl):
            for s in slots:
                self._join_side(l, s)
        cuda = self.device.type == "cuda"
        k_sha, v_sha = self._cent_digests()
        snaps, rbs = [], []
        for s in slots:
            T, r, st = int(self._T_a[0, s]), int(self._r_a[0, s]), int(self._rs_a[0, s])
            rb = self._fmt.swap_row_bytes(T, r, self.page_size, self.M, self.d, self.C)
            meta = dict(version=self._fmt.blob_version, **self._swap_geometry(), T=T, r=r, start=st, seen=int(self._seen_a[0, s]),
                        key_cent_sha256=k_sha, value_cent_sha256=v_sha)
            snaps.append(RequestSnapshot(torch.empty(nl * nk * rb, dtype=torch.uint8, pin_memory=cuda), meta))
            rbs.append(rb)
        table = torch.tensor([[s, sn.meta["T"], sn.meta["r"], sn.meta["start"]] for s, sn in zip(slots, snaps)], dtype=torch.int32).to(self.device)
        layer_bytes = nk * sum(rbs)
        n_live = max(-(-sn.meta["T"] // self.page_size) for sn in snaps)
        ranges = self._swap_ranges(layer_bytes, staging_bytes)
        staging = torch.empty(max(16, ranges[0][1] * layer_bytes), dtype=torch.uint8, device=self.device)
        for l0, n in ranges:
            offs = np.concatenate([[0], np.cumsum([n * nk * rb for rb in rbs])]).astype(np.int64)
            self._fmt.swap_pages(L.MILLION_SWAP_PACK, self._page_ids_all, self.key_page_pool, self.value_page_pool, self._kres_all,
                                 self._vres_all, self._lengths_all, table, torch.from_numpy(offs[:-1].copy()).to(self.device), staging,
                                 M=self.M, C=self.C, page_size=self.page_size, layer0=l0, n_layers=n, n_pages_bound=n_live)
            for i, sn in enumerate(snaps):
                sn.blob[l0 * nk * rbs[i]:(l0 + n) * nk * rbs[i]].copy_(staging[int(offs[i]):int(offs[i + 1])], non_blocking=True)
        if cuda:
            torch.cuda.current_stream().synchronize()
        if release:
            for s in slots:
                self.release(s)
        return snaps[0] if one else snaps

    def snapshot_request(self, b):
        """swap_out(b, release=False): the slot keeps decoding, the snapshot is what it holds now."""
        return self.swap_out(b, release=False)

    def swap_in(self, b, snap, check_codebooks=True, staging_bytes=64 << 20):
        """Restore a RequestSnapshot into the empty slot b: paging on demand allocates private pages for it, a preallocated table
        uses its fixed ids; the blob goes host to device into a staging buffer of at most staging_bytes (at least one layer) and
        ONE launch per range of layers (ops.cache_swap) writes the pages, the window rows at their ring positions and the
        device lengths rows.  Refused, before anything changes (RuntimeError): a slot that holds tokens, a snapshot of another
        format version or geometry, more tokens than max_tokens, fewer free pages than the request needs (on demand), a blob of
        the wrong size, and - unless check_codebooks=False - codebooks other than the ones the codes were made with."""
        self._no_sinks("swap_in")
        self._no_wide("swap_in")
        return self._swap_in(b, snap, check_codebooks, staging_bytes)

    def _swap_in(self, b, snap, check_codebooks, staging_bytes):
        """swap_in() behind its refusals; it reads the snapshot version of the cache's format alone (1: 8-bit codes, 2: wide
        codes, packed or not - `packed` is no part of the geometry; paged_turns.swap_in)."""
        b = int(b)
        meta, blob = snap.meta, snap.blob
        nk, nl, ps = self.num_key_value_heads, self.layer_num, self.page_size
        if not 0 <= b < self.bs:
            raise RuntimeError(f"swap_in: slot {b} outside [0, {self.bs})")
        if self._T_a[:, b].any() or self._r_a[:, b].any():
            raise RuntimeError(f"swap_in: slot {b} holds tokens (release it first)")
        if meta.get("version") != self._fmt.blob_version:
            raise RuntimeError(f"swap_in: snapshot format version {meta.get('version')}, this library reads {self._fmt.blob_version}"
                               + (f" into a cache with nbits={self.nbits}" if self.nbits > 8 else ""))
        mine = self._swap_geometry()
        for key in _SNAPSHOT_GEOMETRY:
            if meta.get(key) != mine[key]:
                raise RuntimeError(f"swap_in: the snapshot has {key}={meta.get(key)}, this cache {mine[key]}")
        T, r, st, seen = (int(meta[key]) for key in ("T", "r", "start", "seen"))
        cap = self.extended_residual_size
        if T < 0 or not 0 <= r <= cap or not 0 <= st < max(cap, 1) or seen < 0:
            raise RuntimeError(f"swap_in: inconsistent snapshot T={T} r={r} start={st} seen={seen}")
        if T > self.max_tokens:
            raise RuntimeError(f"swap_in: {T} tokens exceed max_tokens={self.max_tokens}")
        rb = self._fmt.swap_row_bytes(T, r, ps, self.M, self.d, self.C)
        if blob.dtype != torch.uint8 or blob.dim() != 1 or blob.numel() != nl * nk * rb:
            raise RuntimeError(f"swap_in: a uint8 blob of {nl * nk * rb} bytes expected, got {blob.dtype} {tuple(blob.shape)}")
        n_live = -(-T // ps)
        if not self.preallocate:
            pm = self.page_manager
            returned = sum(len(self._host_pids[l][b][h]) for l in range(nl) for h in range(nk))
            room = pm.max_pages - pm.current_active_pages if pm.max_pages is not None else nl * nk * n_live      # (allocate_pages grows the pool)
            if len(pm.free_pages) + returned + room < nl * nk * n_live:
                raise RuntimeError(f"swap_in: {nl * nk * n_live} free pages needed, {len(pm.free_pages) + returned + room} left")
        if check_codebooks and (meta.get("key_cent_sha256"), meta.get("value_cent_sha256")) != self._cent_digests():
            raise RuntimeError("swap_in: the snapshot's codes were made with other codebooks (check_codebooks=False restores it anyway)")
        if not self.preallocate:
            for l in range(nl):
                for h in range(nk):
                    for pid in self._host_pids[l][b][h]:      # pages of an empty slot hold no token
                        self.page_manager.free_page(pid)
                    self._host_pids[l][b][h] = []
                self._pages_a[l, b] = 0
            for l in range(nl):
                self._assign_pages(l, n_live, b)
        dev = torch.tensor([b, T, r, st], dtype=torch.int32).to(self.device)
        table, offs = dev.view(1, 4), torch.zeros(1, dtype=torch.int64, device=self.device)
        ranges = self._swap_ranges(nk * rb, staging_bytes)
        staging = torch.empty(max(16, ranges[0][1] * nk * rb), dtype=torch.uint8, device=self.device)
        for l0, n in ranges:
            staging[:n * nk * rb].copy_(blob[l0 * nk * rb:(l0 + n) * nk * rb], non_blocking=True)
            self._fmt.swap_pages(L.MILLION_SWAP_UNPACK, self._page_ids_all, self.key_page_pool, self.value_page_pool, self._kres_all,
                                 self._vres_all, self._lengths_all, table, offs, staging, M=self.M, C=self.C, page_size=ps, layer0=l0,
                                 n_layers=n, n_pages_bound=n_live)
        self._note_restored(b, meta)

    def cleanup(self):
        """Reference PagedPQCache.cleanup (paged_pq_utils.py:1082-1118): drop every request's codes and window; the pools
        and (preallocated) page tables stay."""
        for b in range(self.bs):
            self.release(b)
        for l in range(self.layer_num):
            self.key_residual_cache[l].zero_()
            self.value_residual_cache[l].zero_()
        if self.sink_tokens:
            self._ksink_all.zero_()
            self._vsink_all.zero_()

    def _codes_rowmajor(self, layer_idx, T):
        """(bs, nh_k, T, M) row-major K and V codes gathered from the pages (dequantise-then-attend path only)."""
        npg = (T + self.page_size - 1) // self.page_size
        ids = self.page_ids[layer_idx][:, :, :npg].long()
        kc = self.key_page_pool[ids].reshape(self.bs, self.num_key_value_heads, npg * self.page_size, self.M)[:, :, :T]
        vc = self.value_page_pool[ids].permute(0, 1, 2, 4, 3).reshape(self.bs, self.num_key_value_heads, npg * self.page_size, self.M)[:, :, :T]
        return kc.contiguous(), vc.contiguous()

    def update(self, key_states, value_states, layer_idx, distort_recent=False):
        """The reference's non-kernel path on the paged store (paged_pq_utils.py:322-339 -> pq_utils.py:166-220): encode and
        store the new K/V rows into pages, return the full-length fp16 K/V for a dense attention - the dequantised past
        followed by the new rows as they are (or dequantised too with distort_recent).  No residual window on this path.
        extend() attends a block of new tokens to the codes and the window without the fp16 past."""
        self._no_sinks("update (the dequantise-then-attend path)")
        self._no_wide("update (the dequantise-then-attend path)")
        if not self._lockstep(layer_idx) or self._r_a[layer_idx, 0]:
            raise RuntimeError("PagedPQCache.update: lockstep requests and an empty residual window expected")
        n = key_states.size(2)
        T0 = int(self._T_a[layer_idx, 0])
        self._store(key_states, value_states, layer_idx, n)
        upto = T0 + n if distort_recent else T0
        if upto:
            kc, vc = self._codes_rowmajor(layer_idx, upto)
            past_k, past_v = ops.pq_decode(kc, self.key_cent), ops.pq_decode(vc, self.value_cent)
        else:
            past_k = past_v = None
        if distort_recent:
            return past_k, past_v
        if past_k is None:
            return key_states, value_states
        return torch.cat([past_k, key_states.to(past_k.dtype)], dim=2), torch.cat([past_v, value_states.to(past_v.dtype)], dim=2)

    def flush_to_pages(self, layer_idx: int, use_dev_lengths=False):
        """Encode the oldest page_size residual rows into a new K page and V page and move the window on
        (paged_pq_utils.py:130-210) - ONE launch (million_pq_flush): K encode, V encode and, with device-resident
        lengths, their advance.  Requests at different lengths (recycled slots): only those whose window is full flush -
        the launch reads every request's lengths on the device and skips the others (min_r).  A cache with wider codes keeps
        the lockstep-only _flush_wide."""
        if self.nbits > 8:
            full = self._r_a[layer_idx] >= self.extended_residual_size
            return self._flush_wide(layer_idx, use_dev_lengths, self._lockstep(layer_idx), full)
        return self._flush_pages(layer_idx, use_dev_lengths)

    def _flush_pages(self, layer_idx, use_dev_lengths):
        """The flush in one encode launch of the cache's format (ops.CodeFormat.flush_pages: ops.pq_flush, ops.pq_flush_wide):
        flush_to_pages of an 8-bit cache, and how million_amd.paged_turns flushes a cache of any format, requests at different
        lengths included."""
        cap, ps = self.extended_residual_size, self.page_size
        full = self._r_a[layer_idx] >= cap
        lock = self._lockstep(layer_idx)
        # lockstep: the host flushes at r >= page_size, the device (min_r = cap with device lengths) only full windows - the
        # host mirror must not move when the device will not (a direct call with page_size <= r < cap)
        if lock and self._r_a[layer_idx, 0] < (cap if use_dev_lengths else ps):
            return
        if not lock and not full.any():
            return
        if not lock and not use_dev_lengths:
            raise RuntimeError("PagedPQCache: requests at different lengths need use_dev_lengths=True")
        for b in (None,) if lock else np.flatnonzero(full):
            self._reserve(layer_idx, ps, b)      # pages are reserved per flushing request
        self._fmt.flush_pages(self.key_residual_cache[layer_idx], self.value_residual_cache[layer_idx], self._cents()[0],
                              self.key_page_pool, self.value_page_pool, self.page_ids[layer_idx],
                              n=ps, page_size=ps, token_start=int(self._T_a[layer_idx, 0]), x_row_start=int(self._rs_a[layer_idx, 0]),
                              dev_lengths=self.lengths[layer_idx] if use_dev_lengths else None,
                              min_r=cap if use_dev_lengths else 0)      # device lengths: only full windows flush (a captured step serves ragged batches too)
        self._dev_rows_stale |= not use_dev_lengths
        self._note_flushed(layer_idx if lock else (layer_idx, full))

    def _flush_wide(self, layer_idx, use_dev_lengths, lock, full):
        """flush_to_pages of a cache with uint16 codes (million_pq_flush is uint8-only): the two encodes of the in-line flush as
        two ops.pq_encode_into launches - K pages and V pages out of the ring window (x_row_start / x_row_mod) - and, with
        device-resident lengths, million_lengths_advance.  Lockstep requests only: the encodes take T and the ring start from
        the host mirror.  Codes, pages, window and lengths afterwards are the uint8 rule's with a wider code."""
        cap, ps = self.extended_residual_size, self.page_size
        if not lock:
            if not full.any():
                return
            raise RuntimeError(f"PagedPQCache: the flush of a cache with nbits={self.nbits} serves requests in lockstep only "
                               "(requests at different lengths: DESIGN.md 4.14)")
        if self._r_a[layer_idx, 0] < (cap if use_dev_lengths else ps):      # as the uint8 flush: the mirror moves when the device does
            return
        self._encode_to_pages(self.key_residual_cache[layer_idx], self.value_residual_cache[layer_idx], layer_idx, ps,
                              x_row_start=int(self._rs_a[layer_idx, 0]), x_row_mod=cap)
        if use_dev_lengths:
            ops.lengths_advance(self.lengths[layer_idx], ps, cap)
        self._dev_rows_stale |= not use_dev_lengths
        self._note_flushed(layer_idx)

    # ---- encode-ahead: the flush without a flush step ---------------------------------------------------------------
    # The reference flushes the oldest page_size window rows when the window is full (paged_pq_utils.py:359-361).  Those
    # rows are complete page_size steps after the previous flush - extended_residual_size - page_size steps BEFORE they
    # are flushed - and never change again, and a PQ code depends on nothing but its row and the codebook.  begin_step()
    # therefore encodes them early: ONE launch for all layers (million_pq_flush_layers, advance = 0) on a side stream,
    # in a step that needs nothing from it, next to that step's attention launches (the kernel's 4-wave, <= 32-register
    # workgroups fit on a CU beside an attention workgroup; nobody waits for it before the end of the step).  The flush
    # step itself is then a commit: the lengths move (host mirror; device mirror: one million_lengths_advance launch for
    # all layers) and no code is computed.  Codes, pages and lengths after the commit are exactly those of the in-line
    # flush; whatever cannot be served this way (requests at different lengths, a step that was skipped) falls back to it.
    def next_step_kind(self) -> str:
        """'plain' | 'pre' (encode-ahead rides along) | 'commit' (flush step, codes already there) | 'flush' (flush step)."""
        if self.nbits > 8:      # uint16 codes: this method's flush is the in-line one (encode-ahead: paged_turns.next_step_kind)
            return "flush" if (self._r_a >= self.extended_residual_size).any() else "plain"
        return self._next_step_kind()

    def _next_step_kind(self) -> str:
        """next_step_kind of an 8-bit cache, and of a cache of any format through million_amd.paged_turns."""
        cap = self.extended_residual_size
        full = self._r_a >= cap
        if full.any():
            return "commit" if full.all() and self._pre_a.all() else "flush"
        if (not self._pre_a.all() and self._r_a[0, 0] >= self.encode_ahead_at() and self._r_a[0, 0] >= self.page_size
                and self._all_lockstep()):
            groups = self._ea_groups()
            for gi, (g0, g1) in enumerate(groups):
                if not self._pre_a[g0:g1].all():
                    return "pre" if len(groups) == 1 else f"pre{gi}"
        return "plain"

    # (layer, request) pairs a step encodes ahead by default.  8-bit codes: 32 (below).  Wide codes: a pair is d x C units of work
    # (a 'pre' launch is 16 x the uint8 one's work per pair and more, and a wave of it scans a whole codebook row), and a step hides
    # EA_WIDE_UNITS of them per request up to 4 requests under its attention launches: measured at the Llama-3.1-8B shape
    # (profiles/encode_ahead_wide.txt) - 4 pairs per step at (d 128, C 4096) and one request, 16 at eight, 64 at
    # (C 1024) and eight; more pairs per step show in the step, fewer add steps, and every 'pre' step costs a fixed 50 - 100 us
    EA_PAIRS, EA_WIDE_UNITS = 32, 1 << 21

    def _ea_pairs(self) -> int:
        """(layer, request) pairs one step encodes ahead by default."""
        if self.nbits <= 8:
            return self.EA_PAIRS
        return max(1, self.EA_WIDE_UNITS * min(self.bs, 4) // (self.d * self.C))

    def _ea_groups(self):
        """Layer ranges encoded ahead per step: all layers in one step up to 32 (layer, request) pairs, else spread over
        consecutive steps (at 8 requests the attention launches leave few idle issue slots: all layers in one step made
        that step 1.6 x a plain one; 4 layers per step over 8 steps: see DESIGN.md 4.4).  A wide cache spreads by _ea_pairs()
        pairs per step.  encode_ahead_steps overrides either; page_size - 16 steps is the cap on the spread."""
        n = self.encode_ahead_steps
        if n is None:
            n = -(-self.bs * self.layer_num // self._ea_pairs())
        n = max(1, min(int(n), self.layer_num, max(1, self.page_size - 16)))
        per = -(-self.layer_num // n)
        return [(g0, min(g0 + per, self.layer_num)) for g0 in range(0, self.layer_num, per)]

    def encode_ahead_at(self) -> int:
        """Window fill at which the oldest page is encoded ahead (a few steps after the previous flush)."""
        return self.extended_residual_size - self.page_size + min(8, max(self.page_size // 8, 1))

    def _all_lockstep(self) -> bool:
        return all((a == a[0, 0]).all() for a in (self._T_a, self._r_a, self._rs_a))

    def begin_step(self, use_dev_lengths=False) -> str:
        """Call at the start of every decode step, before layer 0 (then decode every layer, in order).  Returns the kind of
        the step (next_step_kind).  Without it decoding_with_pages flushes in line, as the reference does."""
        if self.nbits > 8:      # reported only: decoding_with_pages flushes in line (encode-ahead: paged_turns.begin_step)
            return self.next_step_kind()
        return self._begin_step(use_dev_lengths)

    def _begin_step(self, use_dev_lengths) -> str:
        """begin_step of an 8-bit cache, and of a cache of any format through million_amd.paged_turns: the encode launch is the
        format's (ops.CodeFormat.flush_pages with advance=False: ops.pq_flush, ops.pq_flush_wide)."""
        kind = self._next_step_kind()
        cap, ps = self.extended_residual_size, self.page_size
        if kind == "commit":
            if use_dev_lengths:
                ops.lengths_advance(self._lengths_all.view(-1, 4), ps, cap)      # every layer, every request: one launch
            self._dev_rows_stale |= not use_dev_lengths
            self._note_flushed(...)
        elif kind == "flush":
            self.flush_ahead(use_dev_lengths=use_dev_lengths)
        elif kind.startswith("pre"):
            groups = self._ea_groups()
            G0, G1 = groups[int(kind[3:] or 0)]
            if not self._reserve(0, ps, ask=True):
                return "plain"      # the flush step will raise, as before
            for l in range(G0, G1):      # (pages on demand)
                self._reserve(l, ps)
            main = torch.cuda.current_stream()
            if self._side is None:
                self._side = torch.cuda.Stream(device=self.device)
            self._side.wait_stream(main)      # behind the appends of the previous step (the rows themselves are older)
            with torch.cuda.stream(self._side):
                # a grid of ONE layer's size whose workgroups walk the layers (one flush workgroup per CU at a time: what fits
                # beside an attention workgroup), in `encode_ahead_launches` launches
                nl_ = self.encode_ahead_launches
                if nl_ is None:
                    # replayed from a hipGraph: one launch per layer (the work trickles through the whole step: measured
                    # 1.04 x a plain step against 1.09 x for one long launch); eager: one launch (the host pays per launch).
                    # The rule was measured on the 8-bit kernel and is kept for the wide one, whose launches walk their
                    # pairs themselves (profiles/encode_ahead_wide.txt)
                    nl_ = self.layer_num if torch.cuda.is_current_stream_capturing() else 1
                nl_ = max(1, min(int(nl_), G1 - G0))
                per = (G1 - G0 + nl_ - 1) // nl_
                for g0 in range(G0, G1, per):
                    g1 = min(g0 + per, G1)
                    self._fmt.flush_pages(self._kres_all[g0:g1], self._vres_all[g0:g1], self._cents()[0], self.key_page_pool,
                                          self.value_page_pool, self._page_ids_all[g0:g1], n=ps, page_size=ps, token_start=int(self._T_a[0, 0]),
                                          x_row_start=int(self._rs_a[0, 0]),
                                          dev_lengths=self._lengths_all[g0:g1] if use_dev_lengths else None,
                                          min_r=ps if use_dev_lengths else 0, advance=False)
            self._pre_a[G0:G1] = 1
            self._pre_join = True      # joined behind the last layer's attention (decoding_with_pages)
        return kind

    def flush_ahead(self, use_dev_lengths=False, depth=2):
        """Flush the full windows of this step on a side stream instead of in front of each layer's attention: a layer's
        window rows and lengths do not depend on the current step's computation, so its flush launch (a 4-wave, 21-register
        kernel that fits on a CU beside an attention workgroup) runs under the attention launches of the layers before
        it; decoding_with_pages(layer) only waits for its own layer's flush event.  Call it at the start of a decode step
        (next_step_flushes() says when); every layer must then be decoded in this step, in order (the side stream is
        joined layer by layer - inside a hipGraph capture this becomes a fork / join of graph branches).
        The launches are issued `depth` layers ahead of the attention that needs them, not all at once: the host (and a
        replayed hipGraph, which submits its nodes in capture order) otherwise spends 32 flush submissions before the
        first attention launch gets out - measured: the main branch of the replayed step started ~300 us late.
        Results are identical to the in-line flush."""
        cap = self.extended_residual_size
        if self.nbits > 8:      # uint16 codes: decoding_with_pages flushes in line
            return
        todo = [l for l in range(self.layer_num) if (self._r_a[l] >= cap).any()]
        if not todo:
            return
        main = torch.cuda.current_stream()
        if self._side is None:
            self._side = torch.cuda.Stream(device=self.device)      # (a high-priority side stream changes nothing: measured)
        self._side.wait_stream(main)      # fork: behind everything this stream has queued (the previous step's appends)
        self._ahead = (todo, use_dev_lengths, max(1, int(depth)))
        self._ahead_issue(upto_layer=-1)

    def _ahead_issue(self, upto_layer):
        """Issue the pending side-stream flushes of the layers <= upto_layer + depth (in layer order)."""
        todo, use_dl, depth = self._ahead
        n = 0
        while n < len(todo) and todo[n] <= upto_layer + depth:
            n += 1
        if n:
            if upto_layer >= 0:
                # behind the attention launches issued so far (layers < upto_layer): a graph replay submits its nodes in
                # an order of the runtime's choosing - without this edge ROCm submitted the whole flush chain before the
                # first attention node (main branch ~300 us late); with it any topological order interleaves the two
                # chains.  The flush then has the attention launches of layers upto_layer .. upto_layer + depth - 1 to hide under.
                ev = torch.cuda.Event()
                ev.record(torch.cuda.current_stream())
                self._side.wait_event(ev)
            with torch.cuda.stream(self._side):
                for l in todo[:n]:
                    self.flush_to_pages(l, use_dev_lengths=use_dl)
                    ev = torch.cuda.Event()
                    ev.record(self._side)
                    self._flush_events[l] = ev
            del todo[:n]
        if not todo:
            self._ahead = None

    def decoding_with_pages(self, query_states, key_states, value_states, layer_idx, out=None, use_dev_lengths=False,
                            return_lse=False, lse=None):
        """One decode step of one layer (paged_pq_utils.py:341-386): flush if the window is full, append the
        new token's K/V row, fused attention over pages + window.  With use_dev_lengths=True every length
        is read on the device (the host mirror is still advanced), which makes the call graph-capturable and lets
        requests of different lengths share the launch.  return_lse=True (or an lse= buffer, fp32 (bs, nh, 1)): returns
        (out, lse), every head's log-sum-exp over the keys it attended to (ops.pq_decode_attn)."""
        cap = self.extended_residual_size
        if not self._join_flush(layer_idx) and (self._r_a[layer_idx] >= cap).any():      # not flushed ahead on the side stream: :359-361
            self.flush_to_pages(layer_idx, use_dev_lengths=use_dev_lengths)
        lock = self._lockstep(layer_idx)
        if not lock and not use_dev_lengths:
            raise RuntimeError("PagedPQCache: requests at different lengths need use_dev_lengths=True")
        r, rs = int(self._r_a[layer_idx, 0]), int(self._rs_a[layer_idx, 0])
        dl = self.lengths[layer_idx] if use_dev_lengths else None
        if self._ws is None:      # one workspace per cache (calls of one cache are stream-ordered)
            need = self._fmt.decode_workspace(query_states, self.key_residual_cache[layer_idx], M=self.M, C=self.C, page_size=self.page_size)
            self._ws = torch.zeros(need, dtype=torch.uint8, device=self.device)
        self._note_appended(layer_idx)
        self._dev_rows_stale |= not use_dev_lengths
        want_lse = return_lse or lse is not None
        if self.sink_tokens and not want_lse:      # the sink merge needs the past part's lse: one buffer per cache
            if self._sink_lse is None:
                self._sink_lse = torch.empty(self.bs, self.nh, 1, dtype=torch.float32, device=self.device)
            lse = self._sink_lse
        # append (:377-380) + attention (:386) in ONE launch: the new row is attended to and parked in the window.  The format's op:
        # pq_decode_attn, or the same launch over uint16 codes or packed pages with the codebooks as they are (csrc/attn_wide.hip)
        res = self._fmt.decode_pages(
            query_states, self.key_page_pool, self.value_page_pool, *self._cents(),
            self.key_residual_cache[layer_idx], self.value_residual_cache[layer_idx], r, M=self.M, C=self.C, page_ids=self.page_ids[layer_idx],
            k_new=key_states, v_new=value_states, n_tokens=self.max_tokens if use_dev_lengths else int(self._T_a[layer_idx, 0]),
            resid_start=rs, page_size=self.page_size, out=out, dev_lengths=dl, workspace=self._ws,
            **({"return_lse": True, "lse": lse} if return_lse or lse is not None else {}))
        if self.sink_tokens:      # the count is read on the device: a captured step follows release and a new prompt
            self._sink_merge(layer_idx, query_states, res[0].view(query_states.shape), res[1])
            res = res if want_lse else res[0]
        if self._pre_join and layer_idx == self.layer_num - 1:
            torch.cuda.current_stream().wait_stream(self._side)      # the step's encode-ahead launch ends with the step
            self._pre_join = False
        return res

    # the reference's non-paged entry point keeps working on the paged store
    decoding = decoding_with_pages

    # ---- draft verification: verify n rows per request without storing them, then commit the accepted ones -----------------
    # The draft rows of a request sit at consecutive positions and see the same past, so their attention over [codes; window]
    # is ONE decode launch with the rows as query heads (q (bs, nh, n, d) viewed as (bs, nh n, 1, d): virtual head h n + i
    # lies under kv head h // G); ops.attn_block_merge adds the causal part among the rows and parks their K/V in a staging
    # buffer.  Nothing is stored before acceptance is known, so nothing is rolled back: commit() appends the accepted rows
    # of every layer in one ops.window_commit, leaving the cache as that many decode steps would have.
    VERIFY_MAX_ROWS = 16

    def _verify_route(self, n) -> str:
        """The route verify() takes by default, from the measurement in profiles/verify_attn.txt (tools/verify_bench.py): "heads"
        while a kv head serves at most 64 rows (n G <= 64) - 0.19 to 0.67 of the chunk route's time at every measured shape, the
        decode launch growing by one pass over the codes per 16 rows - else chunk attention, which is not measured against it
        there.  A wide cache (paged_turns.verify) has its own rule: _verify_route_wide."""
        if not self._fmt.prepared:
            return self._verify_route_wide(n)
        return "heads" if n * (self.nh // self.num_key_value_heads) <= 64 else "chunk"

    VERIFY_WIDE_HEADS_ROWS, VERIFY_WIDE_HEADS_TOKENS, VERIFY_WIDE_SHORT_ROWS = 16, 16384, 8

    def _verify_route_wide(self, n) -> str:
        """The default route of paged_turns.verify on a cache with nbits 9 .. 12, from profiles/verify_wide.txt
        (tools/verify_wide_bench.py).  The "heads" route is ONE launch of the wide decode kernel, which has 16 score columns: it
        exists while a kv head has at most VERIFY_WIDE_HEADS_ROWS = 16 rows (n G <= 16); beyond that "chunk" is the only route.
        Measured at the Llama-3.1-8B shape (G = 4; 4K and 32K tokens; 1 and 8 requests - nothing else): at 32K "heads" is faster at
        every shape (0.73 to 0.97 of "chunk"); at 4K it is faster only with at most 8 rows and one request (0.66 to 0.76), else
        5 to 18 % slower.  So: "heads" when the longest request holds at least VERIFY_WIDE_HEADS_TOKENS tokens (nothing is measured
        between 4K and 32K: the line is drawn at 16K), below that only for at most VERIFY_WIDE_SHORT_ROWS rows of a single request.
        The lengths are the host mirror's, over every layer and slot: between steps, where verify runs, the layers agree."""
        rows = n * (self.nh // self.num_key_value_heads)
        if rows > self.VERIFY_WIDE_HEADS_ROWS:
            return "chunk"
        if int(self._T_a.max()) >= self.VERIFY_WIDE_HEADS_TOKENS:
            return "heads"
        return "heads" if rows <= self.VERIFY_WIDE_SHORT_ROWS and self.bs == 1 else "chunk"

    def _verify_books(self):
        """(codebooks, prepared blobs) as the format's verify and commit jobs take them: a job over 8-bit codes reads the prepared
        blobs alone, a wide one the codebooks as they are."""
        return ((None, None) if self._fmt.prepared else (self.key_cent, self.value_cent)), (self._kprep, self._vprep)

    def _mirror_sig(self):
        return (self._T_a.copy(), self._r_a.copy(), self._rs_a.copy())

    def _verify_trees(self, tree, n, who="verify"):
        """verify()'s tree= as bs tuples of n parents: one sequence of parents shared by every slot, or bs of them."""
        tree = list(tree)
        per_slot = len(tree) > 0 and all(isinstance(t, (list, tuple, np.ndarray)) for t in tree)
        if per_slot and len(tree) != self.bs:
            raise RuntimeError(f"{who}: {len(tree)} trees for {self.bs} slots (one sequence of parents for all, or one per slot)")
        try:
            return tuple(tuple(spec_tree.check_parents(t, n)) for t in (tree if per_slot else [tree] * self.bs))
        except (ValueError, TypeError) as e:
            raise RuntimeError(f"{who}: tree: {e}") from None

    def verify(self, query_states, key_states, value_states, layer_idx, n_draft=None, use_dev_lengths=True, route=None,
               return_lse=False, tree=None):
        """Attention of n <= 16 draft tokens per request over [the codes; the window; the draft rows, causally], one layer:
        q (bs, nh, n, d), K/V (bs, nh_k, n, d) -> out (bs, nh, n, d) (and lse (bs, nh, n) with return_lse).  Pure: lengths,
        pages, window and host mirror do not move; the rows' K/V are parked in a staging buffer of the cache for commit().
        n_draft: bs host ints in [0, n], the rows each slot verifies (default: n); rows past them are returned as zeros
        (lse -inf) and their q / K / V may hold anything.  route: "heads" - one decode launch over the rows as query heads,
        then ops.attn_block_merge; "chunk" - ops.pq_chunk_attn with the rows as chunk; None: _verify_route.  A side-stream
        flush that begin_step scheduled for the layer is joined first, as decoding_with_pages joins it.
        tree: the draft is a tree, not a chain - n parent indices shared by every slot, or bs such sequences; parents[i] in
        [-1, i) (a parent precedes its children; -1: a root, several allowed).  Node i is row i and sees its ancestors and
        itself instead of the rows j <= i (spec_tree.ancestor_masks, ops.attn_block_merge(dev_mask=)); n_draft[b] live nodes
        are a prefix of the tree.  The attention over the past is the chain's launch - it never looks at the order among the
        rows - on either route; "chunk" then runs chunk attention over the past only and the same masked block merge.  A
        malformed tree is refused (RuntimeError) before anything runs; commit() then takes path=."""
        self._no_wide("verify")
        return self._verify("verify", query_states, key_states, value_states, layer_idx, n_draft, use_dev_lengths, route, return_lse, tree)

    def _verify(self, who, query_states, key_states, value_states, layer_idx, n_draft, use_dev_lengths, route, return_lse, tree):
        """verify() for a cache of any format: the public method refuses the wide ones first, million_amd.paged_turns serves them
        from here (who: the caller's name in the messages).  The launches over the codes are the format's (ops.CodeFormat.decode_pages
        without an append, chunk_op); the block merge, the staging rows and the sink merge never see a code."""
        bs, nh, n, d = query_states.shape
        nk = self.num_key_value_heads
        if bs != self.bs or nh != self.nh or d != self.d or key_states.shape != (bs, nk, n, d) or value_states.shape != key_states.shape:
            raise RuntimeError(f"{who}: q (bs, nh, n, d) and K/V (bs, nh_k, n, d) of this cache expected, got {tuple(query_states.shape)} "
                               f"{tuple(key_states.shape)} {tuple(value_states.shape)}")
        if not 1 <= n <= self.VERIFY_MAX_ROWS:
            raise RuntimeError(f"{who}: {n} draft rows (1 .. {self.VERIFY_MAX_ROWS})")
        n_draft = [n] * bs if n_draft is None else [int(x) for x in n_draft]
        if len(n_draft) != bs or any(not 0 <= x <= n for x in n_draft):
            raise RuntimeError(f"{who}: one n_draft per slot, each in [0, {n}]")
        route = self._verify_route(n) if route is None else route
        if route not in ("heads", "chunk"):
            raise RuntimeError(f"{who}: route {route!r} ('heads', 'chunk' or None)")
        if route == "heads" and not self._fmt.prepared and n * (nh // nk) > self.VERIFY_WIDE_HEADS_ROWS:
            raise RuntimeError(f"{who}: route='heads' serves at most {self.VERIFY_WIDE_HEADS_ROWS} rows per kv head on a cache with nbits={self.nbits} "
                               f"(one launch of the wide decode kernel), got n * nh / nh_k = {n * (nh // nk)}; use route='chunk' (or None)")
        trees = None if tree is None else self._verify_trees(tree, n, who)
        self._join_flush(layer_idx)
        if not use_dev_lengths and not self._lockstep(layer_idx):
            raise RuntimeError("PagedPQCache: requests at different lengths need use_dev_lengths=True")
        rec = self._verify_rec
        sig = self._mirror_sig()
        if (rec is None or rec["n"] != n or rec["n_draft"] != n_draft or rec.get("tree") != trees
                or any(not np.array_equal(a, b) for a, b in zip(rec["sig"], sig))):
            rec = self._verify_rec = {"n": n, "n_draft": n_draft, "sig": sig, "layers": set(),
                                      "dev_n": torch.tensor(n_draft, dtype=torch.int32).to(self.device)}
            if trees is not None:      # the ancestor masks, once per record
                rec["tree"] = trees
                rec["dev_mask"] = torch.from_numpy(np.stack([spec_tree.ancestor_masks(t) for t in trees])).to(self.device)
        dev_n = rec["dev_n"]
        masked = {} if trees is None else {"dev_mask": rec["dev_mask"]}
        if self._kstage is None:
            shape = (self.layer_num, self.bs, nk, self.VERIFY_MAX_ROWS, self.d)
            self._kstage = torch.zeros(shape, dtype=self.scalar_t, device=self.device)
            self._vstage = torch.zeros(shape, dtype=self.scalar_t, device=self.device)
        ks, vs = self._kstage[layer_idx], self._vstage[layer_idx]
        T, r, rs = int(self._T_a[layer_idx, 0]), int(self._r_a[layer_idx, 0]), int(self._rs_a[layer_idx, 0])
        dl = self.lengths[layer_idx] if use_dev_lengths else None
        ids = self.page_ids[layer_idx]
        kres, vres = self.key_residual_cache[layer_idx], self.value_residual_cache[layer_idx]
        sinks = bool(self.sink_tokens)
        want_lse = return_lse or sinks
        if route == "heads":
            qv = query_states.contiguous()
            qh = qv.view(bs, nh * n, 1, d)
            ws = self._ws_verify
            if n not in ws:      # the decode launch's workspace for nh n heads: zeroed once, every call leaves it ready
                need = self._fmt.decode_workspace(qh, kres, M=self.M, C=self.C, page_size=self.page_size)
                ws[n] = torch.zeros(need, dtype=torch.uint8, device=self.device)
            out_a, lse_a = self._fmt.decode_pages(qh, self.key_page_pool, self.value_page_pool, *self._verify_books(), kres, vres, r,
                                                  M=self.M, C=self.C, n_tokens=self.max_tokens if use_dev_lengths else T, resid_start=rs,
                                                  page_ids=ids, page_size=self.page_size, dev_lengths=dl, workspace=ws[n], return_lse=True)
            out_a, lse_a = out_a.view(bs, nh, n, d), lse_a.view(bs, nh, n)
            res = ops.attn_block_merge(qv, key_states, value_states, out_a, lse_a, dev_n, out=out_a, return_lse=want_lse,
                                       k_stage=ks, v_stage=vs, **masked)
        elif trees is not None:      # chunk attention over the past only (the chunk kernel knows chains), then the masked block
            bound = int(self._T_a[layer_idx].max()) if use_dev_lengths else T
            out_a, lse_a = self._fmt.chunk_op(who, None)(query_states, None, None, self.key_page_pool, self.value_page_pool, *self._verify_books(),
                                                         kres, vres, r, M=self.M, C=self.C, n_tokens=bound, resid_start=rs,
                                                         k_page_ids=ids, v_page_ids=ids, page_size=self.page_size, dev_lengths=dl, dev_n_q=dev_n,
                                                         return_lse=True)
            res = ops.attn_block_merge(query_states, key_states, value_states, out_a, lse_a, dev_n, out=out_a, return_lse=want_lse,
                                       k_stage=ks, v_stage=vs, **masked)
        else:
            bound = int(self._T_a[layer_idx].max()) if use_dev_lengths else T
            res = self._fmt.chunk_op(who, None)(query_states, key_states, value_states, self.key_page_pool, self.value_page_pool,
                                                *self._verify_books(), kres, vres, r, M=self.M, C=self.C, n_tokens=bound, resid_start=rs, k_page_ids=ids,
                                                v_page_ids=ids, page_size=self.page_size, dev_lengths=dl, dev_n_q=dev_n,
                                                **({"return_lse": True} if want_lse else {}))
            ks[:, :, :n].copy_(key_states)
            vs[:, :, :n].copy_(value_states)
        if sinks:      # behind the block / tree merge, on its (out, lse): every draft row lies behind the sinks
            self._sink_merge(layer_idx, query_states, res[0], res[1], dev_n=dev_n)
            res = res if return_lse else res[0]
        rec["layers"].add(layer_idx)
        return res

    def _note_committed(self, n_accept):
        """commit() appended n_accept[b] rows to the window of slot b in every layer, as that many decode steps: a window the
        rows overflow was flushed once first (_note_flushed: T, r, the ring start, the encoded-ahead flag), then the append rule."""
        cap = self.extended_residual_size
        for b, a in enumerate(n_accept):
            if a:
                over = self._r_a[:, b] + a > cap
                if over.any():
                    self._note_flushed((over, b))
                self._r_a[:, b] += a
                self._seen_a[:, b] += a

    def commit(self, n_accept=None, *, path=None):
        """Append the first n_accept[b] of the rows verify() staged to the window of slot b, in every layer and in ONE call
        (ops.window_commit), exactly as n_accept[b] decode steps with those rows would have: codes, pages, window rows, host
        and device lengths; decoding_with_pages, begin_step, fork, swap_out and extend_* go on as after those steps.
        n_accept: bs host ints, 0 <= n_accept[b] <= n_draft[b] of the verify() that must have run for every layer since the
        cache last moved.  Call it between steps, as fork: refused (RuntimeError, before anything moves) mid-step, while a
        side-stream flush is pending, without a full verify, and when a slot's flush would pass max_tokens or the free
        pages.  A finished encode-ahead launch (begin_step) is joined first; pages on demand are taken before the launch.
        path (after verify(tree=), which needs it): bs sequences of node indices, each empty or a chain of the slot's tree from
        a root - parents[p[0]] == -1, parents[p[k]] == p[k - 1], every node below n_draft[b]; the rows of the path are appended
        in its order (ops.window_commit(dev_rows=)) and n_accept[b] = len(path[b]) (an n_accept given too must say the same).
        After a verify() without a tree, path[b] can only be range(a)."""
        self._no_wide("commit")
        return self._commit("commit", n_accept, path)

    def _commit(self, who, n_accept, path):
        """commit() for a cache of any format, as _verify: the one launch pair is the format's (ops.CodeFormat.commit_pages)."""
        rec = self._verify_rec
        if path is not None:
            try:
                path = [[int(x) for x in p] for p in path]
            except TypeError:
                raise RuntimeError(f"{who}: path is one sequence of node indices per slot") from None
            if n_accept is None:
                n_accept = [len(p) for p in path]
        elif n_accept is None:
            raise RuntimeError(f"{who}: n_accept or path expected")
        n_accept = [int(x) for x in n_accept]
        nl, ps, cap, nk = self.layer_num, self.page_size, self.extended_residual_size, self.num_key_value_heads
        cols = (self._T_a, self._r_a, self._rs_a)
        if self._ahead is not None or self._flush_events or any((c != c[0]).any() for c in cols):
            raise RuntimeError(f"{who}: the cache is mid-step (layers at different lengths, or a side-stream flush pending); commit between steps")
        if rec is None or len(rec["layers"]) != nl or any(not np.array_equal(a, b) for a, b in zip(rec["sig"], self._mirror_sig())):
            raise RuntimeError(f"{who}: verify() must have run for every layer, with the same n_draft, since the cache last moved")
        if len(n_accept) != self.bs or any(not 0 <= a <= nd for a, nd in zip(n_accept, rec["n_draft"])):
            raise RuntimeError(f"{who}: one n_accept per slot, each in [0, n_draft[b]] (n_draft = {rec['n_draft']})")
        trees = rec.get("tree")
        if path is None:
            if trees is not None:
                raise RuntimeError(f"{who}: the verification was of a tree: path= names the accepted chain of every slot")
        else:
            if len(path) != self.bs or [len(p) for p in path] != n_accept:
                raise RuntimeError(f"{who}: one path per slot, of n_accept[b] nodes (n_accept = {n_accept})")
            for b, p in enumerate(path):
                if trees is None:
                    if p != list(range(len(p))):
                        raise RuntimeError(f"{who}: path of slot {b} {p}: the verification was of a chain, whose paths are range(a)")
                elif not spec_tree.is_path(trees[b], p, rec["n_draft"][b]):
                    raise RuntimeError(f"{who}: path of slot {b} {p} is no chain from a root of its tree {list(trees[b])} below "
                                       f"n_draft = {rec['n_draft'][b]}")
        flush = [b for b, a in enumerate(n_accept) if a and self._r_a[0, b] + a > cap]
        for b in flush:
            if int(self._T_a[0, b]) + ps > self.max_tokens:
                raise RuntimeError(f"PagedPQCache: {int(self._T_a[0, b]) + ps} tokens exceed max_tokens={self.max_tokens}")
        if not self.preallocate and flush:
            pm = self.page_manager
            need = sum(max(0, -(-(int(self._T_a[l, b]) + ps) // ps) - int(self._pages_a[l, b])) for l in range(nl) for b in flush) * nk
            room = pm.max_pages - pm.current_active_pages if pm.max_pages is not None else need
            if len(pm.free_pages) + room < need:
                raise RuntimeError(f"{who}: {need} free pages needed, {len(pm.free_pages) + room} left")
        if self._pre_join:
            torch.cuda.current_stream().wait_stream(self._side)      # rows encoded ahead: a flush below encodes them again, same codes
            self._pre_join = False
        for b in flush:
            for l in range(nl):
                self._reserve(l, ps, b)
        self._verify_rec = None
        if not any(n_accept):
            return
        self._refresh_device_rows()      # window_commit reads and advances every slot's device rows
        dev_n = torch.tensor(n_accept, dtype=torch.int32).to(self.device)
        rows = {}
        if trees is not None:
            idx = np.zeros((self.bs, rec["n"]), np.int32)
            for b, p in enumerate(path):
                idx[b, :len(p)] = p
            rows["dev_rows"] = torch.from_numpy(idx).to(self.device)
        self._fmt.commit_pages(self._kstage, self._vstage, self._kres_all, self._vres_all, *self._verify_books(), self.key_page_pool,
                               self.value_page_pool, self._page_ids_all, self._lengths_all, dev_n, M=self.M, C=self.C, n_bound=rec["n"], **rows)
        self._note_committed(n_accept)

    # ---- host mirror management for captured (hipGraph) decode steps ------------------------------
    # During stream capture the Python above runs once (advancing the host mirror) but no kernel
    # executes; under replay the kernels run but no Python does.  The harness therefore restores the
    # mirror after capture and calls note_replayed_step() after every replay.
    def host_state(self):
        """(seen, r, T, resid_start), each (layers, requests) - what set_host_state takes back (it also takes one value per
        layer for all requests)."""
        return (self._seen_a.copy(), self._r_a.copy(), self._T_a.copy(), self._rs_a.copy(), self._pre_a.copy())

    def set_host_state(self, st):
        """(seen, r, T, resid_start[, encoded-ahead flags]); four entries: the flags are cleared."""
        for arr, v in zip((self._seen_a, self._r_a, self._T_a, self._rs_a), st):
            self._set_rows(arr, v)
        self._pre_a[:] = 0
        if len(st) > 4:
            self._set_rows(self._pre_a, st[4])

    def capture_states(self, st=None):
        """[(kind, host state)] - one host state per kind of step, for capturing one hipGraph per kind with device-resident
        lengths (begin_step + all layers).  st: the state to derive them from (default: now)."""
        st = self.host_state() if st is None else st
        L_, cap = self.layer_num, self.extended_residual_size
        r_now = int(st[1][0][0])
        r_plain = r_now if r_now < cap else 0
        groups = self._ea_groups()
        pre = [("pre" if len(groups) == 1 else f"pre{gi}",
                (st[0], [self.encode_ahead_at() + gi] * L_, st[2], st[3], [1 if l < g0 else 0 for l in range(L_)]))
               for gi, (g0, g1) in enumerate(groups)]
        return [("plain", (st[0], [r_plain] * L_, st[2], st[3], [1] * L_))] + pre + [
                ("commit", (st[0], [cap] * L_, st[2], st[3], [1] * L_)),
                ("flush", (st[0], [cap] * L_, st[2], st[3], [0] * L_))]

    def next_step_flushes(self, layer_idx: int = 0) -> bool:
        return bool((self._r_a[layer_idx] >= self.extended_residual_size).any())

    def note_replayed_step(self, kind=None):
        """The host-mirror transitions of one replayed step of the given kind (default: next_step_kind())."""
        kind = self.next_step_kind() if kind is None else kind
        self._note_replayed(kind)

    def _note_replayed(self, kind):
        cap, ps = self.extended_residual_size, self.page_size
        if kind in ("commit", "flush"):
            self._note_flushed(self._r_a >= cap)
        elif kind.startswith("pre"):
            g0, g1 = self._ea_groups()[int(kind[3:] or 0)]
            if self._reserve(0, ps, ask=True):      # (else begin_step encoded nothing)
                self._pre_a[g0:g1] = 1
        self._note_appended()

    def code_bytes_per_token(self) -> float:
        """Bytes one token's codes take per kv head and side: M codes of 1 byte (nbits 8), 2 bytes (nbits 9 .. 12), or
        (8 + h) / 8 bytes in packed pages."""
        if self.packed:
            return self.M * (8 + ops.packed_hi_bits(self.C)) / 8
        return float(self.M * self.key_page_pool.element_size())

    def pq_cache_size(self):
        """Bytes of the codes the live tokens hold in the pools, K and V."""
        return 2 * self.num_key_value_heads * self.code_bytes_per_token() * float(self._T_a.sum())

    def get_cache_stats(self) -> Dict:
        """paged_pq_utils.py:898-939 (same keys) + the page-manager counters."""
        layer_stats = [{"layer_idx": l, "seen_tokens": self.seen_tokens[l], "residual_tokens": self.residualed_tokens[l],
                        "key_cache_tokens": self._T[l], "value_cache_tokens": self._T[l]} for l in range(self.layer_num)]
        mb = 1024 * 1024
        cache_mb = float(self.pq_cache_size()) / mb
        resid_mb = sum(c.numel() * c.element_size() for c in self.key_residual_cache + self.value_residual_cache) / mb
        sink_mb = 2 * self.layer_num * self.bs * self.num_key_value_heads * self.sink_tokens * self.d * 2 / mb      # K and V buffers, fp16
        return {"layer_stats": layer_stats, "total_memory_usage_mb": cache_mb + resid_mb + sink_mb,
                "memory_breakdown": {"cache_memory_mb": cache_mb, "residual_memory_mb": resid_mb, "sink_memory_mb": sink_mb,
                                     "prefill_residual_memory_mb": 0.0, "total_memory_mb": cache_mb + resid_mb + sink_mb},
                "sink_tokens": self.sink_tokens, "sink_rows_live": int(self._sink_a.sum()),
                "page_manager": self.page_manager.get_stats()}
