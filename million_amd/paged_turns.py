"""Later turns on a wide PagedPQCache: extend / extend_request for caches with nbits 9 .. 12, packed or not.

PagedPQCache's own extend methods serve 8-bit caches and refuse the wide ones by name.  The kernels a wide cache
needs for a later turn exist - chunk attention over uint16 pages (ops.pq_chunk_attn_wide) and over packed pages
(ops.pq_chunk_attn_packed), and the block route over either (ops.pq_chunk_attn_blocks) - so this module serves such a cache from
outside, as shared_prefix.py serves a frozen prompt: it drives the cache through `ops` and through the cache's own store step.

The two functions mean, word for word, what PagedPQCache.extend / extend_request mean on an 8-bit cache: pending side work of
the layer is joined, an empty cache or slot is prefilled, otherwise the new rows attend [the codes in the pages; the residual
window; themselves, causally] and cache._store() then leaves the cache as prefill() of the whole sequence would - the window in
ring order and then the new rows encoded behind T (into uint16 or packed pages), the window emptied, host and device lengths
advanced.  A packed cache never sees a uint16 copy of its pool.

    route            packed cache                            unpacked cache
    None / "chunk"   ops.pq_chunk_attn_packed                ops.pq_chunk_attn_wide
    "blocks"         ops.pq_chunk_attn_blocks(packed=True)   ops.pq_chunk_attn_blocks

extend_ragged, prefill_ragged, fork, swap, verify / commit and sinks on wide caches stay refused by the cache."""
from __future__ import annotations

from . import ops


def _attend_op(cache, who, route):
    """(op, extra keyword arguments) of a call on this cache; a route that does not exist is a ValueError."""
    if route is None or route == "chunk":
        return (ops.pq_chunk_attn_packed if cache.packed else ops.pq_chunk_attn_wide), {}
    if route == "blocks":
        return ops.pq_chunk_attn_blocks, ({"packed": True} if cache.packed else {})
    raise ValueError(f"paged_turns.{who}: route={route!r} (None, 'chunk' or 'blocks')")


def _extend_slot(cache, attend, kw, q, k, v, layer_idx, b, return_lse=False, all_rows=False):
    """b = None: every request (lockstep); else request b with batch-1 tensors: PagedPQCache._extend_slot for a wide cache."""
    i, sel = (0, slice(None)) if b is None else (b, slice(b, b + 1))
    T, r, rs = int(cache._T_a[layer_idx, i]), int(cache._r_a[layer_idx, i]), int(cache._rs_a[layer_idx, i])
    n = k.size(2)      # (the callers checked the capacity)
    ids =cache.page_ids[layer_idx][sel]
    out = attend(q, k, v, cache.key_page_pool, cache.value_page_pool, cache.key_cent, cache.value_cent,
                 cache.key_residual_cache[layer_idx][sel], cache.value_residual_cache[layer_idx][sel], r,
                 M=cache.M, C=cache.C, n_tokens=T, resid_start=rs, k_page_ids=ids, v_page_ids=ids, page_size=cache.page_size,
                 **({"return_lse": True} if return_lse else {}), **kw)
    cache._store(k, v, layer_idx, n, b, all_rows=all_rows)      # the window in ring order, then the new rows
    return out


def extend(cache, query_states, key_states, value_states, layer_idx, route=None):
    """PagedPQCache.extend for a cache with nbits 9 .. 12 (packed or not): n new tokens of one layer, every request in lockstep.
    Returns their attention (bs, nh, n, d); the cache is left as prefill() of the whole sequence leaves it.  On an empty cache
    this is cache.prefill().  A cache with nbits = 8 is handed to its own method."""
    if cache.nbits <= 8:
        return cache.extend(query_states, key_states, value_states, layer_idx, route=route)
    attend, kw = _attend_op(cache, "extend", route)      # a route that does not exist is said first
    if not cache._lockstep(layer_idx):
        raise RuntimeError("paged_turns.extend: requests are at different lengths; use extend_request(cache, b, ...)")
    n = key_states.size(2)
    if int(cache._T_a[layer_idx, 0]) + int(cache._r_a[layer_idx, 0]) + n > cache.max_tokens:
        raise RuntimeError(f"PagedPQCache: {int(cache._T_a[layer_idx, 0]) + int(cache._r_a[layer_idx, 0]) + n} tokens exceed "
                           f"max_tokens={cache.max_tokens}")
    cache._join_side(layer_idx)
    if cache._T_a[layer_idx, 0] == 0 and cache._r_a[layer_idx, 0] == 0:
        return cache.prefill(query_states, key_states, value_states, layer_idx)
    return _extend_slot(cache, attend, kw, query_states, key_states, value_states, layer_idx, None)


def extend_request(cache, b, query_states, key_states, value_states, layer_idx, return_lse=False, route=None):
    """PagedPQCache.extend_request for a cache with nbits 9 .. 12 (packed or not): extend() for ONE request (tensors of batch 1)
    in slot b; the other slots and their lengths are not touched.  On an empty slot this is cache.prefill_request() - with
    return_lse=True chunk attention over the chunk alone and the same store, as on an 8-bit cache (an empty slot keeps these
    routes whatever `route` says).  return_lse=True: (out, lse), lse fp32 (1, nh, n)."""
    if cache.nbits <= 8:
        return cache.extend_request(b, query_states, key_states, value_states, layer_idx, return_lse=return_lse, route=route)
    attend, kw = _attend_op(cache, "extend_request", route)
    if key_states.size(0) != 1 or query_states.size(0) != 1:
        raise RuntimeError("paged_turns.extend_request: tensors of batch 1")
    n = key_states.size(2)
    if int(cache._T_a[layer_idx, b]) + int(cache._r_a[layer_idx, b]) + n > cache.max_tokens:
        raise RuntimeError(f"PagedPQCache: {int(cache._T_a[layer_idx, b]) + int(cache._r_a[layer_idx, b]) + n} tokens exceed "
                           f"max_tokens={cache.max_tokens}")
    cache._join_side(layer_idx, b)
    if cache._T_a[layer_idx, b] == 0 and cache._r_a[layer_idx, b] == 0:
        if return_lse:
            chunk, ckw = _attend_op(cache, "extend_request", None)
            return _extend_slot(cache, chunk, ckw, query_states, key_states, value_states, layer_idx, b, return_lse=True, all_rows=True)
        return cache.prefill_request(b, query_states, key_states, value_states, layer_idx)
    return _extend_slot(cache, attend, kw, query_states, key_states, value_states, layer_idx, b, return_lse=return_lse)
