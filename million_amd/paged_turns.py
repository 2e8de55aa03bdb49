"""Later turns on a wide PagedPQCache: extend / extend_request for caches with nbits 9 .. 12, packed or not.

PagedPQCache's own extend methods serve 8-bit caches and refuse the wide ones by name.  The kernels a wide cache
needs for a later turn exist - chunk attention over uint16 pages (ops.pq_chunk_attn_wide) and over packed pages
(ops.pq_chunk_attn_packed), and the block route over either (ops.pq_chunk_attn_blocks) - so this module opens them from outside,
as shared_prefix.py serves a frozen prompt.

The turn logic is the cache's, in one copy: PagedPQCache._extend / _extend_request check the route, the lockstep and the capacity
before anything is joined or launched, join pending side work of the layer, prefill an empty cache or slot, and otherwise let the
new rows attend [the codes in the pages; the residual window; themselves, causally] through the op of the cache's format
(ops.CodeFormat.chunk_op) before cache._store() leaves the cache as prefill() of the whole sequence would.  The
cache's public methods are those bodies behind the refusal of wide caches; the two functions here are those bodies without it,
and so mean, word for word, what PagedPQCache.extend / extend_request mean on an 8-bit cache.  A packed cache never sees a uint16
copy of its pool.

    route            packed cache                            unpacked cache
    None / "chunk"   ops.pq_chunk_attn_packed                ops.pq_chunk_attn_wide
    "blocks"         ops.pq_chunk_attn_blocks(packed=True)   ops.pq_chunk_attn_blocks

extend_ragged, prefill_ragged, fork, swap, verify / commit and sinks on wide caches stay refused by the cache."""
from __future__ import annotations


def extend(cache, query_states, key_states, value_states, layer_idx, route=None):
    """PagedPQCache.extend for a cache with nbits 9 .. 12 (packed or not): n new tokens of one layer, every request in lockstep.
    Returns their attention (bs, nh, n, d); the cache is left as prefill() of the whole sequence leaves it.  On an empty cache
    this is cache.prefill().  A cache with nbits = 8 is handed to its own method."""
    if cache.nbits <= 8:
        return cache.extend(query_states, key_states, value_states, layer_idx, route=route)
    return cache._extend("paged_turns.extend", "paged_turns.extend: requests are at different lengths; use extend_request(cache, b, ...)",
                         query_states, key_states, value_states, layer_idx, route)


def extend_request(cache, b, query_states, key_states, value_states, layer_idx, return_lse=False, route=None):
    """PagedPQCache.extend_request for a cache with nbits 9 .. 12 (packed or not): extend() for ONE request (tensors of batch 1)
    in slot b; the other slots and their lengths are not touched.  On an empty slot this is cache.prefill_request() - with
    return_lse=True chunk attention over the chunk alone and the same store, as on an 8-bit cache (an empty slot keeps these
    routes whatever `route` says).  return_lse=True: (out, lse), lse fp32 (1, nh, n)."""
    if cache.nbits <= 8:
        return cache.extend_request(b, query_states, key_states, value_states, layer_idx, return_lse=return_lse, route=route)
    return cache._extend_request("paged_turns.extend_request", b, query_states, key_states, value_states, layer_idx, return_lse, route)
