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

Requests at different lengths.  The cache's own flush of a wide cache is two encode launches that take T and the
ring start from the host, so it serves lockstep batches only, and its ragged calls are refused.  The functions below open the
ragged life the same way - the bodies are the cache's (PagedPQCache._flush_pages, which is flush_to_pages of an 8-bit cache;
_prefill_ragged, _extend_ragged), the launches the format's (ops.CodeFormat.flush_pages, store_ragged_pages, chunk_op):

    call             packed cache                                   unpacked cache
    flush / decode   ops.pq_flush_wide(packed=True)                 ops.pq_flush_wide
    prefill_ragged   ops.prefill_attn(dev_spans=), then the store   the same
    extend_ragged    ops.pq_chunk_attn_packed(dev_lengths=, dev_n_q=)   ops.pq_chunk_attn_wide(dev_lengths=, dev_n_q=)
    device_store     ops.pq_store_ragged_wide(packed=True)          ops.pq_store_ragged_wide

Draft verification.  verify / commit below are PagedPQCache._verify / _commit, the bodies of the cache's own
methods, with the launches of the cache's format (ops.CodeFormat.decode_pages, chunk_op, commit_pages); the block merge
(ops.attn_block_merge, chain or dev_mask=) takes fp16 rows and (out, lse) and never sees a code:

    call / route       packed cache                                  unpacked cache
    verify "heads"     ops.pq_decode_attn_packed, no append          ops.pq_decode_attn_wide, no append   then ops.attn_block_merge
                       (the kernel has 16 score columns: n nh / nh_k <= 16, else refused - "chunk" has no such limit)
    verify "chunk"     ops.pq_chunk_attn_packed(dev_n_q=)            ops.pq_chunk_attn_wide(dev_n_q=)   (a tree: over the past only,
                                                                                                    then the masked block merge)
    commit             ops.window_commit_wide(packed=True)           ops.window_commit_wide         (dev_rows= for a tree's path)

Fork and swap.  fork / swap_out / snapshot_request / swap_in below are PagedPQCache._fork / _swap_out / _swap_in,
the bodies of the cache's own methods - the same host-mirror transitions, page sharing and free-page accounting - with the
launches of the cache's format (ops.CodeFormat.fork_pages, swap_pages, swap_row_bytes):

    call                  packed cache                          unpacked cache
    fork                  ops.cache_fork_wide(packed=True)      ops.cache_fork_wide
    swap_out / swap_in    ops.cache_swap_wide(packed=True)      ops.cache_swap_wide       blob format 2, snapshot version 2

Blob format 2 holds packed pages whatever the pool holds, so a snapshot of an unpacked cache is (8 + h) / 16 of its code bytes and
restores into a packed cache of the same geometry, and the other way round: `packed` is no part of a snapshot's geometry.

Encode-ahead.  next_step_kind / begin_step / note_replayed_step below are PagedPQCache._next_step_kind /
_begin_step / _note_replayed, the bodies of the cache's own methods: the oldest page of window rows is encoded a few steps after
the previous flush by ONE launch per range of layers on a side stream beside that step's attention launches
(ops.CodeFormat.flush_pages with advance=False: ops.pq_flush_wide -> million_pq_flush_wide_layers, 4-wave workgroups that walk the
(layer, request) pairs), and the flush step is a 'commit': ops.lengths_advance over every layer's rows and the host mirror, no
code computed.  decode() above needs nothing new: after a 'commit' no window is full, and on 'flush' - requests at different
lengths, a begin_step that was skipped, flags cleared by fork / release / verify-commit - it flushes in line as before.

    call               packed cache                                        unpacked cache
    begin_step 'pre'   ops.pq_flush_wide(packed=True, advance=False)       ops.pq_flush_wide(advance=False)
    begin_step 'commit'   ops.lengths_advance (device lengths) and the mirror, whatever the format

The cache's own methods keep doing on a wide cache exactly what they did: decoding_with_pages / flush_to_pages flush in lockstep
only, prefill_ragged / extend_ragged, verify / commit, fork, swap_out / snapshot_request / swap_in raise NotImplementedError,
next_step_kind / begin_step report 'plain' / 'flush' and launch nothing, flush_ahead does nothing.  Sinks, SharedPrefix, a
side-stream flush_ahead and a wide backend of the lifecycle drivers stay unbuilt on wide caches."""
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


def flush(cache, layer_idx, use_dev_lengths=False):
    """PagedPQCache.flush_to_pages for a cache with nbits 9 .. 12 (packed or not), requests at different lengths included: the
    8-bit cache's own body (PagedPQCache._flush_pages) - lockstep with host lengths flushes at r >= page_size, with device lengths
    only the full windows flush (the launch reads every request's row and skips the others), requests at different lengths need
    use_dev_lengths=True -
    in one encode launch (ops.pq_flush_wide) plus, with device lengths, its one-thread-per-request advance.  A cache with
    nbits = 8 is handed to its own method."""
    if cache.nbits <= 8:
        return cache.flush_to_pages(layer_idx, use_dev_lengths=use_dev_lengths)
    return cache._flush_pages(layer_idx, use_dev_lengths)


def decode(cache, query_states, key_states, value_states, layer_idx, out=None, use_dev_lengths=False, return_lse=False, lse=None):
    """PagedPQCache.decoding_with_pages for a cache with nbits 9 .. 12 (packed or not) whose requests may be at different
    lengths: the full windows are flushed here first (flush() above), so none is full when the cache's own method runs - its
    flush does nothing and the step is its unchanged fused launch.  Captured, a step is one graph per step kind
    (cache.next_step_kind(): 'plain' / 'flush'; with begin_step() below in front of layer 0: next_step_kind() below), as for 8-bit
    caches: the flush launch of a captured 'flush' step is gated on the device (min_r), so its replays follow the rows.  A cache
    with nbits = 8 is handed to its own method."""
    if cache.nbits > 8 and (cache._r_a[layer_idx] >= cache.extended_residual_size).any():
        cache._flush_pages(layer_idx, use_dev_lengths)
    return cache.decoding_with_pages(query_states, key_states, value_states, layer_idx, out=out, use_dev_lengths=use_dev_lengths,
                                     return_lse=return_lse, lse=lse)


def next_step_kind(cache) -> str:
    """PagedPQCache.next_step_kind for a cache with nbits 9 .. 12 (packed or not), with the 8-bit method's meaning word for word:
    'plain' | 'pre' / 'preN' (encode-ahead rides along; N: the layers are spread over several steps) | 'commit' (flush step, the
    codes are already in their pages) | 'flush' (flush step: decode() flushes in line).  A cache with nbits = 8 is handed to its
    own method."""
    if cache.nbits <= 8:
        return cache.next_step_kind()
    return cache._next_step_kind()


def begin_step(cache, use_dev_lengths=False) -> str:
    """PagedPQCache.begin_step for a cache with nbits 9 .. 12 (packed or not): call at the start of every decode step, before
    layer 0, then decode() every layer in order.  Returns the kind of the step (next_step_kind above).  'pre' / 'preN': the oldest
    page of window rows of the step's layers is encoded into its pages by one ops.pq_flush_wide(advance=False) launch per range
    of layers on a side stream, joined behind the last layer's attention; 'commit': the lengths move (with device lengths ONE
    ops.lengths_advance over every layer's rows) and no code is computed; 'flush' launches nothing here: decode() flushes in line.
    Without this call decode() flushes in line at every flush step, as before.  A cache with nbits = 8 is handed to its own
    method."""
    if cache.nbits <= 8:
        return cache.begin_step(use_dev_lengths=use_dev_lengths)
    return cache._begin_step(use_dev_lengths)


def note_replayed_step(cache, kind=None):
    """PagedPQCache.note_replayed_step for a cache with nbits 9 .. 12 (packed or not): the host-mirror transitions of one replayed
    step (a hipGraph captured per kind from cache.capture_states()) of the given kind - default: next_step_kind(cache) above.
    A cache with nbits = 8 is handed to its own method."""
    if cache.nbits <= 8:
        return cache.note_replayed_step(kind)
    cache._note_replayed(next_step_kind(cache) if kind is None else kind)


def prefill_ragged(cache, query_states, key_states, value_states, layer_idx, n_new, device_store=False, return_lse=False):
    """PagedPQCache.prefill_ragged for a cache with nbits 9 .. 12 (packed or not): the prompts of several empty slots, of
    different lengths, in ONE attention launch; every slot with n_new[b] > 0 is left as cache.prefill_request(b, ...) with its
    own rows leaves it.  device_store=True: the stores are ONE ops.pq_store_ragged_wide call behind the attention launch - same
    pages, same codes, same lengths.  A cache with nbits = 8 is handed to its own method."""
    if cache.nbits <= 8:
        return cache.prefill_ragged(query_states, key_states, value_states, layer_idx, n_new, device_store=device_store, return_lse=return_lse)
    return cache._prefill_ragged("paged_turns.prefill_ragged", query_states, key_states, value_states, layer_idx, n_new, device_store, return_lse)


def extend_ragged(cache, query_states, key_states, value_states, layer_idx, n_new, device_store=False):
    """PagedPQCache.extend_ragged for a cache with nbits 9 .. 12 (packed or not): extend_request() for every slot in ONE
    attention launch (ops.pq_chunk_attn_wide / ops.pq_chunk_attn_packed with dev_lengths= / dev_n_q=); every slot with
    n_new[b] > 0 is left as extend_request(cache, b, ...) above leaves it, the others are not touched.  device_store=True: the
    stores are ONE ops.pq_store_ragged_wide call.  A cache with nbits = 8 is handed to its own method."""
    if cache.nbits <= 8:
        return cache.extend_ragged(query_states, key_states, value_states, layer_idx, n_new, device_store=device_store)
    return cache._extend_ragged("paged_turns.extend_ragged", query_states, key_states, value_states, layer_idx, n_new, device_store)


def verify(cache, query_states, key_states, value_states, layer_idx, n_draft=None, use_dev_lengths=True, route=None, return_lse=False,
           tree=None):
    """PagedPQCache.verify for a cache with nbits 9 .. 12 (packed or not): the attention of n <= 16 draft tokens per request over
    [the codes; the window; the draft rows, causally - or, tree=, along their ancestors], one layer, q (bs, nh, n, d), K/V
    (bs, nh_k, n, d) -> out (bs, nh, n, d) (and lse with return_lse).  Pure: pages, window, lengths and host mirror do not move;
    the rows' K/V are parked for commit().  n_draft, tree, use_dev_lengths and return_lse mean what they mean there.  route:
    "heads" - the decode launch of the format over the rows as query heads, then ops.attn_block_merge: one launch of a kernel with
    16 score columns, so n nh / nh_k <= 16 or the call is refused before anything is joined or recorded;
    "chunk" - the chunk attention of the cache's format with the rows as chunk; None: cache._verify_route(n), the wide rule.  A
    cache with nbits = 8 is handed to its own method."""
    if cache.nbits <= 8:
        return cache.verify(query_states, key_states, value_states, layer_idx, n_draft=n_draft, use_dev_lengths=use_dev_lengths, route=route,
                            return_lse=return_lse, tree=tree)
    return cache._verify("paged_turns.verify", query_states, key_states, value_states, layer_idx, n_draft, use_dev_lengths, route, return_lse, tree)


def commit(cache, n_accept=None, *, path=None):
    """PagedPQCache.commit for a cache with nbits 9 .. 12 (packed or not): the first n_accept[b] rows (path=: the accepted chain of a
    tree) that verify() above staged join the window of slot b in every layer in ONE call (ops.window_commit_wide), exactly as that
    many decode() steps above would have left codes, pages, window rows, host and device lengths; decode, flush, extend* and
    release go on as after those steps.  Every refusal of the 8-bit method holds, before anything moves.  A cache with nbits = 8
    is handed to its own method."""
    if cache.nbits <= 8:
        return cache.commit(n_accept, path=path)
    return cache._commit("paged_turns.commit", n_accept, path)


def fork(cache, src, dst, n_tokens=None):
    """PagedPQCache.fork for a cache with nbits 9 .. 12 (packed or not): slot(s) dst become a copy of slot src - of its first
    n_tokens coded tokens and no window, when n_tokens is given - in every layer and in ONE launch (ops.cache_fork_wide): what
    prefill_request of the same prompt and the same decode steps would have left there, bit for bit, without the prompt pass.
    Paging on demand shares the full code pages and copies the partial tail page into a fresh id; a preallocated table gets a copy
    of every live page.  Shared pages are safe under the wide page writers as they are under the 8-bit ones: nothing ever writes a
    token below a request's T, and in a packed page every high byte belongs to one token, so a store of the tokens from T on never
    reads, modifies or zeroes a byte of a shared token.  The destinations go on with decode / flush / extend* / verify / commit
    above.  Every refusal of the 8-bit method holds, before anything moves.  A cache with nbits = 8 is handed to its own method."""
    if cache.nbits <= 8:
        return cache.fork(src, dst, n_tokens=n_tokens)
    return cache._fork(src, dst, n_tokens)


def swap_out(cache, b, release=True, staging_bytes=64 << 20):
    """PagedPQCache.swap_out for a cache with nbits 9 .. 12 (packed or not): slot(s) b as RequestSnapshot(s) in host memory - blob
    format 2, meta["version"] = 2 -, packed by ONE launch per range of layers (ops.cache_swap_wide) through a staging buffer of at
    most staging_bytes; release=True then releases the slot(s).  The blob holds packed pages whatever the cache's pools hold, so
    the snapshot goes back into a packed or an unpacked cache of the same geometry and codebooks.  A cache with nbits = 8 is handed
    to its own method."""
    if cache.nbits <= 8:
        return cache.swap_out(b, release=release, staging_bytes=staging_bytes)
    cache._no_sinks("swap_out / snapshot_request")
    return cache._swap_out(b, release, staging_bytes)


def snapshot_request(cache, b):
    """swap_out(cache, b, release=False): the slot keeps decoding, the snapshot is what it holds now."""
    return swap_out(cache, b, release=False)


def swap_in(cache, b, snap, check_codebooks=True, staging_bytes=64 << 20):
    """PagedPQCache.swap_in for a cache with nbits 9 .. 12 (packed or not): a version-2 RequestSnapshot into the empty slot b -
    pages allocated on demand or the fixed ids of a preallocated table, ONE launch per range of layers (ops.cache_swap_wide).
    Every refusal of the 8-bit method holds, before anything changes; a version-1 snapshot is one of them (and a version-2
    snapshot is refused by an 8-bit cache).  A cache with nbits = 8 is handed to its own method."""
    if cache.nbits <= 8:
        return cache.swap_in(b, snap, check_codebooks=check_codebooks, staging_bytes=staging_bytes)
    cache._no_sinks("swap_in")
    return cache._swap_in(b, snap, check_codebooks, staging_bytes)
