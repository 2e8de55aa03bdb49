"""numpy restatement of million_cache_swap_wide's contract (include/million_hip.h): blob format 2, what PACK may read and every
byte either direction writes, over uint16 pools - K (n_pool, page_size, M), V (n_pool, M, page_size) - and over packed pools
(uint8 (n_pool, page_bytes)); and of million_cache_fork_wide, which is tests/cache_fork_model.py's rules over pages of either
kind.  Composed from tests/cache_swap_model.py (entries, clamps, windows, the lengths row) and tests/packed_model.py (planes).
Written from the contract, not from the kernels: it walks entries, layers, heads, pages and tokens in plain loops and knows
nothing of tasks, vectors or byte masks."""
import numpy as np

from tests import cache_fork_model as FM
from tests import cache_swap_model as SM
from tests import packed_model as P

PACK, UNPACK = SM.PACK, SM.UNPACK
VERSION = 2


def row_bytes(T, r, page_size, M, d, C):
    """Bytes of one (layer, kv head) row: packed K pages, packed V pages, K window, V window."""
    return 2 * (-(-T // page_size)) * P.page_bytes(page_size, M, C) + 4 * r * d


def is_packed(pool):
    return pool.dtype == np.uint8 and pool.ndim == 2


def entries(table, offsets, *, bs, nhk, page_size, M, d, C, resid_cap, n_pages_bound, n_layers, blob_bytes):
    """[(slot, T, r, start, offset, row_bytes)] of the entries that take part: format 1's rule with format 2's row bytes."""
    out = []
    for e, off in zip(table, offsets):
        slot, T, r, st = SM.clamp_entry(e, page_size=page_size, n_pages_bound=n_pages_bound, resid_cap=resid_cap)
        off = int(off)
        rb = row_bytes(T, r, page_size, M, d, C)
        if not 0 <= slot < bs or off < 0 or off % 16 or off + n_layers * nhk * rb > blob_bytes:
            continue
        out.append((slot, T, r, st, off, rb))
    return out


def _codes(pool, pid, side, page_size, M, C):
    """The uint16 codes of one page of either kind of pool, as its readers see them: code & (C - 1)."""
    page = P.unpack(pool[pid][None], side, page_size, M, C)[0] if is_packed(pool) else pool[pid]
    return page.astype(np.uint16) & np.uint16(C - 1)


def canonical_page(pool, pid, side, live, page_size, M, C):
    """One page of the blob: the packed page of the page's first `live` tokens, every byte of a later token zero."""
    codes = np.zeros((page_size, M) if side == "k" else (M, page_size), np.uint16)
    if 0 <= pid < pool.shape[0]:
        src = _codes(pool, pid, side, page_size, M, C)
        if side == "k":
            codes[:live] = src[:live]
        else:
            codes[:, :live] = src[:, :live]
    return P.pack(codes[None], side, C)[0]


def _call(page_ids, k_res, layer0, n_layers, n_pages_bound):
    n_all, bs, nhk, npc = page_ids.shape
    n_layers = n_all - layer0 if n_layers is None else n_layers
    bound = npc if n_pages_bound is None else n_pages_bound
    assert 0 <= layer0 and n_layers >= 1 and layer0 + n_layers <= n_all and 0 <= bound <= npc
    return bs, nhk, k_res.shape[3], k_res.shape[4], n_layers, bound


def pack(page_ids, k_pool, v_pool, k_res, v_res, table, offsets, blob, *, page_size, M, C, layer0=0, n_layers=None, n_pages_bound=None):
    """Writes `blob` (1-D uint8) in place, nothing else.  Returns the entries that took part."""
    bs, nhk, cap, d, n_layers, bound = _call(page_ids, k_res, layer0, n_layers, n_pages_bound)
    took = entries(table, offsets, bs=bs, nhk=nhk, page_size=page_size, M=M, d=d, C=C, resid_cap=cap, n_pages_bound=bound,
                   n_layers=n_layers, blob_bytes=blob.size)
    for slot, T, r, st, off, rb in took:
        n_live = -(-T // page_size)
        ring = (st + np.arange(r)) % cap if cap else np.zeros(0, np.int64)
        for lc in range(n_layers):
            l = layer0 + lc
            for h in range(nhk):
                lives = [min(page_size, T - j * page_size) for j in range(n_live)]
                parts = [canonical_page(k_pool, int(page_ids[l, slot, h, j]), "k", lives[j], page_size, M, C) for j in range(n_live)]
                parts += [canonical_page(v_pool, int(page_ids[l, slot, h, j]), "v", lives[j], page_size, M, C) for j in range(n_live)]
                parts += [np.ascontiguousarray(k_res[l, slot, h][ring]).view(np.uint8).reshape(-1),
                          np.ascontiguousarray(v_res[l, slot, h][ring]).view(np.uint8).reshape(-1)]
                row = np.concatenate(parts)
                assert row.size == rb
                o = off + (lc * nhk + h) * rb
                blob[o:o + rb] = row
    return took


def unpack(page_ids, k_pool, v_pool, k_res, v_res, lengths, table, offsets, blob, *, page_size, M, C, layer0=0, n_layers=None,
           n_pages_bound=None):
    """Writes pools, windows and lengths in place; never the table or the blob.  A packed pool gets the blob's bytes; a uint16
    pool (low byte | field << 8) & (C - 1) per code and 0 for the codes of tokens >= T.  Returns (layer, slot, head, j, id) written."""
    bs, nhk, cap, d, n_layers, bound = _call(page_ids, k_res, layer0, n_layers, n_pages_bound)
    pb = P.page_bytes(page_size, M, C)
    written = []
    for slot, T, r, st, off, rb in entries(table, offsets, bs=bs, nhk=nhk, page_size=page_size, M=M, d=d, C=C, resid_cap=cap,
                                           n_pages_bound=bound, n_layers=n_layers, blob_bytes=blob.size):
        n_live = -(-T // page_size)
        ring = (st + np.arange(r)) % cap if cap else np.zeros(0, np.int64)
        for lc in range(n_layers):
            l = layer0 + lc
            for h in range(nhk):
                o = off + (lc * nhk + h) * rb
                row = blob[o:o + rb]
                for j in range(n_live):
                    pid = int(page_ids[l, slot, h, j])
                    if not 0 <= pid < k_pool.shape[0]:
                        continue
                    live = min(page_size, T - j * page_size)
                    for side, pool, page in (("k", k_pool, row[j * pb:(j + 1) * pb]), ("v", v_pool, row[(n_live + j) * pb:(n_live + j + 1) * pb])):
                        if is_packed(pool):
                            pool[pid] = page
                            continue
                        codes = P.unpack(page[None], side, page_size, M, C)[0] & np.uint16(C - 1)
                        if side == "k":
                            codes[live:] = 0
                        else:
                            codes[:, live:] = 0
                        pool[pid] = codes
                    written.append((l, slot, h, j, pid))
                w0 = 2 * n_live * pb
                k_res[l, slot, h][ring] = row[w0:w0 + 2 * r * d].copy().view(k_res.dtype).reshape(r, d)
                v_res[l, slot, h][ring] = row[w0 + 2 * r * d:w0 + 4 * r * d].copy().view(v_res.dtype).reshape(r, d)
            lengths[l, slot] = (T, r, st, 0)
    return written


def live_codes(page_ids, k_pool, v_pool, slot, T, *, page_size, M, C):
    """The codes a request IS, whatever pages and whichever kind of pool hold them: K and V (layers, nh_k, T, M) uint16."""
    n_all, _, nhk, _ = page_ids.shape
    k = np.zeros((n_all, nhk, T, M), np.uint16)
    v = np.zeros((n_all, nhk, T, M), np.uint16)
    for l in range(n_all):
        for h in range(nhk):
            for j in range(-(-T // page_size)):
                pid, t0 = int(page_ids[l, slot, h, j]), j * page_size
                n = min(page_size, T - t0)
                k[l, h, t0:t0 + n] = _codes(k_pool, pid, "k", page_size, M, C)[:n]
                v[l, h, t0:t0 + n] = _codes(v_pool, pid, "v", page_size, M, C)[:, :n].T
    return k, v


def fork(page_ids, k_pool, v_pool, k_res, v_res, lengths, dst_slots, tail_ids, *, page_size, src, mode, n_pages_bound, prefix_tokens=-1):
    """tests/cache_fork_model.py's fork over pools of either kind: a page is pool[id], whole (a packed page: both planes)."""
    n_layers, bs, nhk, _ = page_ids.shape
    n_pool, cap = k_pool.shape[0], k_res.shape[3]
    assert 0 <= src < bs and mode in (FM.SHARE, FM.COPY) and 0 <= n_pages_bound <= page_ids.shape[3]
    copied = []
    for jd, dst in FM.takes_part(dst_slots, bs, src).items():
        for l in range(n_layers):
            T, r, st = FM.clamp_row(lengths[l, src], page_size=page_size, n_pages_bound=n_pages_bound, resid_cap=cap, prefix_tokens=prefix_tokens)
            full, tail = divmod(T, page_size)
            n_live = full + (1 if tail else 0)
            for h in range(nhk):
                for j in range(n_live):
                    sid = int(page_ids[l, src, h, j])
                    if mode == FM.SHARE:
                        e = sid if j < full else int(tail_ids[jd, l, h])
                        page_ids[l, dst, h, j] = e
                    else:
                        e = int(page_ids[l, dst, h, j])
                    if e != sid and 0 <= e < n_pool and 0 <= sid < n_pool:
                        k_pool[e] = k_pool[sid]
                        v_pool[e] = v_pool[sid]
                        copied.append((l, dst, h, j, sid, e))
                if prefix_tokens < 0:
                    k_res[l, dst, h] = k_res[l, src, h]
                    v_res[l, dst, h] = v_res[l, src, h]
            lengths[l, dst] = (T, r, st, 0)
    return copied


def as_ops_stubs(log=None):
    """Stand-ins for million_amd.ops.cache_fork_wide / cache_swap_wide on CPU tensors: the same signatures, the model's effect."""
    import torch

    def np_of(t):      # numpy views share the tensors' memory
        return t.view(torch.int16).numpy().view(np.uint16) if t.dtype == torch.uint16 else t.numpy()

    view16 = lambda t: t.view(torch.int16).numpy()

    def geometry(k_pool, page_size, M):
        return (page_size, M) if k_pool.dim() == 2 else tuple(k_pool.shape[1:])

    def cache_fork_wide(page_ids, k_pool, v_pool, k_res, v_res, dev_lengths, dst_slots, tail_ids, *, src, share, n_pages_bound=None,
                        prefix_tokens=-1, C, packed=False, page_size=None, M=None):
        assert packed == (k_pool.dim() == 2)
        if log is not None:
            log.append(dict(op="fork", src=src, share=share, n_pages_bound=n_pages_bound, prefix_tokens=prefix_tokens, C=C, packed=packed,
                            dst_slots=dst_slots.tolist(), tail_ids=None if tail_ids is None else tail_ids.tolist()))
        fork(page_ids.numpy(), np_of(k_pool), np_of(v_pool), view16(k_res), view16(v_res), dev_lengths.numpy(), dst_slots.numpy(),
             None if tail_ids is None else tail_ids.numpy(), page_size=geometry(k_pool, page_size, M)[0], src=src,
             mode=FM.SHARE if share else FM.COPY, n_pages_bound=page_ids.shape[3] if n_pages_bound is None else n_pages_bound,
             prefix_tokens=prefix_tokens)

    def cache_swap_wide(direction, page_ids, k_pool, v_pool, k_res, v_res, dev_lengths, slot_table, blob_offsets, blob, *, layer0=0,
                        n_layers=None, n_pages_bound=None, C, packed=False, page_size=None, M=None):
        assert packed == (k_pool.dim() == 2)
        if log is not None:
            log.append(dict(op="swap", direction=direction, layer0=layer0, n_layers=n_layers, n_pages_bound=n_pages_bound, C=C, packed=packed,
                            slot_table=slot_table.tolist(), blob_offsets=blob_offsets.tolist(), blob_bytes=blob.numel()))
        ps, m = geometry(k_pool, page_size, M)
        kw = dict(page_size=ps, M=m, C=C, layer0=layer0, n_layers=n_layers, n_pages_bound=n_pages_bound)
        if direction == PACK:
            pack(page_ids.numpy(), np_of(k_pool), np_of(v_pool), view16(k_res), view16(v_res), slot_table.numpy(), blob_offsets.numpy(),
                 blob.numpy(), **kw)
        else:
            unpack(page_ids.numpy(), np_of(k_pool), np_of(v_pool), view16(k_res), view16(v_res), dev_lengths.numpy(), slot_table.numpy(),
                   blob_offsets.numpy(), blob.numpy(), **kw)

    return cache_fork_wide, cache_swap_wide
