"""numpy restatement of million_cache_swap's contract (include/million_hip.h): blob format 1, what PACK may read and every
byte either direction writes.  The GPU tests compare the kernel with it byte for byte; the CPU tests run the host bookkeeping
of PagedPQCache.swap_out / swap_in on it (as_ops_stub).  Written from the contract, not from the kernel: it walks entries,
layers, heads, pages and window rows in plain loops and knows nothing of tasks, groups or vectors."""
import numpy as np

PACK, UNPACK = 0, 1
VERSION = 1


def row_bytes(T, r, page_size, M, d):
    """Bytes of one (layer, kv head) row: K pages, V pages, K window, V window."""
    return 2 * (-(-T // page_size)) * page_size * M + 4 * r * d


def clamp_entry(entry, *, page_size, n_pages_bound, resid_cap):
    """(slot, T, r, start) of a table row {slot, T, r, start} as the call uses it."""
    slot, T, r, st = (int(x) for x in entry)
    T = min(max(T, 0), n_pages_bound * page_size)
    r = min(max(r, 0), resid_cap)
    st = st if 0 <= st < resid_cap else 0
    return slot, T, r, st


def entries(table, offsets, *, bs, nhk, page_size, M, d, resid_cap, n_pages_bound, n_layers, blob_bytes):
    """[(slot, T, r, start, offset, row_bytes)] of the entries that take part."""
    out = []
    for e, off in zip(table, offsets):
        slot, T, r, st = clamp_entry(e, page_size=page_size, n_pages_bound=n_pages_bound, resid_cap=resid_cap)
        off = int(off)
        rb = row_bytes(T, r, page_size, M, d)
        if not 0 <= slot < bs or off < 0 or off % 16 or off + n_layers * nhk * rb > blob_bytes:
            continue
        out.append((slot, T, r, st, off, rb))
    return out


def _geometry(page_ids, k_pool, k_res):
    n_all, bs, nhk, _ = page_ids.shape
    n_pool, ps, M = k_pool.shape
    return n_all, bs, nhk, n_pool, ps, M, k_res.shape[3], k_res.shape[4]


def pack(page_ids, k_pool, v_pool, k_res, v_res, table, offsets, blob, *, layer0=0, n_layers=None, n_pages_bound=None):
    """Writes `blob` (1-D uint8) in place, nothing else.  page_ids (layers, bs, nh_k, n_pages_cap) int32, k_pool (n_pool,
    page_size, M), v_pool (n_pool, M, page_size) uint8, k_res / v_res (layers, bs, nh_k, cap, d) any 16-bit dtype, table
    (n_slots, 4) {slot, T, r, start}, offsets (n_slots,).  Returns the entries that took part."""
    n_all, bs, nhk, n_pool, ps, M, cap, d = _geometry(page_ids, k_pool, k_res)
    n_layers = n_all - layer0 if n_layers is None else n_layers
    bound = page_ids.shape[3] if n_pages_bound is None else n_pages_bound
    assert 0 <= layer0 and n_layers >= 1 and layer0 + n_layers <= n_all and 0 <= bound <= page_ids.shape[3]
    took = entries(table, offsets, bs=bs, nhk=nhk, page_size=ps, M=M, d=d, resid_cap=cap, n_pages_bound=bound, n_layers=n_layers,
                   blob_bytes=blob.size)
    for slot, T, r, st, off, rb in took:
        n_live = -(-T // ps)
        ring = (st + np.arange(r)) % cap if cap else np.zeros(0, np.int64)
        for lc in range(n_layers):
            l = layer0 + lc
            for h in range(nhk):
                k = np.zeros((n_live, ps, M), np.uint8)
                v = np.zeros((n_live, M, ps), np.uint8)
                for j in range(n_live):
                    pid = int(page_ids[l, slot, h, j])
                    if 0 <= pid < n_pool:
                        live = min(ps, T - j * ps)
                        k[j, :live] = k_pool[pid, :live]
                        v[j, :, :live] = v_pool[pid, :, :live]
                row = np.concatenate([k.reshape(-1), v.reshape(-1), np.ascontiguousarray(k_res[l, slot, h][ring]).view(np.uint8).reshape(-1),
                                      np.ascontiguousarray(v_res[l, slot, h][ring]).view(np.uint8).reshape(-1)])
                assert row.size == rb
                o = off + (lc * nhk + h) * rb
                blob[o:o + rb] = row
    return took


def unpack(page_ids, k_pool, v_pool, k_res, v_res, lengths, table, offsets, blob, *, layer0=0, n_layers=None, n_pages_bound=None):
    """Writes pools, windows and lengths (layers, bs, 4) in place; never the table or the blob.  Entries that name the same slot
    overlap (the contract leaves the result open; here the last one wins).  Returns the list of
    (layer, slot, head, page j, id) written."""
    n_all, bs, nhk, n_pool, ps, M, cap, d = _geometry(page_ids, k_pool, k_res)
    n_layers = n_all - layer0 if n_layers is None else n_layers
    bound = page_ids.shape[3] if n_pages_bound is None else n_pages_bound
    assert 0 <= layer0 and n_layers >= 1 and layer0 + n_layers <= n_all and 0 <= bound <= page_ids.shape[3]
    written = []
    for slot, T, r, st, off, rb in entries(table, offsets, bs=bs, nhk=nhk, page_size=ps, M=M, d=d, resid_cap=cap, n_pages_bound=bound,
                                           n_layers=n_layers, blob_bytes=blob.size):
        n_live = -(-T // ps)
        ring = (st + np.arange(r)) % cap if cap else np.zeros(0, np.int64)
        for lc in range(n_layers):
            l = layer0 + lc
            for h in range(nhk):
                o = off + (lc * nhk + h) * rb
                row = blob[o:o + rb]
                pb = ps * M
                for j in range(n_live):
                    pid = int(page_ids[l, slot, h, j])
                    if 0 <= pid < n_pool:
                        k_pool[pid] = row[j * pb:(j + 1) * pb].reshape(ps, M)
                        v_pool[pid] = row[(n_live + j) * pb:(n_live + j + 1) * pb].reshape(M, ps)
                        written.append((l, slot, h, j, pid))
                w0 = 2 * n_live * pb
                k_res[l, slot, h][ring] = row[w0:w0 + 2 * r * d].copy().view(k_res.dtype).reshape(r, d)
                v_res[l, slot, h][ring] = row[w0 + 2 * r * d:w0 + 4 * r * d].copy().view(v_res.dtype).reshape(r, d)
            lengths[l, slot] = (T, r, st, 0)
    return written


def live_data(page_ids, k_pool, v_pool, k_res, v_res, slot, T, r, st):
    """What a request IS, whatever pages hold it: K and V codes (layers, nh_k, T, M) row-major and the window rows (layers, nh_k,
    r, d) of both sides in ring order."""
    n_all, bs, nhk, n_pool, ps, M, cap, d = _geometry(page_ids, k_pool, k_res)
    n = -(-T // ps)
    ids = page_ids[:, slot, :, :n].astype(np.int64)
    k = k_pool[ids].reshape(n_all, nhk, n * ps, M)[:, :, :T]
    v = v_pool[ids].transpose(0, 1, 2, 4, 3).reshape(n_all, nhk, n * ps, M)[:, :, :T]
    ring = (st + np.arange(r)) % cap
    return k, v, k_res[:, slot][:, :, ring], v_res[:, slot][:, :, ring]


def as_ops_stub(log=None):
    """A stand-in for million_amd.ops.cache_swap on CPU tensors: the same signature, the model's effect."""
    import torch

    def cache_swap(direction, page_ids, k_pool, v_pool, k_res, v_res, dev_lengths, slot_table, blob_offsets, blob, *, layer0=0,
                   n_layers=None, n_pages_bound=None):
        if log is not None:
            log.append(dict(direction=direction, layer0=layer0, n_layers=n_layers, n_pages_bound=n_pages_bound,
                            slot_table=slot_table.tolist(), blob_offsets=blob_offsets.tolist(), blob_bytes=blob.numel()))
        view16 = lambda t: t.view(torch.int16).numpy()      # numpy views share the tensors' memory
        kw = dict(layer0=layer0, n_layers=n_layers, n_pages_bound=n_pages_bound)
        if direction == PACK:
            pack(page_ids.numpy(), k_pool.numpy(), v_pool.numpy(), view16(k_res), view16(v_res), slot_table.numpy(), blob_offsets.numpy(),
                 blob.numpy(), **kw)
        else:
            unpack(page_ids.numpy(), k_pool.numpy(), v_pool.numpy(), view16(k_res), view16(v_res), dev_lengths.numpy(), slot_table.numpy(),
                   blob_offsets.numpy(), blob.numpy(), **kw)
    return cache_swap
