"""numpy restatement of million_cache_fork's contract (include/million_hip.h): what the call may read, and every byte it
writes.  The GPU tests compare the kernel with it byte for byte; the CPU tests run the host bookkeeping of PagedPQCache.fork on
it (as_ops_stub).  Written from the contract, not from the kernel: it walks destinations, layers, heads and pages in plain
loops and knows nothing of tasks, groups or vectors."""
import numpy as np

SHARE, COPY = 0, 1


def clamp_row(row, *, page_size, n_pages_bound, resid_cap, prefix_tokens=-1):
    """(T, r, start) of a source lengths row {T, r, start, word 3} as the call uses it."""
    T, r, st = int(row[0]), int(row[1]), int(row[2])
    T = min(max(T, 0), n_pages_bound * page_size)
    r = min(max(r, 0), resid_cap)
    st = st if 0 <= st < resid_cap else 0
    if prefix_tokens >= 0:
        T, r, st = min(T, prefix_tokens), 0, 0
    return T, r, st


def takes_part(dst_slots, bs, src):
    """Index into dst_slots -> slot, for the destinations that take part: inside [0, bs), not the source, and not named by an
    earlier entry."""
    out, seen = {}, set()
    for jd, b in enumerate(int(x) for x in dst_slots):
        if 0 <= b < bs and b != src and b not in seen:
            out[jd] = b
        seen.add(b)
    return out


def fork(page_ids, k_pool, v_pool, k_res, v_res, lengths, dst_slots, tail_ids, *, src, mode, n_pages_bound, prefix_tokens=-1):
    """In place.  page_ids (layers, bs, nh_k, n_pages_cap) int32, k_pool (n_pool, page_size, M), v_pool (n_pool, M, page_size)
    uint8, k_res / v_res (layers, bs, nh_k, cap, d) any 16-bit dtype, lengths (layers, bs, 4) int32, dst_slots (n_dst,),
    tail_ids (n_dst, layers, nh_k) or None (COPY).  Returns the list of (layer, slot, head, page j, from id, to id) copied."""
    n_layers, bs, nhk, _ = page_ids.shape
    n_pool, page_size, _ = k_pool.shape
    cap = k_res.shape[3]
    assert 0 <= src < bs and mode in (SHARE, COPY) and 0 <= n_pages_bound <= page_ids.shape[3]
    # every source value is taken before anything is written: the source is never a destination, so the order is free
    copied = []
    for jd, dst in takes_part(dst_slots, bs, src).items():
        for l in range(n_layers):
            T, r, st = clamp_row(lengths[l, src], page_size=page_size, n_pages_bound=n_pages_bound, resid_cap=cap,
                                 prefix_tokens=prefix_tokens)
            full, tail = divmod(T, page_size)
            n_live = full + (1 if tail else 0)
            for h in range(nhk):
                for j in range(n_live):
                    sid = int(page_ids[l, src, h, j])
                    if mode == SHARE:
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


def as_ops_stub(log=None):
    """A stand-in for million_amd.ops.cache_fork on CPU tensors: the same signature, the model's effect."""
    import torch

    def cache_fork(page_ids, k_pool, v_pool, k_res, v_res, dev_lengths, dst_slots, tail_ids, *, src, share, n_pages_bound=None,
                   prefix_tokens=-1):
        if log is not None:
            log.append(dict(src=src, share=share, n_pages_bound=n_pages_bound, prefix_tokens=prefix_tokens,
                            dst_slots=dst_slots.tolist(), tail_ids=None if tail_ids is None else tail_ids.tolist()))
        view16 = lambda t: t.view(torch.int16).numpy()      # numpy views share the tensors' memory
        fork(page_ids.numpy(), k_pool.numpy(), v_pool.numpy(), view16(k_res), view16(v_res), dev_lengths.numpy(),
             dst_slots.numpy(), None if tail_ids is None else tail_ids.numpy(), src=src, mode=SHARE if share else COPY,
             n_pages_bound=page_ids.shape[3] if n_pages_bound is None else n_pages_bound, prefix_tokens=prefix_tokens)
    return cache_fork
