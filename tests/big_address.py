"""Far addresses: page ids and strides that put the bytes a kernel touches past 2^31 and 2^32 bytes from the base of its
buffer, each with a compact twin - the same call on the same data a few MiB from the base.  Shared by
test_big_address_gpu.py (torch tensors on the device) and test_big_address_host.py (numpy arrays, the boundary scaled down);
numpy plus lazy torch, importable without a GPU.

A pool of any page geometry is a view of the first n_pool * page_bytes bytes of one flat uint8 buffer of FLAT_BYTES bytes
filled with SENTINEL: (n_pool, ps, M) for K, (n_pool, M, ps) for V.  0xA5 is a valid code at C = 256 and is masked into range
at C = 128, so a reader that lands on a page nobody scattered gets finite, wrong codes - which only the bitwise comparison
with the twin (and the twin's own check against the oracle) shows.

Pools of 2-byte codes (code_bytes = 2; test_big_address_wide_gpu.py) are the same bytes seen as uint16: (n_pool, ps, M) /
(n_pool, M, ps) words, page_bytes = ps * M * 2, the sentinel word SENTINEL16 = 0xA5A5.  A kernel over such a pool may keep its
offset in code words; the page ids reach byte 2^31 and byte 2^32 at half the values of a uint8 pool of the same (ps, M), and
a word offset truncated to 31 bits wraps exactly at byte 2^32 (aliased_words, signed_word_read): that is the reachable wide
case, and the far tables are held sensitive to it beside the byte truncations.  0xA5A5 & (C - 1) is a valid, wrong code at
every C in 512 .. 4096, as 0xA5 is at C = 256.

Covered on the GPU: every uint8 kernel (test_big_address_gpu.py); the 16-bit decode and chunk attention, pq_gather_rows at
both widths, pq_encode_into to uint16 pages, prompt attention with lse, the merges (attn_merge, attn_block_merge,
attn_sink_merge) over far views, the block route and a wide PagedPQCache past 4 GiB (test_big_address_wide_gpu.py).

Out of scope: element index 2^32 (a tensor of 8 GiB of fp16), and with it a code-word offset of 32 bits (a uint16 pool of
8 GiB).  far_view puts index 1 of its leading dimension past element 2^31, which for fp16 is also past byte 2^32; no test
here reaches element 2^32.

The sensitivity model (aliased, truncating_read / truncating_write, enc_table_test) is what makes the case that the GPU tests
would fail on a dropped cast: test_big_address_host.py runs the same helpers against readers and writers that truncate on
purpose."""
from __future__ import annotations

import numpy as np

SENTINEL = 0xA5
SENTINEL16 = 0xA5A5                # the same bytes as a code word: & (C - 1) makes it a valid, wrong code at every C in 512 .. 4096
HI = 2 ** 32                       # the second boundary; the first is HI / 2
FLAT_BYTES = HI + 2 ** 20          # 64 pages of the largest geometry (2-byte codes: 16 KiB) past the boundary; 8 KiB pages leave room to spare
SCAN_CHUNK = 256 << 20             # the sentinel scan never makes a temporary larger than a chunk's mask

# (page_size, M) of every pool test_big_address_gpu.py builds
GEOMS = [(64, 64), (64, 32), (64, 16), (32, 64), (32, 32), (32, 16), (128, 64), (128, 32), (128, 16)]
# (page_size, M) of the pools of 2-byte codes test_big_address_wide_gpu.py builds: n_pool leaves 64 pages past HI, FLAT_BYTES 1 MiB
WIDE_GEOMS = [(64, 64), (128, 32), (32, 64), (64, 32), (32, 16)]
assert all(n_ * m_ * 2 <= 16 << 10 and (HI // (n_ * m_ * 2) + 64) * n_ * m_ * 2 <= FLAT_BYTES for n_, m_ in WIDE_GEOMS)
TABLE = (2, 2, 10)                 # (bs, nh_k, pages per row) of the decode tests: >= 9 live pages per row


def n_pool(page_bytes: int, hi: int = HI) -> int:
    """Pages of a pool: those below hi and 64 spare ones past it - 32 for a 32 KiB page (pq_gather_rows at page size 128 over
    2-byte codes of M = 64), the most FLAT_BYTES holds; every smaller page has its 64."""
    return hi // page_bytes + min(64, (FLAT_BYTES - HI) // page_bytes)


def boundary_ids(page_bytes: int, hi: int = HI) -> list:
    lo = hi // 2 // page_bytes
    h = hi // page_bytes
    return [0, lo - 1, lo, lo + 1, h - 1, h, h + 1, n_pool(page_bytes, hi) - 1]


def far_ids(n: int, page_bytes: int, seed: int, hi: int = HI) -> np.ndarray:
    """n distinct page ids (int64): the eight boundary ids first, the rest dealt in turn from the three bands - below hi / 2,
    between the boundaries, past hi - so that every run of three consecutive entries (every table row) has pages in all
    bands while the free ids of the last band (61 of its 64 pages; 29 of 32 at 32 KiB pages) last; after that the first two
    bands alternate."""
    first = boundary_ids(page_bytes, hi)
    assert n >= len(first) and hi % (2 * page_bytes) == 0
    lo, h, np_ = hi // 2 // page_bytes, hi // page_bytes, n_pool(page_bytes, hi)
    rs = np.random.RandomState(seed)
    bands = [rs.permutation(np.arange(2, lo - 1)), rs.permutation(np.arange(lo + 2, h - 1)), rs.permutation(np.arange(h + 2, np_ - 1))]
    need = n - len(first)
    assert need <= len(bands[0]) + len(bands[1]), "table larger than the pool"
    out, taken, k = list(first), [0, 0, 0], 0
    while len(out) < n:
        b = k % 3
        k += 1
        if taken[b] < len(bands[b]):
            out.append(int(bands[b][taken[b]]))
            taken[b] += 1
    ids = np.asarray(out, np.int64)
    assert len(set(out)) == n and ids.min() >= 0 and ids.max() < np_
    return ids


def band_of(ids, page_bytes: int, hi: int = HI) -> np.ndarray:
    """0, 1 or 2: the page starts below hi / 2, below hi, or past it."""
    off = np.asarray(ids, np.int64) * page_bytes
    return (off >= hi // 2).astype(np.int64) + (off >= hi)


def aliased(ids, page_bytes: int, bits: int) -> np.ndarray:
    """The page a reader or writer hits that truncates the byte offset id * page_bytes to `bits` bits."""
    return ((np.asarray(ids, np.int64) * page_bytes) & ((1 << bits) - 1)) // page_bytes


def aliased_words(ids, page_bytes: int, bits: int, code_bytes: int = 2) -> np.ndarray:
    """The element-index form: the page hit when the offset in code words, id * (page_bytes / code_bytes), is truncated to
    `bits` bits.  With 2-byte codes 31 bits in words is byte 2^32."""
    assert page_bytes % code_bytes == 0
    words = page_bytes // code_bytes
    return ((np.asarray(ids, np.int64) * words) & ((1 << bits) - 1)) // words


def sensitive_rows(table: np.ndarray, page_bytes: int, bits: int, code_bytes: int = 0) -> np.ndarray:
    """For every (b, kv head) row of a page table (..., n_pages): does at least one of its pages alias, under truncation to
    `bits` bits, to a page that is not its own and that holds the sentinel or another row's codes (that is: a page no entry of
    this row names)?  A row for which this is False could be read through a truncating kernel without anyone noticing.
    code_bytes = 0: the byte offset is truncated; else the offset in code words of that size (aliased_words)."""
    t = np.asarray(table, np.int64)
    rows = t.reshape(-1, t.shape[-1])
    res = []
    for row in rows:
        al = aliased_words(row, page_bytes, bits, code_bytes) if code_bytes else aliased(row, page_bytes, bits)
        own = set(row.tolist())
        res.append(any(int(a) != int(i) and int(a) not in own for a, i in zip(al, row)))
    return np.asarray(res).reshape(t.shape[:-1])


# ---- the two backends: numpy arrays on the host, torch tensors on the device ------------------------------------------------
def _is_np(x) -> bool:
    return isinstance(x, np.ndarray)


def _index(ids, like):
    if _is_np(like):
        return np.asarray(ids, np.int64)
    import torch
    if isinstance(ids, torch.Tensor):
        return ids.to(device=like.device, dtype=torch.int64)
    return torch.from_numpy(np.asarray(ids, np.int64)).to(like.device)


def pool_view(flat, page_bytes: int, shape_tail, hi: int = HI, code_bytes: int = 1):
    """(n_pool, *shape_tail) view of the first n_pool * page_bytes bytes of a flat uint8 buffer; code_bytes = 2: the same bytes
    as uint16 words, shape_tail in words."""
    np_ = n_pool(page_bytes, hi)
    assert code_bytes in (1, 2) and int(np.prod(shape_tail)) * code_bytes == page_bytes and np_ * page_bytes <= flat.shape[0]
    v = flat[:np_ * page_bytes]
    if code_bytes == 2:
        v = v.view(np.uint16) if _is_np(v) else v.view(_torch().uint16)
    return v.reshape(np_, *shape_tail) if _is_np(v) else v.view(np_, *shape_tail)


def _torch():
    import torch
    return torch


def _signed(t):
    """A torch uint16 tensor as its int16 bits (indexing, index assignment and comparison are int16's); anything else as is."""
    return t.view(_torch().int16) if not _is_np(t) and t.dtype == _torch().uint16 else t


def scatter_pool(big_view, compact_pool, ids) -> None:
    """Page i of the compact pool goes to page ids[i] of the big view; everything else keeps the sentinel.  (The compact twin
    is the same call with arange ids.)"""
    idx = _index(ids, big_view)
    assert idx.shape[0] == compact_pool.shape[0] and tuple(big_view.shape[1:]) == tuple(compact_pool.shape[1:])
    assert big_view.dtype == compact_pool.dtype
    assert int(idx.min()) >= 0 and int(idx.max()) < big_view.shape[0]      # every far id lies inside the allocation
    _signed(big_view)[idx] = _signed(compact_pool)


def gather_pool(big_view, ids):
    got = _signed(big_view)[_index(ids, big_view)]
    return got if got.dtype == big_view.dtype else got.view(big_view.dtype)


def only_sentinel(flat) -> bool:
    """The whole flat buffer equals the sentinel; scanned in chunks of at most SCAN_CHUNK bytes, eight bytes per compare."""
    n = flat.shape[0]
    assert n % 8 == 0 and SCAN_CHUNK % 8 == 0
    word = int.from_bytes(bytes([SENTINEL]) * 8, "little", signed=True)
    if _is_np(flat):
        return all(bool((flat[o:o + SCAN_CHUNK].view(np.int64) == word).all()) for o in range(0, n, SCAN_CHUNK))
    import torch
    bad = torch.zeros((), dtype=torch.bool, device=flat.device)
    for o in range(0, n, SCAN_CHUNK):
        bad |= (flat[o:o + SCAN_CHUNK].view(torch.int64) != word).any()
    return not bool(bad.item())


def assert_only_these_pages(big_view, ids, expected_pages, flat, what: str = "") -> None:
    """(1) the listed pages equal expected_pages byte for byte; (2) with them overwritten by the sentinel, the whole flat
    buffer the view lies in is sentinel: nothing was written anywhere else.  Destroys the listed pages."""
    idx = _index(ids, big_view)
    assert big_view.dtype == expected_pages.dtype
    big_view = _signed(big_view)
    got = big_view[idx]
    if _is_np(got):
        same = np.array_equal(got, expected_pages)
    else:
        import torch
        same = torch.equal(got, _signed(expected_pages).to(got.device))
    assert same, f"{what}: the pages named by the table differ from the expected pages"
    big_view[idx] = {1: SENTINEL, 2: SENTINEL16 - (0 if _is_np(big_view) else 1 << 16)}[big_view.dtype.itemsize]
    assert only_sentinel(flat), f"{what}: bytes outside the pages named by the table were written"


def far_stride(n_elems_per_index: int, align_elems: int = 8, hi: int = HI) -> int:
    """A leading stride (in fp16 elements) that puts index 1 past element hi / 2 - past byte hi - and keeps 16-byte alignment."""
    s = hi // 2 + 8 * align_elems
    assert s % align_elems == 0 and s >= n_elems_per_index
    return s


def far_view(flat, shape, strides, dtype):
    """as_strided view over a flat uint8 device buffer reinterpreted as dtype; shape / strides in elements of dtype.  The view
    must end inside the buffer."""
    t = flat.view(dtype)
    last = sum((n - 1) * s for n, s in zip(shape, strides))
    assert all(n > 0 for n in shape) and last < t.shape[0], (shape, strides, t.shape[0])
    return t.as_strided(tuple(shape), tuple(strides))


# ---- readers and writers that truncate on purpose (host model of a dropped cast) --------------------------------------------
def truncating_read(flat: np.ndarray, ids, page_bytes: int, bits: int) -> np.ndarray:
    """What a kernel reads that computes page offsets in `bits` bits: (len(ids), page_bytes)."""
    off = (np.asarray(ids, np.int64) * page_bytes) & ((1 << bits) - 1)
    return np.stack([flat[o:o + page_bytes] for o in off])


def truncating_write(flat: np.ndarray, ids, pages: np.ndarray, page_bytes: int, bits: int) -> None:
    off = (np.asarray(ids, np.int64) * page_bytes) & ((1 << bits) - 1)
    for o, pg in zip(off, pages.reshape(len(off), page_bytes)):
        flat[o:o + page_bytes] = pg


def signed_word_read(flat: np.ndarray, ids, page_bytes: int, bits: int, code_bytes: int = 2) -> np.ndarray:
    """What a kernel reads that keeps the offset in code words in a SIGNED integer of bits + 1 bits (31 value bits: C's int):
    past 2^bits words the index goes negative - before the base of the pool; the model reduces it into the buffer (modulo its
    length in words), where a real kernel would leave its allocation.  (len(ids), page_bytes) bytes."""
    words = page_bytes // code_bytes
    w = flat.view({1: np.uint8, 2: np.uint16}[code_bytes])
    off = np.asarray(ids, np.int64) * words
    off = (off + (1 << bits)) % (1 << (bits + 1)) - (1 << bits)
    off %= w.shape[0]
    return np.stack([np.take(w, np.arange(o, o + words), mode="wrap") for o in off]).view(np.uint8)


# ---- host model of the encoders' "inside the page table" decision (encode.hip), in C's int arithmetic ------------------------
def _i32(x: int) -> int:
    return (int(x) + 2 ** 31) % 2 ** 32 - 2 ** 31


def _cdiv(a: int, b: int) -> int:      # C division truncates toward zero
    q = abs(a) // abs(b)
    return q if (a < 0) == (b < 0) else -q


def enc_table_test(tok0: int, t: int, page_size: int, n_pages_cap: int, wrapping_sum: bool):
    """(stores, page, offset) for lane t of a call whose first destination token is tok0.  wrapping_sum=True is the form the
    kernels had: tok = tok0 + t in int, dropped when tok0 < 0 or tok / page_size >= n_pages_cap.  False is the form they have:
    dropped when tok0 < 0 or tok0 > n_pages_cap * page_size - 1 - t."""
    if wrapping_sum:
        tok = _i32(tok0 + t)
        if tok0 < 0 or _cdiv(tok, page_size) >= n_pages_cap:
            return False, None, None
    else:
        if tok0 < 0 or tok0 > n_pages_cap * page_size - 1 - t:
            return False, None, None
        tok = tok0 + t
    page = _cdiv(tok, page_size)
    return True, page, tok - page * page_size


def flush_advance(T: int, r: int, st: int, n_flush: int, cap_tok: int, rcap: int, wrapping_sum: bool):
    """The length row the flush kernel writes back, in int arithmetic; wrapping_sum as above."""
    T = 0 if T < 0 else T
    if wrapping_sum:
        T = cap_tok if _i32(T + n_flush) > cap_tok else _i32(T + n_flush)
        r = 0 if _i32(r - n_flush) < 0 else _i32(r - n_flush)
    else:
        T = cap_tok if T > cap_tok - n_flush else T + n_flush
        r = 0 if r < n_flush else r - n_flush
    st = st if 0 <= st < rcap else 0
    return T, r, (st + n_flush) % rcap
