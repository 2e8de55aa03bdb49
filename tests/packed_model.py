"""Packed code pages in numpy, written from the format text of include/million_hip.h ("Packed code pages"), not from the kernels.

A code of C in 512 .. 4096 centroids is its low byte and h high bits (h = 2 up to C = 1024, else 4).  A page is its low plane,
then its high plane: K low (page_size, M), K high (page_size, M h / 8); V low (M, page_size), V high (M h / 8, page_size).  The
h bits of subspace m sit at bit h (m mod 8/h) of high byte m / (8/h) of their token.  numpy only: importable without a GPU."""
import numpy as np


def hi_bits(C: int) -> int:
    assert C in (512, 1024, 2048, 4096), C
    return 2 if C <= 1024 else 4


def page_bytes(page_size: int, M: int, C: int) -> int:
    return page_size * M * (8 + hi_bits(C)) // 8


def _fold(fields, h, axis):
    """(.., M, ..) fields of h bits along `axis` -> (.., M h / 8, ..) bytes: 8/h neighbouring subspaces per byte, the first lowest."""
    per = 8 // h
    f = np.moveaxis(fields.astype(np.uint8), axis, -1)
    f = f.reshape(*f.shape[:-1], f.shape[-1] // per, per)
    byte = np.zeros(f.shape[:-1], np.uint8)
    for i in range(per):
        byte |= f[..., i] << (h * i)
    return np.moveaxis(byte, -1, axis)


def _unfold(byte, h, axis):
    per = 8 // h
    b = np.moveaxis(byte, axis, -1)
    f = np.stack([(b >> (h * i)) & ((1 << h) - 1) for i in range(per)], axis=-1)
    return np.moveaxis(f.reshape(*b.shape[:-1], b.shape[-1] * per), -1, axis)


def planes(codes, side, C):
    """uint16 pages (.., page_size, M) for side "k", (.., M, page_size) for side "v" -> (low plane, high plane), uint8."""
    h = hi_bits(C)
    codes = np.asarray(codes, np.uint16)
    lo = (codes & 0xFF).astype(np.uint8)
    hi = _fold((codes >> 8) & ((1 << h) - 1), h, -1 if side == "k" else -2)
    return lo, hi


def pack(codes, side, C):
    """uint16 pages (n, page_size, M) / (n, M, page_size) -> packed pages uint8 (n, page_bytes)."""
    lo, hi = planes(codes, side, C)
    n = lo.shape[0]
    return np.concatenate([lo.reshape(n, -1), hi.reshape(n, -1)], axis=1)


def unpack(packed, side, page_size, M, C):
    """Packed pages uint8 (n, page_bytes) -> uint16 pages; the inverse of pack for codes below 2**(8 + h)."""
    h = hi_bits(C)
    n = packed.shape[0]
    assert packed.dtype == np.uint8 and packed.shape[1] == page_bytes(page_size, M, C)
    if side == "k":
        lo = packed[:, :page_size * M].reshape(n, page_size, M)
        hi = _unfold(packed[:, page_size * M:].reshape(n, page_size, M * h // 8), h, -1)
    else:
        lo = packed[:, :page_size * M].reshape(n, M, page_size)
        hi = _unfold(packed[:, page_size * M:].reshape(n, M * h // 8, page_size), h, -2)
    return lo.astype(np.uint16) | (hi.astype(np.uint16) << 8)


def put_tokens(page, side, offsets, codes, page_size, M, C):
    """Store the codes (n, M) of the tokens at `offsets` (n,) of ONE packed page (page_bytes,) in place: only those tokens' bytes -
    their low bytes and their own high bytes - change."""
    h = hi_bits(C)
    offsets = np.asarray(offsets)
    codes = np.asarray(codes, np.uint16).reshape(len(offsets), M)
    lo = (codes & 0xFF).astype(np.uint8)
    hi = _fold((codes >> 8) & ((1 << h) - 1), h, -1)      # (n, M h / 8)
    if side == "k":
        page[:page_size * M].reshape(page_size, M)[offsets] = lo
        page[page_size * M:].reshape(page_size, M * h // 8)[offsets] = hi
    else:
        page[:page_size * M].reshape(M, page_size)[:, offsets] = lo.T
        page[page_size * M:].reshape(M * h // 8, page_size)[:, offsets] = hi.T


def store(pool, side, ids_row, token_start, codes, page_size, M, C):
    """Tokens [token_start, token_start + n) of one (b, kv head) - codes (n, M) - into the packed pool (n_pool, page_bytes)
    through its row of page ids, as million_pq_encode_packed stores them."""
    n = codes.shape[0]
    t = token_start
    while t < token_start + n:
        pg, off = divmod(t, page_size)
        m = min(page_size - off, token_start + n - t)
        put_tokens(pool[ids_row[pg]], side, np.arange(off, off + m), codes[t - token_start:t - token_start + m], page_size, M, C)
        t += m
