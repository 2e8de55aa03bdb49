"""Host side of the far-address tests (tests/big_address.py): the page tables test_big_address_gpu.py and
test_big_address_wide_gpu.py use would expose a kernel that truncates a byte offset to 31 or 32 bits - or, over 2-byte codes,
an offset in code words to 31 bits, unsigned or signed - shown on a model - no GPU.  scatter_pool / assert_only_these_pages run
on a numpy pool with the boundary scaled down to 2^16 against a reader and a writer that truncate on purpose; the encoders'
table test is run in C's int arithmetic in its old (wrapping sum) and present form."""
import numpy as np
import pytest

from tests import big_address as BA

HI16 = 2 ** 16      # the scaled-down second boundary (the first: 2^15)


def _table(page_bytes, hi=BA.HI, seed=0):
    bs, nhk, npg = BA.TABLE
    return BA.far_ids(bs * nhk * npg, page_bytes, seed, hi).reshape(bs, nhk, npg)


# (ps, M, code bytes, bits, truncated offset counted in words of that many bytes - 0: in bytes)
_SENS = [(ps, M, 1, bits, 0, f"ps{ps}M{M}-{bits}") for bits in (31, 32) for ps, M in BA.GEOMS] + \
        [(ps, M, 2, bits, w, f"wide-ps{ps}M{M}-{'w' if w else 'b'}{bits}") for bits, w in ((31, 0), (32, 0), (31, 2)) for ps, M in BA.WIDE_GEOMS]


@pytest.mark.parametrize("ps,M,cb,bits,words", [c[:5] for c in _SENS], ids=[c[5] for c in _SENS])
def test_far_table_is_sensitive_to_truncation(ps, M, cb, bits, words):
    """Every (b, kv head) row of the far table has a page that a `bits`-bit byte offset sends to a page holding the sentinel
    or another row's codes; every row has pages on both sides of both boundaries; the first row has the boundary ids.  Pools of
    2-byte codes (cb = 2): the same for the byte offset, and for an offset in code words truncated to 31 bits (byte 2^32)."""
    B = ps * M * cb
    t = _table(B)
    assert BA.sensitive_rows(t, B, bits, words).all(), BA.sensitive_rows(t, B, bits, words)
    assert t.max() < BA.n_pool(B) and (t.max() + 1) * B <= BA.FLAT_BYTES
    for row in t.reshape(-1, t.shape[-1]):
        assert set(BA.band_of(row, B).tolist()) == {0, 1, 2}
    assert t[0, 0, :8].tolist() == BA.boundary_ids(B)
    assert BA.band_of(BA.boundary_ids(B), B).tolist() == [0, 0, 1, 1, 1, 2, 2, 2]
    if words:      # 31 bits in 2-byte words and 32 bits in bytes are one truncation
        assert np.array_equal(BA.aliased_words(t, B, bits, words), BA.aliased(t, B, bits + 1))


@pytest.mark.parametrize("bits", [31, 32])
def test_compact_table_is_not_sensitive(bits):
    """The control: with arange ids in place of far_ids the sensitivity predicate is False for every row - a suite whose
    largest id is a few thousand cannot see a truncated offset."""
    bs, nhk, npg = BA.TABLE
    for ps, M in BA.GEOMS:
        t = np.arange(bs * nhk * npg, dtype=np.int64).reshape(bs, nhk, npg)
        assert not BA.sensitive_rows(t, ps * M, bits).any()
    for ps, M in BA.WIDE_GEOMS:
        t = np.arange(bs * nhk * npg, dtype=np.int64).reshape(bs, nhk, npg)
        assert not BA.sensitive_rows(t, ps * M * 2, bits).any() and not BA.sensitive_rows(t, ps * M * 2, 31, 2).any()


HI22 = 2 ** 22      # the boundary scaled for the page sizes of the 2-byte pools (8 KiB pages: 512 below it)
WIDE_PAGE_BYTES = sorted({ps * M * 2 for ps, M in BA.WIDE_GEOMS})
# (page bytes, boundary, code bytes, bits, truncated offset counted in words of that many bytes - 0: in bytes)
_TRUNC = [(pb, HI16, 1, bits, 0, f"{pb}-{bits}") for bits in (15, 16) for pb in (256, 1024)] + \
         [(pb, HI22, 2, bits, w, f"wide{pb}-{'w' if w else 'b'}{bits}") for bits, w in ((21, 0), (22, 0), (21, 2)) for pb in WIDE_PAGE_BYTES]


def _pool_case(page_bytes, hi, cb, seed):
    bs, nhk, npg = BA.TABLE
    n = bs * nhk * npg
    rs = np.random.RandomState(seed)
    dt = {1: np.uint8, 2: np.uint16}[cb]
    compact = rs.randint(0, 256 ** cb, (n, page_bytes // cb)).astype(dt)
    ids = BA.far_ids(n, page_bytes, 3, hi)
    flat = np.full(hi + 64 * page_bytes, BA.SENTINEL, np.uint8)
    big = BA.pool_view(flat, page_bytes, (page_bytes // cb,), hi, cb)
    assert big.dtype == dt and (cb == 1 or int(big[0, 0]) == BA.SENTINEL16)
    return n, compact, ids, flat, big


@pytest.mark.parametrize("page_bytes,hi,cb,bits,words", [c[:5] for c in _TRUNC], ids=[c[5] for c in _TRUNC])
def test_truncating_reader_and_writer_are_caught(page_bytes, hi, cb, bits, words):
    """Boundary scaled to 2^16: a pool scattered to far ids reads back through the table as its compact twin and passes
    assert_only_these_pages; a reader that truncates the byte offset returns other bytes for every table row; a writer that
    truncates fails assert_only_these_pages (pages missing where the table names them, or bytes outside them).  The page
    sizes of the 2-byte pools, on a uint16 pool with the boundary at 2^22: byte offsets of 21 and 22 bits and a word offset of
    21 bits (the scaled 31 / 32 / 31)."""
    bs, nhk, npg = BA.TABLE
    n, compact, ids, flat, big = _pool_case(page_bytes, hi, cb, page_bytes + bits)
    assert BA.sensitive_rows(ids.reshape(BA.TABLE), page_bytes, bits, words).all()
    byte_bits = bits + (1 if words == 2 else 0)      # a word offset of `bits` bits wraps where a byte offset of bits + 1 does
    BA.scatter_pool(big, compact, ids)
    np.testing.assert_array_equal(BA.gather_pool(big, ids), compact)                     # the honest reader
    got = BA.truncating_read(flat, ids, page_bytes, byte_bits).reshape(bs * nhk, npg, page_bytes)
    want = compact.view(np.uint8).reshape(bs * nhk, npg, page_bytes)
    assert all(not np.array_equal(g, w) for g, w in zip(got, want)), "a truncating reader went unnoticed in some row"
    BA.assert_only_these_pages(big, ids, compact, flat, "honest writer")
    assert BA.only_sentinel(flat)
    # the truncating writer
    BA.truncating_write(flat, ids, compact.view(np.uint8), page_bytes, byte_bits)
    with pytest.raises(AssertionError):
        BA.assert_only_these_pages(big, ids, compact, flat, "truncating writer")
    # a writer that puts every page right and one byte elsewhere
    flat[:] = BA.SENTINEL
    BA.scatter_pool(big, compact, ids)
    stray = int(np.setdiff1d(np.arange(big.shape[0]), ids)[-1])
    big[stray, 5] ^= 1
    with pytest.raises(AssertionError, match="outside"):
        BA.assert_only_these_pages(big, ids, compact, flat, "stray byte")


@pytest.mark.parametrize("page_bytes", WIDE_PAGE_BYTES)
def test_signed_word_index_is_caught(page_bytes):
    """A uint16 pool read through an offset in code words kept in a signed integer (31 value bits at full scale, 21 here): past
    byte 2^32 the index is negative; reduced into the buffer it returns other bytes for every table row.  Below the boundary
    the signed reader is the honest one, so only the pages past it show the fault - every row has some."""
    bs, nhk, npg = BA.TABLE
    n, compact, ids, flat, big = _pool_case(page_bytes, HI22, 2, page_bytes + 7)
    BA.scatter_pool(big, compact, ids)
    off_words = ids * (page_bytes // 2)
    assert (off_words >= 2 ** 21).any() and ((off_words + 2 ** 21) % 2 ** 22 - 2 ** 21 < 0).sum() == (off_words >= 2 ** 21).sum()
    got = BA.signed_word_read(flat, ids, page_bytes, 21)
    want = compact.view(np.uint8).reshape(n, page_bytes)
    past = BA.band_of(ids, page_bytes, HI22) == 2
    assert np.array_equal(got[~past], want[~past]) and not any(np.array_equal(g, w) for g, w in zip(got[past], want[past]))
    rows = lambda a: a.reshape(bs * nhk, npg, page_bytes)
    assert all(not np.array_equal(g, w) for g, w in zip(rows(got), rows(want))), "a signed word index went unnoticed in some row"


def test_encoder_table_test_does_not_wrap():
    """The encoders' 'inside the page table' decision in C's int arithmetic, for the destination tokens the GPU test feeds
    (test_flush_device_lengths_are_clamped_not_trusted): the present form drops every lane; the form with the wrapping sum
    tok0 + t lets lanes through with a negative page and offset - an index far below the base of the page table."""
    ps, n_pages, IMAX = 64, 3, 2 ** 31 - 1
    for n in (64, 128):
        starts = [IMAX, IMAX - 31, 2 ** 31 - ps, IMAX - n, 2 ** 31 - n + 1, -2 ** 31, n_pages * ps + 5000, -64]
        leaked = set()
        for tok0 in starts:
            for t in range(n):
                assert BA.enc_table_test(tok0, t, ps, n_pages, wrapping_sum=False)[0] is False, (tok0, t)
                ok, page, off = BA.enc_table_test(tok0, t, ps, n_pages, wrapping_sum=True)
                if ok:
                    assert page < 0 or off < 0
                    leaked.add(tok0)
        assert leaked == {IMAX, IMAX - 31, 2 ** 31 - ps, 2 ** 31 - n + 1} - ({2 ** 31 - ps} if n <= ps else set()), leaked
    # inside the table both forms agree, lane by lane, up to the table's last token
    for tok0 in (0, 1, ps - 1, ps, n_pages * ps - 64, n_pages * ps - 63, n_pages * ps - 1, n_pages * ps):
        for t in range(64):
            assert BA.enc_table_test(tok0, t, ps, n_pages, False) == BA.enc_table_test(tok0, t, ps, n_pages, True)
            assert BA.enc_table_test(tok0, t, ps, n_pages, False)[0] == (tok0 + t < n_pages * ps)


def test_flush_advance_does_not_wrap():
    """The length row the flush writes back: inside its ranges for every start at the edges of int in the present form; the
    form with T + n_flush in int wrote a negative T back."""
    n, cap_tok, rcap, IMAX = 64, 192, 128, 2 ** 31 - 1
    for T in (IMAX, IMAX - 31, IMAX - n, -2 ** 31, 0, 100, cap_tok - n, cap_tok - n + 1):
        for r in (rcap, 10, -2 ** 31, IMAX):
            T2, r2, st2 = BA.flush_advance(T, r, 5, n, cap_tok, rcap, wrapping_sum=False)
            assert 0 <= T2 <= cap_tok and r2 >= 0 and 0 <= st2 < rcap, (T, r, T2, r2)
            assert T2 == min(max(T, 0) + n, cap_tok) and r2 == max(r - n, 0)
    assert BA.flush_advance(IMAX, rcap, 5, n, cap_tok, rcap, wrapping_sum=True)[0] < 0
    assert BA.flush_advance(0, -2 ** 31, 5, n, cap_tok, rcap, wrapping_sum=True)[1] > 0
