"""CPU side of fork and swap on wide caches (million_cache_fork_wide / million_cache_swap_wide, blob format 2):
the symbols are prototyped and refuse bad calls before any launch; the numpy model of format 2 (tests/cache_swap_wide_model.py)
packs a uint16 pool and a packed pool of the same codes to one blob, is the identity on live data and never lets a dead byte
through; and, with the two ops replaced by that model, million_amd.paged_turns.fork / swap_out / swap_in move the host mirror, the
page table and the PageManager's reference counts of a wide cache exactly as an 8-bit twin's own methods move theirs, while the
cache's own four methods still refuse by name with nothing moved."""
import ctypes
import re
from pathlib import Path

import numpy as np
import pytest
import torch

from million_amd import _lib as L
from million_amd import paged_turns
from million_amd.pq_cache import PagedPQCache, RequestSnapshot
from tests import cache_fork_model as FM
from tests import cache_swap_model as SM
from tests import cache_swap_wide_model as WM
from tests import fork_swap_wide_common as X
from tests import packed_model as P

ROOT = Path(__file__).resolve().parents[1]
FORMATS = X.FORMATS


# ---------------------------------------------------------------- symbols, header, row bytes -------------------------------
def test_symbols_are_prototyped_and_documented():
    i32, vp = ctypes.c_int32, ctypes.c_void_p
    assert L.SYMBOLS["million_cache_fork_wide"] == (i32, [ctypes.POINTER(L.ForkDesc)] + [vp] * 8 + [i32, i32, vp])
    assert L.SYMBOLS["million_cache_swap_wide"] == (i32, [ctypes.POINTER(L.SwapDesc)] + [vp] * 9 + [i32, i32, vp])
    header = (ROOT / "include" / "million_hip.h").read_text()
    for name in ("million_cache_fork_wide", "million_cache_swap_wide"):
        assert re.search(r"\bint " + name + r"\(", header), name
    assert "Blob format, version 2" in header
    lib = L.load()
    assert lib.million_cache_fork_wide and lib.million_cache_swap_wide


def test_row_bytes_formula():
    from million_amd import ops
    for d, M, nbits in FORMATS:
        C = 2 ** nbits
        h = 2 if C <= 1024 else 4
        for ps in (32, 64, 128):
            for T in (0, 1, ps - 1, ps, ps + 1, 5 * ps + 3):
                for r in (0, 1, 64):
                    want = 2 * -(-T // ps) * ps * M * (8 + h) // 8 + 4 * r * d
                    assert ops.cache_swap_row_bytes_wide(T, r, ps, M, d, C) == want == WM.row_bytes(T, r, ps, M, d, C) and want % 16 == 0
    assert ops.FMT_U8.swap_row_bytes(70, 3, 32, 64, 128, 256) == ops.cache_swap_row_bytes(70, 3, 32, 64, 128)
    assert ops.FMT_U16.swap_row_bytes(70, 3, 32, 64, 128, 1024) == ops.FMT_PACKED.swap_row_bytes(70, 3, 32, 64, 128, 1024) == WM.row_bytes(70, 3, 32, 64, 128, 1024)
    assert (ops.FMT_U8.fork, ops.FMT_U8.swap, ops.FMT_U8.blob_version) == ("million_cache_fork", "million_cache_swap", 1)
    for fmt in (ops.FMT_U16, ops.FMT_PACKED):
        assert (fmt.fork, fmt.swap, fmt.blob_version) == ("million_cache_fork_wide", "million_cache_swap_wide", 2)


def _descs():
    f, s = L.ForkDesc(), L.SwapDesc()
    f.struct_size, s.struct_size = ctypes.sizeof(L.ForkDesc), ctypes.sizeof(L.SwapDesc)
    for d in (f, s):
        d.n_layers, d.bs, d.nh_k, d.d, d.M, d.page_size, d.n_pages_cap, d.n_pool, d.resid_cap = 2, 3, 2, 128, 64, 32, 4, 64, 64
        d.ids_layer_stride, d.rows_layer_stride, d.lengths_layer_stride, d.n_pages_bound = 24, 3 * 2 * 64 * 128, 12, 4
    f.src, f.n_dst, f.mode, f.prefix_tokens = 0, 1, L.MILLION_FORK_COPY, -1
    s.direction, s.layer0, s.n_layers_call, s.blob_bytes, s.n_slots = L.MILLION_SWAP_PACK, 0, 2, 1 << 20, 1
    return f, s


def test_entries_refuse_before_any_launch():
    """Bad shapes, C, modes and pointers are errors on a machine without a GPU too: nothing was launched.  The order is the 8-bit
    entries': page_size, M (then C), the geometry, mode / direction, the arguments, null pointers, alignment."""
    lib = L.load()
    shape, align, arg = -1, -2, -3      # MILLION_ERR_SHAPE, _ALIGN, _ARG
    buf = ctypes.create_string_buffer(4096)
    a = (ctypes.addressof(buf) + 15) & ~15

    def fork(desc, C=1024, packed=0, ptr=a):
        return lib.million_cache_fork_wide(ctypes.byref(desc), ptr, ptr, ptr, ptr, ptr, ptr, ptr, ptr, C, packed, None)

    def swap(desc, C=1024, packed=0, ptr=a):
        return lib.million_cache_swap_wide(ctypes.byref(desc), ptr, ptr, ptr, ptr, ptr, ptr, ptr, ptr, ptr, C, packed, None)

    def said():
        return lib.million_last_error().decode()

    for call, who in ((fork, "cache_fork_wide"), (swap, "cache_swap_wide")):
        d = _descs()[0 if call is fork else 1]
        d.struct_size = 4
        assert call(d) == arg and "struct_size" in said()
        for field, bad, word in (("page_size", 48, "page_size"), ("M", 24, "M="), ("d", 100, "multiple of 8")):
            d = _descs()[0 if call is fork else 1]
            setattr(d, field, bad)
            assert call(d) == shape and who in said() and word in said(), (who, field, said())
        for C in (256, 768, 8192, 0):
            assert call(_descs()[0 if call is fork else 1], C=C) == shape and "C=" in said()
        d = _descs()[0 if call is fork else 1]
        d.page_size, d.M = 48, 24      # page_size is said first, then M, then C
        assert call(d, C=7) == shape and "page_size" in said()
        d.page_size = 32
        assert call(d, C=7) == shape and "M=" in said()
        d = _descs()[0 if call is fork else 1]
        d.n_pages_bound = 5
        assert call(d) == arg and "n_pages_bound" in said()
        assert call(_descs()[0 if call is fork else 1], ptr=None) == arg and "null" in said()
        assert call(_descs()[0 if call is fork else 1], ptr=a + 4) == align and "aligned" in said()
        for packed in (0, 1):      # nothing to do: OK whatever the pointers
            d = _descs()[0 if call is fork else 1]
            setattr(d, "n_dst" if call is fork else "n_slots", 0)
            assert call(d, packed=packed, ptr=None) == 0
    f, s = _descs()
    f.mode, s.direction = 2, 2
    assert fork(f) == arg and "mode" in said() and swap(s) == arg and "direction" in said()
    s = _descs()[1]
    s.layer0 = 1
    assert swap(s) == arg and "layers" in said()


def test_ops_check_the_pools_before_the_library(monkeypatch):
    from million_amd import ops
    monkeypatch.setattr(ops.L, "load", lambda: pytest.fail("the library was entered"))
    monkeypatch.setattr(ops, "_need_cuda", lambda *a: None)
    ids = torch.zeros(2, 3, 2, 4, dtype=torch.int32)
    res = torch.zeros(2, 3, 2, 64, 128, dtype=torch.float16)
    ln, dst = torch.zeros(2, 3, 4, dtype=torch.int32), torch.zeros(1, dtype=torch.int32)
    u8 = torch.zeros(8, 32, 64, dtype=torch.uint8), torch.zeros(8, 64, 32, dtype=torch.uint8)
    u16 = torch.zeros(8, 32, 64, dtype=torch.uint16), torch.zeros(8, 64, 32, dtype=torch.uint16)
    pk = torch.zeros(8, P.page_bytes(32, 64, 1024), dtype=torch.uint8)

    def fork(k, v, **kw):
        ops.cache_fork_wide(ids, k, v, res, res, ln, dst, None, src=0, share=False, **kw)

    with pytest.raises(RuntimeError, match="uint8 pools hold 8-bit codes"):
        fork(*u8, C=1024)
    with pytest.raises(RuntimeError, match="C=256"):
        fork(*u16, C=256)
    with pytest.raises(RuntimeError, match="page_size= and M="):
        fork(pk, pk, C=1024, packed=True)
    with pytest.raises(RuntimeError, match="packed pool"):
        fork(pk, pk, C=4096, packed=True, page_size=32, M=64)      # 12-bit pages are larger
    with pytest.raises(RuntimeError, match="v_pool must be"):
        fork(u16[0], u16[0], C=1024)
    with pytest.raises(RuntimeError, match="said"):
        fork(*u16, C=1024, page_size=64)
    with pytest.raises(RuntimeError):      # the existing op still takes uint8 pools only
        ops.cache_fork(ids, *u16, res, res, ln, dst, None, src=0, share=False)
    with pytest.raises(RuntimeError, match="uint8 pools hold 8-bit codes"):
        ops.cache_swap_wide(0, ids, *u8, res, res, ln, torch.zeros(1, 4, dtype=torch.int32), torch.zeros(1, dtype=torch.int64),
                            torch.zeros(64, dtype=torch.uint8), C=1024)


# ---------------------------------------------------------------- the model of blob format 2 --------------------------------
LAYERS, BS, NHK, NPC, CAP = X.LAYERS, X.BS, X.NHK, X.NPC, X.CAP
_tables, _layout = X.tables, X.layout


@pytest.mark.parametrize("d,M,nbits", FORMATS)
def test_model_blob_is_canonical_and_round_trips(oracle, d, M, nbits):
    C, ps = 2 ** nbits, 32
    t = _tables(nbits, d, M, C, ps, oracle)
    table = np.asarray([[0, 69, CAP, 5], [1, 33, 1, CAP - 1], [2, 1, 0, 0]], np.int32)
    offs, total = _layout(table, ps, M, d, C)
    kw = dict(page_size=ps, M=M, C=C)
    blobs = {}
    for name, arrs in t.items():
        blobs[name] = np.full(total, 0xA5, np.uint8)
        before = [a.copy() for a in arrs]
        assert len(WM.pack(*arrs[:5], table, offs, blobs[name], **kw)) == 3
        assert all(np.array_equal(a, b) for a, b in zip(arrs, before)), "PACK only reads the cache"
    assert np.array_equal(blobs["u16"], blobs["packed"]), "the blob does not depend on the pool's format"
    blob = blobs["u16"]
    # dead pool bytes never reach the blob: other pool bytes behind the tokens >= T give the same blob, and the planes are zero there
    for name, arrs in t.items():
        other = [a.copy() for a in arrs]
        for slot, T, r, st in table.tolist():
            j, live = divmod(T, ps)
            if live:
                tail = other[0][:, slot, :, j].flatten()
                if name == "u16":
                    other[1][tail, live:] ^= 0x3FF
                    other[2][tail, :, live:] ^= 0x3FF
                else:
                    for pid in tail:
                        P.put_tokens(other[1][pid], "k", np.arange(live, ps), np.full((ps - live, M), C - 1, np.uint16), ps, M, C)
                        P.put_tokens(other[2][pid], "v", np.arange(live, ps), np.full((ps - live, M), C - 1, np.uint16), ps, M, C)
        again = np.full(total, 0xA5, np.uint8)
        WM.pack(*other[:5], table, offs, again, **kw)
        assert np.array_equal(again, blob), name
    pb, rb = P.page_bytes(ps, M, C), WM.row_bytes(33, 1, ps, M, d, C)
    row = blob[offs[1]:offs[1] + rb]      # slot 1: T = 33, token 1 of page 1 is the last live one
    k1, v1 = row[pb:2 * pb], row[3 * pb:4 * pb]
    hrow = M * P.hi_bits(C) // 8
    assert not k1[M:ps * M].any() and not k1[ps * M + hrow:].any() and k1[:M].any()
    assert not v1[:ps * M].reshape(M, ps)[:, 1:].any() and not v1[ps * M:].reshape(-1, ps)[:, 1:].any()
    assert (P.unpack(row[None, :pb], "k", ps, M, C) < C).all(), "every field is code & (C - 1)"
    # unpack o pack is the identity on live data, into either kind of pool, from either kind
    for name in ("u16", "packed"):
        dst = [a.copy() for a in t[name]]
        dst[0] = np.random.RandomState(3).permutation(dst[1].shape[0])[:dst[0].size].reshape(dst[0].shape).astype(np.int32)
        dst[1][...] = 0xA5
        dst[2][...] = 0xA5
        dst[3][...] = 0x7E00
        dst[4][...] = 0x7E00
        keep = [a.copy() for a in dst]
        written = WM.unpack(*dst, table, offs, blob, **kw)
        assert len(written) == LAYERS * NHK * (3 + 2 + 1)
        for slot, T, r, st in table.tolist():
            for src_name in ("u16", "packed"):
                want = WM.live_codes(*t[src_name][:3], slot, T, **kw)
                got = WM.live_codes(*dst[:3], slot, T, **kw)
                assert all(np.array_equal(a, b) for a, b in zip(want, got)), (name, src_name, slot)
            ring = (st + np.arange(r)) % CAP
            assert np.array_equal(dst[3][:, slot][:, :, ring], t["u16"][3][:, slot][:, :, ring])
            dead = np.setdiff1d(np.arange(CAP), ring)
            assert (dst[3][:, slot][:, :, dead] == 0x7E00).all() and (dst[4][:, slot][:, :, dead] == 0x7E00).all()
            assert dst[5][:, slot].tolist() == [[T, r, st, 0]] * LAYERS
        pages = sorted({w[4] for w in written})
        rest = np.setdiff1d(np.arange(dst[1].shape[0]), pages)
        assert np.array_equal(dst[1][rest], keep[1][rest]) and np.array_equal(dst[2][rest], keep[2][rest]), "other pages are untouched"
        if name == "u16":      # whole pages: codes of dead tokens are zero words
            j, live = divmod(33, ps)
            for pid in dst[0][:, 1, :, j].flatten():
                assert not dst[1][pid, live:].any() and not dst[2][pid, :, live:].any()
        again = np.full(total, 0x11, np.uint8)
        WM.pack(*dst[:5], table, offs, again, **kw)
        assert np.array_equal(again, blob)


def test_model_entries_that_take_no_part(oracle):
    d, M, C, ps = 64, 16, 1024, 32
    t = _tables(5, d, M, C, ps, oracle, garbage=False)["packed"]
    table = np.asarray([[-1, 5, 1, 0], [BS, 5, 1, 0], [0, 5, 1, 0], [1, 5, 1, 0], [2, 2 ** 31 - 1, -4, 99]], np.int32)
    rb = WM.row_bytes(5, 1, ps, M, d, C)
    big = WM.row_bytes(NPC * ps, 0, ps, M, d, C)
    offs = np.asarray([0, 0, 8, 0, LAYERS * NHK * rb], np.int64)      # entry 2: no multiple of 16
    blob = np.full(LAYERS * NHK * (rb + big), 0xA5, np.uint8)
    took = WM.pack(*t[:5], table, offs, blob, page_size=ps, M=M, C=C)
    assert [e[:4] for e in took] == [(1, 5, 1, 0), (2, NPC * ps, 0, 0)]
    t[0][0, 1, 0, 0] = -7      # an id outside the pool packs as zeros
    WM.pack(*t[:5], table[3:4], offs[3:4], blob, page_size=ps, M=M, C=C)
    assert not blob[:P.page_bytes(ps, M, C)].any()


# ---------------------------------------------------------------- host bookkeeping through paged_turns ----------------------
GEOM = dict(bs=3, nh=8, num_key_value_heads=2, M=64, layer_num=2, d=128, page_size=32, extended_residual_size=64, max_tokens=256)


def _np16(t):
    return t.view(torch.int16).numpy().view(np.uint16) if t.dtype == torch.uint16 else t.numpy()


def _cache(monkeypatch, nbits, packed, preallocate, log, seed=0):
    """A CPU cache whose slot 0 holds 70 coded tokens and a wrapped window of 40 rows.  The fork and swap ops are the numpy models."""
    from million_amd import ops
    for name in ("pq_encode_into", "pq_encode_into_packed"):
        monkeypatch.setattr(ops, name, lambda *a, **k: None)
    monkeypatch.setattr(ops, "prefill_attn", lambda q, k, v, **kw: torch.zeros_like(q))
    monkeypatch.setattr(ops, "cache_fork", FM.as_ops_stub())
    monkeypatch.setattr(ops, "cache_swap", SM.as_ops_stub(log))
    wide = WM.as_ops_stubs(log)
    monkeypatch.setattr(ops, "cache_fork_wide", wide[0])
    monkeypatch.setattr(ops, "cache_swap_wide", wide[1])
    cache = PagedPQCache(**GEOM, nbits=nbits, dtype=torch.uint8 if nbits == 8 else torch.uint16, packed=packed, preallocate=preallocate,
                         device="cpu")
    C = 2 ** nbits
    cache.key_cent = torch.full((64, C, 2), 0.5, dtype=torch.float16)
    cache.value_cent = torch.full((64, C, 2), 0.25, dtype=torch.float16)
    cache._kprep = cache._vprep = torch.zeros(1, dtype=torch.float16)
    rs = np.random.RandomState(seed)
    n = cache.key_page_pool.shape[0]
    k16, v16 = rs.randint(0, C, (n, 32, 64)).astype(np.uint16), rs.randint(0, C, (n, 64, 32)).astype(np.uint16)
    if packed:
        _np16(cache.key_page_pool)[...], _np16(cache.value_page_pool)[...] = P.pack(k16, "k", C), P.pack(v16, "v", C)
    else:
        _np16(cache.key_page_pool)[...], _np16(cache.value_page_pool)[...] = k16, v16
    g = torch.Generator().manual_seed(seed)
    cache._kres_all.copy_(torch.randn(cache._kres_all.shape, generator=g).half())
    cache._vres_all.copy_(torch.randn(cache._vres_all.shape, generator=g).half())
    _fill(cache, 0, 70, 40, 50, 110)
    return cache


def _fill(cache, b, T, r, rs, seen):
    x = torch.zeros(1, 2, T, 128, dtype=torch.float16)
    for l in range(2):
        cache.prefill_request(b, torch.zeros(1, 8, T, 128, dtype=torch.float16), x, x, l)
    cache._r_a[:, b], cache._rs_a[:, b], cache._seen_a[:, b] = r, rs, seen
    for l in range(2):
        cache._sync_lengths(l, b)


def _books(cache):
    """Everything the host keeps: mirrors, page counts, table, device rows, the PageManager's counts, who owns which page."""
    pm = cache.page_manager
    owned = [[[list(x) for x in b] for b in l] for l in cache._host_pids]
    refs = {p: pm.ref_count(p) for l in owned for b in l for h in b for p in h}
    return ([a.copy() for a in cache.host_state()], cache._pages_a.copy(), cache._page_ids_all.numpy().copy(), cache._lengths_all.numpy().copy(),
            pm.get_stats(), cache.sharing_stats(), owned, refs, sorted(pm.free_pages))


def _books_equal(a, b):
    return (all(np.array_equal(x, y) for x, y in zip(a[0], b[0])) and all(np.array_equal(x, y) for x, y in zip(a[1:4], b[1:4]))
            and a[4:] == b[4:])


def _data(cache):
    return [_np16(t).copy() for t in (cache.key_page_pool, cache.value_page_pool)] + [cache._kres_all.view(torch.int16).numpy().copy(),
                                                                                      cache._vres_all.view(torch.int16).numpy().copy()]


def _live(cache, b, T, r, st):
    kw = dict(page_size=32, M=64, C=cache.C)
    ring = (st + np.arange(r)) % 64
    k, v = WM.live_codes(cache._page_ids_all.numpy(), _np16(cache.key_page_pool), _np16(cache.value_page_pool), b, T, **kw)
    return [k, v, cache._kres_all.view(torch.int16).numpy()[:, b][:, :, ring].copy(), cache._vres_all.view(torch.int16).numpy()[:, b][:, :, ring].copy()]


@pytest.mark.parametrize("preallocate", [False, True], ids=["on-demand", "preallocated"])
@pytest.mark.parametrize("packed", [False, True], ids=["uint16", "packed"])
def test_paged_turns_move_the_books_as_the_8_bit_twin(monkeypatch, packed, preallocate):
    log = []      # of both caches' ops; the wide cache's call is the later one of a step
    twin = _cache(monkeypatch, 8, False, preallocate, log)
    wide = _cache(monkeypatch, 10, packed, preallocate, log)
    assert _books_equal(_books(wide), _books(twin))
    want = _live(wide, 0, 70, 40, 50)

    def both(step, *a, **kw):
        out8 = getattr(twin, step)(*a, **kw)
        out = getattr(paged_turns, step)(wide, *a, **kw)
        assert _books_equal(_books(wide), _books(twin)), step
        return out, out8

    both("fork", 0, 1)
    assert log[-1]["op"] == "fork" and (log[-1]["C"], log[-1]["packed"], log[-1]["share"]) == (1024, packed, not preallocate)
    assert log[-1]["n_pages_bound"] == 3 and log[-1]["prefix_tokens"] == -1
    assert all(np.array_equal(a, b) for a, b in zip(want, _live(wide, 1, 70, 40, 50)))
    if not preallocate:
        assert wide.sharing_stats() == {"shared_pages": 8, "extra_references": 8}
    both("fork", 0, [2], n_tokens=33)
    assert log[-1]["prefix_tokens"] == 33 and wide._lengths_all[:, 2].tolist() == [[33, 0, 0, 0]] * 2
    assert all(np.array_equal(a[:, :, :33], b) for a, b in zip(want[:2], _live(wide, 2, 33, 0, 0)[:2]))
    wide.release(2), twin.release(2)
    snap, snap8 = both("swap_out", 1)
    assert isinstance(snap, RequestSnapshot) and snap.meta["version"] == 2 and snap8.meta["version"] == 1 and "packed" not in snap.meta
    assert {k: v for k, v in snap.meta.items() if k not in ("version", "nbits", "key_cent_sha256", "value_cent_sha256")} == \
           {k: v for k, v in snap8.meta.items() if k not in ("version", "nbits", "key_cent_sha256", "value_cent_sha256")}
    assert snap.meta["nbits"] == 10 and snap.blob.numel() == 2 * 2 * WM.row_bytes(70, 40, 32, 64, 128, 1024)
    assert log[-1]["op"] == "swap" and log[-1]["direction"] == WM.PACK and log[-1]["slot_table"] == [[1, 70, 40, 50]]
    keep, keep8 = both("snapshot_request", 0)
    assert torch.equal(keep.blob, snap.blob), "a fork's snapshot is its source's: the blob is a function of the live data"
    twin.swap_in(2, snap8), paged_turns.swap_in(wide, 2, snap)
    assert _books_equal(_books(wide), _books(twin))
    assert log[-1]["direction"] == WM.UNPACK and log[-1]["slot_table"] == [[2, 70, 40, 50]]
    assert all(np.array_equal(a, b) for a, b in zip(want, _live(wide, 2, 70, 40, 50)))
    wide.release(0), twin.release(0)
    assert _books_equal(_books(wide), _books(twin))
    assert all(np.array_equal(a, b) for a, b in zip(want, _live(wide, 2, 70, 40, 50)))
    several, several8 = both("swap_out", [2], staging_bytes=1)
    assert [(c["layer0"], c["n_layers"]) for c in log[-2:]] == [(0, 1), (1, 1)] and torch.equal(several[0].blob, snap.blob)


@pytest.mark.parametrize("packed", [False, True], ids=["uint16", "packed"])
def test_the_cache_s_own_methods_still_refuse_with_nothing_moved(monkeypatch, packed):
    log = []
    cache = _cache(monkeypatch, 10, packed, False, log)
    snap = paged_turns.snapshot_request(cache, 0)
    del log[:]
    before, data = _books(cache), _data(cache)
    for call in (lambda: cache.fork(0, 1), lambda: cache.fork(0, [1, 2], n_tokens=3), lambda: cache.swap_out(0),
                 lambda: cache.snapshot_request(0), lambda: cache.swap_in(1, snap)):
        with pytest.raises(NotImplementedError, match="nbits"):
            call()
    assert not log and _books_equal(before, _books(cache)) and all(np.array_equal(a, b) for a, b in zip(data, _data(cache)))


def test_snapshot_versions_and_geometry_are_checked_before_any_change(monkeypatch, tmp_path):
    from million_amd import formats
    log = []
    wide = _cache(monkeypatch, 10, False, False, log)
    plain = _cache(monkeypatch, 8, False, False, log)
    other = _cache(monkeypatch, 9, False, False, log)
    snap2, snap1, snap9 = paged_turns.snapshot_request(wide, 0), plain.snapshot_request(0), paged_turns.snapshot_request(other, 0)
    assert (snap2.meta["version"], snap1.meta["version"], snap9.meta["version"]) == (2, 1, 2)
    del log[:]
    for cache, call, word in ((wide, lambda: paged_turns.swap_in(wide, 1, snap1), "version 1"),
                              (plain, lambda: plain.swap_in(1, snap2), "version 2"),
                              (plain, lambda: paged_turns.swap_in(plain, 1, snap2), "version 2"),
                              (wide, lambda: paged_turns.swap_in(wide, 1, snap9), "nbits=9"),
                              (wide, lambda: paged_turns.swap_in(wide, 0, snap2), "holds tokens")):
        before, data = _books(cache), _data(cache)
        with pytest.raises(RuntimeError, match=word):
            call()
        assert not log and _books_equal(before, _books(cache)) and all(np.array_equal(a, b) for a, b in zip(data, _data(cache)))
    # version 2 travels through a file as it is
    back = formats.load_request(formats.save_request(tmp_path / "req.pt", snap2))
    assert back.meta == snap2.meta and torch.equal(back.blob, snap2.blob)
    paged_turns.swap_in(wide, 1, back)
    assert all(np.array_equal(a, b) for a, b in zip(_live(wide, 0, 70, 40, 50), _live(wide, 1, 70, 40, 50)))


@pytest.mark.parametrize("src_packed", [False, True], ids=["from-uint16", "from-packed"])
def test_a_snapshot_crosses_between_packed_and_unpacked_caches(monkeypatch, src_packed):
    log = []
    a = _cache(monkeypatch, 10, src_packed, False, log)
    b = _cache(monkeypatch, 10, not src_packed, True, log, seed=4)
    snap = paged_turns.swap_out(a, 0)
    paged_turns.swap_in(b, 2, snap)
    assert log[-2]["packed"] == src_packed and log[-1]["packed"] == (not src_packed)
    a2 = _cache(monkeypatch, 10, src_packed, False, log)
    assert all(np.array_equal(x, y) for x, y in zip(_live(a2, 0, 70, 40, 50), _live(b, 2, 70, 40, 50)))
    assert torch.equal(paged_turns.snapshot_request(b, 2).blob, snap.blob)
