"""CPU tests of the request swap (million_cache_swap, ops.cache_swap, PagedPQCache.swap_out / swap_in, formats.save_request /
load_request): the descriptor layout and the validation before any launch, the numpy model of blob format 1 the GPU tests
compare against (tests/cache_swap_model.py), the host bookkeeping of swap_out / swap_in with the device call replaced by that
model, and the file round trip."""
import ctypes
import pickle
import subprocess
import sys
import tempfile
from pathlib import Path

import numpy as np
import pytest
import torch

from million_amd.pq_cache import PagedPQCache, RequestSnapshot
from tests import cache_fork_model as FM
from tests import cache_swap_model as SM

ROOT = Path(__file__).resolve().parents[1]
ARG, SHAPE, ALIGN = -3, -1, -2


# ---------------------------------------------------------------- C ABI ----------------------------------------------------
@pytest.fixture(scope="module")
def lib():
    from million_amd import build, _lib
    build.build()
    return _lib.load()


def test_symbol_and_desc_match_the_header(lib):
    from million_amd import _lib
    assert "million_cache_swap" in _lib.SYMBOLS and lib.million_cache_swap.restype is _lib.c_i32
    names = [f[0] for f in _lib.SwapDesc._fields_]
    offs = ", ".join(f"offsetof(million_swap_desc, {n})" for n in names)
    src = ('#include "million_hip.h"\n#include <stdio.h>\n#include <stddef.h>\n'
           f'int main(){{size_t v[] = {{sizeof(million_swap_desc), {offs}, MILLION_SWAP_PACK, MILLION_SWAP_UNPACK}};\n'
           'for (unsigned i = 0; i < sizeof(v) / sizeof(v[0]); ++i) printf("%zu ", v[i]);return 0;}\n')
    with tempfile.TemporaryDirectory() as td:
        (Path(td) / "a.c").write_text(src)
        subprocess.check_call(["gcc", "-std=c11", "-I", str(ROOT / "include"), "-o", f"{td}/a", f"{td}/a.c"])
        vals = list(map(int, subprocess.check_output([f"{td}/a"]).split()))
    assert vals[0] == ctypes.sizeof(_lib.SwapDesc)
    assert vals[1:-2] == [getattr(_lib.SwapDesc, n).offset for n in names]
    assert vals[-2:] == [_lib.MILLION_SWAP_PACK, _lib.MILLION_SWAP_UNPACK] == [SM.PACK, SM.UNPACK]


def _desc(**kw):
    from million_amd import _lib
    d = _lib.SwapDesc()
    d.struct_size = ctypes.sizeof(_lib.SwapDesc)
    d.direction = SM.PACK
    d.n_layers, d.bs, d.nh_k, d.d, d.M, d.page_size, d.n_pages_cap, d.n_pool, d.resid_cap = 3, 4, 2, 128, 64, 64, 8, 192, 128
    d.ids_layer_stride, d.rows_layer_stride, d.lengths_layer_stride = 4 * 2 * 8, 4 * 2 * 128 * 128, 16
    d.layer0, d.n_layers_call, d.n_slots, d.n_pages_bound, d.blob_bytes = 0, 3, 2, 8, 1 << 20
    for k, v in kw.items():
        setattr(d, k, v)
    return d


# fake aligned "device pointers": validation never dereferences them
PTRS = dict(page_ids=0x1000, k_pool=0x2000, v_pool=0x3000, k_resid=0x4000, v_resid=0x5000, dev_lengths=0x6000,
            slot_table=0x7000, blob_offsets=0x8000, blob=0x9000)


def _call(lib, d, **over):
    p = dict(PTRS, **over)
    return lib.million_cache_swap(ctypes.byref(d), *[p[k] for k in PTRS], None)


def test_validation_before_any_launch(lib):
    err = lib.million_last_error
    assert _call(lib, _desc(struct_size=12)) == ARG and b"struct_size" in err()
    assert _call(lib, _desc(direction=2)) == ARG and b"direction=2" in err()
    assert _call(lib, _desc(direction=-1)) == ARG
    for kw in (dict(layer0=-1), dict(layer0=3, n_layers_call=1), dict(layer0=1, n_layers_call=3), dict(n_layers_call=0),
               dict(n_layers_call=-1), dict(n_layers_call=4), dict(layer0=2 ** 31 - 1, n_layers_call=2 ** 31 - 1)):
        assert _call(lib, _desc(**kw)) == ARG and b"layers" in err(), kw
    assert _call(lib, _desc(n_pages_bound=9)) == ARG and _call(lib, _desc(n_slots=-1)) == ARG and _call(lib, _desc(blob_bytes=-1)) == ARG
    for name in ("page_ids", "k_pool", "v_pool", "dev_lengths", "slot_table", "blob_offsets", "blob"):
        assert _call(lib, _desc(), **{name: None}) == ARG and b"null" in err(), name
        assert _call(lib, _desc(direction=SM.UNPACK), **{name: None}) == ARG, name
    assert _call(lib, _desc(), k_resid=None) == ARG and b"window" in err()
    assert _call(lib, _desc(), v_resid=None) == ARG and b"window" in err()
    assert _call(lib, _desc(page_size=48)) == SHAPE and b"page_size=48" in err()
    assert _call(lib, _desc(M=8)) == SHAPE and b"M=8" in err()
    assert _call(lib, _desc(M=128)) == SHAPE
    assert _call(lib, _desc(d=60)) == SHAPE and _call(lib, _desc(bs=0)) == SHAPE and _call(lib, _desc(n_pool=0)) == SHAPE
    assert _call(lib, _desc(n_pages_cap=2 ** 30, n_pages_bound=0)) == SHAPE and _call(lib, _desc(n_layers=0)) == SHAPE
    assert _call(lib, _desc(n_slots=2 ** 28)) == SHAPE and b"tasks" in err()      # the task list must fit 31 bits
    for name in ("k_pool", "v_pool", "k_resid", "v_resid", "blob"):
        assert _call(lib, _desc(), **{name: PTRS[name] + 8}) == ALIGN and b"16-byte" in err(), name
    assert _call(lib, _desc(rows_layer_stride=4 * 2 * 128 * 128 + 4)) == ALIGN
    for name in ("page_ids", "dev_lengths", "slot_table"):
        assert _call(lib, _desc(), **{name: PTRS[name] + 2}) == ALIGN, name
    assert _call(lib, _desc(), blob_offsets=PTRS["blob_offsets"] + 4) == ALIGN and b"8-byte" in err()
    # shape errors come before pointer errors, pointer errors before alignment
    assert _call(lib, _desc(M=8), k_pool=None) == SHAPE and _call(lib, _desc(), k_pool=None, v_pool=PTRS["v_pool"] + 8) == ARG


def test_no_entry_returns_ok(lib):
    assert _call(lib, _desc(n_slots=0)) == 0
    assert lib.million_cache_swap(ctypes.byref(_desc(n_slots=0)), *[None] * 9, None) == 0
    assert lib.million_cache_swap(ctypes.byref(_desc(n_slots=0, direction=SM.UNPACK)), *[None] * 9, None) == 0


def test_swap_kernels_fit_eight_waves_per_simd_without_scratch(lib):
    out = subprocess.run([sys.executable, str(ROOT / "tools" / "kernel_meta.py"), str(ROOT / "million_amd" / "libmillion_hip.so"), "cache_swap"],
                         capture_output=True, text=True, check=True).stdout
    rows = [l for l in out.splitlines() if "cache_swap_kernel" in l]
    assert len(rows) == 2, out
    for row in rows:
        assert "vgpr_spill 0" in row and row.rstrip().endswith("scratch 0 B"), row
        assert int(row.split("vgpr")[1].split()[0]) <= 64 and "lds 0 B" in row, row      # 8 waves per SIMD, no LDS


# ---------------------------------------------------------------- the numpy model ------------------------------------------
def _tables(rs, *, layers=3, bs=4, nhk=2, cap_pages=5, ps=32, M=16, rcap=8, d=8):
    """Random tables with distinct ids per (layer, slot, head, page), random pools, windows and lengths."""
    n_pool = layers * bs * nhk * cap_pages + 7
    ids = rs.permutation(n_pool)[:layers * bs * nhk * cap_pages].reshape(layers, bs, nhk, cap_pages).astype(np.int32)
    kp = rs.randint(0, 256, (n_pool, ps, M)).astype(np.uint8)
    vp = rs.randint(0, 256, (n_pool, M, ps)).astype(np.uint8)
    kr = rs.randint(-30000, 30000, (layers, bs, nhk, rcap, d)).astype(np.int16)
    vr = rs.randint(-30000, 30000, (layers, bs, nhk, rcap, d)).astype(np.int16)
    ln = rs.randint(0, 50, (layers, bs, 4)).astype(np.int32)
    return [ids, kp, vp, kr, vr, ln]


def _blob_for(table, *, layers, nhk, ps, M, d, fill=0xA5):
    sizes = [layers * nhk * SM.row_bytes(int(T), int(r), ps, M, d) for _, T, r, _ in table]
    offs = np.concatenate([[0], np.cumsum(sizes)]).astype(np.int64)
    return np.full(int(offs[-1]), fill, np.uint8), offs[:-1].copy(), sizes


def test_row_bytes_matches_ops():
    from million_amd import ops
    for T in (0, 1, 31, 32, 33, 1000):
        for r in (0, 1, 64):
            for ps, M, d in ((32, 16, 8), (64, 64, 128), (128, 32, 64)):
                want = SM.row_bytes(T, r, ps, M, d)
                assert ops.cache_swap_row_bytes(T, r, ps, M, d) == want == 2 * -(-T // ps) * ps * M + 4 * r * d and want % 16 == 0


def test_model_round_trip_reproduces_the_live_data():
    rs = np.random.RandomState(0)
    src = _tables(rs)
    table = np.asarray([[2, 70, 5, 6], [0, 32, 8, 3], [3, 0, 0, 0], [1, 1, 1, 7]], np.int32)
    blob, offs, sizes = _blob_for(table, layers=3, nhk=2, ps=32, M=16, d=8)
    before = [a.copy() for a in src]
    took = SM.pack(*src[:5], table, offs, blob)
    assert len(took) == 4 and all(np.array_equal(a, b) for a, b in zip(src, before))      # PACK writes only the blob
    assert not (blob == 0xA5).all()
    # into another cache: other ids, other slots (entry i goes to slot 3 - i), everything else random
    dst = _tables(np.random.RandomState(1))
    old = [a.copy() for a in dst]
    t2 = table.copy()
    t2[:, 0] = 3 - t2[:, 0]
    written = SM.unpack(*dst, t2, offs, blob)
    assert np.array_equal(dst[0], old[0])                                                  # UNPACK never writes the table
    for (s_src, T, r, st), s_dst in zip(table.tolist(), t2[:, 0].tolist()):
        for a, b in zip(SM.live_data(*src[:5], s_src, T, r, st), SM.live_data(*dst[:5], s_dst, T, r, st)):
            assert np.array_equal(a, b)
        assert dst[5][:, s_dst].tolist() == [[T, r, st, 0]] * 3
        ring = (st + np.arange(r)) % 8
        rest = np.setdiff1d(np.arange(8), ring)
        assert np.array_equal(dst[3][:, s_dst][:, :, rest], old[3][:, s_dst][:, :, rest])  # ring rows outside the window stay
        assert np.array_equal(dst[4][:, s_dst][:, :, rest], old[4][:, s_dst][:, :, rest])
    touched = {w[-1] for w in written}
    assert len(written) == 3 * 2 * (3 + 1 + 0 + 1) == len(touched)
    rest = np.setdiff1d(np.arange(dst[1].shape[0]), list(touched))
    assert np.array_equal(dst[1][rest], old[1][rest]) and np.array_equal(dst[2][rest], old[2][rest])
    # the restored cache packs to the same blob: the format is canonical
    again = np.full_like(blob, 0x5A)
    SM.pack(*dst[:5], t2, offs, again)
    assert np.array_equal(again, blob)


def test_model_pack_ignores_dead_bytes():
    rs = np.random.RandomState(2)
    a = _tables(rs)
    table = np.asarray([[1, 70, 5, 6]], np.int32)
    blob_a, offs, _ = _blob_for(table, layers=3, nhk=2, ps=32, M=16, d=8)
    SM.pack(*a[:5], table, offs, blob_a)
    b = [x.copy() for x in a]
    ids = a[0][:, 1, :, :3]
    live = np.zeros(a[1].shape[0], bool)
    live[ids.flatten()] = True
    b[1][~live], b[2][~live] = 0xFF, 0xEE                                  # pages the request does not own
    b[1][ids[:, :, 2], 6:], b[2][ids[:, :, 2], :, 6:] = 0xFF, 0xEE         # the tail page past token 70 = 2 * 32 + 6
    b[0][:, 1, :, 3:] = -12345                                             # table entries at or past n_live
    dead = np.setdiff1d(np.arange(8), (6 + np.arange(5)) % 8)
    b[3][:, :, :, dead], b[4][:, :, :, dead] = 0x7E00, 0x7E00              # ring rows outside [start, start + r)
    b[3][:, [0, 2, 3]], b[1][a[0][:, 0].flatten()] = 1, 2                  # other slots
    blob_b = np.full_like(blob_a, 0x11)
    SM.pack(*b[:5], table, offs, blob_b)
    assert np.array_equal(blob_a, blob_b)
    # and the dead bytes of the blob's own tail page are zero
    rb = SM.row_bytes(70, 5, 32, 16, 8)
    row = blob_a[:rb]
    assert not row[2 * 512 + 6 * 16:3 * 512].any() and not row[3 * 512 + 2 * 512:][:512].reshape(16, 32)[:, 6:].any()
    assert row[3 * 512 + 2 * 512:][:512].reshape(16, 32)[:, :6].any()


def test_model_on_untrusted_values():
    rs = np.random.RandomState(3)
    a = _tables(rs)
    n_pool = a[1].shape[0]
    # T past the bound, r past the window, a start outside the ring; slots outside the batch take no part
    table = np.asarray([[1, 100000, 99, 8], [4, 10, 1, 0], [-1, 10, 1, 0], [2, -5, -1, -1]], np.int32)
    eff = np.asarray([[1, 4 * 32, 8, 0], [2, 0, 0, 0]], np.int32)
    blob, offs, sizes = _blob_for(np.asarray([[1, 128, 8, 0], [4, 10, 1, 0], [-1, 10, 1, 0], [2, 0, 0, 0]]), layers=3, nhk=2, ps=32, M=16, d=8)
    took = SM.pack(*a[:5], table, offs, blob, n_pages_bound=4)
    assert [t[:4] for t in took] == [(1, 128, 8, 0), (2, 0, 0, 0)]
    want = np.full_like(blob, 0xA5)
    SM.pack(*a[:5], eff, offs[[0, 3]], want, n_pages_bound=4)
    assert np.array_equal(blob, want) and (blob[offs[1]:offs[3]] == 0xA5).all()
    # ids outside the pool: zeros on pack, skipped on unpack
    a[0][0, 1, 0, 1], a[0][2, 1, 1, 3] = -1, n_pool
    SM.pack(*a[:5], eff[:1], offs[:1], blob, n_pages_bound=4)
    rb = SM.row_bytes(128, 8, 32, 16, 8)
    assert not blob[512:1024].any() and not blob[4 * 512 + 512:][:512].any() and blob[:512].any()
    b = [x.copy() for x in a]
    written = SM.unpack(*b, eff[:1], offs[:1], blob, n_pages_bound=4)
    assert len(written) == 3 * 2 * 4 - 2 and all(0 <= w[-1] < n_pool for w in written)
    # an entry whose rows do not fit the blob, a misaligned or negative offset
    small = np.full(6 * rb - 16, 0xA5, np.uint8)
    assert not SM.pack(*a[:5], eff[:1], np.asarray([0], np.int64), small, n_pages_bound=4) and (small == 0xA5).all()
    assert not SM.pack(*a[:5], eff[:1], np.asarray([8], np.int64), blob, n_pages_bound=4)
    assert not SM.pack(*a[:5], eff[:1], np.asarray([-16], np.int64), blob, n_pages_bound=4)
    # a range of layers is a contiguous byte range and touches its layers only
    blob2 = np.full_like(blob, 0xA5)
    a = _tables(np.random.RandomState(4))
    SM.pack(*a[:5], eff[:1], offs[:1], blob, n_pages_bound=4)
    SM.pack(*a[:5], eff[:1], offs[:1], blob2[2 * rb:], layer0=1, n_layers=1, n_pages_bound=4)
    assert np.array_equal(blob2[2 * rb:4 * rb], blob[2 * rb:4 * rb]) and (blob2[:2 * rb] == 0xA5).all() and (blob2[4 * rb:] == 0xA5).all()
    b = _tables(np.random.RandomState(5))
    old = [x.copy() for x in b]
    SM.unpack(*b, eff[:1], offs[:1], blob[2 * rb:4 * rb], layer0=1, n_layers=1, n_pages_bound=4)
    assert b[5][1, 1].tolist() == [128, 8, 0, 0] and np.array_equal(b[5][[0, 2]], old[5][[0, 2]])
    assert np.array_equal(b[3][[0, 2]], old[3][[0, 2]]) and np.array_equal(b[3][1, 1], a[3][1, 1])


# ---------------------------------------------------------------- host bookkeeping of swap_out / swap_in -------------------
GEOM = dict(bs=3, nh=8, num_key_value_heads=2, M=64, layer_num=2, d=128, page_size=32, extended_residual_size=64, max_tokens=256)


def _cache(monkeypatch, preallocate, log, seed=0, fill=True, **kw):
    """A CPU cache (2 layers, 3 slots, pages of 32, window 64) whose slot 0 holds 70 coded tokens and a wrapped window of 40
    rows; ops.cache_fork and ops.cache_swap are the numpy models."""
    from million_amd import ops
    monkeypatch.setattr(ops, "pq_encode_into", lambda *a, **k: None)
    monkeypatch.setattr(ops, "prefill_attn", lambda q, k, v, **kw: torch.zeros_like(q))
    monkeypatch.setattr(ops, "cache_fork", FM.as_ops_stub())
    monkeypatch.setattr(ops, "cache_swap", SM.as_ops_stub(log))
    cache = PagedPQCache(**dict(GEOM, **kw), preallocate=preallocate, device="cpu")
    cache.key_cent = torch.full((64, 256, 2), 0.5, dtype=torch.float16)
    cache.value_cent = torch.full((64, 256, 2), 0.25, dtype=torch.float16)
    cache._kprep = cache._vprep = torch.zeros(1, dtype=torch.float16)
    g = torch.Generator().manual_seed(seed)
    cache.key_page_pool.copy_(torch.randint(0, 256, cache.key_page_pool.shape, generator=g, dtype=torch.uint8))
    cache.value_page_pool.copy_(torch.randint(0, 256, cache.value_page_pool.shape, generator=g, dtype=torch.uint8))
    cache._kres_all.copy_(torch.randn(cache._kres_all.shape, generator=g).half())
    cache._vres_all.copy_(torch.randn(cache._vres_all.shape, generator=g).half())
    if fill:
        _fill(cache, 0, 70, 40, 50, 110)
    return cache


def _fill(cache, b, T, r, rs, seen):
    x = torch.zeros(1, 2, T, 128, dtype=torch.float16)
    for l in range(2):
        cache.prefill_request(b, torch.zeros(1, 8, T, 128, dtype=torch.float16), x, x, l)
    cache._r_a[:, b], cache._rs_a[:, b], cache._seen_a[:, b] = r, rs, seen
    for l in range(2):
        cache._sync_lengths(l, b)


def _allocated(cache):
    return cache.page_manager.get_stats()["allocated_pages"]


def _live(cache, b, T, r, st):
    view16 = lambda t: t.view(torch.int16).numpy()
    return [x.copy() for x in SM.live_data(cache._page_ids_all.numpy(), cache.key_page_pool.numpy(), cache.value_page_pool.numpy(),
                                          view16(cache._kres_all), view16(cache._vres_all), b, T, r, st)]


def _state(cache):
    return ([a.copy() for a in cache.host_state()], cache._pages_a.copy(), cache._page_ids_all.clone(), cache._lengths_all.clone(),
            cache.key_page_pool.clone(), cache.value_page_pool.clone(), cache._kres_all.clone(), cache._vres_all.clone(),
            cache.page_manager.get_stats(), cache.sharing_stats(), [[[list(x) for x in b] for b in l] for l in cache._host_pids])


def _same(before, after):
    return (all(np.array_equal(a, b) for a, b in zip(before[0], after[0])) and np.array_equal(before[1], after[1])
            and all(torch.equal(a, b) for a, b in zip(before[2:8], after[2:8])) and before[8:] == after[8:])


@pytest.mark.parametrize("preallocate", [False, True], ids=["on-demand", "preallocated"])
def test_swap_out_then_in_moves_the_request_and_the_mirrors(monkeypatch, preallocate):
    log = []
    cache = _cache(monkeypatch, preallocate, log)
    n0 = _allocated(cache)
    want = _live(cache, 0, 70, 40, 50)
    cache._pre_a[:, 0] = 1
    snap = cache.swap_out(0)
    assert isinstance(snap, RequestSnapshot) and snap.blob.dtype == torch.uint8 and snap.blob.dim() == 1
    rb = SM.row_bytes(70, 40, 32, 64, 128)
    assert snap.blob.numel() == 2 * 2 * rb
    assert {k: snap.meta[k] for k in ("version", "layer_num", "nh_k", "d", "M", "nbits", "page_size", "resid_cap", "T", "r", "start", "seen")} == dict(
        version=1, layer_num=2, nh_k=2, d=128, M=64, nbits=8, page_size=32, resid_cap=64, T=70, r=40, start=50, seen=110)
    assert len(snap.meta["key_cent_sha256"]) == 64 and snap.meta["key_cent_sha256"] != snap.meta["value_cent_sha256"]
    assert len(log) == 1 and log[0]["direction"] == SM.PACK and log[0]["slot_table"] == [[0, 70, 40, 50]] and log[0]["n_pages_bound"] == 3
    assert (log[0]["layer0"], log[0]["n_layers"], log[0]["blob_offsets"]) == (0, 2, [0])
    # released: mirrors, device rows and (on demand) pages are those of an empty slot
    for arr in (cache._T_a, cache._r_a, cache._rs_a, cache._seen_a, cache._pre_a):
        assert not arr[:, 0].any()
    assert not cache._lengths_all[:, 0].any()
    assert _allocated(cache) == (n0 if preallocate else 0)
    if not preallocate:
        assert cache._pages_a[:, 0].tolist() == [0, 0] and cache._host_pids[0][0] == [[], []]
    # something else uses the slot and the pages in between
    _fill(cache, 0, 33, 0, 0, 33)
    g = torch.Generator().manual_seed(9)
    cache.key_page_pool.copy_(torch.randint(0, 256, cache.key_page_pool.shape, generator=g, dtype=torch.uint8))
    cache.value_page_pool.copy_(torch.randint(0, 256, cache.value_page_pool.shape, generator=g, dtype=torch.uint8))
    cache._kres_all.copy_(torch.randn(cache._kres_all.shape, generator=g).half())
    ids_before = cache._page_ids_all.clone()
    del log[:]
    cache.swap_in(2, snap)
    assert len(log) == 1 and log[0]["direction"] == SM.UNPACK and log[0]["slot_table"] == [[2, 70, 40, 50]] and log[0]["blob_offsets"] == [0]
    for arr, v in ((cache._T_a, 70), (cache._r_a, 40), (cache._rs_a, 50), (cache._seen_a, 110), (cache._pre_a, 0)):
        assert arr[:, 2].tolist() == [v, v]
    assert cache._T_a[:, 0].tolist() == [33, 33] and cache._lengths_all[:, 0].tolist() == [[33, 0, 0, 0]] * 2
    assert cache._lengths_all[:, 2].tolist() == [[70, 40, 50, 0]] * 2 and not cache._lengths_all[:, 1].any()
    for a, b in zip(want, _live(cache, 2, 70, 40, 50)):
        assert np.array_equal(a, b)
    if preallocate:
        assert torch.equal(cache._page_ids_all, ids_before) and _allocated(cache) == n0
    else:
        assert _allocated(cache) == 2 * 2 * (2 + 3) and cache._pages_a[:, 2].tolist() == [3, 3]
        mine = [p for l in range(2) for h in range(2) for p in cache._host_pids[l][2][h]]
        other = [p for l in range(2) for h in range(2) for p in cache._host_pids[l][0][h]]
        assert len(set(mine)) == 12 and not set(mine) & set(other) and all(cache.page_manager.ref_count(p) == 1 for p in mine)
        for l in range(2):
            for h in range(2):
                assert cache.page_ids[l][2, h, :3].tolist() == cache._host_pids[l][2][h]
    assert cache.sharing_stats() == {"shared_pages": 0, "extra_references": 0}
    cache.release(2)
    cache.release(0)
    assert _allocated(cache) == (n0 if preallocate else 0)


def test_swap_of_several_slots_in_bounded_ranges(monkeypatch):
    log = []
    cache = _cache(monkeypatch, False, log)
    _fill(cache, 2, 5, 3, 0, 8)
    want = [_live(cache, 0, 70, 40, 50), _live(cache, 2, 5, 3, 0)]
    keep = cache.snapshot_request(0)
    assert len(log) == 1 and cache._T_a[:, 0].tolist() == [70, 70] and _allocated(cache) == 2 * 2 * (3 + 1)      # nothing released
    del log[:]
    snaps = cache.swap_out([0, 2], staging_bytes=1)                    # one layer per range
    assert torch.equal(snaps[0].blob, keep.blob) and snaps[0].meta == keep.meta
    rb = [SM.row_bytes(70, 40, 32, 64, 128), SM.row_bytes(5, 3, 32, 64, 128)]
    assert [(c["layer0"], c["n_layers"], c["blob_offsets"], c["blob_bytes"]) for c in log] == [(l, 1, [0, 2 * rb[0]], 2 * sum(rb)) for l in (0, 1)]
    assert [s.blob.numel() for s in snaps] == [4 * rb[0], 4 * rb[1]] and _allocated(cache) == 0
    del log[:]
    cache.swap_in(1, snaps[1], staging_bytes=1)
    cache.swap_in(2, snaps[0], staging_bytes=2 * rb[0])
    assert [(c["layer0"], c["n_layers"]) for c in log] == [(0, 1), (1, 1), (0, 1), (1, 1)]
    for a, b in zip(want[0] + want[1], _live(cache, 2, 70, 40, 50) + _live(cache, 1, 5, 3, 0)):
        assert np.array_equal(a, b)
    assert cache._lengths_all.tolist() == [[[0, 0, 0, 0], [5, 3, 0, 0], [70, 40, 50, 0]]] * 2


def test_swap_out_of_a_sibling_leaves_shared_pages_with_the_other(monkeypatch):
    log = []
    cache = _cache(monkeypatch, False, log)
    cache.fork(0, [1, 2])
    assert _allocated(cache) == 12 + 8 and cache.sharing_stats() == {"shared_pages": 8, "extra_references": 16}
    want = _live(cache, 1, 70, 40, 50)
    pools = (cache.key_page_pool.clone(), cache.value_page_pool.clone())
    snap = cache.swap_out(1)
    assert _allocated(cache) == 20 - 4 and cache.sharing_stats() == {"shared_pages": 8, "extra_references": 8}
    assert torch.equal(cache.key_page_pool, pools[0]) and torch.equal(cache.value_page_pool, pools[1])
    for a, b in zip(want, _live(cache, 0, 70, 40, 50)):                # the siblings hold the same request
        assert np.array_equal(a, b)
    cache.swap_in(1, snap)
    assert _allocated(cache) == 16 + 12 and cache.sharing_stats() == {"shared_pages": 8, "extra_references": 8}
    mine = [p for l in range(2) for h in range(2) for p in cache._host_pids[l][1][h]]
    assert len(set(mine)) == 12 and all(cache.page_manager.ref_count(p) == 1 for p in mine)
    for a, b in zip(want, _live(cache, 1, 70, 40, 50)):
        assert np.array_equal(a, b)
    for a, b in zip(want, _live(cache, 2, 70, 40, 50)):
        assert np.array_equal(a, b)
    for b in range(3):
        cache.release(b)
    assert _allocated(cache) == 0 and cache.sharing_stats() == {"shared_pages": 0, "extra_references": 0}


@pytest.mark.parametrize("preallocate", [False, True], ids=["on-demand", "preallocated"])
def test_refused_swaps_change_nothing(monkeypatch, preallocate):
    log = []
    cache = _cache(monkeypatch, preallocate, log)
    snap = cache.snapshot_request(0)
    _fill(cache, 1, 5, 0, 0, 5)
    del log[:]
    before = _state(cache)
    for b in (3, -1, [0, 0], [], [0, 3]):
        with pytest.raises(RuntimeError):
            cache.swap_out(b)
    cache._T_a[1, 0] += 32                                             # mid-step: layer 1 has flushed, layer 0 not
    with pytest.raises(RuntimeError, match="mid-step"):
        cache.swap_out(0)
    cache._T_a[1, 0] -= 32
    with pytest.raises(RuntimeError, match="holds tokens"):
        cache.swap_in(1, snap)
    with pytest.raises(RuntimeError, match="holds tokens"):
        cache.swap_in(0, snap)
    with pytest.raises(RuntimeError):
        cache.swap_in(3, snap)
    for key, v in (("layer_num", 3), ("nh_k", 1), ("d", 64), ("M", 32), ("nbits", 4), ("page_size", 64), ("resid_cap", 128), ("version", 2)):
        with pytest.raises(RuntimeError, match=key):
            cache.swap_in(2, RequestSnapshot(snap.blob, dict(snap.meta, **{key: v})))
    with pytest.raises(RuntimeError, match="max_tokens"):
        cache.swap_in(2, RequestSnapshot(snap.blob, dict(snap.meta, T=257)))
    with pytest.raises(RuntimeError, match="bytes expected"):
        cache.swap_in(2, RequestSnapshot(snap.blob[:-16], snap.meta))
    with pytest.raises(RuntimeError, match="codebooks"):
        cache.swap_in(2, RequestSnapshot(snap.blob, dict(snap.meta, key_cent_sha256="0" * 64)))
    cache.value_cent = cache.value_cent + 1                            # the cache's codebook changed since the snapshot
    with pytest.raises(RuntimeError, match="codebooks"):
        cache.swap_in(2, snap)
    cache.value_cent = cache.value_cent - 1
    if not preallocate:                                                # fewer free pages than L * H * n_live = 12
        pm = cache.page_manager
        held = [pm.allocate_page() for _ in range(len(pm.free_pages) - 11)]
        with pytest.raises(RuntimeError, match="free pages"):
            cache.swap_in(2, snap)
        for pid in held:
            pm.free_page(pid)
        before[8]["total_allocations"] += len(held)
        before[8]["page_reuse_count"] = pm.page_reuse_count
    assert not log and _same(before, _state(cache))
    cache.swap_in(2, RequestSnapshot(snap.blob, dict(snap.meta, key_cent_sha256="0" * 64)), check_codebooks=False)
    assert len(log) == 1 and cache._lengths_all[:, 2].tolist() == [[70, 40, 50, 0]] * 2


def test_codebook_digests_are_computed_once_per_codebook(monkeypatch):
    cache = _cache(monkeypatch, True, [])
    first = cache._cent_digests()
    calls = []
    import hashlib
    real = hashlib.sha256
    monkeypatch.setattr(hashlib, "sha256", lambda b: calls.append(1) or real(b))
    assert cache._cent_digests() == first and not calls
    cache.key_cent = cache.value_cent = cache.key_cent.clone()
    again = cache._cent_digests()
    assert len(calls) == 1 and again[0] == again[1] == first[0]


def test_swap_in_into_another_cache_object(monkeypatch):
    a = _cache(monkeypatch, False, [])
    want = _live(a, 0, 70, 40, 50)
    snap = a.swap_out(0)
    for preallocate in (False, True):
        b = _cache(monkeypatch, preallocate, [], seed=5, fill=False)
        b.swap_in(1, snap)
        for x, y in zip(want, _live(b, 1, 70, 40, 50)):
            assert np.array_equal(x, y)
        assert b._T_a.tolist() == [[0, 70, 0]] * 2
    c = _cache(monkeypatch, True, [], fill=False, max_tokens=64)
    with pytest.raises(RuntimeError, match="max_tokens"):
        c.swap_in(0, snap)


# ---------------------------------------------------------------- the file --------------------------------------------------
def test_save_and_load_request_round_trip(tmp_path, monkeypatch):
    from million_amd import formats
    cache = _cache(monkeypatch, False, [])
    snap = cache.snapshot_request(0)
    path = formats.save_request(tmp_path / "req.pt", snap)
    back = formats.load_request(path)
    assert isinstance(back, RequestSnapshot) and torch.equal(back.blob, snap.blob) and back.meta == snap.meta
    assert all(type(v) in (int, str) for v in back.meta.values())
    cache.release(0)
    cache.swap_in(1, back)
    assert cache._lengths_all[:, 1].tolist() == [[70, 40, 50, 0]] * 2


class _NotATensor:
    def __init__(self):
        self.x = 1


def test_load_request_refuses_pickled_objects(tmp_path):
    from million_amd import formats
    p = tmp_path / "bad.pt"
    torch.save({"blob": torch.zeros(16, dtype=torch.uint8), "meta": {"T": 1, "who": _NotATensor()}}, p)
    with pytest.raises(pickle.UnpicklingError):
        formats.load_request(p)
    torch.save(_NotATensor(), p)
    with pytest.raises(pickle.UnpicklingError):
        formats.load_request(p)
    for obj in (torch.zeros(16, dtype=torch.uint8), {"blob": torch.zeros(4, 4, dtype=torch.uint8), "meta": {}},
                {"blob": torch.zeros(16), "meta": {}}, {"blob": torch.zeros(16, dtype=torch.uint8), "meta": {"T": 1.5}},
                {"blob": torch.zeros(16, dtype=torch.uint8)}):
        torch.save(obj, p)
        with pytest.raises(ValueError):
            formats.load_request(p)
