"""CPU tests of the request fork (million_cache_fork, ops.cache_fork, PagedPQCache.fork, PageManager reference counts):
the allocator's counts, the descriptor layout and the validation before any launch, the numpy model the GPU tests compare
against (tests/cache_fork_model.py), and the host bookkeeping of fork with the device call replaced by that model."""
import ctypes
import subprocess
import sys
import tempfile
from pathlib import Path

import numpy as np
import pytest
import torch

from million_amd.pq_cache import PagedPQCache, PageManager
from tests import cache_fork_model as FM

ROOT = Path(__file__).resolve().parents[1]
ARG, SHAPE, ALIGN = -3, -1, -2


# ---------------------------------------------------------------- PageManager ----------------------------------------------
def test_shared_page_survives_its_first_owner():
    pm = PageManager(page_size=64, initial_pages=4, max_pages=4)
    a, b = pm.allocate_page(), pm.allocate_page()
    assert (pm.ref_count(a), pm.ref_count(b), pm.ref_count(3)) == (1, 1, 0)
    assert pm.share_page(a) == 2 and pm.ref_count(a) == 2
    assert pm.sharing_stats() == {"shared_pages": 1, "extra_references": 1}
    assert pm.share_page(a) == 3 and pm.sharing_stats() == {"shared_pages": 1, "extra_references": 2}
    pm.free_page(a)
    pm.free_page(a)
    assert pm.ref_count(a) == 1 and a in pm.allocated_pages and a not in pm.free_pages
    assert pm.sharing_stats() == {"shared_pages": 0, "extra_references": 0}
    assert pm.get_stats()["allocated_pages"] == 2 and pm.get_stats()["free_pages"] == 2
    assert pm.allocate_page() == 2                     # a is still owned: the lowest FREE id is 2
    pm.free_page(a)                                    # the last owner
    assert pm.ref_count(a) == 0 and a in pm.free_pages
    assert pm.allocate_page() == a and pm.page_reuse_count == 1      # reusable now
    pm.free_page(a)
    pm.free_page(a)                                    # a free id: ignored, as ever
    assert pm.get_stats()["free_pages"] == 2


def test_share_page_of_a_free_id_raises():
    pm = PageManager(initial_pages=4, max_pages=4)
    with pytest.raises(RuntimeError, match="not allocated"):
        pm.share_page(0)
    pid = pm.allocate_page()
    pm.free_page(pid)
    with pytest.raises(RuntimeError, match="not allocated"):
        pm.share_page(pid)
    with pytest.raises(RuntimeError, match="not allocated"):
        pm.share_page(12345)
    assert pm.sharing_stats() == {"shared_pages": 0, "extra_references": 0}
    a, b = pm.allocate_page(), pm.allocate_page()
    with pytest.raises(RuntimeError, match="not allocated"):
        pm.share_pages([a, b, 3])                      # all or nothing
    assert pm.sharing_stats() == {"shared_pages": 0, "extra_references": 0}
    pm.share_pages([a, b, a])
    assert (pm.ref_count(a), pm.ref_count(b)) == (3, 2) and pm.sharing_stats() == {"shared_pages": 2, "extra_references": 3}


def test_unshared_sequence_is_what_it_was():
    """The sequence of test_host_logic.test_page_manager_semantics, with the values that test pins and the whole stats
    dictionary: reference counts change nothing for pages never shared."""
    pm = PageManager(page_size=64, initial_pages=4, max_pages=10, M=64)
    ids = [pm.allocate_page() for _ in range(4)]
    assert ids == [0, 1, 2, 3] and pm.get_stats()["free_pages"] == 0
    pm.free_page(2)
    assert pm.allocate_page() == 2 and pm.page_reuse_count == 1
    more = pm.allocate_pages(5)
    assert more == [4, 5, 6, 7, 8] and pm.current_active_pages == 9
    assert pm.allocate_page() == 9
    with pytest.raises(RuntimeError):
        pm.allocate_page()
    pm.free_page(12345)
    assert pm.get_stats() == {"initial_pages": 4, "current_active_pages": 10, "max_pages": 10, "allocated_pages": 10,
                              "free_pages": 0, "utilization": 1.0, "page_reuse_count": 1, "total_allocations": 11,
                              "total_expansions": 2}
    assert all(pm.ref_count(i) == 1 for i in range(10)) and pm.sharing_stats() == {"shared_pages": 0, "extra_references": 0}
    assert all(v == {"allocation_count": 1} for v in pm.allocated_pages.values())


# ---------------------------------------------------------------- C ABI ----------------------------------------------------
@pytest.fixture(scope="module")
def lib():
    from million_amd import build, _lib
    build.build()
    return _lib.load()


def test_symbol_and_desc_match_the_header(lib):
    from million_amd import _lib
    assert "million_cache_fork" in _lib.SYMBOLS and lib.million_cache_fork.restype is _lib.c_i32
    names = [f[0] for f in _lib.ForkDesc._fields_]
    offs = ", ".join(f"offsetof(million_fork_desc, {n})" for n in names)
    src = ('#include "million_hip.h"\n#include <stdio.h>\n#include <stddef.h>\n'
           f'int main(){{size_t v[] = {{sizeof(million_fork_desc), {offs}, MILLION_FORK_SHARE, MILLION_FORK_COPY}};\n'
           'for (unsigned i = 0; i < sizeof(v) / sizeof(v[0]); ++i) printf("%zu ", v[i]);return 0;}\n')
    with tempfile.TemporaryDirectory() as td:
        (Path(td) / "a.c").write_text(src)
        subprocess.check_call(["gcc", "-std=c11", "-I", str(ROOT / "include"), "-o", f"{td}/a", f"{td}/a.c"])
        vals = list(map(int, subprocess.check_output([f"{td}/a"]).split()))
    assert vals[0] == ctypes.sizeof(_lib.ForkDesc)
    assert vals[1:-2] == [getattr(_lib.ForkDesc, n).offset for n in names]
    assert vals[-2:] == [_lib.MILLION_FORK_SHARE, _lib.MILLION_FORK_COPY] == [FM.SHARE, FM.COPY]


def _desc(**kw):
    from million_amd import _lib
    d = _lib.ForkDesc()
    d.struct_size = ctypes.sizeof(_lib.ForkDesc)
    d.n_layers, d.bs, d.nh_k, d.d, d.M, d.page_size, d.n_pages_cap, d.n_pool, d.resid_cap = 3, 4, 2, 128, 64, 64, 8, 192, 128
    d.ids_layer_stride, d.rows_layer_stride, d.lengths_layer_stride = 4 * 2 * 8, 4 * 2 * 128 * 128, 16
    d.src, d.n_dst, d.mode, d.n_pages_bound, d.prefix_tokens = 0, 2, FM.SHARE, 8, -1
    for k, v in kw.items():
        setattr(d, k, v)
    return d


# fake aligned "device pointers": validation never dereferences them
PTRS = dict(page_ids=0x1000, k_pool=0x2000, v_pool=0x3000, k_resid=0x4000, v_resid=0x5000, dev_lengths=0x6000,
            dst_slots=0x7000, tail_ids=0x8000)


def _call(lib, d, **over):
    p = dict(PTRS, **over)
    return lib.million_cache_fork(ctypes.byref(d), *[p[k] for k in PTRS], None)


def test_validation_before_any_launch(lib):
    err = lib.million_last_error
    assert _call(lib, _desc(struct_size=12)) == ARG and b"struct_size" in err()
    for name in ("page_ids", "k_pool", "v_pool", "dev_lengths", "dst_slots"):
        assert _call(lib, _desc(), **{name: None}) == ARG and b"null" in err(), name
    assert _call(lib, _desc(), k_resid=None) == ARG and b"window" in err()
    assert _call(lib, _desc(), v_resid=None) == ARG and b"window" in err()
    assert _call(lib, _desc(), tail_ids=None) == ARG and b"tail_ids" in err()          # SHARE needs them
    assert _call(lib, _desc(src=4)) == ARG and b"src=4" in err()
    assert _call(lib, _desc(src=-1)) == ARG
    assert _call(lib, _desc(mode=2)) == ARG and b"mode=2" in err()
    assert _call(lib, _desc(n_pages_bound=9)) == ARG and _call(lib, _desc(n_dst=-1)) == ARG
    assert _call(lib, _desc(page_size=48)) == SHAPE and b"page_size=48" in err()
    assert _call(lib, _desc(M=8)) == SHAPE and b"M=8" in err()
    assert _call(lib, _desc(M=128)) == SHAPE
    assert _call(lib, _desc(d=60)) == SHAPE and _call(lib, _desc(bs=0)) == SHAPE and _call(lib, _desc(n_pool=0)) == SHAPE
    for name in ("k_pool", "v_pool", "k_resid", "v_resid"):
        assert _call(lib, _desc(), **{name: PTRS[name] + 8}) == ALIGN and b"16-byte" in err(), name
    assert _call(lib, _desc(rows_layer_stride=4 * 2 * 128 * 128 + 4)) == ALIGN
    assert _call(lib, _desc(), page_ids=PTRS["page_ids"] + 2) == ALIGN
    # shape errors come before pointer errors, pointer errors before alignment
    assert _call(lib, _desc(M=8), k_pool=None) == SHAPE and _call(lib, _desc(), k_pool=None, v_pool=PTRS["v_pool"] + 8) == ARG


def test_no_destination_returns_ok(lib):
    assert _call(lib, _desc(n_dst=0)) == 0
    assert lib.million_cache_fork(ctypes.byref(_desc(n_dst=0)), *[None] * 8, None) == 0
    assert lib.million_cache_fork(ctypes.byref(_desc(n_dst=0, mode=FM.COPY)), *[None] * 8, None) == 0


def test_fork_kernel_fits_four_waves_per_simd_without_scratch(lib):
    out = subprocess.run([sys.executable, str(ROOT / "tools" / "kernel_meta.py"), str(ROOT / "million_amd" / "libmillion_hip.so"), "cache_fork"],
                         capture_output=True, text=True, check=True).stdout
    rows = [l for l in out.splitlines() if "cache_fork_kernel" in l]
    assert len(rows) == 1, out
    assert "vgpr_spill 0" in rows[0] and rows[0].rstrip().endswith("scratch 0 B"), rows[0]
    assert int(rows[0].split("vgpr")[1].split()[0]) <= 128, rows[0]


# ---------------------------------------------------------------- the numpy model ------------------------------------------
def _tables(rs, *, layers=3, bs=4, nhk=2, cap_pages=5, ps=32, M=16, rcap=8, d=8, lengths=(70, 5, 3)):
    """Random tables with distinct ids per (layer, slot, head, page), pools with a per-page pattern, distinct window rows."""
    n_pool = layers * bs * nhk * cap_pages + 7
    ids = rs.permutation(n_pool)[:layers * bs * nhk * cap_pages].reshape(layers, bs, nhk, cap_pages).astype(np.int32)
    kp = (np.arange(n_pool)[:, None, None] * 3 + np.arange(ps)[None, :, None] + np.arange(M)[None, None, :]).astype(np.uint8)
    vp = (np.arange(n_pool)[:, None, None] * 5 + np.arange(M)[None, :, None] + 2 * np.arange(ps)[None, None, :]).astype(np.uint8)
    kr = rs.randint(-30000, 30000, (layers, bs, nhk, rcap, d)).astype(np.int16)
    vr = rs.randint(-30000, 30000, (layers, bs, nhk, rcap, d)).astype(np.int16)
    ln = rs.randint(0, 50, (layers, bs, 4)).astype(np.int32)
    ln[:, 0] = list(lengths) + [0x7EADBEEF]
    return [ids, kp, vp, kr, vr, ln]


def _run(arrs, dst, tail, **kw):
    new = [a.copy() for a in arrs]
    copied = FM.fork(*new, np.asarray(dst, np.int32), tail, **kw)
    return new, copied


def test_model_copy_mode():
    rs = np.random.RandomState(0)
    old = _tables(rs)
    new, copied = _run(old, [2, 3], None, src=0, mode=FM.COPY, n_pages_bound=5)
    ids, kp, vp, kr, vr, ln = new
    assert np.array_equal(ids, old[0])                                 # COPY never writes the table
    assert len(copied) == 3 * 2 * 2 * 3                                # 70 tokens on pages of 32: 3 live pages
    for l, b, h, j in [(0, 2, 0, 0), (2, 3, 1, 2)]:
        assert np.array_equal(kp[ids[l, b, h, j]], old[1][ids[l, 0, h, j]]) and np.array_equal(vp[ids[l, b, h, j]], old[2][ids[l, 0, h, j]])
    touched = {e for *_, e in copied}
    assert touched == set(ids[:, 2:, :, :3].flatten().tolist())
    rest = np.setdiff1d(np.arange(kp.shape[0]), list(touched))
    assert np.array_equal(kp[rest], old[1][rest]) and np.array_equal(vp[rest], old[2][rest])
    assert np.array_equal(kr[:, 2], old[3][:, 0]) and np.array_equal(vr[:, 3], old[4][:, 0])      # all rows, ring positions kept
    assert np.array_equal(kr[:, :2], old[3][:, :2]) and np.array_equal(vr[:, :2], old[4][:, :2])
    assert ln[:, 2].tolist() == [[70, 5, 3, 0]] * 3 and ln[:, 3].tolist() == [[70, 5, 3, 0]] * 3
    assert np.array_equal(ln[:, :2], old[5][:, :2])                    # the source row (word 3 too) and slot 1


def test_model_share_mode_and_prefix():
    rs = np.random.RandomState(1)
    old = _tables(rs)
    n_pool = old[1].shape[0]
    tail = np.arange(n_pool - 7, n_pool - 7 + 6, dtype=np.int32).reshape(1, 3, 2)      # ids no table names
    new, copied = _run(old, [1], tail, src=0, mode=FM.SHARE, n_pages_bound=5)
    ids = new[0]
    assert np.array_equal(ids[:, 1, :, :2], old[0][:, 0, :, :2]) and np.array_equal(ids[:, 1, :, 2], tail[0])
    assert np.array_equal(ids[:, 1, :, 3:], old[0][:, 1, :, 3:])       # entries at or past n_live: not written
    assert sorted(e for *_, e in copied) == sorted(tail.flatten().tolist())            # the tail page alone is copied
    assert np.array_equal(new[1][tail[0, 1, 0]], old[1][old[0][1, 0, 0, 2]])
    assert new[5][:, 1].tolist() == [[70, 5, 3, 0]] * 3
    # a prefix on a page boundary: no tail page, no copy, no window; 40: the second page becomes the private tail
    for p, n_full, n_copied in ((64, 2, 0), (40, 1, 6), (0, 0, 0), (1000, 2, 6)):
        new, copied = _run(old, [1], tail, src=0, mode=FM.SHARE, n_pages_bound=5, prefix_tokens=p)
        T = min(70, p)
        assert new[5][:, 1].tolist() == [[T, 0, 0, 0]] * 3 and len(copied) == n_copied
        assert np.array_equal(new[0][:, 1, :, :n_full], old[0][:, 0, :, :n_full])
        assert np.array_equal(new[3], old[3]) and np.array_equal(new[4], old[4])


def test_model_on_untrusted_values():
    rs = np.random.RandomState(2)
    # T above the bound, r above the window, a start out of range
    old = _tables(rs, lengths=(100000, 99, 8))
    new, copied = _run(old, [1], None, src=0, mode=FM.COPY, n_pages_bound=4)
    assert new[5][:, 1].tolist() == [[4 * 32, 8, 0, 0]] * 3 and len(copied) == 3 * 2 * 4
    assert np.array_equal(new[1][old[0][:, 1, :, 4]], old[1][old[0][:, 1, :, 4]])       # the page past the bound is not touched
    old = _tables(rs, lengths=(-5, -1, -1))
    new, copied = _run(old, [1], None, src=0, mode=FM.COPY, n_pages_bound=4)
    assert new[5][:, 1].tolist() == [[0, 0, 0, 0]] * 3 and not copied
    # ids outside the pool, on either side: that page's copy is dropped, the others go through
    old = _tables(rs)
    n_pool = old[1].shape[0]
    old[0][0, 0, 0, 1] = n_pool          # a source id
    old[0][1, 2, 1, 0] = -1              # a destination id
    old[0][2, 2, 0, 2] = 1 << 30
    new, copied = _run(old, [2], None, src=0, mode=FM.COPY, n_pages_bound=5)
    assert len(copied) == 3 * 2 * 3 - 3 and np.array_equal(new[0], old[0])
    assert not {(0, 2, 0, 1), (1, 2, 1, 0), (2, 2, 0, 2)} & {c[:4] for c in copied}
    # dst = src, slots outside [0, bs) and a repeated slot take no part
    old = _tables(rs)
    new, copied = _run(old, [0, -1, 4, 3, 3], None, src=0, mode=FM.COPY, n_pages_bound=5)
    assert {c[1] for c in copied} == {3} and len(copied) == 3 * 2 * 3
    assert all(np.array_equal(a[:, :3], b[:, :3]) for a, b in zip((new[0], new[3], new[4], new[5]), (old[0], old[3], old[4], old[5])))
    assert FM.takes_part([0, -1, 4, 3, 3], 4, 0) == {3: 3}
    # a destination whose entry equals the source's: nothing to copy for that page
    old = _tables(rs)
    old[0][0, 1, 0, 0] = old[0][0, 0, 0, 0]
    new, copied = _run(old, [1], None, src=0, mode=FM.COPY, n_pages_bound=5)
    assert (0, 1, 0, 0) not in {c[:4] for c in copied} and len(copied) == 3 * 2 * 3 - 1


# ---------------------------------------------------------------- host bookkeeping of fork ---------------------------------
def _cache(monkeypatch, preallocate, log):
    """A CPU cache (2 layers, 3 slots, pages of 32, window 64) whose slot 0 holds 70 coded tokens and a wrapped window of 40
    rows; ops.cache_fork is the numpy model."""
    from million_amd import ops
    monkeypatch.setattr(ops, "pq_encode_into", lambda *a, **k: None)
    monkeypatch.setattr(ops, "prefill_attn", lambda q, k, v, **kw: torch.zeros_like(q))
    monkeypatch.setattr(ops, "cache_fork", FM.as_ops_stub(log))
    cache = PagedPQCache(bs=3, nh=8, num_key_value_heads=2, M=64, layer_num=2, d=128, page_size=32, extended_residual_size=64,
                         max_tokens=256, preallocate=preallocate, device="cpu")
    cache.key_cent = cache.value_cent = torch.zeros(64, 256, 2, dtype=torch.float16)
    cache._kprep = cache._vprep = torch.zeros(1, dtype=torch.float16)
    x = torch.zeros(1, 2, 70, 128, dtype=torch.float16)
    for l in range(2):
        cache.prefill_request(0, torch.zeros(1, 8, 70, 128, dtype=torch.float16), x, x, l)
    cache._r_a[:, 0], cache._rs_a[:, 0], cache._seen_a[:, 0] = 40, 50, 110
    for l in range(2):
        cache._sync_lengths(l, 0)
    g = torch.Generator().manual_seed(0)
    cache.key_page_pool.copy_(torch.randint(0, 256, cache.key_page_pool.shape, generator=g, dtype=torch.uint8))
    cache.value_page_pool.copy_(torch.randint(0, 256, cache.value_page_pool.shape, generator=g, dtype=torch.uint8))
    cache._kres_all.copy_(torch.randn(cache._kres_all.shape, generator=g).half())
    cache._vres_all.copy_(torch.randn(cache._vres_all.shape, generator=g).half())
    return cache


def _allocated(cache):
    return cache.page_manager.get_stats()["allocated_pages"]


def test_fork_shares_pages_on_demand(monkeypatch):
    log = []
    cache = _cache(monkeypatch, False, log)
    src_pids = [[list(cache._host_pids[l][0][h]) for h in range(2)] for l in range(2)]
    assert _allocated(cache) == 2 * 2 * 3                              # 70 tokens: 3 pages per (layer, kv head)
    cache._pre_a[:, 0] = 1
    cache.fork(0, [1, 2])
    assert len(log) == 1 and log[0]["share"] and log[0]["dst_slots"] == [1, 2] and log[0]["n_pages_bound"] == 3
    assert log[0]["prefix_tokens"] == -1
    tails = np.asarray(log[0]["tail_ids"])
    assert tails.shape == (2, 2, 2) and len(set(tails.flatten().tolist())) == 8
    # 12 source pages, 8 private tail pages; the 8 full source pages have three owners each
    assert _allocated(cache) == 12 + 8
    assert cache.sharing_stats() == {"shared_pages": 8, "extra_references": 16}
    for l in range(2):
        for h in range(2):
            for j, b in enumerate((1, 2)):
                assert cache._host_pids[l][b][h] == src_pids[l][h][:2] + [tails[j, l, h]]
                assert cache.page_ids[l][b, h, :3].tolist() == cache._host_pids[l][b][h]
                assert torch.equal(cache.key_page_pool[tails[j, l, h]], cache.key_page_pool[src_pids[l][h][2]])
                assert torch.equal(cache.value_page_pool[tails[j, l, h]], cache.value_page_pool[src_pids[l][h][2]])
            assert cache.page_manager.ref_count(src_pids[l][h][0]) == 3 and cache.page_manager.ref_count(src_pids[l][h][2]) == 1
    assert cache._pages_a.tolist() == [[3, 3, 3]] * 2
    for arr, v in ((cache._T_a, 70), (cache._r_a, 40), (cache._rs_a, 50), (cache._seen_a, 110)):
        assert arr.tolist() == [[v] * 3] * 2
    assert cache._pre_a.tolist() == [[0, 0, 0]] * 2                    # the source's encode-ahead is joined, as extend does
    assert cache._lengths_all.tolist() == [[[70, 40, 50, 0]] * 3] * 2
    assert torch.equal(cache._kres_all[:, 1], cache._kres_all[:, 0]) and torch.equal(cache._vres_all[:, 2], cache._vres_all[:, 0])
    # the source leaves first: its full pages stay with the forks, only its tail pages come back
    cache.release(0)
    assert _allocated(cache) == 20 - 4 and cache.sharing_stats() == {"shared_pages": 8, "extra_references": 8}
    assert all(cache.page_manager.ref_count(src_pids[l][h][0]) == 2 for l in range(2) for h in range(2))
    cache.release(1)
    assert _allocated(cache) == 16 - 4 and cache.sharing_stats() == {"shared_pages": 0, "extra_references": 0}
    cache.release(2)
    assert _allocated(cache) == 0 and cache.page_manager.get_stats()["free_pages"] == cache.page_manager.current_active_pages
    assert cache._pages_a.sum() == 0 and not cache._T_a.any()


def test_fork_after_steps_with_host_lengths_reads_fresh_device_rows(monkeypatch):
    """Decode steps with use_dev_lengths=False move the host mirror and leave the device rows where they were; the fork kernel
    reads the source's T, r and start from its device row.  fork must write the rows from the mirror first: the forks get the
    source's lengths of now - and every live page of it - not those of its last step with device lengths."""
    from million_amd import ops
    log = []
    cache = _cache(monkeypatch, False, log)
    monkeypatch.setattr(ops, "decode_workspace_bytes", lambda *a, **k: 16)
    monkeypatch.setattr(ops, "pq_flush", lambda *a, **k: None)
    seen = []
    monkeypatch.setattr(ops, "pq_decode_attn", lambda q, *a, dev_lengths=None, **k: (seen.append(dev_lengths), torch.zeros_like(q))[1])
    for b in (1, 2):      # lockstep: every slot at slot 0's lengths
        for arr in (cache._T_a, cache._r_a, cache._rs_a, cache._seen_a):
            arr[:, b] = arr[:, 0]
    q, x = torch.zeros(3, 8, 1, 128, dtype=torch.float16), torch.zeros(3, 2, 1, 128, dtype=torch.float16)
    for _ in range(30):      # r: 40 -> 64 (24 steps), a flush of 32 rows (T: 70 -> 102, a fourth page), 6 more steps
        for l in range(2):
            cache.decoding_with_pages(q, x, x, l)
    assert seen and all(d is None for d in seen)
    assert cache._T_a[:, 0].tolist() == [102, 102] and cache._r_a[:, 0].tolist() == [38, 38] and cache._rs_a[:, 0].tolist() == [18, 18]
    assert cache._lengths_all[:, 0].tolist() == [[70, 40, 50, 0]] * 2      # the device rows did not move
    for b in (1, 2):
        cache._T_a[:, b] = cache._r_a[:, b] = cache._rs_a[:, b] = cache._seen_a[:, b] = 0
    cache.fork(0, [1, 2])
    assert log[-1]["n_pages_bound"] == 4
    assert cache._lengths_all.tolist() == [[[102, 38, 18, 0]] * 3] * 2
    for l in range(2):
        for h in range(2):
            for b in (1, 2):
                assert cache.page_ids[l][b, h, :4].tolist() == cache._host_pids[l][b][h] and len(cache._host_pids[l][b][h]) == 4
                assert cache._host_pids[l][b][h][:3] == cache._host_pids[l][0][h][:3]
                assert torch.equal(cache.key_page_pool[cache._host_pids[l][b][h][3]], cache.key_page_pool[cache._host_pids[l][0][h][3]])


def test_fork_on_a_page_boundary_and_of_a_prefix(monkeypatch):
    log = []
    cache = _cache(monkeypatch, False, log)
    cache.fork(0, 1, n_tokens=64)                                      # two full pages: nothing to allocate, nothing copied
    assert _allocated(cache) == 12 and cache.sharing_stats() == {"shared_pages": 8, "extra_references": 8}
    assert log[0]["prefix_tokens"] == 64 and log[0]["n_pages_bound"] == 2 and (np.asarray(log[0]["tail_ids"]) == -1).all()
    assert cache._lengths_all[:, 1].tolist() == [[64, 0, 0, 0]] * 2 and cache._pages_a[:, 1].tolist() == [2, 2]
    assert [a[:, 1].tolist() for a in (cache._T_a, cache._r_a, cache._rs_a, cache._seen_a)] == [[64, 64], [0, 0], [0, 0], [64, 64]]
    assert not torch.equal(cache._kres_all[:, 1], cache._kres_all[:, 0])      # no window with a prefix
    cache.fork(0, 2, n_tokens=40)                                      # one full page shared, the second copied as a tail
    assert _allocated(cache) == 12 + 4 and cache.sharing_stats() == {"shared_pages": 8, "extra_references": 12}
    assert [a[:, 2].tolist() for a in (cache._T_a, cache._r_a, cache._rs_a, cache._seen_a)] == [[40, 40], [0, 0], [0, 0], [40, 40]]
    for b in (2, 1, 0):
        cache.release(b)
    assert _allocated(cache) == 0 and cache.sharing_stats() == {"shared_pages": 0, "extra_references": 0}


def test_fork_copies_into_a_preallocated_table(monkeypatch):
    log = []
    cache = _cache(monkeypatch, True, log)
    ids = cache._page_ids_all.clone()
    n_alloc = _allocated(cache)
    cache.fork(0, 2)
    assert len(log) == 1 and not log[0]["share"] and log[0]["tail_ids"] is None and log[0]["n_pages_bound"] == 3
    assert torch.equal(cache._page_ids_all, ids) and _allocated(cache) == n_alloc
    assert cache.sharing_stats() == {"shared_pages": 0, "extra_references": 0}
    for l in range(2):
        for h in range(2):
            for j in range(3):
                assert torch.equal(cache.key_page_pool[ids[l, 2, h, j]], cache.key_page_pool[ids[l, 0, h, j]])
                assert torch.equal(cache.value_page_pool[ids[l, 2, h, j]], cache.value_page_pool[ids[l, 0, h, j]])
            assert not torch.equal(cache.key_page_pool[ids[l, 2, h, 3]], cache.key_page_pool[ids[l, 0, h, 3]])
    assert cache._lengths_all.tolist() == [[[70, 40, 50, 0], [0, 0, 0, 0], [70, 40, 50, 0]]] * 2
    assert cache._T_a.tolist() == [[70, 0, 70]] * 2 and cache._seen_a.tolist() == [[110, 0, 110]] * 2
    cache.release(0)
    assert _allocated(cache) == n_alloc and cache._T_a.tolist() == [[0, 0, 70]] * 2


@pytest.mark.parametrize("preallocate", [True, False], ids=["preallocated", "on-demand"])
def test_fork_refuses_before_anything_moves(monkeypatch, preallocate):
    log = []
    cache = _cache(monkeypatch, preallocate, log)
    x = torch.zeros(1, 2, 5, 128, dtype=torch.float16)
    for l in range(2):
        cache.prefill_request(1, torch.zeros(1, 8, 5, 128, dtype=torch.float16), x, x, l)
    snap = lambda: ([a.copy() for a in cache.host_state()], cache._pages_a.copy(), cache._page_ids_all.clone(), cache._lengths_all.clone(),
                    cache.key_page_pool.clone(), cache.page_manager.get_stats(), cache.sharing_stats(),
                    [[[list(x) for x in b] for b in l] for l in cache._host_pids])
    before = snap()
    for args, kw in (((0, 1), {}), ((0, 0), {}), ((0, [2, 0]), {}), ((0, [2, 2]), {}), ((0, 3), {}), ((3, 2), {}), ((0, []), {}),
                     ((0, 2), dict(n_tokens=71)), ((0, 2), dict(n_tokens=-1))):
        with pytest.raises(RuntimeError):
            cache.fork(*args, **kw)
    cache._T_a[1, 0] += 32                                             # the source mid-step: layer 1 has flushed, layer 0 not
    with pytest.raises(RuntimeError, match="mid-step"):
        cache.fork(0, 2)
    cache._T_a[1, 0] -= 32
    if not preallocate:                                                # no free page for the private tail pages
        pm = cache.page_manager
        held = [pm.allocate_page() for _ in range(len(pm.free_pages) - 3)]
        with pytest.raises(RuntimeError, match="free pages"):
            cache.fork(0, 2)
        for pid in held:
            pm.free_page(pid)
        before[5]["total_allocations"] += len(held)
        before[5]["page_reuse_count"] = pm.page_reuse_count
    after = snap()
    assert not log
    assert all(np.array_equal(a, b) for a, b in zip(before[0], after[0])) and np.array_equal(before[1], after[1])
    assert all(torch.equal(a, b) for a, b in zip(before[2:5], after[2:5])) and before[5:] == after[5:]
