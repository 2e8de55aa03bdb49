"""CPU tests of the one-launch ragged store (million_pq_store_ragged, ops.pq_store_ragged, PagedPQCache.extend_ragged /
prefill_ragged with device_store=True): descriptor layout, validation before any launch, the host bookkeeping with `ops`
monkeypatched, the numpy model the GPU tests compare against (tests/store_ragged_model.py), and the kernels' register /
scratch figures."""
import ctypes
import subprocess
import sys
import tempfile
from pathlib import Path

import numpy as np
import pytest
import torch

from tests import store_ragged_model as SM
from tests.test_chunk_attn_host import _cpu_paged_cache
from tests.test_chunk_ragged_host import _ragged_cache

ROOT = Path(__file__).resolve().parents[1]
ARG, SHAPE, ALIGN = -3, -1, -2


@pytest.fixture(scope="module")
def lib():
    from million_amd import build, _lib
    build.build()
    return _lib.load()


def test_desc_matches_header(lib):
    from million_amd import _lib
    names = [f[0] for f in _lib.StoreRaggedDesc._fields_]
    offs = ", ".join(f"offsetof(million_store_ragged_desc, {n})" for n in names)
    src = ('#include "million_hip.h"\n#include <stdio.h>\n#include <stddef.h>\n'
           f'int main(){{size_t v[] = {{sizeof(million_store_ragged_desc), {offs}}};\n'
           'for (unsigned i = 0; i < sizeof(v) / sizeof(v[0]); ++i) printf("%zu ", v[i]);return 0;}\n')
    with tempfile.TemporaryDirectory() as td:
        (Path(td) / "a.c").write_text(src)
        subprocess.check_call(["gcc", "-std=c11", "-I", str(ROOT / "include"), "-o", f"{td}/a", f"{td}/a.c"])
        vals = list(map(int, subprocess.check_output([f"{td}/a"]).split()))
    assert vals[0] == ctypes.sizeof(_lib.StoreRaggedDesc)
    assert vals[1:] == [getattr(_lib.StoreRaggedDesc, n).offset for n in names]
    assert names[0] == "struct_size" and vals[1] == 0


def _desc(**kw):
    from million_amd import _lib
    d = _lib.StoreRaggedDesc()
    d.struct_size = ctypes.sizeof(_lib.StoreRaggedDesc)
    d.bs, d.nh_k, d.d, d.M, d.C, d.n_bound = 4, 2, 128, 64, 256, 70
    d.kn_stride_b, d.kn_stride_h, d.kn_stride_n = 2 * 70 * 128, 70 * 128, 128
    d.vn_stride_b, d.vn_stride_h, d.vn_stride_n = 2 * 70 * 128, 70 * 128, 128
    d.resid_cap, d.resid_stride_b, d.resid_stride_h = 64, 2 * 64 * 128, 64 * 128
    d.page_size, d.n_pages_cap = 32, 8
    for k, v in kw.items():
        setattr(d, k, v)
    return d


# fake aligned "device pointers": validation never dereferences them
PTRS = dict(k_new=0x1000, v_new=0x2000, k_resid=0x3000, v_resid=0x4000, k_prep=0x5000, v_prep=0x6000, k_pool=0x7000,
            v_pool=0x8000, page_ids=0x9000, dev_lengths=0xA000, dev_n=0xB000)


def _call(lib, d, **over):
    p = dict(PTRS, **over)
    return lib.million_pq_store_ragged(ctypes.byref(d), *[p[k] for k in PTRS], None)


def test_validation_without_gpu(lib):
    err = lib.million_last_error
    assert _call(lib, _desc(struct_size=12)) == ARG and b"struct_size" in err()
    assert _call(lib, _desc(), dev_n=None) == ARG and b"dev_n" in err()
    assert _call(lib, _desc(), dev_lengths=None) == ARG and b"dev_lengths" in err()
    assert _call(lib, _desc(), k_resid=None) == ARG and b"window" in err()
    assert _call(lib, _desc(), v_resid=None) == ARG and b"window" in err()
    assert _call(lib, _desc(), k_prep=None) == ARG and b"prepared" in err()        # an unprepared codebook
    assert _call(lib, _desc(), v_prep=None) == ARG and b"prepared" in err()
    assert _call(lib, _desc(), page_ids=None) == ARG and b"page_ids" in err()
    assert _call(lib, _desc(), k_new=PTRS["k_new"] + 2) == ALIGN and b"aligned" in err()
    assert _call(lib, _desc(), v_pool=PTRS["v_pool"] + 2) == ALIGN and b"aligned" in err()
    assert _call(lib, _desc(vn_stride_n=129)) == ALIGN and b"strides" in err()
    assert _call(lib, _desc(resid_stride_h=64 * 128 + 4)) == ALIGN and b"strides" in err()
    assert _call(lib, _desc(page_size=48)) == SHAPE and b"page_size=48" in err()
    assert _call(lib, _desc(d=96)) == SHAPE and b"d=96" in err()
    for bad in (dict(M=8), dict(d=64, M=128), dict(C=257), dict(C=0), dict(bs=0), dict(n_bound=-1), dict(n_pages_cap=0),
                dict(bs=20000, nh_k=2)):
        assert _call(lib, _desc(**bad)) == SHAPE, bad


def test_n_bound_zero_returns_ok(lib):
    assert _call(lib, _desc(n_bound=0)) == 0
    assert lib.million_pq_store_ragged(ctypes.byref(_desc(n_bound=0)), *[None] * 11, None) == 0


# ---------------------------------------------------------------- bookkeeping with ops monkeypatched ------------------------
def _patched(monkeypatch, calls):
    from million_amd import ops
    cache = _ragged_cache(monkeypatch, calls)      # slots at (96, 40, 50), (32, 0, 0), (0, 0, 0); layer 0 encoded ahead
    monkeypatch.setattr(ops, "pq_store_ragged", lambda *a, **k: calls.append(("store", a, k)))
    return cache


def test_extend_ragged_device_store_bookkeeping(monkeypatch):
    calls = []
    cache = _patched(monkeypatch, calls)
    before = cache.lengths[0].clone()
    ids_before = cache.page_ids[0].clone()
    x = torch.zeros(3, 2, 10, 128, dtype=torch.float16)
    out = cache.extend_ragged(torch.zeros(3, 8, 10, 128, dtype=torch.float16), x, x, 0, [10, 0, 7], device_store=True)
    assert out.shape == (3, 8, 10, 128)
    # exactly one attention call, then one store call, no pq_encode_into
    assert [c[0] for c in calls] == ["attn", "store"]
    attn_kw = calls[0][2]
    a, kw = calls[1][1], calls[1][2]
    k_new, v_new, k_res, v_res, k_prep, v_prep, k_pool, v_pool, page_ids, dev_lengths, dev_n = a
    assert k_new is x and v_new is x
    assert k_res.data_ptr() == cache.key_residual_cache[0].data_ptr() and v_res.data_ptr() == cache.value_residual_cache[0].data_ptr()
    assert k_pool is cache.key_page_pool and v_pool is cache.value_page_pool
    assert page_ids.data_ptr() == cache.page_ids[0].data_ptr() and page_ids.shape == cache.page_ids[0].shape
    # the cache's own device rows, and the attention's dev_n
    assert dev_lengths.data_ptr() == cache.lengths[0].data_ptr() and dev_lengths.shape == (3, 4)
    assert dev_n is attn_kw["dev_n_q"] and dev_n.dtype == torch.int32 and dev_n.tolist() == [10, 0, 7]
    assert attn_kw["dev_lengths"].data_ptr() == cache.lengths[0].data_ptr()
    assert kw == dict(M=64, C=256, page_size=32)
    # the mirror moved through its owners; the device rows are the call's to advance: no kernel ran, so they are unchanged
    assert list(cache._T_a[0]) == [146, 32, 7] and list(cache._r_a[0]) == [0, 0, 0] and list(cache._rs_a[0]) == [0, 0, 0]
    assert list(cache._seen_a[0]) == [146, 32, 7]
    assert list(cache._pre_a[0]) == [0, 1, 0]                      # encode-ahead joined per slot
    assert torch.equal(cache.lengths[0], before)
    assert torch.equal(cache.page_ids[0], ids_before)              # a preallocated table
    assert list(cache._T_a[1]) == [0, 0, 0]                        # the other layer is untouched


def test_extend_ragged_device_store_rejects_before_any_call(monkeypatch):
    calls = []
    cache = _patched(monkeypatch, calls)
    x = lambda n: torch.zeros(3, 2, n, 128, dtype=torch.float16)
    q = lambda n: torch.zeros(3, 8, n, 128, dtype=torch.float16)
    state = (cache._T_a.copy(), cache._r_a.copy(), cache._pre_a.copy(), cache.lengths[0].clone(), cache._pages_a.copy())
    for n, n_new in ((10, [10, 7]), (10, [10, 0, 11]), (10, [10, -1, 0]), (1000, [900, 0, 5])):
        with pytest.raises(RuntimeError):
            cache.extend_ragged(q(n), x(n), x(n), 0, n_new, device_store=True)
    assert not calls
    assert (cache._T_a == state[0]).all() and (cache._r_a == state[1]).all() and (cache._pre_a == state[2]).all()
    assert torch.equal(cache.lengths[0], state[3]) and (cache._pages_a == state[4]).all()


def test_default_keeps_the_host_driven_call_list(monkeypatch):
    calls = []
    cache = _patched(monkeypatch, calls)
    x = torch.zeros(3, 2, 10, 128, dtype=torch.float16)
    cache.extend_ragged(torch.zeros(3, 8, 10, 128, dtype=torch.float16), x, x, 0, [10, 0, 7], device_store=False)
    assert [c[0] for c in calls] == ["attn"] + ["enc"] * 6
    enc = [c[1] for c in calls[1:]]
    assert [(e["token_start"], e["n"], e["x_row_start"], e["x_row_mod"], e["page_ids"].data_ptr()) for e in enc] == \
        [(96, 40, 50, 64, cache.page_ids[0][0:1].data_ptr())] * 2 + [(136, 10, 0, 0, cache.page_ids[0][0:1].data_ptr())] * 2 + \
        [(0, 7, 0, 0, cache.page_ids[0][2:3].data_ptr())] * 2
    assert cache.lengths[0].tolist() == [[146, 0, 0, 0], [32, 0, 0, 0], [7, 0, 0, 0]]      # written from the host


def test_prefill_ragged_device_store_bookkeeping(monkeypatch):
    from million_amd import ops
    calls = []
    cache = _cpu_paged_cache(monkeypatch, calls)
    monkeypatch.setattr(ops, "prefill_attn", lambda q, k, v, **kw: (calls.append(("prefill", kw)), torch.zeros_like(q))[1])
    monkeypatch.setattr(ops, "pq_store_ragged", lambda *a, **k: calls.append(("store", a, k)))
    cache._T_a[0, 1], cache._r_a[0, 1], cache._rs_a[0, 1], cache._seen_a[0, 1] = 96, 40, 50, 136      # slot 1 is mid-sequence
    cache._sync_lengths(0)
    before = cache.lengths[0].clone()
    x = lambda n: torch.zeros(3, 2, n, 128, dtype=torch.float16)
    q = lambda n: torch.zeros(3, 8, n, 128, dtype=torch.float16)
    with pytest.raises(RuntimeError, match="extend_ragged"):
        cache.prefill_ragged(q(10), x(10), x(10), 0, [10, 1, 7], device_store=True)            # slot 1 holds tokens
    with pytest.raises(RuntimeError, match="max_tokens"):
        cache.prefill_ragged(q(1030), x(1030), x(1030), 0, [5, 0, 1030], device_store=True)
    assert not calls and list(cache._T_a[0]) == [0, 96, 0]
    K = x(10)
    cache.prefill_ragged(q(10), K, K, 0, [10, 0, 7], device_store=True)
    assert [c[0] for c in calls] == ["prefill", "store"]
    a = calls[1][1]
    assert a[0] is K and a[9].data_ptr() == cache.lengths[0].data_ptr()
    assert a[10].dtype == torch.int32 and a[10].tolist() == [10, 0, 7]
    assert list(cache._T_a[0]) == [10, 96, 7] and list(cache._r_a[0]) == [0, 40, 0] and list(cache._seen_a[0]) == [10, 136, 7]
    assert list(cache._rs_a[0]) == [0, 50, 0]
    assert torch.equal(cache.lengths[0], before)                   # the device rows are the call's to advance


def test_device_store_reserves_pages_on_demand_before_the_launch(monkeypatch):
    from million_amd import ops
    from million_amd.pq_cache import PagedPQCache
    calls = []
    seen_pages = []
    monkeypatch.setattr(ops, "pq_chunk_attn", lambda q, *a, **k: (calls.append("attn"), seen_pages.append(cache._pages_a[0].copy()), torch.zeros_like(q))[2])
    monkeypatch.setattr(ops, "pq_encode_into", lambda *a, **k: calls.append("enc"))
    monkeypatch.setattr(ops, "pq_store_ragged", lambda *a, **k: (calls.append("store"), seen_pages.append(cache._pages_a[0].copy())))
    cache = PagedPQCache(bs=3, nh=8, num_key_value_heads=2, M=64, layer_num=1, d=128, page_size=32, extended_residual_size=64,
                         max_tokens=1024, preallocate=False, device="cpu")
    cache.key_cent = cache.value_cent = torch.zeros(64, 256, 2, dtype=torch.float16)
    cache._kprep = cache._vprep = torch.zeros(1, dtype=torch.float16)
    cache._assign_pages(0, 3, 0)
    cache._T_a[0, 0], cache._r_a[0, 0], cache._rs_a[0, 0], cache._seen_a[0, 0] = 70, 40, 50, 110
    x = torch.zeros(3, 2, 30, 128, dtype=torch.float16)
    cache.extend_ragged(torch.zeros(3, 8, 30, 128, dtype=torch.float16), x, x, 0, [30, 0, 9], device_store=True)
    assert calls == ["attn", "store"]
    # 70 + 40 + 30 = 140 tokens: 5 pages; 9 tokens: 1 page; slot 1: none - all there before the first launch
    assert all(list(p) == [5, 0, 1] for p in seen_pages)
    assert (cache.page_ids[0][0, :, :5] >= 0).all() and len(set(cache.page_ids[0][0].flatten().tolist()[:5])) == 5


# ---------------------------------------------------------------- the numpy model ------------------------------------------
GEOM = dict(page_size=32, n_pages_cap=8, resid_cap=SM.CAP, n_bound=SM.N_BOUND)


def test_model_on_the_case_table():
    p0, p1, p2, p3 = SM.plans(SM.CASES, **GEOM)
    # slot 0: ring rows 50..63 then 0..25 (40 of them), then new rows 0..29, at tokens 70..139
    assert p0.src == [("win", i) for i in list(range(50, 64)) + list(range(0, 26))] + [("new", i) for i in range(30)]
    assert list(p0.tokens) == list(range(70, 140)) and p0.kept.all() and p0.T_after == 140
    assert p0.pages_written(32) == [2, 3, 4]
    # slot 1 takes no part, whatever its window holds
    assert not p1.live and p1.src == [] and p1.T_after is None
    assert p2.src == [("new", i) for i in range(9)] and list(p2.tokens) == list(range(9)) and p2.T_after == 9
    assert p3.src == [("win", i) for i in range(64)] + [("new", i) for i in range(70)]
    assert list(p3.tokens) == list(range(64, 198)) and p3.T_after == 198 and p3.pages_written(32) == [2, 3, 4, 5, 6]
    lengths = np.array([[T, r, s, 0x7EADBEEF] for T, r, s, _ in SM.CASES], np.int32)
    after = SM.advance(lengths, [c[3] for c in SM.CASES], **GEOM)
    assert after.tolist() == [[140, 0, 0, 0x7EADBEEF], [32, 17, 3, 0x7EADBEEF], [9, 0, 0, 0x7EADBEEF], [198, 0, 0, 0x7EADBEEF]]
    # page size does not move tokens, only pages
    for ps, cap in ((64, 4), (128, 2)):
        q0 = SM.Plan(SM.CASES[0], page_size=ps, n_pages_cap=cap, resid_cap=SM.CAP, n_bound=SM.N_BOUND)
        assert list(q0.tokens) == list(p0.tokens) and q0.src == p0.src and q0.kept.all()


def test_model_on_untrusted_rows():
    u0, u1, u2, u3 = SM.plans(SM.UNTRUSTED, **GEOM)
    # T = -5 -> 0, r = 1000 -> 64, start = 64 -> 0, n = 1000 -> 70
    assert (u0.T, u0.r, u0.start, u0.n) == (0, 64, 0, 70)
    assert u0.src == [("win", i) for i in range(64)] + [("new", i) for i in range(70)] and u0.T_after == 134 and u0.kept.all()
    # the last rows lie past the table: tokens 250 .. 255 are stored, 256 .. 269 dropped, T stops at the capacity
    assert list(u1.tokens[u1.kept]) == list(range(250, 256)) and (~u1.kept).sum() == 14 and u1.T_after == 256
    assert u1.pages_written(32) == [7]
    # T past the table: every store dropped; r = -3 -> 0, start = -1 -> 0
    assert (u2.T, u2.r, u2.start, u2.n) == (256, 0, 0, 5) and not u2.kept.any() and u2.T_after == 256 and u2.pages_written(32) == []
    # n = -4 -> 0: no part, and the row - untrusted as it is - stays
    assert not u3.live
    lengths = np.array([[T, r, s, 7] for T, r, s, _ in SM.UNTRUSTED], np.int64).clip(-2 ** 31, 2 ** 31 - 1).astype(np.int32)
    after = SM.advance(lengths, [c[3] for c in SM.UNTRUSTED], **GEOM)
    assert after.tolist() == [[134, 0, 0, 7], [256, 0, 0, 7], [256, 0, 0, 7], [40, 10, 70, 7]]


@pytest.mark.parametrize("ps,cap,prefill,steps", [(32, 64, 70, 200), (64, 128, 5, 300), (32, 64, 0, 63)])
def test_model_ring_order_follows_the_paging_policy(oracle, ps, cap, prefill, steps):
    """oracle.PagedPolicy gives (T, r) of a request after `steps` decode steps behind a prompt; decode token i sits in ring row
    i % cap (the window starts at row 0 and every flush moves the start by one page).  The model's source order must be the
    sequence order: source row j is position T + j, i.e. ring row (T + j - prefill) % cap - and T + r + n tokens are stored."""
    pol = oracle.PagedPolicy(page_size=ps, residual=cap, prefill=prefill)
    for i in range(steps):
        T, r = pol.step()
    start = (pol.flushes * ps) % cap
    assert T + r == prefill + steps
    p = SM.Plan((T, r, start, 11), page_size=ps, n_pages_cap=64, resid_cap=cap, n_bound=16)
    assert [i for kind, i in p.src if kind == "win"] == [(T + j - prefill) % cap for j in range(r)]
    assert p.src[r:] == [("new", j) for j in range(11)]
    assert list(p.tokens) == list(range(T, T + r + 11)) and p.T_after == prefill + steps + 11


def test_model_rows_and_scatter():
    rs_ = np.random.RandomState(0)
    win, new = rs_.standard_normal((2, 64, 8)), rs_.standard_normal((2, 70, 8))
    p = SM.Plan(SM.CASES[0], **GEOM)
    rows = p.rows_of(win, new)
    assert rows.shape == (2, 70, 8) and np.array_equal(rows[:, 0], win[:, 50]) and np.array_equal(rows[:, 14], win[:, 0])
    assert np.array_equal(rows[:, 40], new[:, 0]) and np.array_equal(rows[:, 69], new[:, 29])
    ids = np.arange(4 * 2 * 8).reshape(4, 2, 8)[:, :, ::-1].copy()
    kp, vp = np.full((64, 32, 4), 0xA5, np.uint8), np.full((64, 4, 32), 0xA5, np.uint8)
    kc = rs_.randint(0, 100, (2, 70, 4)).astype(np.uint8)
    SM.scatter(kp, vp, ids, 0, p, kc, kc + 100)
    # token 70 = page 2, offset 6; token 139 = page 4, offset 11
    assert np.array_equal(kp[ids[0, 1, 2], 6], kc[1, 0]) and np.array_equal(vp[ids[0, 1, 4], :, 11], kc[1, 69] + 100)
    assert (kp[ids[0, 0, 2], :6] == 0xA5).all() and (kp[ids[0, 0, 4], 12:] == 0xA5).all()
    assert (kp != 0xA5).any(axis=(1, 2)).sum() == 6      # three pages per kv head, no other page touched


# ---------------------------------------------------------------- kernel metadata -------------------------------------------
def test_every_store_ragged_instance_has_no_scratch_no_spills_no_lds(lib):
    """paged_store_kernel<DM, P> (csrc/paged_store.h): the store's instances (P = StoreRaggedParams), the commit's (WindowCommitParams)
    and the wide store's two (StoreRaggedWideParams: d / M is 2 or 4)."""
    out = subprocess.run([sys.executable, str(ROOT / "tools" / "kernel_meta.py"), str(ROOT / "million_amd" / "libmillion_hip.so"), "paged_store_kernel"],
                         capture_output=True, text=True, check=True).stdout
    for params, dms in (("StoreRaggedParams", "1248"), ("WindowCommitParams", "1248"), ("StoreRaggedWideParams", "24")):
        rows = [l for l in out.splitlines() if "paged_store_kernel" in l and params in l]
        assert sorted(l.split()[0][l.index("ILi"):][:5] for l in rows) == [f"ILi{dm}E" for dm in dms], out
        for l in rows:
            assert l.rstrip().endswith("vgpr_spill 0 sgpr_spill 0 scratch 0 B"), l
            assert " lds 0 B " in l, l
