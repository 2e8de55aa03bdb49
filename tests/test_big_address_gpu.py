"""Far addresses on the GPU (tests/big_address.py): every call runs twice - once through page ids and strides that put its bytes
past 2^31 and 2^32 bytes from the base of a 4 GiB buffer, once as its compact twin - and everything the call writes must be
bitwise equal.  The twin is also held against the suite's oracle at the suite's bars, so two equal wrongs cannot pass.
tests/test_big_address_host.py shows on a model that these tables catch a byte offset truncated to 31 or 32 bits.

A form whose compact call is not bitwise repeatable run to run (the twin is called twice) is compared far-against-oracle at the
same bars instead and prints a BIGADDR line naming itself."""
import ctypes
import zlib

import numpy as np
import pytest

from tests import big_address as BA
from tests import flash_inputs, lse_ref, synth
from tests.test_chunk_attn_gpu import model as chunk_model, _state as chunk_state
from tests.test_gpu_parity import _check

pytestmark = pytest.mark.gpu

NEED_FREE = 12 << 30
S16 = -23131          # 0xA5A5 as int16: the sentinel seen through an fp16 view


@pytest.fixture(scope="module")
def env():
    import torch
    assert torch.cuda.is_available(), "GPU tests need an MI355X"
    from million_amd import ops, _lib
    _lib.load()
    return torch, ops


class _Flats:
    """The two flat device buffers every far pool and far view of this file lies in (about 8.1 GiB together): made when a test
    first asks for them, dropped by the one test that brings pools of that size of its own."""
    def __init__(self, torch):
        self.torch, self.bufs = torch, None

    def get(self):
        if self.bufs is None:
            free = self.torch.cuda.mem_get_info()[0]
            if free < NEED_FREE:
                pytest.skip(f"{free / 2 ** 30:.1f} GiB of device memory free, the far buffers want {NEED_FREE >> 30} GiB")
            self.bufs = tuple(self.torch.empty(BA.FLAT_BYTES, dtype=self.torch.uint8, device="cuda") for _ in range(2))
        return self.bufs

    def drop(self):
        self.bufs = None
        self.torch.cuda.empty_cache()


@pytest.fixture(scope="module")
def flat_store(env):
    store = _Flats(env[0])
    yield store
    store.drop()


@pytest.fixture
def far(flat_store):
    flats = flat_store.get()
    for f in flats:
        f.fill_(BA.SENTINEL)
    return flats


def _cu(torch, a):
    return None if a is None else torch.from_numpy(np.ascontiguousarray(a)).cuda()


def _bits(t):
    return t.detach().cpu().contiguous().numpy().tobytes()


def _same(far_t, twin_t, twin2_t, what, vs_oracle):
    """far == twin bitwise when the twin repeats itself bitwise; else far against the oracle at the twin's bar."""
    if _bits(twin_t) == _bits(twin2_t):
        assert _bits(far_t) == _bits(twin_t), f"{what}: the far call differs from its compact twin"
    else:
        print(f"BIGADDR not bitwise repeatable: {what}")
        vs_oracle(far_t, f"{what} (far)")


def _assert_far(tab, page_bytes):
    """The table cannot pass vacuously: every row has pages in all three bands and a page that a 31-bit and a 32-bit offset
    would send to bytes that are not the row's."""
    assert BA.sensitive_rows(tab, page_bytes, 31).all() and BA.sensitive_rows(tab, page_bytes, 32).all()
    assert all(set(BA.band_of(row, page_bytes).tolist()) == {0, 1, 2} for row in tab.reshape(-1, tab.shape[-1]))


def _far_table(torch, ids_c, page_bytes, seed, i64=False):
    """Compact ids (any shape, a bijection onto arange) -> (far ids of the pages in compact order, the far table)."""
    n = int(ids_c.max()) + 1
    fid = BA.far_ids(n, page_bytes, seed)
    tab = fid[ids_c]
    _assert_far(tab, page_bytes)
    return fid, _cu(torch, tab.astype(np.int64 if i64 else np.int32))


def _far_pools(torch, far, ps, M, kpool_c, vpool_c, fid, code_bytes=1):
    B = ps * M * code_bytes
    kbig, vbig = BA.pool_view(far[0], B, (ps, M), code_bytes=code_bytes), BA.pool_view(far[1], B, (M, ps), code_bytes=code_bytes)
    BA.scatter_pool(kbig, kpool_c, fid)
    BA.scatter_pool(vbig, vpool_c, fid)
    return kbig, vbig


# ----------------------------------------------------------------------------- 7. one PagedPQCache whose pools pass 4 GiB ---
# The cache's own zeroed pools (2 x 4.0 GiB) stand in for the far buffers, which the test drops first (the next far test makes
# them again) - so no more than about 9 GiB is live at a time, whatever the order of the tests.
def _slot_bits(torch, cache, b):
    """What slot b is, whatever pages hold it: lengths rows, both windows, K and V codes of its T tokens in every layer."""
    T, ps = int(cache._T_a[0, b]), cache.page_size
    n_live = -(-T // ps)
    ids = cache._page_ids_all[:, b, :, :n_live].long()
    nl, nhk = ids.shape[:2]
    k = cache.key_page_pool[ids.reshape(-1)].reshape(nl, nhk, n_live * ps, cache.M)[:, :, :T]
    v = cache.value_page_pool[ids.reshape(-1)].reshape(nl, nhk, n_live, cache.M, ps).permute(0, 1, 2, 4, 3).reshape(nl, nhk, n_live * ps, cache.M)[:, :, :T]
    return dict(lengths=_bits(cache._lengths_all[:, b]), k_win=_bits(cache._kres_all[:, b]), v_win=_bits(cache._vres_all[:, b]),
                k_codes=_bits(k), v_codes=_bits(v)), k.cpu().numpy(), v.cpu().numpy(), ids.cpu().numpy()


def test_paged_cache_pools_past_4gib(env, oracle, flat_store):
    """A PagedPQCache (paging on demand, 8 KiB pages) whose K and V pools are 4 GiB + 64 pages each, against a compact twin of
    the same geometry: page ids are burnt through page_manager.allocate_pages so that the prompt's pages straddle id
    2^31 / 8192 and the first flush's pages straddle 2^32 / 8192; everything later (fork's tail page, swap_in's pages) lies
    past 4 GiB or in the released ids around the boundaries.  After prefill, decode across a flush, fork, swap_out / swap_in and
    verify + commit: outputs, lengths rows, windows and the slots' codes read through their tables are the twin's, bit for
    bit; the twin's codes and outputs are the oracle's, and after fork, swap and commit its device lengths rows are what the
    steps amount to.  Both slots hold prompts of one length, so every launch is shaped by the host lengths
    (use_dev_lengths=False): the bound max_tokens, which differs between the two caches, shapes no launch.  Steps with host
    lengths leave the device rows behind the mirror; fork and commit, whose kernels read them, must bring them up first."""
    torch, ops = env
    from million_amd.pq_cache import PagedPQCache
    flat_store.drop()
    free = torch.cuda.mem_get_info()[0]
    if free < NEED_FREE:
        pytest.skip(f"{free / 2 ** 30:.1f} GiB of device memory free, the cache's pools want {NEED_FREE >> 30} GiB")
    nl, bs, nh, nhk, d, M, ps, cap, n_prompt, n_dec, n_ver = 2, 2, 8, 2, 128, 64, 128, 128, 300, 129, 4
    B = ps * M
    lo_id, hi_id = 2 ** 31 // B, 2 ** 32 // B
    pages_cap = -(-(hi_id + 64 + 1) // (nl * bs * nhk))
    assert nl * bs * nhk * pages_cap > hi_id + 64
    rs_ = np.random.RandomState(2024)
    f = lambda *s_: rs_.standard_normal(s_).astype(np.float16)
    N = n_prompt + n_dec + n_ver
    K, V, ck, cv = f(nl, bs, nhk, N, d), f(nl, bs, nhk, N, d), f(M, 256, d // M), f(M, 256, d // M)
    qp, qd, qv = f(1, nh, n_prompt, d), f(n_dec, nl, bs, nh, 1, d), f(nl, bs, nh, n_ver, d)
    geom = dict(bs=bs, nh=nh, num_key_value_heads=nhk, M=M, layer_num=nl, d=d, page_size=ps, extended_residual_size=cap, preallocate=False,
                device="cuda")
    caches = {"far": PagedPQCache(max_tokens=pages_cap * ps, **geom), "twin": PagedPQCache(max_tokens=8 * ps, **geom)}
    assert caches["far"].key_page_pool.numel() > 2 ** 32 + 64 * B and caches["far"].key_page_pool.shape[0] == nl * bs * nhk * pages_cap
    for c in caches.values():
        c.set_cent(_cu(torch, ck), _cu(torch, cv))
    pm = caches["far"].page_manager

    def burn_to(next_id):
        lowest = min(pm.free_pages)
        assert lowest <= next_id
        pm.allocate_pages(next_id - lowest)
        assert min(pm.free_pages) == next_id

    def same_state(what, slots=(0, 1)):
        far_ids = []
        for b in slots:
            (sf, kf, vf, idf), (st, kt, vt, _) = _slot_bits(torch, caches["far"], b), _slot_bits(torch, caches["twin"], b)
            for nm in sf:
                assert sf[nm] == st[nm], f"{what}: slot {b}: {nm} of the cache past 4 GiB differs from the twin's"
            T = kt.shape[2]
            assert T == int(caches["twin"]._T_a[0, b])
            for nm, got, want in (("K", kt, oracle.pq_encode(K[:, b, :, :T], ck)), ("V", vt, oracle.pq_encode(V[:, b, :, :T], cv))):
                bad = np.argwhere((got != want).any(axis=-1))
                assert bad.size == 0, (f"{what}: slot {b}: the twin's {nm} codes are not the oracle's at {len(bad)} (layer, kv head, token), "
                                       f"first {bad[0].tolist()}, last {bad[-1].tolist()}")
            far_ids.append(idf)
        return far_ids

    # phase 1: the prompts; the pages of slot 0, layer 0 straddle byte 2^31 of the pools
    burn_to(lo_id - 3)
    for c in caches.values():
        for b in range(bs):
            for l in range(nl):
                c.prefill_request(b, _cu(torch, qp), _cu(torch, K[l, b:b + 1, :, :n_prompt]), _cu(torch, V[l, b:b + 1, :, :n_prompt]), l)
    ids1 = np.concatenate([i.ravel() for i in same_state("prefill")])
    assert ids1.min() < lo_id <= ids1.max() < hi_id, (ids1.min(), ids1.max())
    # phase 2: decode until the window has flushed once; the flush's pages straddle byte 2^32
    burn_to(hi_id - 3)
    outs = {name: [] for name in caches}
    for i in range(n_dec):
        for l in range(nl):
            t = n_prompt + i
            for name, c in caches.items():
                outs[name].append(c.decoding_with_pages(_cu(torch, qd[i, l]), _cu(torch, K[l, :, :, t:t + 1]), _cu(torch, V[l, :, :, t:t + 1]), l).clone())
    torch.cuda.synchronize()
    assert _bits(torch.stack(outs["far"])) == _bits(torch.stack(outs["twin"])), "decode outputs differ from the twin's"
    T, r = n_prompt + ps, n_dec - ps
    assert caches["far"]._T_a.tolist() == [[T] * bs] * nl and caches["far"]._r_a.tolist() == [[r] * bs] * nl
    ids2 = np.concatenate([i[:, :, -1].ravel() for i in same_state("decode across a flush")])      # the page the flush filled
    assert ids2.min() < hi_id <= ids2.max(), (ids2.min(), ids2.max())
    for l in range(nl):      # the twin's last step against the oracle: codes of T tokens, r window rows from the ring's start
        st = int(caches["twin"]._rs_a[l, 0])
        kres, vres = np.zeros((bs, nhk, cap, d), np.float16), np.zeros((bs, nhk, cap, d), np.float16)
        kres[:, :, :r], vres[:, :, :r] = K[l, :, :, T:T + r], V[l, :, :, T:T + r]
        gold = oracle.decode_attn(qd[n_dec - 1, l], oracle.pq_encode(K[l, :, :, :T], ck), oracle.pq_encode(V[l, :, :, :T], cv), ck, cv, kres, vres, r)
        _check(outs["twin"][-nl + l].cpu().numpy(), gold, f"twin, last decode step, layer {l} (ring start {st})")
    # phase 3: fork slot 0 into slot 1 (shared full pages, one copied tail page per layer and kv head)
    K[:, 1], V[:, 1] = K[:, 0].copy(), V[:, 0].copy()      # slot 1's history is slot 0's from here on
    for c in caches.values():
        c.release(1)
        c.fork(0, 1)
        st = int(c._rs_a[0, 0])
        assert c._lengths_all.cpu().tolist() == [[[T, r, st, 0]] * bs] * nl, "fork: the device rows are not the source's lengths"
    same_state("fork")
    # phase 4: slot 1 out to host memory and back into fresh pages
    for c in caches.values():
        c.swap_in(1, c.swap_out(1))
        assert c._lengths_all.cpu().tolist() == [[[T, r, st, 0]] * bs] * nl
    ids4 = same_state("swap_out / swap_in")[1]
    # phase 5: verify four draft rows per slot, commit three and two of them
    t0 = T + r
    vout = {name: [c.verify(_cu(torch, qv[l]), _cu(torch, K[l, :, :, t0:t0 + n_ver]), _cu(torch, V[l, :, :, t0:t0 + n_ver]), l,
                            use_dev_lengths=False).clone() for l in range(nl)] for name, c in caches.items()}
    torch.cuda.synchronize()
    assert _bits(torch.stack(vout["far"])) == _bits(torch.stack(vout["twin"])), "verify outputs differ from the twin's"
    for l in range(nl):
        gold = chunk_model(oracle, qv[l], oracle.pq_encode(K[l, :, :, :T], ck), oracle.pq_encode(V[l, :, :, :T], cv), ck, cv,
                           K[l, :, :, T:T + r], V[l, :, :, T:T + r], K[l, :, :, t0:t0 + n_ver], V[l, :, :, t0:t0 + n_ver])
        _check(vout["twin"][l].float().cpu().numpy(), gold, f"twin, verify, layer {l}")
    for c in caches.values():
        c.commit([3, 2])
        assert c._r_a.tolist() == [[r + 3, r + 2]] * nl and c._lengths_all.cpu().tolist() == [[[T, r + 3, st, 0], [T, r + 2, st, 0]]] * nl
    same_state("verify + commit")
    for name, c in caches.items():      # the committed rows are the window's newest, in order
        for b, a in enumerate((3, 2)):
            slots = [(st + r + i) % cap for i in range(a)]
            assert np.array_equal(c._kres_all[:, b][:, :, slots].cpu().numpy(), K[:, b, :, t0:t0 + a]), f"{name}: committed K rows of slot {b}"
            assert np.array_equal(c._vres_all[:, b][:, :, slots].cpu().numpy(), V[:, b, :, t0:t0 + a]), f"{name}: committed V rows of slot {b}"
    assert ops.tail_faults() == 0
    # the slots' tables held ids on both sides of both boundaries, so none of this passed on low ids alone
    seen = np.concatenate([ids1, ids2, ids4.ravel()])
    assert (seen < lo_id).any() and ((seen >= lo_id) & (seen < hi_id)).any() and (seen >= hi_id).any()
    for c in caches.values():
        c.cleanup()
    caches.clear()
    del pm, c
    import gc
    gc.collect()
    torch.cuda.empty_cache()


# ------------------------------------------------------------------------------------------ 1. decode attention, far pages ---
# name, d, M, C, G, policy, ps, kind (million_attn_kernel_kind: 1 MFMA lean / streaming, 3 tile, 0 scalar)
DECODE_FORMS = [
    ("lean-d128-M64", 128, 64, 256, 4, 0, 64, 1), ("lean-d128-M32", 128, 32, 256, 4, 0, 128, 1),
    ("lean-d128-M64-C128", 128, 64, 128, 4, 0, 64, 1), ("lean-d64-M32", 64, 32, 256, 4, 0, 64, 1),
    ("lean-d64-M16", 64, 16, 256, 4, 0, 128, 1), ("lean-d64-M64", 64, 64, 256, 4, 0, 64, 1),
    ("stream-M64", 128, 64, 256, 4, 16, 64, 1), ("stream-M32", 128, 32, 256, 8, 16, 64, 1),
    ("stream-M32-dm4", 128, 32, 256, 4, 16, 128, 1), ("stream-M16", 128, 16, 256, 4, 0, 64, 1),
    ("stream-M64-C128", 128, 64, 128, 4, 16, 64, 1), ("stream-M64-ps32", 128, 64, 256, 4, 0, 32, 1),
    ("tile-d64-M32-ps32", 64, 32, 256, 4, 0, 32, 3), ("generic-d128-M64", 128, 64, 256, 4, 1, 64, 0),
]
BY_FORM = {f[0]: f for f in DECODE_FORMS}


def _decode_pair(torch, ops, oracle, far, form, *, i64=False, lse=False, append=False):
    name, d, M, C, G, policy, ps, kind = form
    bs, nhk, npg = BA.TABLE
    assert (ps, M) in BA.GEOMS
    T, r, cap = npg * ps - 7, 17, 128
    c = synth.attn_case(zlib.crc32(name.encode()) % 10000, bs, G * nhk, nhk, d, M, C, T, r, Lt=cap)
    kpool_c, ids_c = oracle.k_rowmajor_to_pool(c["k_codes"], ps)
    vpool_c, _ = oracle.v_rowmajor_to_pool(c["v_codes"], ps)
    assert ids_c.shape == BA.TABLE
    fid, tab_far = _far_table(torch, ids_c, ps * M, 11, i64)
    kpc, vpc = _cu(torch, kpool_c), _cu(torch, vpool_c)
    kbig, vbig = _far_pools(torch, far, ps, M, kpc, vpc, fid)
    tab_c = _cu(torch, ids_c.astype(np.int64 if i64 else np.int32))
    t = {k: _cu(torch, v) for k, v in c.items() if isinstance(v, np.ndarray)}
    kp, vp = ops.prepare_cents(t["k_cents"], cache=False), ops.prepare_cents(t["v_cents"], cache=False)
    k_new = v_new = None
    if append:
        rs_ = np.random.RandomState(3)
        k_new, v_new = (_cu(torch, rs_.standard_normal((bs, nhk, 1, d)).astype(np.float16)) for _ in range(2))
    desc = ops.make_attn_desc(t["q"], t["k_res"], nh_k=nhk, M=M, C=C, n_tokens=T, r=r, k_paged=True, v_paged=True, page_size=ps,
                              n_pages_cap=npg, page_ids_i64=i64, k_codes=kpc, v_codes=vpc,
                              dev_lengths=torch.zeros(bs, 4, dtype=torch.int32, device="cuda") if append else None)
    ops.set_force_generic(policy)
    try:
        assert ops.attn_kernel_kind(desc) == kind, (name, ops.attn_kernel_kind(desc))

        def call(kpool, vpool, tab):
            kr, vr = t["k_res"].clone(), t["v_res"].clone()
            dl = torch.tensor([[T, r, 0, 0]] * bs, dtype=torch.int32, device="cuda") if append else None
            res = ops.pq_decode_attn(t["q"], kpool, vpool, kp, vp, kr, vr, r, M=M, C=C, n_tokens=T, k_page_ids=tab, v_page_ids=tab,
                                     page_size=ps, out=torch.full_like(t["q"], float("nan")), dev_lengths=dl, k_new=k_new, v_new=v_new,
                                     return_lse=lse)
            torch.cuda.synchronize()
            out, l = res if lse else (res, None)
            return dict(out=out, lse=l, k_res=kr, v_res=vr, lengths=dl)

        twin, twin2, got = call(kpc, vpc, tab_c), call(kpc, vpc, tab_c), call(kbig, vbig, tab_far)
    finally:
        ops.set_force_generic(0)
    assert ops.tail_faults() == 0
    kres, vres, r_eff = c["k_res"], c["v_res"], r
    if append:
        kres, vres, r_eff = kres.copy(), vres.copy(), r + 1
        kres[:, :, r], vres[:, :, r] = k_new.cpu().numpy()[:, :, 0], v_new.cpu().numpy()[:, :, 0]
    gold = oracle.decode_attn(c["q"], c["k_codes"], c["v_codes"], c["k_cents"], c["v_cents"], kres, vres, r_eff, return_lse=lse)
    gold, gold_lse = gold if lse else (gold, None)
    vs_out = lambda o, what: _check(o.cpu().numpy(), gold, what)
    vs_out(twin["out"], f"{name} twin")
    _same(got["out"], twin["out"], twin2["out"], f"decode {name} i64={i64} out", vs_out)
    if lse:
        vs_lse = lambda l, what: np.testing.assert_allclose(l.cpu().numpy()[:, :, 0], gold_lse, rtol=0, atol=lse_ref.LSE_TOL, err_msg=what)
        vs_lse(twin["lse"], f"{name} twin lse")
        _same(got["lse"], twin["lse"], twin2["lse"], f"decode {name} i64={i64} lse", vs_lse)
    if append:      # the window row and the lengths row the call writes
        np.testing.assert_array_equal(twin["k_res"].cpu().numpy(), kres)
        np.testing.assert_array_equal(twin["v_res"].cpu().numpy(), vres)
        assert twin["lengths"].cpu().tolist() == [[T, r + 1, 0, 0]] * bs
        for nm in ("k_res", "v_res", "lengths"):
            assert _bits(got[nm]) == _bits(twin[nm]), f"{name}: {nm} after the far call differs from the twin's"
    # the call reads the pools and writes none of them
    BA.assert_only_these_pages(kbig, fid, kpc, far[0], f"{name} K pool")
    BA.assert_only_these_pages(vbig, fid, vpc, far[1], f"{name} V pool")


@pytest.mark.parametrize("i64", [False, True], ids=["i32", "i64"])
@pytest.mark.parametrize("form", DECODE_FORMS, ids=[f[0] for f in DECODE_FORMS])
def test_decode_far_pages(form, i64, env, oracle, far):
    """Every decode-attention instance family reads K and V pages on both sides of byte 2^31 and byte 2^32 of its pools:
    int32 ids (mode 0 of the MFMA kernels) and int64 ids (mode 2)."""
    torch, ops = env
    _decode_pair(torch, ops, oracle, far, form, i64=i64)


@pytest.mark.parametrize("name", ["lean-d128-M64", "stream-M64"])
def test_decode_far_pages_lse(name, env, oracle, far):
    torch, ops = env
    _decode_pair(torch, ops, oracle, far, BY_FORM[name], lse=True)


@pytest.mark.parametrize("name,i64", [("lean-d128-M32", False), ("stream-M64-C128", True)])
def test_decode_far_pages_append_device_lengths(name, i64, env, oracle, far):
    torch, ops = env
    _decode_pair(torch, ops, oracle, far, BY_FORM[name], i64=i64, append=True)


def test_decode_rowmajor_k_dense_v_far(env, oracle, far):
    """Row-major K with dense V pages (mode 1): the V page of (b, kv head, page) is bh * n_pages_cap + page, no table.  With
    n_pages_cap = 349530 the rows of bh = 2 start past byte 2^31 and those of bh = 3 past byte 2^32 of the dense pool.  The
    dense pool is the caller's through the C entry (ops.pq_decode_attn builds its own, sized by the context, from row-major
    V: a context that long is no few-second test); the twin has n_pages_cap = the live pages."""
    torch, ops = env
    from million_amd import _lib as L
    bs, nh, nhk, d, M, C, ps, T, r, cap = 2, 8, 2, 128, 64, 256, 64, 633, 17, 128
    cap_far = 349530
    npg = -(-T // ps)
    assert 2 * cap_far * ps * M > 2 ** 31 and 3 * cap_far * ps * M > 2 ** 32 and 3 * cap_far + npg <= BA.n_pool(ps * M)
    c = synth.attn_case(4242, bs, nh, nhk, d, M, C, T, r, Lt=cap)
    t = {k: _cu(torch, v) for k, v in c.items() if isinstance(v, np.ndarray)}
    kp, vp = ops.prepare_cents(t["k_cents"], cache=False), ops.prepare_cents(t["v_cents"], cache=False)
    vpool_c, ids_c = oracle.v_rowmajor_to_pool(c["v_codes"], ps)      # pages in (b, h, page) order: the dense layout at cap = npg
    vpc = _cu(torch, vpool_c)
    fid = (np.arange(bs * nhk)[:, None] * cap_far + np.arange(npg)[None, :]).ravel()
    assert set(BA.band_of(fid, ps * M).tolist()) == {0, 1, 2}
    vbig = BA.pool_view(far[1], ps * M, (M, ps))
    BA.scatter_pool(vbig, vpc, fid)
    lib = L.load()

    def call(vpool, n_pages_cap):
        desc = ops.make_attn_desc(t["q"], t["k_res"], nh_k=nhk, M=M, C=C, n_tokens=T, r=r, k_paged=False, v_paged=True, page_size=ps,
                                  n_pages_cap=n_pages_cap, k_codes=t["k_codes"], v_pages_dense=True)
        assert ops.attn_kernel_kind(desc) == 1
        ws = ops.attn_workspace(desc, t["q"].device)
        out = torch.full_like(t["q"], float("nan"))
        L.check(lib.million_pq_decode_attn(ctypes.byref(desc), t["q"].data_ptr(), t["k_codes"].data_ptr(), vpool.data_ptr(), None, None,
                                           kp.data_ptr(), vp.data_ptr(), t["k_res"].data_ptr(), t["v_res"].data_ptr(), out.data_ptr(),
                                           ws.data_ptr(), ws.numel(), torch.cuda.current_stream().cuda_stream), "million_pq_decode_attn")
        torch.cuda.synchronize()
        return out

    twin, twin2, got = call(vpc, npg), call(vpc, npg), call(vbig, cap_far)
    gold = oracle.decode_attn(**c)
    vs = lambda o, what: _check(o.cpu().numpy(), gold, what)
    vs(twin, "dense V twin")
    _same(got, twin, twin2, "decode row-major K, dense V", vs)
    BA.assert_only_these_pages(vbig, fid, vpc, far[1], "dense V pool")


# ---------------------------------------------------------------------------------------- 2. decode attention, far strides ---
def _fill_view(view, src):
    view.copy_(src)
    return view


@pytest.mark.parametrize("T", [633, 0], ids=["T633", "T0-window-only"])
def test_decode_far_window_and_rowmajor_k_strides(T, env, oracle, far):
    """k_res / v_res whose batch stride puts request 1 past element 2^31 (byte 2^32), with a fused append writing into that
    window; row-major K codes whose batch stride puts request 1 past byte 2^32 (V paged, compact); T = 0: the window alone
    (tile kernel)."""
    torch, ops = env
    bs, nh, nhk, d, M, C, ps, r, cap = 2, 8, 2, 128, 64, 256, 64, 17, 128
    c = synth.attn_case(777 + T, bs, nh, nhk, d, M, C, T, r, Lt=cap)
    t = {k: _cu(torch, v) for k, v in c.items() if isinstance(v, np.ndarray)}
    kp, vp = ops.prepare_cents(t["k_cents"], cache=False), ops.prepare_cents(t["v_cents"], cache=False)
    rs_ = np.random.RandomState(5)
    k_new, v_new = (_cu(torch, rs_.standard_normal((bs, nhk, 1, d)).astype(np.float16)) for _ in range(2))
    sb = BA.far_stride(nhk * cap * d)
    res_shape, res_strides = (bs, nhk, cap, d), (sb, cap * d, d, 1)
    Tc = max(T, 1)
    ksb = BA.HI + 64      # bytes = uint8 elements
    kc_far = BA.far_view(far[0], (bs, nhk, Tc, M), (ksb, Tc * M, M, 1), torch.uint8)
    # the far K codes live in the first buffer, behind the window's bytes of each request
    woff = 1 << 18
    kres_far = BA.far_view(far[0][2 * woff:], res_shape, res_strides, torch.float16)
    vres_far = BA.far_view(far[1], res_shape, res_strides, torch.float16)
    assert kres_far.stride(0) * 2 > 2 ** 32 and kc_far.stride(0) > 2 ** 32 and Tc * M * nhk <= 2 * woff
    if T:
        vpool_c, ids_c = oracle.v_rowmajor_to_pool(c["v_codes"], ps)
        vpc, tab = _cu(torch, vpool_c), _cu(torch, ids_c.astype(np.int32))

    desc = ops.make_attn_desc(t["q"], kres_far, nh_k=nhk, M=M, C=C, n_tokens=T, r=r, v_paged=bool(T), page_size=ps if T else 0,
                              n_pages_cap=-(-T // ps), k_codes=kc_far if T else t["k_codes"], v_codes=vpc if T else t["v_codes"])
    assert ops.attn_kernel_kind(desc) == (1 if T else 3)      # the MFMA kernel (row-major K, paged V); T = 0: the tile kernel

    def call(kc, kr, vr):
        if T:
            kw = dict(n_tokens=T, v_page_ids=tab, page_size=ps)
            vc = vpc
        else:
            kw, vc = dict(n_tokens=0), t["v_codes"]
        out = ops.pq_decode_attn(t["q"], kc, vc, kp, vp, kr, vr, r, M=M, C=C, out=torch.full_like(t["q"], float("nan")),
                                 k_new=k_new, v_new=v_new, **kw)
        torch.cuda.synchronize()
        return out

    def twin_call():
        kr, vr = t["k_res"].clone(), t["v_res"].clone()
        return call(t["k_codes"], kr, vr), kr, vr

    (o1, kr1, vr1), (o2, _, _) = twin_call(), twin_call()
    if T:
        _fill_view(kc_far, t["k_codes"])
    _fill_view(kres_far, t["k_res"])
    _fill_view(vres_far, t["v_res"])
    og = call(kc_far if T else t["k_codes"], kres_far, vres_far)
    kres, vres = c["k_res"].copy(), c["v_res"].copy()
    kres[:, :, r], vres[:, :, r] = k_new.cpu().numpy()[:, :, 0], v_new.cpu().numpy()[:, :, 0]
    gold = oracle.decode_attn(c["q"], c["k_codes"], c["v_codes"], c["k_cents"], c["v_cents"], kres, vres, r + 1)
    vs = lambda o, what: _check(o.cpu().numpy(), gold, what)
    vs(o1, "far strides twin")
    np.testing.assert_array_equal(kr1.cpu().numpy(), kres)
    np.testing.assert_array_equal(vr1.cpu().numpy(), vres)
    _same(og, o1, o2, f"decode far strides T={T}", vs)
    assert _bits(kres_far) == _bits(kr1) and _bits(vres_far) == _bits(vr1), "the far window after the append differs from the twin's"
    # nothing else was written: the views back to the sentinel, then both buffers are sentinel
    kres_far.view(torch.int16).fill_(S16)
    vres_far.view(torch.int16).fill_(S16)
    kc_far.fill_(BA.SENTINEL)
    assert BA.only_sentinel(far[0]) and BA.only_sentinel(far[1])


# ------------------------------------------------------------------------------------------------------ 3. chunk attention ---
@pytest.mark.parametrize("n_q", [1, 16])
@pytest.mark.parametrize("i64", [False, True], ids=["i32", "i64"])
def test_chunk_attn_far_pages_and_strides(i64, n_q, env, oracle, far):
    """Chunk attention over far pages; q, k_chunk, v_chunk and out with request 1 past element 2^31.  The pools take the low
    bytes of the buffers' tails only through their pages, the views lie in the 64 spare pages' worth past every page."""
    torch, ops = env
    bs, nhk, npg = BA.TABLE
    d, M, C, G, ps, r, cap, rstart = 128, 64, 256, 4, 64, 40, 64, 50
    nh, T = G * nhk, npg * ps - 7
    st = chunk_state(np.random.RandomState(100 + n_q), bs, nh, nhk, d, M, C, n_q, T, r, cap, rstart, True)
    kpool_c, ids_c = oracle.k_rowmajor_to_pool(st["k_codes"], ps)
    vpool_c, _ = oracle.v_rowmajor_to_pool(st["v_codes"], ps)
    dt = np.int64 if i64 else np.int32
    # far ids that leave the first 16 pages of the pools alone: request 0 of the strided views lies there
    low = 16
    fid = BA.far_ids(bs * nhk * npg + 24, ps * M, 21)
    fid = fid[fid >= low][:bs * nhk * npg]
    tabn = fid[ids_c]
    _assert_far(tabn, ps * M)
    kpc, vpc = _cu(torch, kpool_c), _cu(torch, vpool_c)
    kbig, vbig = _far_pools(torch, far, ps, M, kpc, vpc, fid)
    t = {k: _cu(torch, v) for k, v in st.items() if isinstance(v, np.ndarray)}
    kp, vp = ops.prepare_cents(t["k_cents"], cache=False), ops.prepare_cents(t["v_cents"], cache=False)
    # strided views: request 0 in page 0 of the pools' buffers, request 1 in the bytes past the pools' last page
    page_elems = ps * M // 2
    sb = BA.n_pool(ps * M) * page_elems      # elements from page 0 to the first byte past the pool
    assert sb > 2 ** 31 and sb % 8 == 0
    qn, cn = nh * n_q * d, nhk * n_q * d
    assert qn + cn <= low * page_elems and fid.min() >= low and (qn + cn) * 2 <= BA.FLAT_BYTES - 2 * sb
    mk = lambda flat, off, heads: BA.far_view(flat[2 * off:], (bs, heads, n_q, d), (sb, n_q * d, d, 1), torch.float16)
    q_far, kch_far = mk(far[0], 0, nh), mk(far[0], qn, nhk)
    out_far, vch_far = mk(far[1], 0, nh), mk(far[1], qn, nhk)
    _fill_view(q_far, t["q"]); _fill_view(kch_far, t["k_ch"]); _fill_view(vch_far, t["v_ch"])

    def call(q, kch, vch, kpool, vpool, tab, out):
        res = ops.pq_chunk_attn(q, kch, vch, kpool, vpool, kp, vp, t["k_res"], t["v_res"], r, M=M, C=C, n_tokens=T, resid_start=rstart,
                                k_page_ids=tab, v_page_ids=tab, page_size=ps, out=out)
        torch.cuda.synchronize()
        return res

    tab_c, tab_far = _cu(torch, ids_c.astype(dt)), _cu(torch, tabn.astype(dt))
    new_out = lambda: torch.full((bs, nh, n_q, d), float("nan"), dtype=torch.float16, device="cuda")
    twin = call(t["q"], t["k_ch"], t["v_ch"], kpc, vpc, tab_c, new_out())
    twin2 = call(t["q"], t["k_ch"], t["v_ch"], kpc, vpc, tab_c, new_out())
    got = call(q_far, kch_far, vch_far, kbig, vbig, tab_far, out_far)
    assert got.data_ptr() == out_far.data_ptr()
    gold = chunk_model(oracle, st["q"], st["k_codes"], st["v_codes"], st["k_cents"], st["v_cents"], st["k_win"], st["v_win"],
                       st["k_ch"], st["v_ch"])
    vs = lambda o, what: _check(o.float().cpu().numpy(), gold, what)
    vs(twin, "chunk twin")
    _same(got, twin, twin2, f"chunk far pages i64={i64} n_q={n_q}", vs)
    for v in (q_far, kch_far, out_far, vch_far):
        v.view(torch.int16).fill_(S16)
    BA.assert_only_these_pages(kbig, fid, kpc, far[0], "chunk K pool")
    BA.assert_only_these_pages(vbig, fid, vpc, far[1], "chunk V pool")


@pytest.mark.parametrize("n_q", [1, 16])
def test_chunk_attn_far_window_and_rowmajor_strides(n_q, env, oracle, far):
    """Chunk attention with k_res / v_res whose batch stride puts request 1 past element 2^31 and row-major K and V codes
    whose batch stride puts request 1 past byte 2^32 (the layout of test_decode_far_window_and_rowmajor_k_strides, both
    sides)."""
    torch, ops = env
    bs, nh, nhk, d, M, C, T, r, cap, rstart = 2, 8, 2, 128, 64, 256, 633, 40, 64, 50
    st = chunk_state(np.random.RandomState(200 + n_q), bs, nh, nhk, d, M, C, n_q, T, r, cap, rstart, True)
    t = {k: _cu(torch, v) for k, v in st.items() if isinstance(v, np.ndarray)}
    kp, vp = ops.prepare_cents(t["k_cents"], cache=False), ops.prepare_cents(t["v_cents"], cache=False)
    sb, ksb, woff = BA.far_stride(nhk * cap * d), BA.HI + 64, 1 << 18
    assert nhk * T * M <= 2 * woff
    mk_res = lambda flat: BA.far_view(flat[2 * woff:], (bs, nhk, cap, d), (sb, cap * d, d, 1), torch.float16)
    mk_codes = lambda flat: BA.far_view(flat, (bs, nhk, T, M), (ksb, T * M, M, 1), torch.uint8)
    kres_far, vres_far, kc_far, vc_far = mk_res(far[0]), mk_res(far[1]), mk_codes(far[0]), mk_codes(far[1])
    assert kres_far.stride(0) * 2 > 2 ** 32 and kc_far.stride(0) > 2 ** 32
    _fill_view(kres_far, t["k_res"]); _fill_view(vres_far, t["v_res"]); _fill_view(kc_far, t["k_codes"]); _fill_view(vc_far, t["v_codes"])

    def call(kc, vc, kr, vr):
        out = ops.pq_chunk_attn(t["q"], t["k_ch"], t["v_ch"], kc, vc, kp, vp, kr, vr, r, M=M, C=C, n_tokens=T, resid_start=rstart,
                                out=torch.full((bs, nh, n_q, d), float("nan"), dtype=torch.float16, device="cuda"))
        torch.cuda.synchronize()
        return out

    twin, twin2 = (call(t["k_codes"], t["v_codes"], t["k_res"], t["v_res"]) for _ in range(2))
    got = call(kc_far, vc_far, kres_far, vres_far)
    gold = chunk_model(oracle, st["q"], st["k_codes"], st["v_codes"], st["k_cents"], st["v_cents"], st["k_win"], st["v_win"],
                       st["k_ch"], st["v_ch"])
    vs = lambda o, what: _check(o.float().cpu().numpy(), gold, what)
    vs(twin, "chunk far strides twin")
    _same(got, twin, twin2, f"chunk far window and row-major strides n_q={n_q}", vs)
    # the call reads the views and writes none of them; nothing else in the buffers was written
    assert _bits(kres_far) == _bits(t["k_res"]) and _bits(vres_far) == _bits(t["v_res"])
    assert _bits(kc_far) == _bits(t["k_codes"]) and _bits(vc_far) == _bits(t["v_codes"])
    kres_far.view(torch.int16).fill_(S16); vres_far.view(torch.int16).fill_(S16)
    kc_far.fill_(BA.SENTINEL); vc_far.fill_(BA.SENTINEL)
    assert BA.only_sentinel(far[0]) and BA.only_sentinel(far[1])


def test_chunk_attn_far_pages_ragged(env, oracle, far):
    """One ragged call: per-request lengths and query counts read on the device, far pages."""
    torch, ops = env
    bs, nhk, npg = BA.TABLE
    d, M, C, G, ps, cap, n_q = 128, 64, 256, 4, 64, 64, 16
    nh, T = G * nhk, npg * ps - 7
    lens = [[T, 40, 50, 0], [T - 300, 9, 3, 0]]
    nq = [16, 5]
    st = chunk_state(np.random.RandomState(31), bs, nh, nhk, d, M, C, n_q, T, 0, cap, 0, True)
    kpool_c, ids_c = oracle.k_rowmajor_to_pool(st["k_codes"], ps)
    vpool_c, _ = oracle.v_rowmajor_to_pool(st["v_codes"], ps)
    fid, tab_far = _far_table(torch, ids_c, ps * M, 23)
    kpc, vpc = _cu(torch, kpool_c), _cu(torch, vpool_c)
    kbig, vbig = _far_pools(torch, far, ps, M, kpc, vpc, fid)
    t = {k: _cu(torch, v) for k, v in st.items() if isinstance(v, np.ndarray)}
    kp, vp = ops.prepare_cents(t["k_cents"], cache=False), ops.prepare_cents(t["v_cents"], cache=False)
    dl, dn = torch.tensor(lens, dtype=torch.int32, device="cuda"), torch.tensor(nq, dtype=torch.int32, device="cuda")

    def call(kpool, vpool, tab):
        out = ops.pq_chunk_attn(t["q"], t["k_ch"], t["v_ch"], kpool, vpool, kp, vp, t["k_res"], t["v_res"], 0, M=M, C=C, n_tokens=T,
                                k_page_ids=tab, v_page_ids=tab, page_size=ps, dev_lengths=dl, dev_n_q=dn,
                                out=torch.full((bs, nh, n_q, d), float("nan"), dtype=torch.float16, device="cuda"))
        torch.cuda.synchronize()
        return out

    tab_c = _cu(torch, ids_c.astype(np.int32))
    twin, twin2, got = call(kpc, vpc, tab_c), call(kpc, vpc, tab_c), call(kbig, vbig, tab_far)

    def vs(o, what):
        o = o.float().cpu().numpy()
        for b in range(bs):
            Tb, rb, sb_, _ = lens[b]
            ring = (sb_ + np.arange(rb)) % cap
            g = chunk_model(oracle, st["q"][b:b + 1, :, :nq[b]], st["k_codes"][b:b + 1, :, :Tb], st["v_codes"][b:b + 1, :, :Tb],
                            st["k_cents"], st["v_cents"], st["k_res"][b:b + 1][:, :, ring], st["v_res"][b:b + 1][:, :, ring],
                            st["k_ch"][b:b + 1, :, :nq[b]], st["v_ch"][b:b + 1, :, :nq[b]])
            _check(o[b:b + 1, :, :nq[b]], g, f"{what} request {b}")
            assert not o[b, :, nq[b]:].any(), f"{what}: rows past n_q of request {b}"

    vs(twin, "ragged chunk twin")
    _same(got, twin, twin2, "chunk far pages, ragged", vs)
    BA.assert_only_these_pages(kbig, fid, kpc, far[0], "ragged chunk K pool")
    BA.assert_only_these_pages(vbig, fid, vpc, far[1], "ragged chunk V pool")


# ----------------------------------------------------------------------------------------------------- 4. prompt attention ---
@pytest.mark.parametrize("ragged", [False, True], ids=["dense", "dev_spans"])
@pytest.mark.parametrize("d", [128, 64])
def test_prefill_far_strides(d, ragged, env, far):
    """q, k, v and out as views whose request 1 starts past element 2^31; n = 257; one ragged call with dev_spans."""
    torch, ops = env
    bs, nh, nhk, n = 2, 4, 2, 257
    rs_ = np.random.RandomState(40 + d)
    q, k, v = (rs_.standard_normal((bs, h, n, d)).astype(np.float16) for h in (nh, nhk, nhk))
    qn, kn = nh * n * d, nhk * n * d
    sb = BA.far_stride(qn + 2 * kn)
    assert sb + qn + 2 * kn <= BA.FLAT_BYTES // 2
    mk = lambda flat, off, heads: BA.far_view(flat[2 * off:], (bs, heads, n, d), (sb, n * d, d, 1), torch.float16)
    q_far, k_far, v_far, out_far = mk(far[0], 0, nh), mk(far[0], qn, nhk), mk(far[0], qn + kn, nhk), mk(far[1], 0, nh)
    tq, tk, tv = _cu(torch, q), _cu(torch, k), _cu(torch, v)
    _fill_view(q_far, tq); _fill_view(k_far, tk); _fill_view(v_far, tv)
    spans = [[257, 257, 0, 0], [100, 190, 90, 0]]
    ds = torch.tensor(spans, dtype=torch.int32, device="cuda") if ragged else None

    def call(q_, k_, v_, out):
        o = ops.prefill_attn(q_, k_, v_, out=out, dev_spans=ds)
        torch.cuda.synchronize()
        return o

    new_out = lambda: torch.full((bs, nh, n, d), float("nan"), dtype=torch.float16, device="cuda")
    twin, twin2 = call(tq, tk, tv, new_out()), call(tq, tk, tv, new_out())
    got = call(q_far, k_far, v_far, out_far)
    assert got.data_ptr() == out_far.data_ptr() and out_far.stride(0) > 2 ** 31

    def vs(o, what):
        o = o.float().cpu().numpy()
        if not ragged:
            flash_inputs.check_rows(o, flash_inputs.prefill_gold(q, k, v), what, tag="BIGADDR")
            return
        for b, (nq_, nkv_, p0, _) in enumerate(spans):
            g = flash_inputs.prefill_gold(q[b:b + 1, :, :nq_], k[b:b + 1, :, :nkv_], v[b:b + 1, :, :nkv_], q_pos0=p0)
            flash_inputs.check_rows(o[b:b + 1, :, :nq_], g, f"{what} request {b}", tag="BIGADDR")
            assert not o[b, :, nq_:].any()

    vs(twin, f"prefill d={d} twin")
    _same(got, twin, twin2, f"prefill far strides d={d} ragged={ragged}", vs)
    for vw in (q_far, k_far, v_far, out_far):
        vw.view(torch.int16).fill_(S16)
    assert BA.only_sentinel(far[0]) and BA.only_sentinel(far[1])


# -------------------------------------------------------------------------------------------------- 5. encoders, far pages ---
def _sentinel_pool(torch, n, *tail):
    return torch.full((n, *tail), BA.SENTINEL, dtype=torch.uint8, device="cuda")


@pytest.mark.parametrize("which,bs,nhk,n", [("small", 2, 2, 200), ("bulk", 2, 2, 980)])
def test_encode_into_far_pages(which, bs, nhk, n, env, oracle, far):
    """pq_encode_into, the small (LDS) and the bulk (scalar-operand) kernel, into K pages and transposed V pages named by far
    ids; the twin's pools start as sentinel too, so partly written pages compare byte for byte."""
    torch, ops = env
    from million_amd import _lib as L
    d, M, C, ps, tok0 = 128, 64, 256, 64, 37
    npg = max(BA.TABLE[2], -(-(tok0 + n) // ps))      # small: 4 of 10 pages per row written; bulk: 16 blocks of 64 rows x 4 (b, kv head) = 1024 waves of 4 subspaces
    assert (which == "bulk") == (-(-n // 64) * 4 * 4 * bs * nhk >= 1024)
    c = synth.encode_case(60 + n, bs, nhk, n, d, M, C)
    X, cents = _cu(torch, c["X"]), _cu(torch, c["cents"])
    ids_c = np.arange(bs * nhk * npg).reshape(bs, nhk, npg)
    fid, tab_far = _far_table(torch, ids_c, ps * M, 31)
    tab_c = _cu(torch, ids_c.astype(np.int32))
    kbig, vbig = BA.pool_view(far[0], ps * M, (ps, M)), BA.pool_view(far[1], ps * M, (M, ps))
    kc, vc = _sentinel_pool(torch, ids_c.size, ps, M), _sentinel_pool(torch, ids_c.size, M, ps)
    for kpool, vpool, tab in ((kc, vc, tab_c), (kbig, vbig, tab_far)):
        kw = dict(token_start=tok0, n=n, page_ids=tab, page_size=ps)
        ops.pq_encode_into(X, cents, kpool, layout=L.MILLION_CODES_KPAGES, **kw)
        ops.pq_encode_into(X, cents, vpool, layout=L.MILLION_CODES_VPAGES, **kw)
    torch.cuda.synchronize()
    gold = oracle.pq_encode(c["X"], c["cents"])
    kn, vn = kc.cpu().numpy(), vc.cpu().numpy()
    want_k = np.full((bs, nhk, npg * ps, M), BA.SENTINEL, np.uint8)
    want_k[:, :, tok0:tok0 + n] = gold
    np.testing.assert_array_equal(oracle.pool_to_k_rowmajor(kn, ids_c, npg * ps), want_k)
    np.testing.assert_array_equal(oracle.pool_to_v_rowmajor(vn, ids_c, npg * ps), want_k)
    BA.assert_only_these_pages(kbig, fid, kc, far[0], f"encode {which} K pages")
    BA.assert_only_these_pages(vbig, fid, vc, far[1], f"encode {which} V pages")


def test_encode_into_far_rowmajor_strides(env, oracle, far):
    """Row-major destination whose batch stride (dsb, bytes) and source whose batch stride (xsb, elements) put request 1 past
    byte 2^32."""
    torch, ops = env
    bs, nhk, n, d, M, C, tok0, Tcap = 2, 2, 200, 128, 64, 256, 37, 300
    c = synth.encode_case(91, bs, nhk, n, d, M, C)
    X, cents = _cu(torch, c["X"]), _cu(torch, c["cents"])
    x_far = BA.far_view(far[0], (bs, nhk, n, d), (BA.far_stride(nhk * n * d), n * d, d, 1), torch.float16)
    dst_far = BA.far_view(far[1], (bs, nhk, Tcap, M), (BA.HI + 64, Tcap * M, M, 1), torch.uint8)
    _fill_view(x_far, X)
    twin = _sentinel_pool(torch, bs, nhk, Tcap, M)
    ops.pq_encode_into(X, cents, twin, token_start=tok0, n=n)
    ops.pq_encode_into(x_far, cents, dst_far, token_start=tok0, n=n)
    torch.cuda.synchronize()
    want = np.full((bs, nhk, Tcap, M), BA.SENTINEL, np.uint8)
    want[:, :, tok0:tok0 + n] = oracle.pq_encode(c["X"], c["cents"])
    np.testing.assert_array_equal(twin.cpu().numpy(), want)
    assert _bits(dst_far) == _bits(twin)
    assert _bits(x_far) == _bits(X)
    dst_far.fill_(BA.SENTINEL)
    x_far.view(torch.int16).fill_(S16)
    assert BA.only_sentinel(far[0]) and BA.only_sentinel(far[1])


def test_flush_far_pages(env, oracle, far):
    """pq_flush, one layer: K and V pages named by far ids, device lengths advanced."""
    torch, ops = env
    bs, nhk, d, M, C, ps, cap, npg = 2, 2, 128, 64, 256, 64, 128, 10
    rs_ = np.random.RandomState(8)
    f = lambda *s: rs_.standard_normal(s).astype(np.float16)
    kw_, vw_, ck, cv = f(bs, nhk, cap, d), f(bs, nhk, cap, d), f(M, C, d // M), f(M, C, d // M)
    T0, start = [5 * ps, 9 * ps], [cap - 9, 30]      # per request: the sixth page, the table's last page
    ids_c = np.arange(bs * nhk * npg).reshape(bs, nhk, npg)
    fid, tab_far = _far_table(torch, ids_c, ps * M, 41)
    tab_c = _cu(torch, ids_c.astype(np.int32))
    kbig, vbig = BA.pool_view(far[0], ps * M, (ps, M)), BA.pool_view(far[1], ps * M, (M, ps))
    kc, vc = _sentinel_pool(torch, ids_c.size, ps, M), _sentinel_pool(torch, ids_c.size, M, ps)
    dls = []
    for kpool, vpool, tab in ((kc, vc, tab_c), (kbig, vbig, tab_far)):
        dl = torch.tensor([[T0[b], cap, start[b], 0] for b in range(bs)], dtype=torch.int32, device="cuda")
        ops.pq_flush(_cu(torch, kw_), _cu(torch, vw_), _cu(torch, ck), _cu(torch, cv), kpool, vpool, tab, n=ps, page_size=ps, dev_lengths=dl)
        torch.cuda.synchronize()
        dls.append(dl.cpu().tolist())
    assert dls[0] == dls[1] == [[T0[b] + ps, cap - ps, (start[b] + ps) % cap, 0] for b in range(bs)]
    kn, vn = kc.cpu().numpy(), vc.cpu().numpy()
    for b in range(bs):
        rows = (np.arange(ps) + start[b]) % cap
        gk, gv = oracle.pq_encode(kw_[b:b + 1][:, :, rows], ck), oracle.pq_encode(vw_[b:b + 1][:, :, rows], cv)
        for h in range(nhk):
            np.testing.assert_array_equal(kn[ids_c[b, h, T0[b] // ps]], gk[0, h])
            np.testing.assert_array_equal(vn[ids_c[b, h, T0[b] // ps]], gv[0, h].T)
    written = ids_c[np.arange(bs), :, [T0[b] // ps for b in range(bs)]].ravel()
    rest = np.setdiff1d(ids_c.ravel(), written)
    assert (kn[rest] == BA.SENTINEL).all() and (vn[rest] == BA.SENTINEL).all()
    BA.assert_only_these_pages(kbig, fid, kc, far[0], "flush K pages")
    BA.assert_only_these_pages(vbig, fid, vc, far[1], "flush V pages")


def test_flush_layers_far_layer_strides(env, oracle, far):
    """The multi-layer flush with layer 1 far: the page table's layer stride puts layer 1 past byte 2^32 of the first buffer,
    the windows' layer stride puts layer 1 past element 2^31 of the second (K and V windows side by side).  The pools are
    compact here: the two buffers hold the table and the windows."""
    torch, ops = env
    nl, bs, nhk, d, M, C, ps, cap, npg = 2, 2, 2, 128, 64, 256, 64, 128, 4
    rs_ = np.random.RandomState(9)
    f = lambda *s: rs_.standard_normal(s).astype(np.float16)
    kw_, vw_, ck, cv = f(nl, bs, nhk, cap, d), f(nl, bs, nhk, cap, d), f(M, C, d // M), f(M, C, d // M)
    ids = rs_.permutation(nl * bs * nhk * npg).reshape(nl, bs, nhk, npg).astype(np.int32)
    lens = np.array([[[ps * (1 + (l + b) % 3), cap, (17 * l + 40 * b) % cap, 0] for b in range(bs)] for l in range(nl)], np.int32)
    per = bs * nhk * cap * d
    ls_rows = BA.far_stride(2 * per)
    assert ls_rows % 8 == 0
    k_far = BA.far_view(far[1], (nl, bs, nhk, cap, d), (ls_rows, nhk * cap * d, cap * d, d, 1), torch.float16)
    v_far = BA.far_view(far[1][2 * per:], (nl, bs, nhk, cap, d), (ls_rows, nhk * cap * d, cap * d, d, 1), torch.float16)
    ls_ids = BA.HI // 4 + 16
    ids_far = BA.far_view(far[0], (nl, bs, nhk, npg), (ls_ids, nhk * npg, npg, 1), torch.int32)
    assert ids_far.stride(0) * 4 > 2 ** 32 and k_far.stride(0) > 2 ** 31
    _fill_view(k_far, _cu(torch, kw_)); _fill_view(v_far, _cu(torch, vw_)); _fill_view(ids_far, _cu(torch, ids))
    n_pool = ids.size
    res = []
    # ops.pq_flush wants a contiguous layered table: the far one goes through the C entry, as the twin does
    from million_amd import _lib as L
    lib = L.load()
    for kr, vr, tab in ((_cu(torch, kw_), _cu(torch, vw_), _cu(torch, ids)), (k_far, v_far, ids_far)):
        kpool, vpool = _sentinel_pool(torch, n_pool, ps, M), _sentinel_pool(torch, n_pool, M, ps)
        dl = _cu(torch, lens)
        desc = L.EncodeDesc()
        desc.struct_size = ctypes.sizeof(L.EncodeDesc)
        desc.bs, desc.nh_k, desc.n, desc.d, desc.M, desc.C = bs, nhk, ps, d, M, C
        desc.x_stride_b, desc.x_stride_h, desc.x_stride_n = kr.stride(1), kr.stride(2), kr.stride(3)
        desc.x_row_start, desc.x_row_mod = 0, cap
        desc.dst_layout, desc.page_size, desc.n_pages_cap = L.MILLION_CODES_KPAGES, ps, npg
        desc.dev_lengths = dl.data_ptr()
        ckd, cvd = _cu(torch, ck), _cu(torch, cv)
        L.check(lib.million_pq_flush_layers(ctypes.byref(desc), kr.data_ptr(), vr.data_ptr(), ckd.data_ptr(), cvd.data_ptr(),
                                            kpool.data_ptr(), vpool.data_ptr(), tab.data_ptr(), dl.data_ptr(), cap, 0, nl,
                                            kr.stride(0), tab.stride(0), dl.stride(0), 1, torch.cuda.current_stream().cuda_stream),
                "million_pq_flush_layers")
        torch.cuda.synchronize()
        res.append((kpool, vpool, dl))
    (kc, vc, dlc), (kf, vf, dlf) = res
    assert _bits(kf) == _bits(kc) and _bits(vf) == _bits(vc) and _bits(dlf) == _bits(dlc)
    kn, vn = kc.cpu().numpy(), vc.cpu().numpy()
    written = []
    for l in range(nl):
        for b in range(bs):
            T0, _, st, _ = lens[l, b]
            rows = (np.arange(ps) + st) % cap
            gk, gv = oracle.pq_encode(kw_[l, b:b + 1][:, :, rows], ck), oracle.pq_encode(vw_[l, b:b + 1][:, :, rows], cv)
            for h in range(nhk):
                pid = ids[l, b, h, T0 // ps]
                written.append(pid)
                np.testing.assert_array_equal(kn[pid], gk[0, h])
                np.testing.assert_array_equal(vn[pid], gv[0, h].T)
            assert dlc.cpu().numpy()[l, b].tolist() == [T0 + ps, cap - ps, (st + ps) % cap, 0]
    rest = np.setdiff1d(np.arange(n_pool), written)
    assert (kn[rest] == BA.SENTINEL).all() and (vn[rest] == BA.SENTINEL).all()
    # the far inputs are untouched, and nothing else in the buffers was written
    assert _bits(k_far) == _bits(_cu(torch, kw_)) and _bits(ids_far) == _bits(_cu(torch, ids))
    k_far.view(torch.int16).fill_(S16); v_far.view(torch.int16).fill_(S16)
    ids_far.view(torch.int32).fill_(int.from_bytes(bytes([BA.SENTINEL]) * 4, "little", signed=True))
    assert BA.only_sentinel(far[0]) and BA.only_sentinel(far[1])


def test_store_ragged_far_pages(env, oracle, far):
    """pq_store_ragged: window rows and new rows of a ragged batch encoded behind each request's tokens, into far pages."""
    torch, ops = env
    bs, nhk, d, M, C, ps, cap, npg, n = 2, 2, 128, 64, 256, 64, 64, 10, 70
    rs_ = np.random.RandomState(12)
    f = lambda *s: rs_.standard_normal(s).astype(np.float16)
    kn_, vn_, kr_, vr_, ck, cv = f(bs, nhk, n, d), f(bs, nhk, n, d), f(bs, nhk, cap, d), f(bs, nhk, cap, d), f(M, C, d // M), f(M, C, d // M)
    lens, dn = [[3 * ps + 11, 40, 50, 0], [7 * ps, 9, 3, 0]], [70, 33]
    ids_c = np.arange(bs * nhk * npg).reshape(bs, nhk, npg)
    fid, tab_far = _far_table(torch, ids_c, ps * M, 51)
    tab_c = _cu(torch, ids_c.astype(np.int32))
    kbig, vbig = BA.pool_view(far[0], ps * M, (ps, M)), BA.pool_view(far[1], ps * M, (M, ps))
    kc, vc = _sentinel_pool(torch, ids_c.size, ps, M), _sentinel_pool(torch, ids_c.size, M, ps)
    kp, vp = ops.prepare_cents(_cu(torch, ck), cache=False), ops.prepare_cents(_cu(torch, cv), cache=False)
    dls = []
    for kpool, vpool, tab in ((kc, vc, tab_c), (kbig, vbig, tab_far)):
        dl = torch.tensor(lens, dtype=torch.int32, device="cuda")
        ops.pq_store_ragged(_cu(torch, kn_), _cu(torch, vn_), _cu(torch, kr_), _cu(torch, vr_), kp, vp, kpool, vpool, tab, dl,
                            torch.tensor(dn, dtype=torch.int32, device="cuda"), M=M, C=C, page_size=ps)
        torch.cuda.synchronize()
        dls.append(dl.cpu().tolist())
    assert dls[0] == dls[1] == [[lens[b][0] + lens[b][1] + dn[b], 0, 0, 0] for b in range(bs)]
    krow = oracle.pool_to_k_rowmajor(kc.cpu().numpy(), ids_c, npg * ps)
    vrow = oracle.pool_to_v_rowmajor(vc.cpu().numpy(), ids_c, npg * ps)
    for b in range(bs):
        T, r, st, _ = lens[b]
        ring = (st + np.arange(r)) % cap
        xs_k = np.concatenate([kr_[b:b + 1][:, :, ring], kn_[b:b + 1, :, :dn[b]]], axis=2)
        xs_v = np.concatenate([vr_[b:b + 1][:, :, ring], vn_[b:b + 1, :, :dn[b]]], axis=2)
        np.testing.assert_array_equal(krow[b:b + 1, :, T:T + r + dn[b]], oracle.pq_encode(xs_k, ck))
        np.testing.assert_array_equal(vrow[b:b + 1, :, T:T + r + dn[b]], oracle.pq_encode(xs_v, cv))
        assert (krow[b, :, :T] == BA.SENTINEL).all() and (krow[b, :, T + r + dn[b]:] == BA.SENTINEL).all()
    BA.assert_only_these_pages(kbig, fid, kc, far[0], "store_ragged K pages")
    BA.assert_only_these_pages(vbig, fid, vc, far[1], "store_ragged V pages")


def test_window_commit_far_pages(env, oracle, far):
    """window_commit with and without dev_rows: a request whose window overflows has its oldest page encoded into a far page,
    the rest of the new rows go to the ring, the lengths advance; the other request only appends."""
    torch, ops = env
    from tests import verify_model as VM
    nl, bs, nhk, d, M, C, ps, cap, npg, nb = 2, 2, 2, 128, 64, 256, 64, 64, 5, 12
    rs_ = np.random.RandomState(14)
    f = lambda *s: rs_.standard_normal(s).astype(np.float16)
    kn_, vn_, kr_, vr_, ck, cv = f(nl, bs, nhk, nb, d), f(nl, bs, nhk, nb, d), f(nl, bs, nhk, cap, d), f(nl, bs, nhk, cap, d), f(M, C, d // M), f(M, C, d // M)
    lens = np.array([[[3 * ps, 60, 50, 0], [ps, 20, 7, 0]]] * nl, np.int32)
    a = [12, 5]
    ids_c = np.arange(nl * bs * nhk * npg).reshape(nl, bs, nhk, npg)
    fid = BA.far_ids(ids_c.size, ps * M, 61)
    _assert_far(fid[ids_c].reshape(nl * bs, nhk * npg), ps * M)      # per (layer, request): the page a commit writes is one of these
    kbig, vbig = BA.pool_view(far[0], ps * M, (ps, M)), BA.pool_view(far[1], ps * M, (M, ps))
    kp, vp = ops.prepare_cents(_cu(torch, ck), cache=False), ops.prepare_cents(_cu(torch, cv), cache=False)
    for rows in (None, np.array([[11, 0, 3, 3, 7, 1, 2, 9, 10, 4, 5, 6], [2, 2, 0, 8, 11, 0, 0, 0, 0, 0, 0, 0]], np.int32)):
        for fl in far:
            fl.fill_(BA.SENTINEL)
        res = []
        kc, vc = _sentinel_pool(torch, ids_c.size, ps, M), _sentinel_pool(torch, ids_c.size, M, ps)
        for kpool, vpool, tab in ((kc, vc, ids_c), (kbig, vbig, fid[ids_c])):
            kr, vr, dl = _cu(torch, kr_), _cu(torch, vr_), _cu(torch, lens)
            ops.window_commit(_cu(torch, kn_), _cu(torch, vn_), kr, vr, kp, vp, kpool, vpool, _cu(torch, tab.astype(np.int32)), dl,
                              torch.tensor(a, dtype=torch.int32, device="cuda"), M=M, C=C, n_bound=nb,
                              **({} if rows is None else dict(dev_rows=_cu(torch, rows))))
            torch.cuda.synchronize()
            res.append((kr, vr, dl))
        (krc, vrc, dlc), (krf, vrf, dlf) = res
        kn, vn = kc.cpu().numpy(), vc.cpu().numpy()
        written = []
        for l in range(nl):
            for b in range(bs):
                T, r, st, _ = lens[l, b].tolist()
                pick = list(range(a[b])) if rows is None else [min(max(int(x), 0), nb - 1) for x in rows[b][:a[b]]]
                T2, r2, st2, coded, ring = VM.commit_sequential(T, r, st, a[b], ps, cap, rows=[("n", i) for i in pick])
                assert dlc.cpu().numpy()[l, b].tolist() == [T2, r2, st2, 0]
                src = lambda e, win, new: (win[l, b:b + 1, :, (st + e[1]) % cap] if e[0] == "w" else new[l, b:b + 1, :, e[1]])
                for slot, e in VM.live_ring(ring, r2, st2, cap).items():
                    np.testing.assert_array_equal(krc.cpu().numpy()[l, b, :, slot], src(e, kr_, kn_)[0])
                    np.testing.assert_array_equal(vrc.cpu().numpy()[l, b, :, slot], src(e, vr_, vn_)[0])
                if coded:
                    toks = sorted(coded)
                    assert toks == list(range(T, T + ps)) and T % ps == 0
                    gk = oracle.pq_encode(np.stack([src(coded[t], kr_, kn_) for t in toks], axis=2), ck)
                    gv = oracle.pq_encode(np.stack([src(coded[t], vr_, vn_) for t in toks], axis=2), cv)
                    for h in range(nhk):
                        pid = ids_c[l, b, h, T // ps]
                        written.append(pid)
                        np.testing.assert_array_equal(kn[pid], gk[0, h])
                        np.testing.assert_array_equal(vn[pid], gv[0, h].T)
        assert len(written) == nl * nhk
        rest = np.setdiff1d(ids_c.ravel(), written)
        assert (kn[rest] == BA.SENTINEL).all() and (vn[rest] == BA.SENTINEL).all()
        assert _bits(krf) == _bits(krc) and _bits(vrf) == _bits(vrc) and _bits(dlf) == _bits(dlc)
        BA.assert_only_these_pages(kbig, fid, kc, far[0], "window_commit K pages")
        BA.assert_only_these_pages(vbig, fid, vc, far[1], "window_commit V pages")


# ---------------------------------------------------------------------------------------------- 6. cache_fork, cache_swap ---
# Four layers of tables and windows inside the far buffers, one layer stride S for both (bytes): layer 0 at the base, layers 1
# and 2 inside the pools' span (the far ids keep clear of those bytes), layer 3 past the pools' last page - past byte 2^32.
L_N, L_BS, L_NHK, L_D, L_M, L_PS, L_CAP, L_NPG = 4, 2, 2, 128, 64, 64, 128, 10
L_B = L_PS * L_M
L_WIN = L_BS * L_NHK * L_CAP * L_D * 2                       # bytes of a layer's window
L_IDS_OFF, L_RES = L_WIN + 65536, 2 * L_WIN                  # the layer's table lies behind its window; bytes kept free per layer
L_S = -(-(BA.n_pool(L_B) * L_B) // (3 * 16)) * 16            # 3 S >= the pools' bytes; a multiple of 16


def _layer_clear_ids(ids, spare, seed):
    """Compact id -> far id, clear of the layers' bytes; dealt in table order, so that every table row has pages in every band."""
    n = ids.size + spare.size
    fid = BA.far_ids(n + 64, L_B, seed)
    lo, hi = fid * L_B, fid * L_B + L_B
    clear = np.ones(len(fid), bool)
    for l in range(L_N):
        clear &= ~((lo < l * L_S + L_RES) & (hi > l * L_S))
    fid = fid[clear][:n]
    assert len(fid) == n
    c2f = np.empty(n, np.int64)
    c2f[np.concatenate([ids.ravel(), spare.ravel()])] = fid
    return c2f


def _layered_host(seed, T_rows):
    """Compact arrays [ids, k_pool, v_pool, k_res, v_res, lengths] (windows as int16 bits) and the ids no table names."""
    rs_ = np.random.RandomState(seed)
    n_tab = L_N * L_BS * L_NHK * L_NPG
    n_pool = n_tab + 12
    perm = rs_.permutation(n_pool)
    ids = perm[:n_tab].reshape(L_N, L_BS, L_NHK, L_NPG).astype(np.int32)
    kp = rs_.randint(0, 256, (n_pool, L_PS, L_M)).astype(np.uint8)
    vp = rs_.randint(0, 256, (n_pool, L_M, L_PS)).astype(np.uint8)
    kr = rs_.standard_normal((L_N, L_BS, L_NHK, L_CAP, L_D)).astype(np.float16).view(np.int16)
    vr = rs_.standard_normal((L_N, L_BS, L_NHK, L_CAP, L_D)).astype(np.float16).view(np.int16)
    ln = rs_.randint(1, 200, (L_N, L_BS, 4)).astype(np.int32)
    for b, row in T_rows.items():
        ln[:, b] = row
    return [ids, kp, vp, kr, vr, ln], perm[n_tab:].astype(np.int32)


def _layered_dev(torch, host):
    dev = [_cu(torch, a) for a in host]
    dev[3], dev[4] = dev[3].view(torch.float16), dev[4].view(torch.float16)
    return dev


def _layered_far(torch, far, host, c2f):
    """The same state with the pools scattered to far ids, the table and the windows as far-strided views of the buffers."""
    assert L_S % 16 == 0 and 3 * L_S >= BA.n_pool(L_B) * L_B and 3 * L_S + L_RES <= BA.FLAT_BYTES and 2 * L_S > 2 ** 31
    ids, kp, vp, kr, vr, ln = host
    kbig, vbig = BA.pool_view(far[0], L_B, (L_PS, L_M)), BA.pool_view(far[1], L_B, (L_M, L_PS))
    BA.scatter_pool(kbig, _cu(torch, kp), c2f)
    BA.scatter_pool(vbig, _cu(torch, vp), c2f)
    wshape, wstr = (L_N, L_BS, L_NHK, L_CAP, L_D), (L_S // 2, L_NHK * L_CAP * L_D, L_CAP * L_D, L_D, 1)
    kr_f, vr_f = BA.far_view(far[0], wshape, wstr, torch.float16), BA.far_view(far[1], wshape, wstr, torch.float16)
    ids_f = BA.far_view(far[0][L_IDS_OFF:], ids.shape, (L_S // 4, L_NHK * L_NPG, L_NPG, 1), torch.int32)
    kr_f.copy_(_cu(torch, kr).view(torch.float16))
    vr_f.copy_(_cu(torch, vr).view(torch.float16))
    ids_f.copy_(_cu(torch, c2f[ids].astype(np.int32)))
    assert ids_f.stride(0) * 4 == kr_f.stride(0) * 2 == L_S
    return [ids_f, kbig, vbig, kr_f, vr_f, _cu(torch, ln)]


def _layered_check(torch, far, dev_far, want, c2f, what):
    """The far state equals the model's (= the twin's) state: table through the id map, windows, lengths, every page of the
    pools through the map - and nothing else in the buffers was written."""
    ids_f, kbig, vbig, kr_f, vr_f, ln_f = dev_far
    assert np.array_equal(ids_f.cpu().numpy(), c2f[want[0]]), f"{what}: table"
    assert _bits(kr_f.view(torch.int16)) == want[3].tobytes() and _bits(vr_f.view(torch.int16)) == want[4].tobytes(), f"{what}: windows"
    assert np.array_equal(ln_f.cpu().numpy(), want[5]), f"{what}: lengths"
    kr_f.view(torch.int16).fill_(S16); vr_f.view(torch.int16).fill_(S16)
    ids_f.fill_(int.from_bytes(bytes([BA.SENTINEL]) * 4, "little", signed=True))
    BA.assert_only_these_pages(kbig, c2f, _cu(torch, want[1]), far[0], f"{what}: K pool")
    BA.assert_only_these_pages(vbig, c2f, _cu(torch, want[2]), far[1], f"{what}: V pool")


def _twin_equals(dev, want, what):
    for name, w, g in zip(("page_ids", "k_pool", "v_pool", "k_resid", "v_resid", "lengths"), want, dev):
        gn = g.cpu().numpy()
        gn = gn.view(np.int16) if gn.dtype == np.float16 else gn
        assert np.array_equal(gn, w), f"{what}: the twin's {name} differs from the model"


@pytest.mark.parametrize("mode", ["copy", "share"])
def test_cache_fork_far(mode, env, far):
    """million_cache_fork, slot 0 -> slot 1 in four layers: every id far, the table's and the windows' layer stride far."""
    torch, ops = env
    from tests import cache_fork_model as FM
    T = (L_NPG - 1) * L_PS + 20
    host, spare = _layered_host(70, {0: (T, 60, 100, 0x7EADBEEF)})
    dst = np.array([1], np.int32)
    tail = spare[:L_N * L_NHK].reshape(1, L_N, L_NHK).copy() if mode == "share" else None
    want = [a.copy() for a in host]
    copied = FM.fork(*want, dst, tail, src=0, mode=FM.SHARE if mode == "share" else FM.COPY, n_pages_bound=L_NPG)
    assert len(copied) == (1 if mode == "share" else L_NPG) * L_N * L_NHK
    c2f = _layer_clear_ids(host[0], spare, 71)
    tabf = c2f[host[0]]
    _assert_far(tabf, L_B)      # source and destination rows alike: pages in every band
    twin = _layered_dev(torch, host)
    dev_far = _layered_far(torch, far, host, c2f)
    for dev, tl in ((twin, tail), (dev_far, None if tail is None else c2f[tail].astype(np.int32))):
        ops.cache_fork(*dev, _cu(torch, dst), _cu(torch, tl), src=0, share=mode == "share", n_pages_bound=L_NPG)
        torch.cuda.synchronize()
    _twin_equals(twin, want, f"fork {mode}")
    _layered_check(torch, far, dev_far, want, c2f, f"fork {mode}")


def test_cache_swap_far(env, far):
    """million_cache_swap: pack two requests from far pages, far tables and far windows into a blob - the twin's blob, byte for
    byte - then unpack the blob into other far ids of another cache state."""
    torch, ops = env
    from million_amd import _lib as L
    from tests import cache_swap_model as SM
    table = np.array([[0, (L_NPG - 1) * L_PS + 20, 60, 100], [1, 3 * L_PS, L_CAP, 5]], np.int32)
    src, spare = _layered_host(80, {})
    sizes = [L_N * L_NHK * SM.row_bytes(T, r, L_PS, L_M, L_D) for _, T, r, _ in table.tolist()]
    offs = np.concatenate([[0], np.cumsum(sizes)])[:-1].astype(np.int64)
    total, guard = int(np.sum(sizes)), 256
    blob0 = np.full(total + guard, 0x3C, np.uint8)
    want_blob = blob0.copy()
    SM.pack(*src[:5], table, offs, want_blob[:total])
    c2f = _layer_clear_ids(src[0], spare, 81)
    _assert_far(c2f[src[0]], L_B)
    blobs = []
    for dev in (_layered_dev(torch, src), _layered_far(torch, far, src, c2f)):
        blob = _cu(torch, blob0)
        ops.cache_swap(L.MILLION_SWAP_PACK, *dev, _cu(torch, table), _cu(torch, offs), blob[:total])
        torch.cuda.synchronize()
        blobs.append(blob.cpu().numpy())
        last = dev
    assert np.array_equal(blobs[0], want_blob), "the twin's blob differs from the model's"
    assert np.array_equal(blobs[1], want_blob), "the blob packed from far pages differs from the twin's"
    _layered_check(torch, far, last, src, c2f, "swap pack (nothing but the blob is written)")
    # unpack: entry i into slot 1 - i of another state, through another id map
    for fl in far:
        fl.fill_(BA.SENTINEL)
    t2 = table.copy()
    t2[:, 0] = 1 - t2[:, 0]
    dst, spare2 = _layered_host(90, {})
    want = [a.copy() for a in dst]
    SM.unpack(*want, t2, offs, want_blob[:total])
    c2f2 = _layer_clear_ids(dst[0], spare2, 91)
    _assert_far(c2f2[dst[0]], L_B)
    assert not np.array_equal(c2f, c2f2)
    twin, dev_far = _layered_dev(torch, dst), _layered_far(torch, far, dst, c2f2)
    for dev in (twin, dev_far):
        ops.cache_swap(L.MILLION_SWAP_UNPACK, *dev, _cu(torch, t2), _cu(torch, offs), _cu(torch, want_blob)[:total])
        torch.cuda.synchronize()
    _twin_equals(twin, want, "swap unpack")
    _layered_check(torch, far, dev_far, want, c2f2, "swap unpack")
