"""GPU tests of chunk attention (million_pq_chunk_attn, ops.pq_chunk_attn) and of the caches' extend(): a block of new query
tokens against [PQ codes; residual window; the block itself, causally].  fp64 model here: oracle.pq_decode for the
dequantisation, numpy for the attention.  Bars: rel-L2 < 1e-3 and mean-abs < 1e-3 (test_gpu_parity.py), outputs finite."""
import zlib

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

REL_TOL = 1e-3
MEAN_ABS_TOL = 1e-3


@pytest.fixture(scope="module")
def env():
    import torch
    assert torch.cuda.is_available(), "GPU tests need an MI355X"
    from million_amd import ops, _lib
    _lib.load()
    return torch, ops


def _check(out, gold, what=""):
    out = np.asarray(out, dtype=np.float64)
    gold = np.asarray(gold, dtype=np.float64)
    assert np.isfinite(out).all(), f"{what}: non-finite output"
    rel = np.linalg.norm(out - gold) / max(np.linalg.norm(gold), 1e-30)
    mae = np.abs(out - gold).mean()
    assert rel < REL_TOL and mae < MEAN_ABS_TOL, f"{what}: rel={rel:.3e} mean_abs={mae:.3e}"
    return rel


def model(oracle, q, k_codes, v_codes, k_cents, v_cents, k_win, v_win, k_ch, v_ch, rows=None):
    """fp64: q (bs, nh, n_q, d); codes (bs, nh_k, T, M); window rows in ring order (bs, nh_k, r, d); chunk (bs, nh_k, n_c, d)
    or None.  rows: query rows to evaluate (default all)."""
    bs, nh, n_q, d = q.shape
    nhk = k_win.shape[1]
    G = nh // nhk
    T = k_codes.shape[2]
    parts_k = [oracle.pq_decode(k_codes, k_cents).astype(np.float64)] if T else []
    parts_v = [oracle.pq_decode(v_codes, v_cents).astype(np.float64)] if T else []
    parts_k.append(k_win.astype(np.float64))
    parts_v.append(v_win.astype(np.float64))
    n_c = 0
    if k_ch is not None:
        parts_k.append(k_ch.astype(np.float64))
        parts_v.append(v_ch.astype(np.float64))
        n_c = k_ch.shape[2]
    K, V = np.concatenate(parts_k, axis=2), np.concatenate(parts_v, axis=2)
    n_past = K.shape[2] - n_c
    rows = np.arange(n_q) if rows is None else np.asarray(rows)
    out = np.zeros((bs, nh, len(rows), d))
    for b in range(bs):
        for h in range(nh):
            s = q[b, h, rows].astype(np.float64) @ K[b, h // G].T / np.sqrt(d)
            if n_c:
                j = np.arange(n_c)[None, :]
                s[:, n_past:] = np.where(j <= rows[:, None], s[:, n_past:], -np.inf)
            if s.shape[1] == 0:
                continue
            m = s.max(axis=1, keepdims=True)
            p = np.exp(s - m)
            out[b, h] = (p @ V[b, h // G]) / p.sum(axis=1, keepdims=True)
    return out


def _state(rs_, bs, nh, nhk, d, M, C, n_q, T, r, cap, rstart, chunk, T_cap=None):
    f = lambda *s: rs_.standard_normal(s).astype(np.float16)
    T_cap = T if T_cap is None else T_cap
    st = dict(q=f(bs, nh, n_q, d), k_cents=f(M, C, d // M), v_cents=f(M, C, d // M),
              k_codes=rs_.randint(0, C, (bs, nhk, T, M)).astype(np.uint8),
              v_codes=rs_.randint(0, C, (bs, nhk, T, M)).astype(np.uint8),
              k_res=f(bs, nhk, cap, d), v_res=f(bs, nhk, cap, d), r=r, rs=rstart)
    st["k_ch"], st["v_ch"] = (f(bs, nhk, n_q, d), f(bs, nhk, n_q, d)) if chunk else (None, None)
    ring = (rstart + np.arange(r)) % cap
    st["k_win"], st["v_win"] = st["k_res"][:, :, ring], st["v_res"][:, :, ring]
    return st


def _run(torch, ops, oracle, st, M, C, layout="rowmajor", ps=64, i64=False, poison=False, extra_pages=3):
    dev = lambda a: None if a is None else torch.from_numpy(np.ascontiguousarray(a)).cuda()
    T = st["k_codes"].shape[2]
    k_res, v_res = st["k_res"].copy(), st["v_res"].copy()
    if poison:      # window rows outside the valid span of the ring hold NaN
        cap = k_res.shape[2]
        valid = set(((st["rs"] + np.arange(st["r"])) % cap).tolist())
        bad = [i for i in range(cap) if i not in valid]
        k_res[:, :, bad] = np.float16("nan")
        v_res[:, :, bad] = np.float16("nan")
    kp = ops.prepare_cents(dev(st["k_cents"]), cache=False)
    vp = ops.prepare_cents(dev(st["v_cents"]), cache=False)
    kw = {}
    if layout == "rowmajor":
        pad = 64 if poison else 0
        kc = np.full(st["k_codes"].shape[:2] + (T + pad, M), 0xFF, np.uint8)
        vc = kc.copy()
        kc[:, :, :T], vc[:, :, :T] = st["k_codes"], st["v_codes"]
        k_codes, v_codes = dev(kc), dev(vc)
    else:
        vpool, ids = oracle.v_rowmajor_to_pool(st["v_codes"], ps)
        kpool, _ = oracle.k_rowmajor_to_pool(st["k_codes"], ps)
        if poison:      # the last page's tail past T and every unused pool page hold 0xFF
            n_pg = ids.shape[2]
            tail = T - (n_pg - 1) * ps
            if T and tail < ps:
                for pid in ids[:, :, -1].ravel():
                    kpool[pid, tail:, :] = 0xFF
                    vpool[pid, :, tail:] = 0xFF
        # unused pages, then a shuffle: physical page order must not matter
        kpool = np.concatenate([kpool, np.full((extra_pages,) + kpool.shape[1:], 0xFF if poison else 0, np.uint8)])
        vpool = np.concatenate([vpool, np.full((extra_pages,) + vpool.shape[1:], 0xFF if poison else 0, np.uint8)])
        perm = np.random.RandomState(5).permutation(kpool.shape[0])
        inv = np.argsort(perm)
        kpool, vpool, ids = kpool[perm], vpool[perm], inv[ids]
        ids = ids.reshape(ids.shape[0], ids.shape[1], -1)
        if ids.shape[2] == 0:
            ids = np.zeros(ids.shape[:2] + (1,), np.int64)
        ids_t = dev(ids.astype(np.int64 if i64 else np.int32))
        k_codes, v_codes = dev(kpool), dev(vpool)
        kw = dict(k_page_ids=ids_t, v_page_ids=ids_t, page_size=ps)
    out = ops.pq_chunk_attn(dev(st["q"]), dev(st["k_ch"]), dev(st["v_ch"]), k_codes, v_codes, kp, vp, dev(k_res), dev(v_res),
                            st["r"], M=M, C=C, n_tokens=T, resid_start=st["rs"], **kw)
    torch.cuda.synchronize()
    return out.float().cpu().numpy()


# (d, M, C, G, n_q, T, window, chunk, layout, ps, i64)
GRID = [
    (128, 64, 256, 4, 16, 1000, "17", True, "rowmajor", 0, False),
    (128, 64, 256, 8, 1, 4097, "wrap", False, "paged", 64, True),
    (128, 64, 128, 1, 65, 63, "0", True, "paged", 32, False),
    (128, 32, 256, 4, 3, 64, "wrap", True, "rowmajor", 0, False),
    (128, 32, 128, 8, 257, 1, "17", True, "paged", 128, True),
    (128, 16, 256, 1, 16, 4097, "0", False, "paged", 32, False),
    (128, 16, 128, 4, 65, 1000, "wrap", True, "rowmajor", 0, False),
    (64, 64, 256, 8, 3, 1000, "17", True, "paged", 64, False),
    (64, 64, 128, 4, 257, 64, "wrap", False, "rowmajor", 0, False),
    (64, 32, 256, 1, 1, 0, "17", True, "rowmajor", 0, False),
    (64, 32, 128, 8, 16, 4097, "0", True, "paged", 128, True),
    (64, 16, 256, 4, 65, 63, "wrap", True, "paged", 32, True),
    (64, 16, 128, 1, 257, 1000, "17", False, "rowmajor", 0, False),
    (128, 64, 256, 4, 65, 0, "0", True, "rowmajor", 0, False),           # a prompt on an empty cache: the chunk only
    (128, 64, 256, 4, 3, 0, "0", False, "rowmajor", 0, False),           # nothing to attend to: out = 0
]


@pytest.mark.parametrize("case", GRID, ids=["-".join(map(str, c)) for c in GRID])
def test_chunk_attn_parity_grid(case, env, oracle):
    torch, ops = env
    d, M, C, G, n_q, T, win, chunk, layout, ps, i64 = case
    nhk = 2
    r, rstart = {"0": (0, 0), "17": (17, 0), "wrap": (100, 90)}[win]
    st = _state(np.random.RandomState(zlib.crc32(repr(case).encode())), 1, G * nhk, nhk, d, M, C, n_q, T, r, 128, rstart, chunk)
    out = _run(torch, ops, oracle, st, M, C, layout, ps, i64)
    gold = model(oracle, st["q"], st["k_codes"], st["v_codes"], st["k_cents"], st["v_cents"], st["k_win"], st["v_win"],
                 st["k_ch"], st["v_ch"])
    if T == 0 and r == 0 and not chunk:
        assert np.all(out == 0)
        return
    _check(out, gold, str(case))


@pytest.mark.parametrize("d,M,C,layout", [(128, 64, 128, "paged"), (128, 32, 256, "rowmajor"), (64, 64, 128, "rowmajor"),
                                          (64, 16, 256, "paged")])
def test_chunk_attn_total(d, M, C, layout, env, oracle):
    """0xFF code bytes past T / in unused pages (an invalid code at C = 128) and NaN window rows outside the ring's valid
    span must not reach a product."""
    torch, ops = env
    st = _state(np.random.RandomState(11), 2, 8, 2, d, M, C, 33, 1000, 40, 64, 50, True)
    out = _run(torch, ops, oracle, st, M, C, layout, 64, False, poison=True)
    gold = model(oracle, st["q"], st["k_codes"], st["v_codes"], st["k_cents"], st["v_cents"], st["k_win"], st["v_win"],
                 st["k_ch"], st["v_ch"])
    _check(out, gold, "total")


def test_chunk_attn_matches_decode_append(env, oracle):
    """n_q = n_c = 1 is a decode step: the same output as the fused append + attention launch."""
    torch, ops = env
    d, M, C = 128, 64, 256
    st = _state(np.random.RandomState(3), 2, 32, 8, d, M, C, 1, 3000, 30, 128, 120, True)
    out = _run(torch, ops, oracle, st, M, C, "paged", 64, False)
    dev = lambda a: torch.from_numpy(np.ascontiguousarray(a)).cuda()
    vpool, ids = oracle.v_rowmajor_to_pool(st["v_codes"], 64)
    kpool, _ = oracle.k_rowmajor_to_pool(st["k_codes"], 64)
    kp = ops.prepare_cents(dev(st["k_cents"]), cache=False)
    vp = ops.prepare_cents(dev(st["v_cents"]), cache=False)
    ids_t = dev(ids.astype(np.int32))
    ref = ops.pq_decode_attn(dev(st["q"]), dev(kpool), dev(vpool), kp, vp, dev(st["k_res"]), dev(st["v_res"]), st["r"], M=M, C=C,
                             n_tokens=3000, resid_start=st["rs"], k_page_ids=ids_t, v_page_ids=ids_t, page_size=64,
                             k_new=dev(st["k_ch"]), v_new=dev(st["v_ch"]))
    torch.cuda.synchronize()
    _check(out, ref.float().cpu().numpy(), "chunk vs decode-append")


@pytest.mark.parametrize("bs,nh,nhk,M,n_q,T", [(1, 8, 2, 32, 16, 131072), (4, 32, 8, 64, 64, 32768), (1, 8, 2, 64, 2048, 8192)],
                         ids=["T128k-M32", "bs4-T32k", "nq2048"])
def test_chunk_attn_long_and_wide(bs, nh, nhk, M, n_q, T, env, oracle):
    torch, ops = env
    st = _state(np.random.RandomState(T % 1000), bs, nh, nhk, 128, M, 256, n_q, T, 77, 128, 100, True)
    out = _run(torch, ops, oracle, st, M, 256, "paged", 64, False)
    rows = np.unique(np.r_[0, 1, n_q - 1, np.random.RandomState(1).randint(0, n_q, 6)])
    gold = model(oracle, st["q"], st["k_codes"], st["v_codes"], st["k_cents"], st["v_cents"], st["k_win"], st["v_win"],
                 st["k_ch"], st["v_ch"], rows=rows)
    _check(out[:, :, rows], gold, "long")


# ---------------------------------------------------------------- caches ------------------------------------------------
def _paged_cache(torch, rs_, bs, nhk=2, d=128, M=64, ps=32, cap=64):
    from million_amd.pq_cache import PagedPQCache
    cache = PagedPQCache(bs=bs, nh=4 * nhk, num_key_value_heads=nhk, M=M, layer_num=1, d=d, page_size=ps,
                         extended_residual_size=cap, max_tokens=2048, device="cuda")
    kc = rs_.standard_normal((M, 256, d // M)).astype(np.float16)
    vc = rs_.standard_normal((M, 256, d // M)).astype(np.float16)
    cache.set_cent(torch.from_numpy(kc).cuda(), torch.from_numpy(vc).cuda())
    return cache, kc, vc


def _decode_gold(oracle, q, Kall, Vall, kc, vc, T, r, cap):
    kcodes, vcodes = oracle.pq_encode(Kall[:, :, :T], kc), oracle.pq_encode(Vall[:, :, :T], vc)
    bs, nhk, _, d = Kall.shape
    kres = np.zeros((bs, nhk, cap, d), np.float16)
    vres = np.zeros((bs, nhk, cap, d), np.float16)
    kres[:, :, :r], vres[:, :, :r] = Kall[:, :, T:T + r], Vall[:, :, T:T + r]
    return oracle.decode_attn(q, kcodes, vcodes, kc, vc, kres, vres, r)


@pytest.mark.parametrize("ahead", [False, True], ids=["plain", "encode-ahead"])
def test_paged_cache_extend(ahead, env, oracle):
    torch, ops = env
    rs_ = np.random.RandomState(21)
    bs, nhk, d, ps, cap = 2, 2, 128, 32, 64
    cache, kc, vc = _paged_cache(torch, rs_, bs, nhk, d, 64, ps, cap)
    n_a, n_dec, n_b, n_after = 100, cap + 6, 40, 10
    n_all = n_a + n_dec + n_b + n_after
    Kall = rs_.standard_normal((bs, nhk, n_all, d)).astype(np.float16)
    Vall = rs_.standard_normal((bs, nhk, n_all, d)).astype(np.float16)
    cu = lambda a: torch.from_numpy(np.ascontiguousarray(a)).cuda()
    qa = rs_.standard_normal((bs, 4 * nhk, n_a, d)).astype(np.float16)
    cache.prefill(cu(qa), cu(Kall[:, :, :n_a]), cu(Vall[:, :, :n_a]), 0)
    for i in range(n_dec):
        t = n_a + i
        q1 = rs_.standard_normal((bs, 4 * nhk, 1, d)).astype(np.float16)
        cache.decoding_with_pages(cu(q1), cu(Kall[:, :, t:t + 1]), cu(Vall[:, :, t:t + 1]), 0)
    T, r, rs = cache._T[0], cache.residualed_tokens[0], cache._rstart[0]
    assert T + r == n_a + n_dec and r > 0 and T > n_a
    if ahead:
        assert cache.begin_step() == "pre"
    t0 = n_a + n_dec
    qb = rs_.standard_normal((bs, 4 * nhk, n_b, d)).astype(np.float16)
    out = cache.extend(cu(qb), cu(Kall[:, :, t0:t0 + n_b]), cu(Vall[:, :, t0:t0 + n_b]), 0)
    torch.cuda.synchronize()
    kcodes, vcodes = oracle.pq_encode(Kall[:, :, :T], kc), oracle.pq_encode(Vall[:, :, :T], vc)
    gold = model(oracle, qb, kcodes, vcodes, kc, vc, Kall[:, :, T:T + r], Vall[:, :, T:T + r], Kall[:, :, t0:t0 + n_b],
                 Vall[:, :, t0:t0 + n_b])
    _check(out.float().cpu().numpy(), gold, "extend")
    n_tot = t0 + n_b
    ids = cache.page_ids[0].cpu().numpy()
    got_k = oracle.pool_to_k_rowmajor(cache.key_page_pool.cpu().numpy(), ids, n_tot)
    got_v = oracle.pool_to_v_rowmajor(cache.value_page_pool.cpu().numpy(), ids, n_tot)
    assert np.array_equal(got_k, oracle.pq_encode(Kall[:, :, :n_tot], kc))
    assert np.array_equal(got_v, oracle.pq_encode(Vall[:, :, :n_tot], vc))
    assert (cache._T[0], cache.residualed_tokens[0], cache._rstart[0]) == (n_tot, 0, 0)
    assert cache.lengths[0].cpu().tolist() == [[n_tot, 0, 0, 0]] * bs
    for i in range(n_after):
        t = n_tot + i
        q1 = rs_.standard_normal((bs, 4 * nhk, 1, d)).astype(np.float16)
        o = cache.decoding_with_pages(cu(q1), cu(Kall[:, :, t:t + 1]), cu(Vall[:, :, t:t + 1]), 0)
        gold = _decode_gold(oracle, q1, Kall, Vall, kc, vc, cache._T[0], cache.residualed_tokens[0], cap)
        _check(o.float().cpu().numpy(), gold, f"decode after extend {i}")


def test_paged_extend_request_continuous_batching(env, oracle):
    """Slot 1 extends while slots 0 and 2 keep decoding (device-resident lengths): their outputs are bit-identical to a run
    without the extend (their work reads only their own lengths) and their device lengths do not move."""
    torch, ops = env
    bs, nhk, d = 3, 2, 128
    cu = lambda a: torch.from_numpy(np.ascontiguousarray(a)).cuda()
    outs = []
    for with_extend in (False, True):
        rs_ = np.random.RandomState(8)
        cache, kc, vc = _paged_cache(torch, rs_, bs, nhk, d)
        K = rs_.standard_normal((bs, nhk, 300, d)).astype(np.float16)
        V = rs_.standard_normal((bs, nhk, 300, d)).astype(np.float16)
        Q = rs_.standard_normal((80, bs, 4 * nhk, 1, d)).astype(np.float16)
        qx = rs_.standard_normal((1, 4 * nhk, 24, d)).astype(np.float16)
        Kx = rs_.standard_normal((1, nhk, 24, d)).astype(np.float16)
        cache.prefill(cu(rs_.standard_normal((bs, 4 * nhk, 90, d)).astype(np.float16)), cu(K[:, :, :90]), cu(V[:, :, :90]), 0)
        got = []
        for i in range(80):
            if with_extend and i == 40:
                before = cache.lengths[0].cpu().numpy().copy()
                T1 = cache._T_a[0, 1] + cache._r_a[0, 1]
                cache.extend_request(1, cu(qx), cu(Kx), cu(Kx), 0)
                after = cache.lengths[0].cpu().numpy()
                assert np.array_equal(after[[0, 2]], before[[0, 2]])
                assert after[1].tolist() == [T1 + 24, 0, 0, 0]
            t = 90 + i
            o = cache.decoding_with_pages(cu(Q[i]), cu(K[:, :, t:t + 1]), cu(V[:, :, t:t + 1]), 0, use_dev_lengths=True)
            got.append(o.cpu().numpy())
        torch.cuda.synchronize()
        outs.append(np.stack(got))
    assert np.array_equal(outs[0][:, [0, 2]], outs[1][:, [0, 2]])
    assert not np.array_equal(outs[0][40:, 1], outs[1][40:, 1])


def test_dynamic_cache_extend(env, oracle):
    torch, ops = env
    from million_amd.pq_cache import DynamicPQCache
    rs_ = np.random.RandomState(4)
    bs, nhk, d, M = 1, 2, 128, 32
    cache = DynamicPQCache(bs=bs, nh=4 * nhk, num_key_value_heads=nhk, M=M, layer_num=1, d=d, max_tokens=1024, device="cuda")
    kc = rs_.standard_normal((M, 256, d // M)).astype(np.float16)
    vc = rs_.standard_normal((M, 256, d // M)).astype(np.float16)
    cache.set_cent(torch.from_numpy(kc).cuda(), torch.from_numpy(vc).cuda())
    cu = lambda a: torch.from_numpy(np.ascontiguousarray(a)).cuda()
    n_a, n_dec, n_b, n_after = 200, d + 6, 50, 10
    n_all = n_a + n_dec + n_b + n_after
    Kall = rs_.standard_normal((bs, nhk, n_all, d)).astype(np.float16)
    Vall = rs_.standard_normal((bs, nhk, n_all, d)).astype(np.float16)
    cache.prefill(cu(rs_.standard_normal((bs, 4 * nhk, n_a, d)).astype(np.float16)), cu(Kall[:, :, :n_a]), cu(Vall[:, :, :n_a]), 0)
    for i in range(n_dec):
        t = n_a + i
        cache.decoding(cu(rs_.standard_normal((bs, 4 * nhk, 1, d)).astype(np.float16)), cu(Kall[:, :, t:t + 1]),
                       cu(Vall[:, :, t:t + 1]), 0)
    T, r = cache._T[0], cache.residualed_tokens[0]
    assert T + r == n_a + n_dec and r == 6
    t0 = n_a + n_dec
    qb = rs_.standard_normal((bs, 4 * nhk, n_b, d)).astype(np.float16)
    out = cache.extend(cu(qb), cu(Kall[:, :, t0:t0 + n_b]), cu(Vall[:, :, t0:t0 + n_b]), 0)
    torch.cuda.synchronize()
    gold = model(oracle, qb, oracle.pq_encode(Kall[:, :, :T], kc), oracle.pq_encode(Vall[:, :, :T], vc), kc, vc,
                 Kall[:, :, T:T + r], Vall[:, :, T:T + r], Kall[:, :, t0:t0 + n_b], Vall[:, :, t0:t0 + n_b])
    _check(out.float().cpu().numpy(), gold, "dynamic extend")
    n_tot = t0 + n_b
    assert np.array_equal(cache._k_store[0][:, :, :n_tot].cpu().numpy(), oracle.pq_encode(Kall[:, :, :n_tot], kc))
    assert np.array_equal(cache._v_store[0][:, :, :n_tot].cpu().numpy(), oracle.pq_encode(Vall[:, :, :n_tot], vc))
    assert (cache._T[0], cache.residualed_tokens[0], cache.seen_tokens[0]) == (n_tot, 0, n_tot)
    for i in range(n_after):
        t = n_tot + i
        q1 = rs_.standard_normal((bs, 4 * nhk, 1, d)).astype(np.float16)
        o = cache.decoding(cu(q1), cu(Kall[:, :, t:t + 1]), cu(Vall[:, :, t:t + 1]), 0)
        gold = _decode_gold(oracle, q1, Kall, Vall, kc, vc, cache._T[0], cache.residualed_tokens[0], d)
        _check(o.float().cpu().numpy(), gold, f"dynamic decode after extend {i}")
