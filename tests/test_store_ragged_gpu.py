"""GPU tests of the one-launch ragged store: million_pq_store_ragged through ops.pq_store_ragged, and PagedPQCache.extend_ragged /
prefill_ragged with device_store=True.  Everything is compared bit for bit: against the existing per-slot route
(ops.pq_encode_into with host values), against the oracle's codes of the source rows in the order of the numpy model
(tests/store_ragged_model.py), and against the model's lengths.  Shapes: bs = 4, nh_k = 2, a window of 64 rows, 70 new rows,
page tables of 256 tokens."""
import numpy as np
import pytest

from tests import store_ragged_model as SM

pytestmark = pytest.mark.gpu

BS, NHK, CAP, NB, CAP_TOK = 4, SM.NH_K, SM.CAP, SM.N_BOUND, SM.CAP_TOK
SHAPES = [(128, 64, 256), (128, 32, 128), (128, 16, 256), (64, 64, 128), (64, 32, 256), (64, 16, 128)]
FILL = 0xA5


@pytest.fixture(scope="module")
def env():
    import torch
    assert torch.cuda.is_available(), "GPU tests need an MI355X"
    from million_amd import ops, _lib
    _lib.load()
    return torch, ops, _lib


class Scene:
    """The inputs of one call: windows, new rows, codebooks, a shuffled page table over a pool with a sentinel page (named by
    every entry the call must not read: past a request's written pages, and all of a non-participant's) and two spare pages."""

    def __init__(self, seed, d, M, C, ps, rows, table_rows=None):
        rs_ = np.random.RandomState(seed)
        f = lambda *s: rs_.standard_normal(s).astype(np.float16)
        self.d, self.M, self.C, self.ps, self.rows = d, M, C, ps, [tuple(r) for r in rows]
        self.npc = CAP_TOK // ps
        self.geom = dict(page_size=ps, n_pages_cap=self.npc, resid_cap=CAP, n_bound=NB)
        self.k_new, self.v_new, self.k_win, self.v_win = f(BS, NHK, NB, d), f(BS, NHK, NB, d), f(BS, NHK, CAP, d), f(BS, NHK, CAP, d)
        self.k_cents, self.v_cents = f(M, C, d // M), f(M, C, d // M)
        self.plans = SM.plans(self.rows, **self.geom)
        n_real = BS * NHK * self.npc
        self.n_pool = n_real + 3
        perm = rs_.permutation(self.n_pool)
        self.sentinel, self.spare = int(perm[n_real]), perm[n_real + 1:]
        self.ids = perm[:n_real].reshape(BS, NHK, self.npc).astype(np.int32)
        # table_rows: the rows whose written pages bound the table (a replayed call: the last state), default this call's
        for b, p in enumerate(SM.plans(table_rows or self.rows, **self.geom)):
            written = p.pages_written(ps)
            self.ids[b, :, (max(written) + 1 if written else 0):] = self.sentinel

    def lengths(self, rows=None, word3=0x7EADBEEF):
        return np.array([[T, r, s, word3] for T, r, s, _ in (rows or self.rows)], np.int32)

    def used_pages(self):
        return sorted({int(self.ids[b, h, pg]) for b, p in enumerate(self.plans) for h in range(NHK) for pg in p.pages_written(self.ps)})

    def tensors(self, torch, ops, poison=False, pool_fill=FILL):
        """Device tensors.  poison: NaN in new rows at or past n_b (all of a non-participant's), NaN in window rows outside
        each ring span, 0xFF in every pool page the call does not write; else zeros there and `pool_fill` in those pages."""
        dev = lambda a: torch.from_numpy(np.ascontiguousarray(a)).cuda()
        junk = np.float16("nan") if poison else np.float16(0)
        k_new, v_new, k_win, v_win = self.k_new.copy(), self.v_new.copy(), self.k_win.copy(), self.v_win.copy()
        for b, p in enumerate(self.plans):
            k_new[b, :, p.n:] = v_new[b, :, p.n:] = junk
            dead = np.setdiff1d(np.arange(CAP), (p.start + np.arange(p.r)) % CAP)
            k_win[b, :, dead] = v_win[b, :, dead] = junk
        kp = np.full((self.n_pool, self.ps, self.M), FILL, np.uint8)
        vp = np.full((self.n_pool, self.M, self.ps), FILL, np.uint8)
        unused = np.setdiff1d(np.arange(self.n_pool), self.used_pages())
        kp[unused] = vp[unused] = 0xFF if poison else pool_fill
        kc, vc = dev(self.k_cents), dev(self.v_cents)
        return dict(k_new=dev(k_new), v_new=dev(v_new), k_win=dev(k_win), v_win=dev(v_win), kc=kc, vc=vc,
                    kprep=ops.prepare_cents(kc, cache=False), vprep=ops.prepare_cents(vc, cache=False),
                    k_pool=dev(kp), v_pool=dev(vp), ids=dev(self.ids))

    def store(self, torch, ops, t, lengths, dev_n, k_pool=None, v_pool=None):
        ops.pq_store_ragged(t["k_new"], t["v_new"], t["k_win"], t["v_win"], t["kprep"], t["vprep"],
                            t["k_pool"] if k_pool is None else k_pool, t["v_pool"] if v_pool is None else v_pool, t["ids"],
                            lengths, dev_n, M=self.M, C=self.C, page_size=self.ps)

    def per_slot(self, ops, L, t, k_pool, v_pool, plans=None):
        """The existing route: per participating slot the window in ring order, then the new rows, K and V, host values."""
        for b, p in enumerate(plans or self.plans):
            if not p.live:
                continue
            sl = slice(b, b + 1)
            kw = dict(page_ids=t["ids"][sl], page_size=self.ps)
            for x_win, x_new, cents, prep, pool, lay in ((t["k_win"], t["k_new"], t["kc"], t["kprep"], k_pool, L.MILLION_CODES_KPAGES),
                                                         (t["v_win"], t["v_new"], t["vc"], t["vprep"], v_pool, L.MILLION_CODES_VPAGES)):
                if p.r:
                    ops.pq_encode_into(x_win[sl], cents, pool, layout=lay, prepared=prep, token_start=p.T, n=p.r, x_row_start=p.start,
                                       x_row_mod=CAP, **kw)
                ops.pq_encode_into(x_new[sl, :, :p.n], cents, pool, layout=lay, prepared=prep, token_start=p.T + p.r, n=p.n, **kw)

    def expected_pools(self, oracle, start_k, start_v):
        """numpy pools after the call: the oracle's codes of each request's source rows, in model order, at the model's tokens."""
        kp, vp = start_k.copy(), start_v.copy()
        for b, p in enumerate(self.plans):
            if p.live:
                kc = oracle.pq_encode(p.rows_of(self.k_win[b], self.k_new[b])[None], self.k_cents)[0]
                vc = oracle.pq_encode(p.rows_of(self.v_win[b], self.v_new[b])[None], self.v_cents)[0]
                SM.scatter(kp, vp, self.ids, b, p, kc, vc)
        return kp, vp


def _run(torch, ops, sc, t, rows=None, word3=0x7EADBEEF):
    rows = rows or sc.rows
    lengths = torch.from_numpy(sc.lengths(rows, word3)).cuda()
    dev_n = torch.tensor([r[3] for r in rows], dtype=torch.int32).cuda()
    sc.store(torch, ops, t, lengths, dev_n)
    torch.cuda.synchronize()
    assert dev_n.tolist() == [r[3] for r in rows], "dev_n is read, never written"
    return t["k_pool"].cpu().numpy(), t["v_pool"].cpu().numpy(), lengths.cpu().numpy()


# ---------------------------------------------------------------- 1. bit-exact: the oracle and the per-slot route ------------
@pytest.mark.parametrize("d,M,C,ps", [s + (ps,) for s in SHAPES[:2] for ps in (32, 64, 128)] + [s + (32,) for s in SHAPES[2:]])
def test_bit_exact_against_oracle_and_per_slot_route(d, M, C, ps, env, oracle):
    torch, ops, L = env
    sc = Scene(d + M + ps, d, M, C, ps, SM.CASES)
    t = sc.tensors(torch, ops)
    k0, v0 = t["k_pool"].cpu().numpy(), t["v_pool"].cpu().numpy()
    assert (k0 == FILL).all() and (v0 == FILL).all()
    ref_k, ref_v = t["k_pool"].clone(), t["v_pool"].clone()
    sc.per_slot(ops, L, t, ref_k, ref_v)
    kp, vp, lengths = _run(torch, ops, sc, t)
    # whole pools, byte for byte, against the existing route from the same start state
    assert np.array_equal(kp, ref_k.cpu().numpy()) and np.array_equal(vp, ref_v.cpu().numpy())
    # the live tokens, read back through the page table, are the oracle's codes of the source rows in model order
    for b, p in enumerate(sc.plans):
        if not p.live:
            continue
        end = p.T + p.r + p.n
        got_k, got_v = oracle.pool_to_k_rowmajor(kp, sc.ids, end)[b, :, p.T:], oracle.pool_to_v_rowmajor(vp, sc.ids, end)[b, :, p.T:]
        assert np.array_equal(got_k, oracle.pq_encode(p.rows_of(sc.k_win[b], sc.k_new[b])[None], sc.k_cents)[0]), ("K", b)
        assert np.array_equal(got_v, oracle.pq_encode(p.rows_of(sc.v_win[b], sc.v_new[b])[None], sc.v_cents)[0]), ("V", b)
    ek, ev = sc.expected_pools(oracle, k0, v0)
    assert np.array_equal(kp, ek) and np.array_equal(vp, ev)
    # lengths: the model's; slot 1's row, the sentinel page and the spare pages are as they were
    assert np.array_equal(lengths, SM.advance(sc.lengths(), [r[3] for r in sc.rows], **sc.geom))
    assert np.array_equal(lengths[1], sc.lengths()[1]) and (lengths[:, 3] == 0x7EADBEEF).all()
    for pg in [sc.sentinel, *sc.spare]:
        assert (kp[pg] == FILL).all() and (vp[pg] == FILL).all()


# ---------------------------------------------------------------- 2. totality --------------------------------------------------
@pytest.mark.parametrize("d,M,C,ps", [(128, 64, 256, 32), (64, 16, 128, 64)])
def test_totality(d, M, C, ps, env, oracle):
    """The same call on the same live data, once inside zeros and once inside what must never be read or overwritten: NaN in
    new rows at or past n_b, in window rows outside each ring span and in all of slot 1's new rows, 0xFF in every pool page the
    call does not write (the sentinel and the spare pages, slot 1's pages, the pages below each T).  The pages the call writes
    and the lengths are byte-equal between the runs; every other page is exactly as it was filled."""
    torch, ops, L = env
    sc = Scene(7, d, M, C, ps, SM.CASES)
    used = sc.used_pages()
    unused = np.setdiff1d(np.arange(sc.n_pool), used)
    runs = []
    for poison, fill in ((False, 0), (True, 0xFF)):
        kp, vp, lengths = _run(torch, ops, sc, sc.tensors(torch, ops, poison=poison, pool_fill=0))
        assert (kp[unused] == fill).all() and (vp[unused] == fill).all(), "a page outside the destination tokens was written"
        runs.append((kp[used], vp[used], lengths))
    for a, b in zip(*runs):
        assert np.array_equal(a, b)
    ek, ev = sc.expected_pools(oracle, np.full_like(kp, FILL), np.full_like(vp, FILL))
    assert np.array_equal(runs[1][0], ek[used]) and np.array_equal(runs[1][1], ev[used])


# ---------------------------------------------------------------- 3. untrusted values ------------------------------------------
def test_untrusted_values_are_clamped(env, oracle):
    """T = -5, r = 1000, start = 64 and n = 1000 in one row; a T whose last rows lie past the page table; a T far past it; a
    negative n.  Pools and lengths are the model's clamped result; every other byte still holds 0xA5."""
    torch, ops, L = env
    sc = Scene(11, 128, 64, 256, 32, SM.UNTRUSTED)
    assert [(p.T, p.r, p.start, p.n) for p in sc.plans] == [(0, 64, 0, 70), (250, 0, 0, 20), (256, 0, 0, 5), (40, 10, 0, 0)]
    t = sc.tensors(torch, ops)
    k0, v0 = t["k_pool"].cpu().numpy(), t["v_pool"].cpu().numpy()
    kp, vp, lengths = _run(torch, ops, sc, t, word3=7)
    ek, ev = sc.expected_pools(oracle, k0, v0)
    assert np.array_equal(kp, ek) and np.array_equal(vp, ev)      # whole pools: the 0xA5 bytes elsewhere included
    assert lengths.tolist() == [[134, 0, 0, 7], [256, 0, 0, 7], [256, 0, 0, 7], [40, 10, 70, 7]]
    assert np.array_equal(lengths, SM.advance(sc.lengths(word3=7), [r[3] for r in sc.rows], **sc.geom))
    # the per-slot route with the clamped host values agrees on what lies inside the table
    ref_k, ref_v = torch.from_numpy(k0).cuda(), torch.from_numpy(v0).cuda()
    sc.per_slot(ops, L, t, ref_k, ref_v, plans=sc.plans[:1])
    torch.cuda.synchronize()
    pages0 = sc.ids[0].flatten()
    assert np.array_equal(kp[pages0], ref_k.cpu().numpy()[pages0]) and np.array_equal(vp[pages0], ref_v.cpu().numpy()[pages0])


# ---------------------------------------------------------------- 4. one captured call, replayed -------------------------------
def test_graph_replay_follows_lengths_rows_and_windows(env, oracle):
    """The call is captured once (two launches in sequence on one stream: no parallel branches) and replayed three times while
    dev_n, the windows and the new rows are rewritten in place; each replay starts from the lengths the previous one left.
    After every replay pools and lengths equal the eager per-slot route driven from the host with the same values."""
    torch, ops, L = env
    steps = [[30, 0, 9, 70], [5, 12, 0, 20], [0, 70, 64, 38]]
    final = [(145, 0, 0, 1), (131, 0, 0, 1), (73, 0, 0, 1), (256, 0, 0, 1)]      # where the three steps leave each T (below)
    sc = Scene(13, 128, 64, 256, 32, SM.CASES, table_rows=[(0, 0, 0, 0)] * 4)
    # the table covers every page the three steps write, in distinct shuffled pages; every entry past them names the sentinel
    rs_ = np.random.RandomState(99)
    perm = [p for p in rs_.permutation(sc.n_pool) if p != sc.sentinel]
    it = iter(perm)
    sc.ids[:] = sc.sentinel
    for b, (T, _, _, _) in enumerate(final):
        for h in range(NHK):
            for pg in range(-(-T // 32)):
                sc.ids[b, h, pg] = next(it)
    t = sc.tensors(torch, ops)
    t["k_pool"].fill_(FILL)
    t["v_pool"].fill_(FILL)
    lengths = torch.from_numpy(sc.lengths(word3=0)).cuda()
    dev_n = torch.zeros(BS, dtype=torch.int32, device="cuda")
    # eager once on scratch copies: module load outside the capture
    sc.store(torch, ops, t, lengths.clone(), torch.ones(BS, dtype=torch.int32, device="cuda"), t["k_pool"].clone(), t["v_pool"].clone())
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        sc.store(torch, ops, t, lengths, dev_n)
    torch.cuda.synchronize()
    assert (t["k_pool"] == FILL).all() and lengths.cpu().numpy().tolist() == sc.lengths(word3=0).tolist()      # captured, not run
    ref_k, ref_v = t["k_pool"].clone(), t["v_pool"].clone()
    state = [tuple(r[:3]) for r in SM.CASES]
    f = lambda *s: torch.from_numpy(rs_.standard_normal(s).astype(np.float16)).cuda()
    for n_new in steps:
        dev_n.copy_(torch.tensor(n_new, dtype=torch.int32))
        for name, rows in (("k_new", NB), ("v_new", NB), ("k_win", CAP), ("v_win", CAP)):
            t[name].copy_(f(BS, NHK, rows, sc.d))
        g.replay()
        torch.cuda.synchronize()
        plans = SM.plans([s + (n,) for s, n in zip(state, n_new)], **sc.geom)
        sc.per_slot(ops, L, t, ref_k, ref_v, plans=plans)
        torch.cuda.synchronize()
        state = [(p.T_after, 0, 0) if p.live else s for p, s in zip(plans, state)]
        assert torch.equal(t["k_pool"], ref_k) and torch.equal(t["v_pool"], ref_v), n_new
        assert lengths.cpu().numpy().tolist() == [list(s) + [0] for s in state], n_new
    assert [s[0] for s in state] == [r[0] for r in final]
    sent = sc.sentinel
    assert (t["k_pool"][sent] == FILL).all() and (t["v_pool"][sent] == FILL).all()


# ---------------------------------------------------------------- 5. extend_ragged(device_store=True) -------------------------
def _live_codes(oracle, cache):
    ids = cache.page_ids[0].cpu().numpy()
    n_max = int(cache._T_a[0].max())
    k = oracle.pool_to_k_rowmajor(cache.key_page_pool.cpu().numpy(), ids, n_max)
    v = oracle.pool_to_v_rowmajor(cache.value_page_pool.cpu().numpy(), ids, n_max)
    return [(k[s, :, :int(cache._T_a[0, s])], v[s, :, :int(cache._T_a[0, s])]) for s in range(cache.bs)]


def _assert_twins(torch, oracle, a, b_):
    for x, y in zip(a.host_state(), b_.host_state()):      # _seen_a, _r_a, _T_a, _rs_a, _pre_a
        assert (x == y).all()
    assert torch.equal(a.lengths[0], b_.lengths[0])
    for s, ((ka, va), (kb, vb)) in enumerate(zip(_live_codes(oracle, a), _live_codes(oracle, b_))):
        assert np.array_equal(ka, kb) and np.array_equal(va, vb), s


@pytest.mark.parametrize("setup", ["plain", "encode-ahead", "on-demand"])
def test_extend_ragged_device_store_matches_host_store(setup, env, oracle):
    """Twin caches in the states of test_extend_ragged_matches_extend_request (a wrapped window, unequal lengths and a released
    slot; or a lockstep batch with rows encoded ahead), once more with pages taken on demand: extend_ragged with
    device_store=True against the default - outputs, mirrors, device rows, the codes of every live token, ten decode steps."""
    torch, ops, L = env
    from million_amd.pq_cache import PagedPQCache
    bs, nhk, d, ps, cap, G = 3, 2, 128, 32, 64, 4
    cu = lambda a: torch.from_numpy(np.ascontiguousarray(a)).cuda()
    rs_ = np.random.RandomState(17)
    n_tot = 400
    K = rs_.standard_normal((bs, nhk, n_tot, d)).astype(np.float16)
    V = rs_.standard_normal((bs, nhk, n_tot, d)).astype(np.float16)
    Q1 = rs_.standard_normal((n_tot, bs, G * nhk, 1, d)).astype(np.float16)
    n_new = [24, 0, 9]
    qx = rs_.standard_normal((bs, G * nhk, 24, d)).astype(np.float16)
    Kx = rs_.standard_normal((bs, nhk, 24, d)).astype(np.float16)
    Vx = rs_.standard_normal((bs, nhk, 24, d)).astype(np.float16)
    cents = np.random.RandomState(3)
    kc, vc = (cents.standard_normal((64, 256, 2)).astype(np.float16) for _ in range(2))
    caches, outs, after = [], [], []
    for device_store in (True, False):
        cache = PagedPQCache(bs=bs, nh=G * nhk, num_key_value_heads=nhk, M=64, layer_num=1, d=d, page_size=ps,
                             extended_residual_size=cap, max_tokens=2048, preallocate=setup != "on-demand", device="cuda")
        cache.set_cent(cu(kc), cu(vc))
        pos = [0] * bs

        def step():
            k1 = np.stack([K[b, :, pos[b]:pos[b] + 1] for b in range(bs)])
            v1 = np.stack([V[b, :, pos[b]:pos[b] + 1] for b in range(bs)])
            cache.decoding_with_pages(cu(Q1[pos[0]]), cu(k1), cu(v1), 0, use_dev_lengths=True)
            for b in range(bs):
                pos[b] += 1

        zq = lambda n_b, n: cu(np.zeros((n_b, G * nhk, n, d), np.float16))
        if setup == "encode-ahead":
            cache.prefill(zq(bs, 70), cu(K[:, :, :70]), cu(V[:, :, :70]), 0)
            pos = [70] * bs
            for _ in range(cache.encode_ahead_at()):
                step()
            assert cache.begin_step(use_dev_lengths=True) == "pre"
        else:
            for b, n in ((0, 70), (1, 33), (2, 5)):
                cache.prefill_request(b, zq(1, n), cu(K[b:b + 1, :, :n]), cu(V[b:b + 1, :, :n]), 0)
                pos[b] = n
            for _ in range(3 * cap):
                if cache._rs_a[0, 0] + cache._r_a[0, 0] > cap and cache._r_a[0, 0] >= 40:
                    break
                step()
            assert cache._rs_a[0, 0] + cache._r_a[0, 0] > cap, "slot 0's window must wrap"
            cache.release(2)
        dev_before = cache.lengths[0].cpu().numpy().copy()
        win1, ids1 = cache.key_residual_cache[0][1].clone(), cache.page_ids[0][1].clone()
        # rows past a slot's n_new hold NaN: never read by the attention launch nor by the store
        qp, Kp, Vp = qx.copy(), Kx.copy(), Vx.copy()
        for b in range(bs):
            qp[b, :, n_new[b]:] = Kp[b, :, n_new[b]:] = Vp[b, :, n_new[b]:] = np.nan
        out = cache.extend_ragged(cu(qp), cu(Kp), cu(Vp), 0, n_new, device_store=device_store).float().cpu().numpy()
        torch.cuda.synchronize()
        assert np.array_equal(cache.lengths[0][1].cpu().numpy(), dev_before[1])      # slot 1: row, window and table untouched
        assert torch.equal(cache.key_residual_cache[0][1], win1) and torch.equal(cache.page_ids[0][1], ids1)
        assert cache.lengths[0][[0, 2], 1:3].cpu().numpy().tolist() == [[0, 0], [0, 0]]
        caches.append(cache)
        outs.append(out)
        dec = []
        for i in range(10):
            o = cache.decoding_with_pages(cu(Q1[300 + i]), cu(K[:, :, 300 + i:301 + i]), cu(V[:, :, 300 + i:301 + i]), 0,
                                          use_dev_lengths=True)
            dec.append(o.cpu().numpy())
        torch.cuda.synchronize()
        after.append(np.stack(dec))
    assert np.isfinite(outs[0]).all() and np.array_equal(outs[0], outs[1])
    _assert_twins(torch, oracle, *caches)
    assert np.array_equal(after[0].view(np.uint16), after[1].view(np.uint16))


# ---------------------------------------------------------------- 6. prefill_ragged(device_store=True) ------------------------
def test_prefill_ragged_device_store_matches_host_store(env, oracle):
    """Prompts of 70 and 5 tokens into the released slots 0 and 2 while slot 1 is mid-decode (codes and window rows)."""
    torch, ops, L = env
    from tests.test_chunk_attn_gpu import _paged_cache
    bs, nhk, d, ps, cap, G = 3, 2, 128, 32, 64, 4
    cu = lambda a: torch.from_numpy(np.ascontiguousarray(a)).cuda()
    rs_ = np.random.RandomState(29)
    n_new, n = [70, 0, 5], 70
    K, V = (rs_.standard_normal((bs, nhk, n + 1, d)).astype(np.float16) for _ in range(2))
    Q = rs_.standard_normal((bs, G * nhk, n, d)).astype(np.float16)
    K1, V1 = (rs_.standard_normal((1, nhk, 47, d)).astype(np.float16) for _ in range(2))
    q1 = rs_.standard_normal((bs, G * nhk, 1, d)).astype(np.float16)
    caches, outs, decs = [], [], []
    for device_store in (True, False):
        cache, kc, vc = _paged_cache(torch, np.random.RandomState(3), bs, nhk, d, 64, ps, cap)
        cache.prefill_request(1, cu(np.zeros((1, G * nhk, 40, d), np.float16)), cu(K1[:, :, :40]), cu(V1[:, :, :40]), 0)
        for i in range(6):
            k1, v1 = np.repeat(K1[:, :, 40 + i:41 + i], bs, axis=0), np.repeat(V1[:, :, 40 + i:41 + i], bs, axis=0)
            cache.decoding_with_pages(cu(q1), cu(k1), cu(v1), 0, use_dev_lengths=True)
        for b in (0, 2):
            cache.release(b)
        assert (cache._T_a[0, 1], cache._r_a[0, 1]) == (40, 6)
        ids1 = cache.page_ids[0][1].long()
        before = (cache.lengths[0][1].clone(), cache.page_ids[0][1].clone(), cache.key_residual_cache[0][1].clone(),
                  cache.value_residual_cache[0][1].clone(), cache.key_page_pool[ids1].clone(), cache.value_page_pool[ids1].clone())
        Qp, Kp, Vp = Q.copy(), K[:, :, :n].copy(), V[:, :, :n].copy()
        for b in range(bs):
            Qp[b, :, n_new[b]:] = Kp[b, :, n_new[b]:] = Vp[b, :, n_new[b]:] = np.nan
        out = cache.prefill_ragged(cu(Qp), cu(Kp), cu(Vp), 0, n_new, device_store=device_store).cpu().numpy()
        torch.cuda.synchronize()
        now = (cache.lengths[0][1], cache.page_ids[0][1], cache.key_residual_cache[0][1], cache.value_residual_cache[0][1],
               cache.key_page_pool[ids1], cache.value_page_pool[ids1])
        for x, y in zip(before, now):      # slot 1: device row, page ids, window and page contents untouched
            assert torch.equal(x.view(torch.int16) if x.dtype == torch.float16 else x, y.view(torch.int16) if y.dtype == torch.float16 else y)
        assert cache.lengths[0].tolist() == [[70, 0, 0, 0], [40, 6, 0, 0], [5, 0, 0, 0]]
        caches.append(cache)
        outs.append(out)
        kd = np.concatenate([K[:1, :, 70:71], K1[:, :, 46:47], K[2:3, :, 5:6]])
        vd = np.concatenate([V[:1, :, 70:71], V1[:, :, 46:47], V[2:3, :, 5:6]])
        decs.append(cache.decoding_with_pages(cu(q1), cu(kd), cu(vd), 0, use_dev_lengths=True).cpu().numpy())
        torch.cuda.synchronize()
    assert np.array_equal(outs[0].view(np.uint16), outs[1].view(np.uint16))
    _assert_twins(torch, oracle, *caches)
    assert torch.equal(caches[0].page_ids[0], caches[1].page_ids[0])
    assert np.array_equal(decs[0].view(np.uint16), decs[1].view(np.uint16))
