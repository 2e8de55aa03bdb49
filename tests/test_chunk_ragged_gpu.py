"""GPU tests of ragged chunk attention: per-request lengths read on the device (million_chunk_attn_desc.dev_lengths /
dev_n_q, ops.pq_chunk_attn(dev_lengths=, dev_n_q=)) and PagedPQCache.extend_ragged.  fp64 model and bars as
test_chunk_attn_gpu.py: rel-L2 < 1e-3 and mean-abs < 1e-3 per request against the model of its own lengths, outputs finite;
everything the contract calls equal is compared bit for bit."""
import numpy as np
import pytest

from tests.test_chunk_attn_gpu import _check, _paged_cache, model

pytestmark = pytest.mark.gpu

CAP = 128      # window rows


@pytest.fixture(scope="module")
def env():
    import torch
    assert torch.cuda.is_available(), "GPU tests need an MI355X"
    from million_amd import ops, _lib
    _lib.load()
    return torch, ops


def _splits(bs, nhk, n_q, G, T):
    blocks = bs * nhk * -(-n_q * G // 256)
    return max(1, min(-(-256 // blocks), -(-T // 64), 64))


class Scene:
    """Live data of a ragged batch - codes up to each T_b, the ring span of each window, the first n_q_b query / chunk rows -
    and two ways of filling everything around it: zeros, or what must never reach a product (0xFF code bytes, NaN rows)."""

    def __init__(self, seed, d, M, C, G, n_q, bound, rows, chunk, layout="paged", ps=64, i64=False, nhk=2):
        rs_ = np.random.RandomState(seed)
        f = lambda *s: rs_.standard_normal(s).astype(np.float16)
        self.d, self.M, self.C, self.G, self.n_q, self.bound, self.chunk = d, M, C, G, n_q, bound, chunk
        self.layout, self.ps, self.i64, self.nhk = layout, ps, i64, nhk
        self.rows = [tuple(r) for r in rows]
        bs = self.bs = len(rows)
        self.q = f(bs, G * nhk, n_q, d)
        self.k_ch, self.v_ch = f(bs, nhk, n_q, d), f(bs, nhk, n_q, d)
        self.k_cents, self.v_cents = f(M, C, d // M), f(M, C, d // M)
        self.k_codes = rs_.randint(0, C, (bs, nhk, bound, M)).astype(np.uint8)
        self.v_codes = rs_.randint(0, C, (bs, nhk, bound, M)).astype(np.uint8)
        self.k_res, self.v_res = f(bs, nhk, CAP, d), f(bs, nhk, CAP, d)

    def lengths(self, rows=None):
        return np.array([[T, r, s, 0x7EADBEEF] for T, r, s, _ in (rows or self.rows)], np.int32)

    def gold(self, oracle, b, rows=None):
        T, r, s, nq = (rows or self.rows)[b]
        nh = self.G * self.nhk
        out = np.zeros((nh, self.n_q, self.d))
        if nq == 0 or (T == 0 and r == 0 and not self.chunk):
            return out
        ring = (s + np.arange(r)) % CAP
        sl = slice(b, b + 1)
        ch = (self.k_ch[sl, :, :nq], self.v_ch[sl, :, :nq]) if self.chunk else (None, None)
        out[:, :nq] = model(oracle, self.q[sl, :, :nq], self.k_codes[sl, :, :T], self.v_codes[sl, :, :T], self.k_cents, self.v_cents,
                            self.k_res[sl][:, :, ring], self.v_res[sl][:, :, ring], ch[0], ch[1])[0]
        return out

    def tensors(self, torch, ops, oracle, poison, rows=None):
        """Device tensors; `poison`: the surroundings hold 0xFF / NaN instead of zeros.  The live data is the same."""
        rows = rows or self.rows
        dev = lambda a: torch.from_numpy(np.ascontiguousarray(a)).cuda()
        nan = np.float16("nan")
        q, k_ch, v_ch = self.q.copy(), self.k_ch.copy(), self.v_ch.copy()
        k_res, v_res = self.k_res.copy(), self.v_res.copy()
        kc, vc = self.k_codes.copy(), self.v_codes.copy()
        fill = 0xFF if poison else 0
        for b, (T, r, s, nq) in enumerate(rows):
            T, nq = min(max(T, 0), self.bound), min(max(nq, 0), self.n_q)
            kc[b, :, T:], vc[b, :, T:] = fill, fill
            q[b, :, nq:] = nan if poison else 0
            k_ch[b, :, nq:] = v_ch[b, :, nq:] = nan if poison else 0
            r = min(max(r, 0), CAP)
            s = s if 0 <= s < CAP else 0
            dead = np.setdiff1d(np.arange(CAP), (s + np.arange(r)) % CAP)
            k_res[b, :, dead] = v_res[b, :, dead] = nan if poison else 0
        t = dict(q=dev(q), k_ch=dev(k_ch) if self.chunk else None, v_ch=dev(v_ch) if self.chunk else None, k_res=dev(k_res),
                 v_res=dev(v_res), kp=ops.prepare_cents(dev(self.k_cents), cache=False),
                 vp=ops.prepare_cents(dev(self.v_cents), cache=False), kw={})
        if self.layout == "rowmajor":
            t["k_codes"], t["v_codes"] = dev(kc), dev(vc)
            return t
        ps = self.ps
        vpool, ids = oracle.v_rowmajor_to_pool(vc, ps)
        kpool, _ = oracle.k_rowmajor_to_pool(kc, ps)
        extra = 3      # unused pool pages; table entries past a request's live pages name one of them
        n_pool = kpool.shape[0]
        kpool = np.concatenate([kpool, np.full((extra,) + kpool.shape[1:], fill, np.uint8)])
        vpool = np.concatenate([vpool, np.full((extra,) + vpool.shape[1:], fill, np.uint8)])
        for b, (T, _, _, _) in enumerate(rows):
            live = -(-min(max(T, 0), self.bound) // ps)
            ids[b, :, live:] = n_pool + np.arange(ids.shape[2] - live) % extra
        perm = np.random.RandomState(5).permutation(kpool.shape[0])      # physical page order must not matter
        inv = np.argsort(perm)
        t["k_codes"], t["v_codes"] = dev(kpool[perm]), dev(vpool[perm])
        ids_t = dev(inv[ids].astype(np.int64 if self.i64 else np.int32))
        t["kw"] = dict(k_page_ids=ids_t, v_page_ids=ids_t, page_size=ps)
        return t

    def run(self, torch, ops, t, *, dev_lengths=None, dev_n_q=None, host=None, poison=False, **more):
        """host = (T, r, resid_start): the lockstep call.  Workspace and out are the caller's, pre-filled when `poison`."""
        nh = self.G * self.nhk
        S = _splits(self.bs, self.nhk, self.n_q, self.G, self.bound if host is None else host[0])
        ws = torch.full((max(self.bs * self.nhk * S * self.n_q * self.G * (self.d + 2) * 4, 16),), 0xFF if poison else 0,
                        dtype=torch.uint8, device="cuda")
        out = torch.full((self.bs, self.n_q, nh, self.d), float("nan") if poison else 0.0, dtype=torch.float16,
                         device="cuda").transpose(1, 2)
        T, r, s = (self.bound, 0, 0) if host is None else host
        got = ops.pq_chunk_attn(t["q"], t["k_ch"], t["v_ch"], t["k_codes"], t["v_codes"], t["kp"], t["vp"], t["k_res"], t["v_res"], r,
                                M=self.M, C=self.C, n_tokens=T, resid_start=s, out=out, workspace=ws, dev_lengths=dev_lengths,
                                dev_n_q=dev_n_q, **t["kw"], **more)
        torch.cuda.synchronize()
        assert got.data_ptr() == out.data_ptr()
        return out.float().cpu().numpy()

    def run_ragged(self, torch, ops, oracle, poison=False, rows=None):
        rows = rows or self.rows
        t = self.tensors(torch, ops, oracle, poison, rows)
        dl = torch.from_numpy(self.lengths(rows)).cuda()
        nq = torch.tensor([r[3] for r in rows], dtype=torch.int32).cuda()
        out = self.run(torch, ops, t, dev_lengths=dl, dev_n_q=nq, poison=poison)
        assert np.array_equal(dl.cpu().numpy(), self.lengths(rows)), "the length rows are read, never written"
        return out

    def check(self, oracle, out, rows=None, what=""):
        rows = rows or self.rows
        for b, (T, r, s, nq) in enumerate(rows):
            gold = self.gold(oracle, b, rows)
            assert np.all(out[b, :, nq:] == 0), f"{what} request {b}: rows past n_q must be zeros"
            if not gold.any():
                assert np.all(out[b] == 0), f"{what} request {b}: nothing to attend to, out = 0"
            else:
                _check(out[b, :, :nq], gold[:, :nq], f"{what} request {b} {rows[b]}")


# ---------------------------------------------------------------- 1. equal lengths: bit for bit the host-length call --------
@pytest.mark.parametrize("d,M,C", [(128, 64, 256), (128, 32, 128), (128, 16, 256), (64, 64, 128), (64, 32, 256), (64, 16, 128)])
@pytest.mark.parametrize("T", [1000, 40], ids=["split", "S1"])
def test_equal_lengths_are_the_host_length_call(d, M, C, T, env, oracle):
    torch, ops = env
    sc = Scene(d + M + T, d, M, C, 4, 5, T, [(T, 100, 90, 5)] * 2, True, layout="paged" if M != 32 else "rowmajor")
    assert (_splits(2, 2, 5, 4, T) > 1) == (T == 1000)
    t = sc.tensors(torch, ops, oracle, False)
    host = sc.run(torch, ops, t, host=(T, 100, 90))
    dl = torch.from_numpy(sc.lengths()).cuda()
    nq = torch.full((2,), 5, dtype=torch.int32, device="cuda")
    for kw in (dict(dev_lengths=dl, dev_n_q=nq), dict(dev_lengths=dl), dict(dev_n_q=nq, host=(T, 100, 90))):
        assert np.array_equal(sc.run(torch, ops, t, **kw), host), sorted(kw)
    sc.check(oracle, host, what="lockstep")


# ---------------------------------------------------------------- 2. / 3. ragged parity, totality ---------------------------
RAGGED = {
    # (d, M, C, G, n_q, bound, rows (T, r, start, n_q_b), chunk, page size, int64 ids)
    "llama-tile": (128, 64, 256, 4, 5, 1000, [(1000, 17, 0, 5), (63, 100, 90, 3), (0, 0, 0, 5), (65, 0, 0, 0)], True, 64, False),
    "invalid-ff": (128, 64, 128, 4, 5, 1000, [(1000, 17, 0, 5), (63, 100, 90, 3), (0, 0, 0, 5), (65, 0, 0, 0)], True, 64, False),
    "diag-chunk": (64, 16, 128, 8, 65, 1000, [(1000, 17, 0, 65), (63, 100, 90, 33), (0, 0, 0, 64), (65, 0, 0, 0)], True, 32, True),
    "diag-past": (64, 16, 128, 8, 65, 1000, [(1000, 17, 0, 65), (63, 100, 90, 33), (0, 0, 0, 64), (65, 0, 0, 0)], False, 32, True),
    "S1": (128, 64, 256, 4, 5, 40, [(40, 17, 0, 5), (1, 100, 90, 3), (0, 0, 0, 5)], True, 64, False),
    "S1-past": (128, 64, 256, 4, 5, 40, [(40, 17, 0, 5), (1, 100, 90, 3), (0, 0, 0, 5)], False, 64, False),
}


@pytest.mark.parametrize("name", list(RAGGED))
def test_ragged_parity_and_totality(name, env, oracle):
    """Every request against the model of its own lengths; then the same live data inside 0xFF code bytes (from T_b to the end
    of the store, unused pool pages, the pages that table entries past a request's live pages name), NaN window rows outside
    each ring span, NaN q / chunk rows past n_q_b, a 0xFF workspace and a NaN `out`: not one bit of the output moves.  At
    C = 128 a 0xFF byte is an invalid code, so a leak that a valid centroid would hide in the bar shows here."""
    torch, ops = env
    d, M, C, G, n_q, bound, rows, chunk, ps, i64 = RAGGED[name]
    sc = Scene(len(name), d, M, C, G, n_q, bound, rows, chunk, ps=ps, i64=i64)
    clean = sc.run_ragged(torch, ops, oracle, poison=False)
    sc.check(oracle, clean, what=name)
    dirty = sc.run_ragged(torch, ops, oracle, poison=True)
    assert np.isfinite(dirty).all(), "poison reached the output"
    assert np.array_equal(clean, dirty)


def test_ragged_rowmajor_and_lengths_without_n_q(env, oracle):
    """Row-major codes, and dev_lengths alone (every request has all n_q rows)."""
    torch, ops = env
    rows = [(777, 128, 5, 9), (64, 1, 127, 9), (0, 64, 64, 9)]
    sc = Scene(2, 128, 32, 256, 2, 9, 777, rows, True, layout="rowmajor")
    t = sc.tensors(torch, ops, oracle, True)
    out = sc.run(torch, ops, t, dev_lengths=torch.from_numpy(sc.lengths()).cuda(), poison=True)
    sc.check(oracle, out, what="rowmajor")


# ---------------------------------------------------------------- 4. untrusted lengths --------------------------------------
def test_untrusted_lengths_are_clamped(env, oracle):
    torch, ops = env
    bad = [(-5, 999, 777, -3), (10 ** 9, -1, -1, 99)]
    good = [(0, CAP, 0, 0), (1000, 0, 0, 5)]
    sc = Scene(4, 128, 64, 256, 4, 5, 1000, good, True)
    t = sc.tensors(torch, ops, oracle, False, good)
    outs = []
    for rows in (good, bad):
        dl = torch.from_numpy(sc.lengths(rows)).cuda()
        nq = torch.tensor([r[3] for r in rows], dtype=torch.int32).cuda()
        outs.append(sc.run(torch, ops, t, dev_lengths=dl, dev_n_q=nq, poison=True))
        assert np.array_equal(dl.cpu().numpy(), sc.lengths(rows))
    assert np.isfinite(outs[1]).all()
    assert np.array_equal(outs[0], outs[1])
    sc.check(oracle, outs[1], good, "clamped")
    # request 0 with all its rows: T = 0, the whole ring from row 0
    good2, bad2 = [(0, CAP, 0, 5), (1000, 0, 0, 0)], [(-5, 999, 777, 99), (10 ** 9, -1, -1, -3)]
    t = sc.tensors(torch, ops, oracle, False, good2)
    outs = []
    for rows in (good2, bad2):
        dl = torch.from_numpy(sc.lengths(rows)).cuda()
        nq = torch.tensor([r[3] for r in rows], dtype=torch.int32).cuda()
        outs.append(sc.run(torch, ops, t, dev_lengths=dl, dev_n_q=nq))
    assert np.array_equal(outs[0], outs[1])
    sc.check(oracle, outs[1], good2, "clamped-2")


# ---------------------------------------------------------------- 5. one captured launch, moving lengths --------------------
def test_graph_replay_follows_the_lengths(env, oracle):
    """One captured call (the attention kernel and the merge, in sequence on one stream: no parallel branches) replayed while
    the requests' lengths move as decode steps and flushes move them."""
    torch, ops = env
    states = [[(63, 5, 0, 5), (1000, 0, 0, 5)], [(65, 128, 90, 5), (1000, 17, 3, 5)], [(128, 0, 0, 5), (936, 64, 64, 5)]]
    sc = Scene(6, 128, 64, 256, 4, 5, 1000, states[0], False)
    # every code up to the bound and every window row is live in some state: no poison
    full = [(1000, CAP, 0, 5)] * 2
    t = sc.tensors(torch, ops, oracle, False, full)
    nh = sc.G * sc.nhk
    S = _splits(2, 2, 5, 4, 1000)
    ws = torch.empty(2 * 2 * S * 5 * 4 * (128 + 2) * 4, dtype=torch.uint8, device="cuda")
    out = torch.zeros(2, 5, nh, 128, dtype=torch.float16, device="cuda").transpose(1, 2)
    lengths = torch.from_numpy(sc.lengths(states[0])).cuda()
    call = lambda dl, o, w: ops.pq_chunk_attn(t["q"], None, None, t["k_codes"], t["v_codes"], t["kp"], t["vp"], t["k_res"], t["v_res"], 0,
                                              M=sc.M, C=sc.C, n_tokens=1000, dev_lengths=dl, workspace=w, out=o, **t["kw"])
    call(lengths, out, ws)      # eager once: module load, kernel attributes
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        call(lengths, out, ws)
    for rows in states:
        lengths.copy_(torch.from_numpy(sc.lengths(rows)))
        out.fill_(float("nan"))
        g.replay()
        torch.cuda.synchronize()
        got = out.float().cpu().numpy()
        eager = sc.run(torch, ops, t, dev_lengths=torch.from_numpy(sc.lengths(rows)).cuda())
        assert np.array_equal(got, eager), rows
        sc.check(oracle, got, rows, "replay")


# ---------------------------------------------------------------- 6. extend_ragged against extend_request -------------------
@pytest.mark.parametrize("ahead", [False, True], ids=["plain", "encode-ahead"])
def test_extend_ragged_matches_extend_request(ahead, env, oracle):
    torch, ops = env
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
    caches, outs, after = [], [], []
    for ragged in (True, False):
        cache, kc, vc = _paged_cache(torch, np.random.RandomState(3), bs, nhk, d, 64, ps, cap)
        pos = [0] * bs      # slot b has consumed K[b, :, :pos[b]]

        def step():
            k1 = np.stack([K[b, :, pos[b]:pos[b] + 1] for b in range(bs)])
            v1 = np.stack([V[b, :, pos[b]:pos[b] + 1] for b in range(bs)])
            cache.decoding_with_pages(cu(Q1[pos[0]]), cu(k1), cu(v1), 0, use_dev_lengths=True)
            for b in range(bs):
                pos[b] += 1

        zq = lambda n_b, n: cu(np.zeros((n_b, G * nhk, n, d), np.float16))
        if ahead:
            # encode-ahead serves lockstep batches: one prompt of 70 for every slot, then decode steps up to its trigger
            cache.prefill(zq(bs, 70), cu(K[:, :, :70]), cu(V[:, :, :70]), 0)
            pos = [70] * bs
            for _ in range(cache.encode_ahead_at()):
                step()
            assert cache.begin_step(use_dev_lengths=True) == "pre"
        else:
            # prompts of 70 / 33 / 5 tokens, decode steps until the windows have flushed once and wrap, slot 2 released: empty
            for b, n in ((0, 70), (1, 33), (2, 5)):
                cache.prefill_request(b, zq(1, n), cu(K[b:b + 1, :, :n]), cu(V[b:b + 1, :, :n]), 0)
                pos[b] = n
            for _ in range(3 * cap):
                if cache._rs_a[0, 0] + cache._r_a[0, 0] > cap and cache._r_a[0, 0] >= 40:
                    break
                step()
            assert cache._rs_a[0, 0] + cache._r_a[0, 0] > cap, "slot 0's window must wrap"
            assert cache._T_a[0, 0] != cache._T_a[0, 1]
            cache.release(2)
            pos[2] = 0
        before = (cache._T_a[0].copy(), cache._r_a[0].copy(), cache._rs_a[0].copy())
        dev_before = cache.lengths[0].cpu().numpy().copy()
        win1 = cache.key_residual_cache[0][1].clone()
        ids1 = cache.page_ids[0][1].clone()
        if ragged:
            out = cache.extend_ragged(cu(qx), cu(Kx), cu(Vx), 0, n_new).float().cpu().numpy()
        else:
            out = np.zeros((bs, G * nhk, 24, d), np.float32)
            for b in (0, 2):
                n = n_new[b]
                o = cache.extend_request(b, cu(qx[b:b + 1, :, :n]), cu(Kx[b:b + 1, :, :n]), cu(Vx[b:b + 1, :, :n]), 0)
                out[b, :, :n] = o.float().cpu().numpy()
        torch.cuda.synchronize()
        # slot 1: device row, window and pages untouched
        assert np.array_equal(cache.lengths[0][1].cpu().numpy(), dev_before[1])
        assert torch.equal(cache.key_residual_cache[0][1], win1) and torch.equal(cache.page_ids[0][1], ids1)
        assert np.all(out[1] == 0) and np.all(out[2, :, 9:] == 0)
        # the fp64 model of each extended slot: its codes before the call, its window in ring order, its own chunk rows
        T0, r0, s0 = before
        for b in (0, 2):
            n = n_new[b]
            hist_k, hist_v = K[b:b + 1, :, :pos[b]], V[b:b + 1, :, :pos[b]]
            Tb, rb = int(T0[b]), int(r0[b])
            assert Tb + rb == pos[b]
            kcodes = oracle.pq_encode(hist_k[:, :, :Tb], kc) if Tb else np.zeros((1, nhk, 0, 64), np.uint8)
            vcodes = oracle.pq_encode(hist_v[:, :, :Tb], vc) if Tb else np.zeros((1, nhk, 0, 64), np.uint8)
            gold = model(oracle, qx[b:b + 1, :, :n], kcodes, vcodes, kc, vc, hist_k[:, :, Tb:Tb + rb], hist_v[:, :, Tb:Tb + rb],
                         Kx[b:b + 1, :, :n], Vx[b:b + 1, :, :n])
            _check(out[b:b + 1, :, :n], gold, f"extend slot {b}")
        caches.append(cache)
        outs.append(out)
        # ten more decode steps: the new rows of slots 0 and 2 follow their chunks
        dec = []
        for i in range(10):
            o = cache.decoding_with_pages(cu(Q1[300 + i]), cu(K[:, :, 300 + i:301 + i]), cu(V[:, :, 300 + i:301 + i]), 0,
                                          use_dev_lengths=True)
            dec.append(o.cpu().numpy())
        torch.cuda.synchronize()
        after.append(np.stack(dec))
    a, b_ = caches
    assert (a._T_a == b_._T_a).all() and (a._r_a == b_._r_a).all() and (a._rs_a == b_._rs_a).all() and (a._seen_a == b_._seen_a).all()
    assert (a._pre_a == b_._pre_a).all()
    assert torch.equal(a.lengths[0], b_.lengths[0])
    ids_a, ids_b = a.page_ids[0].cpu().numpy(), b_.page_ids[0].cpu().numpy()
    n_max = int(a._T_a[0].max())
    for pool in ("key_page_pool", "value_page_pool"):
        back = oracle.pool_to_k_rowmajor if pool == "key_page_pool" else oracle.pool_to_v_rowmajor
        ga, gb = back(getattr(a, pool).cpu().numpy(), ids_a, n_max), back(getattr(b_, pool).cpu().numpy(), ids_b, n_max)
        for s in range(bs):
            T = int(a._T_a[0, s])
            assert np.array_equal(ga[s, :, :T], gb[s, :, :T]), (pool, s)
    assert np.array_equal(after[0], after[1])


# ---------------------------------------------------------------- 7. the diagnostic library: LDS filled with NaN ------------
def test_ragged_lds_poison_child():
    """The ragged parity cases on poisoned memory, in a child process on libmillion_hip_dbgids.so (one library per process),
    whose chunk kernels start from an LDS full of fp16 NaN."""
    import json
    import os
    import subprocess
    import sys
    from pathlib import Path
    root = Path(__file__).resolve().parents[1]
    dbg = root / "million_amd" / "libmillion_hip_dbgids.so"
    assert dbg.exists(), "million_amd/libmillion_hip_dbgids.so not built (make debug-ids)"
    r = subprocess.run([sys.executable, str(root / "tests" / "chunk_ragged_lds_child.py")], env=dict(os.environ, MILLION_HIP_LIB=str(dbg)),
                       capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-4000:]
    res = json.loads(r.stdout.strip().splitlines()[-1])
    assert res["lib"] == dbg.name
    failed = {c["name"]: c["error"] for c in res["cases"] if c["error"]}
    assert not failed, failed
    assert len(res["cases"]) == len(RAGGED)
