"""Encode-ahead on wide paged caches on the GPU (million_pq_flush_wide_layers through ops.pq_flush_wide; million_amd.paged_turns:
begin_step, next_step_kind, note_replayed_step), per code format, uint16 and packed.  Everything is compared bit
for bit.

Op level: 3 layers x 3 requests side by side, rings turned, T off a page boundary.  advance=False writes oracle.pq_encode's codes
at tokens [T, T + n) of every pair that takes part and nothing else - every other pool byte keeps its 0xA5, the device rows keep
every word - whatever the number of pairs in flight (1, 4, the library's rule: 9 pairs walked by fewer workgroups);
ops.lengths_advance then leaves the rows of the rule (tests/ragged_wide_common.py FlushPlan).  advance=True with layers equals one
pq_flush_wide call per layer.  Rows no cache would write are clamped or skipped as the rule says.

Cache level: twin caches, `ref` stepping through paged_turns.decode alone (the in-line flush), `cache` through
paged_turns.begin_step + paged_turns.decode - with host lengths, device lengths, pages on demand, the layers spread over two
steps, and one hipGraph per step kind: the same outputs, mirrors, device rows, windows and live codes after every step, and the
step kinds plain .. pre .. commit, never 'flush'.  Then a 'pre' step followed by verify + commit, by fork, and by release +
prefill_request, each against a twin that never encoded ahead."""
import numpy as np
import pytest

from tests import packed_model as P
from tests import ragged_wide_common as R

pytestmark = pytest.mark.gpu

LAYERS, BS, NHK, NH, PS, CAP, NPC = 3, R.BS, R.NHK, R.NH, R.PS, R.CAP, R.NPC
CASES = [f + (p,) for f in R.FORMATS for p in (False, True)]
WORD3 = 0x7EADBEEF
# {T, r, start} per (layer, request), min_r = 32: T = 45 / 77 leave the tokens in a partly live page, the rings are turned (one
# wraps), request 2 of layer 2 holds too few rows and takes no part
ROWS = [[(45, 40, 40), (70, 35, 10), (33, 33, 5)], [(77, 64, 50), (45, 32, 63), (100, 50, 1)], [(13, 36, 33), (64, 40, 7), (33, 17, 5)]]
HOSTILE = [[(R.INT_MAX, 64, 0), (100, -5, 3), (50, 64, 70)],      # T far past the table; r < 0: no part; a start past the ring reads as 0
           [(R.CAP_TOK - 10, 40, 0), (R.CAP_TOK, 64, 0), (-7, 100, -1)],      # the last 22 tokens past the table; all of them; T < 0, r > cap, start < 0
           [(R.CAP_TOK - 32, 32, 60), (20, 31, 0), (R.CAP_TOK - 31, 33, 64)]]      # the table's last page, filled; r one below min_r; one token past the table


@pytest.fixture(scope="module")
def env():
    import torch
    assert torch.cuda.is_available(), "GPU tests need an MI355X"
    from million_amd import build, ops, _lib
    build.build()
    _lib.load()
    return torch, ops, _lib


class Scene:
    """Layered windows, codebooks and a shuffled page table over a pool with three pages no entry names; the oracle's codes of
    every window row, computed once per format."""
    _memo = {}

    def __new__(cls, oracle, d, M, nbits):
        key = (d, M, nbits)
        if key not in cls._memo:
            self = object.__new__(cls)
            rs = np.random.RandomState(4000 + d + M + nbits)
            f = lambda *s: rs.standard_normal(s).astype(np.float16)
            self.d, self.M, self.C = d, M, 2 ** nbits
            self.k_win, self.v_win = f(LAYERS, BS, NHK, CAP, d), f(LAYERS, BS, NHK, CAP, d)
            self.k_cents, self.v_cents = f(M, self.C, d // M), f(M, self.C, d // M)
            self.n_pool = LAYERS * BS * NHK * NPC + 3
            self.ids = rs.permutation(self.n_pool)[:LAYERS * BS * NHK * NPC].reshape(LAYERS, BS, NHK, NPC).astype(np.int32)
            self.kc = [oracle.pq_encode(self.k_win[l], self.k_cents) for l in range(LAYERS)]      # (BS, NHK, CAP, M)
            self.vc = [oracle.pq_encode(self.v_win[l], self.v_cents) for l in range(LAYERS)]
            assert self.kc[0].dtype == np.uint16 and (self.kc[0] >= 256).any() and (self.vc[0] >= 256).any()
            cls._memo[key] = self
        return cls._memo[key]

    def tensors(self, torch, plans, packed):
        """Device tensors; the window rows no plan reads hold NaN."""
        k_win, v_win = self.k_win.copy(), self.v_win.copy()
        for l in range(LAYERS):
            for b in range(BS):
                dead = np.setdiff1d(np.arange(CAP), plans[l][b].ring if plans[l][b].live else [])
                k_win[l, b][:, dead] = v_win[l, b][:, dead] = np.float16("nan")
        dev = lambda a: R.to_dev(torch, a)
        return dict(k_win=dev(k_win), v_win=dev(v_win), kc=dev(self.k_cents), vc=dev(self.v_cents), ids=dev(self.ids))

    def pools(self, torch, packed):
        return [R.to_dev(torch, a) for a in R.fill_pools(self.n_pool, self.M, self.C, packed)]

    def expect(self, rows, n, min_r, packed):
        plans = [[R.FlushPlan(row, n, min_r) for row in rows[l]] for l in range(LAYERS)]
        want = R.fill_pools(self.n_pool, self.M, self.C, packed)
        for l in range(LAYERS):
            for b, p in enumerate(plans[l]):
                if p.live:
                    R.put(want, self.ids[l, b], p.tokens, p.kept, self.kc[l][b][:, p.ring], self.vc[l][b][:, p.ring], self.M, self.C, packed)
        return plans, want


def _same_pools(torch, got, want, what):
    for side, g, exp in zip("kv", got, want):
        g = R.to_np(torch, g)
        assert np.array_equal(g, exp), f"{what}: {side} pool differs in {int((g != exp).sum())} places"


def _lengths(torch, rows):
    return torch.tensor([[list(r) + [WORD3] for r in layer] for layer in rows], dtype=torch.int32).cuda()


@pytest.mark.parametrize("d,M,nbits,packed", CASES)
def test_encode_ahead_with_device_lengths(d, M, nbits, packed, env, oracle):
    torch, ops, L = env
    sc = Scene(oracle, d, M, nbits)
    plans, want = sc.expect(ROWS, PS, PS, packed)
    assert [[p.live for p in layer] for layer in plans] == [[True] * 3, [True] * 3, [True, True, False]]
    assert plans[0][0].ring[-1] < plans[0][0].ring[0] and all(p.T % PS for layer in plans for p in layer if p.T != 64)
    t = sc.tensors(torch, plans, packed)
    for pif in (1, 4, None):      # 9 pairs over 1 and 4 pairs in flight (some workgroups walk 3 pairs, some 2), and the library's rule
        pools, lengths = sc.pools(torch, packed), _lengths(torch, ROWS)
        before = lengths.clone()
        ops.pq_flush_wide(t["k_win"], t["v_win"], t["kc"], t["vc"], *pools, t["ids"], n=PS, page_size=PS, dev_lengths=lengths, min_r=PS,
                          packed=packed, advance=False, pairs_in_flight=pif)
        torch.cuda.synchronize()
        _same_pools(torch, pools, want, f"pairs_in_flight={pif}")
        assert torch.equal(lengths, before), "encode-ahead writes no word of the device rows"
    ops.lengths_advance(lengths[:2].view(-1, 4), PS, CAP)      # the commit of the layers whose every request took part
    torch.cuda.synchronize()
    got = lengths.cpu().numpy()
    assert got[:2, :, :3].tolist() == [[list(p.after) for p in layer] for layer in plans[:2]] and np.array_equal(got[2], before[2].cpu().numpy())
    assert ops.tail_faults() == 0


@pytest.mark.parametrize("d,M,nbits,packed", CASES)
def test_encode_ahead_with_host_lengths(d, M, nbits, packed, env, oracle):
    """dev_lengths=None: every (layer, request) encodes 32 rows from ring row 40 on to tokens [45, 77)."""
    torch, ops, L = env
    sc = Scene(oracle, d, M, nbits)
    rows = [[(45, CAP, 40)] * BS] * LAYERS
    plans, want = sc.expect(rows, PS, 0, packed)
    t = sc.tensors(torch, plans, packed)
    for pif in (1, 4, None):
        pools = sc.pools(torch, packed)
        ops.pq_flush_wide(t["k_win"], t["v_win"], t["kc"], t["vc"], *pools, t["ids"], n=PS, page_size=PS, token_start=45, x_row_start=40,
                          packed=packed, advance=False, pairs_in_flight=pif)
        torch.cuda.synchronize()
        _same_pools(torch, pools, want, f"host lengths, pairs_in_flight={pif}")
    # fewer rows than a block of tokens, one layer of the three through a view: the other layers' pages stay 0xA5
    rows1 = [[(45, CAP, 40)] * BS if l == 1 else [(0, 0, 0)] * BS for l in range(LAYERS)]
    plans1, want1 = sc.expect(rows1, 7, 1, packed)
    pools = sc.pools(torch, packed)
    ops.pq_flush_wide(t["k_win"][1:2], t["v_win"][1:2], t["kc"], t["vc"], *pools, t["ids"][1:2], n=7, page_size=PS, token_start=45, x_row_start=40,
                      packed=packed, advance=False)
    torch.cuda.synchronize()
    _same_pools(torch, pools, want1, "7 rows of layer 1")


@pytest.mark.parametrize("d,M,nbits,packed", CASES)
def test_layered_flush_equals_one_call_per_layer(d, M, nbits, packed, env, oracle):
    """advance=True with layers: the pools and the rows of LAYERS pq_flush_wide calls, and the rule's."""
    torch, ops, L = env
    sc = Scene(oracle, d, M, nbits)
    plans, want = sc.expect(ROWS, PS, 36, packed)      # min_r = 36: four of the nine take no part
    assert sum(p.live for layer in plans for p in layer) == 5
    t = sc.tensors(torch, plans, packed)
    kw = dict(n=PS, page_size=PS, min_r=36, packed=packed)
    one, one_len = sc.pools(torch, packed), _lengths(torch, ROWS)
    for l in range(LAYERS):
        ops.pq_flush_wide(t["k_win"][l], t["v_win"][l], t["kc"], t["vc"], *one, t["ids"][l], dev_lengths=one_len[l], **kw)
    all_, all_len = sc.pools(torch, packed), _lengths(torch, ROWS)
    ops.pq_flush_wide(t["k_win"], t["v_win"], t["kc"], t["vc"], *all_, t["ids"], dev_lengths=all_len, **kw)
    torch.cuda.synchronize()
    _same_pools(torch, all_, want, "layered flush")
    _same_pools(torch, one, want, "one call per layer")
    assert torch.equal(all_len, one_len)
    got = all_len.cpu().numpy()
    assert got[:, :, :3].tolist() == [[list(p.after) for p in layer] for layer in plans] and (got[:, :, 3] == WORD3).all()
    # host lengths: nothing to advance, the same pools as the encode-ahead form
    rows = [[(45, CAP, 40)] * BS] * LAYERS
    plans, want = sc.expect(rows, PS, 0, packed)
    t = sc.tensors(torch, plans, packed)
    pools = sc.pools(torch, packed)
    ops.pq_flush_wide(t["k_win"], t["v_win"], t["kc"], t["vc"], *pools, t["ids"], n=PS, page_size=PS, token_start=45, x_row_start=40, packed=packed)
    torch.cuda.synchronize()
    _same_pools(torch, pools, want, "layered flush, host lengths")


@pytest.mark.parametrize("packed", [False, True])
@pytest.mark.parametrize("which", [0, 1])
def test_encode_ahead_rows_are_clamped_not_trusted(which, packed, env, oracle):
    """Rows no cache would write, advance=False: clamped as load_len_row clamps them, a request below min_r skipped, a token past
    the table dropped - the whole pool is the rule's, the 0xA5 bytes included; no row is written."""
    torch, ops, L = env
    d, M, nbits = R.FORMATS[which]
    sc = Scene(oracle, d, M, nbits)
    plans, want = sc.expect(HOSTILE, PS, PS, packed)
    assert [[p.live for p in layer] for layer in plans] == [[True, False, True], [True, True, True], [True, False, True]]
    assert [[int(p.kept.sum()) for p in layer] for layer in plans] == [[0, 32, 32], [10, 0, 32], [32, 32, 31]]
    assert (plans[0][2].start, plans[1][2].T, plans[1][2].r, plans[1][2].start, plans[2][2].start) == (0, 0, CAP, 0, 0)
    t = sc.tensors(torch, plans, packed)
    for pif in (2, None):
        pools, lengths = sc.pools(torch, packed), _lengths(torch, HOSTILE)
        before = lengths.clone()
        ops.pq_flush_wide(t["k_win"], t["v_win"], t["kc"], t["vc"], *pools, t["ids"], n=PS, page_size=PS, dev_lengths=lengths, min_r=PS,
                          packed=packed, advance=False, pairs_in_flight=pif)
        torch.cuda.synchronize()
        _same_pools(torch, pools, want, f"hostile rows, pairs_in_flight={pif}")
        assert torch.equal(lengths, before)
    assert ops.tail_faults() == 0


# ---------------------------------------------------------------- the cache --------------------------------------------------
CBS, CL, N_PROMPT, N_DEC = 2, 3, 45, 100      # the window fills at step 64, then every 32 steps: 'pre' at 36 and 68, 'commit' at 64 and 96


class Streams:
    _memo = {}

    def __new__(cls, d, M, nbits):
        key = (d, M, nbits)
        if key not in cls._memo:
            self = object.__new__(cls)
            rs = np.random.RandomState(7000 + nbits + d)
            h = lambda *s: rs.standard_normal(s).astype(np.float16)
            self.d, self.M, self.C = d, M, 2 ** nbits
            self.ck, self.cv = h(M, self.C, d // M), h(M, self.C, d // M)
            n = N_PROMPT + N_DEC + 40
            self.K, self.V, self.Q = h(CL, CBS + 1, NHK, n, d), h(CL, CBS + 1, NHK, n, d), h(CL, CBS + 1, NH, n, d)
            cls._memo[key] = self
        return cls._memo[key]


def _cache(torch, s, nbits, packed, preallocate=True, bs=CBS, prompt=N_PROMPT):
    from million_amd.pq_cache import PagedPQCache
    c = PagedPQCache(bs=bs, nh=NH, num_key_value_heads=NHK, M=s.M, layer_num=CL, d=s.d, page_size=PS, extended_residual_size=CAP,
                     max_tokens=R.MAX_TOKENS, nbits=nbits, dtype=torch.uint16, packed=packed, preallocate=preallocate, device="cuda")
    c.set_cent(R.to_dev(torch, s.ck), R.to_dev(torch, s.cv))
    if prompt:
        for l in range(CL):
            c.prefill(*(R.to_dev(torch, X[l][:bs, :, :prompt]) for X in (s.Q, s.K, s.V)), l)
    return c


def _unpacked(torch, c):
    pools = [R.to_np(torch, c.key_page_pool), R.to_np(torch, c.value_page_pool)]
    return [P.unpack(pools[0], "k", PS, c.M, c.C), P.unpack(pools[1], "v", PS, c.M, c.C)] if c.packed else pools


def _twins(torch, a, b, what, dev_rows):
    """Mirrors, device rows, windows, and the live codes each slot reaches through its own page table."""
    for x, y in zip(a.host_state()[:4], b.host_state()[:4]):
        assert np.array_equal(x, y), (what, "mirror")
    assert torch.equal(a._kres_all.view(torch.int16), b._kres_all.view(torch.int16)) and torch.equal(a._vres_all.view(torch.int16), b._vres_all.view(torch.int16)), (what, "windows")
    if dev_rows:
        rows = a._lengths_all.cpu().numpy()
        assert np.array_equal(rows, b._lengths_all.cpu().numpy()), (what, "device rows")
        assert np.array_equal(rows[:, :, 0], a._T_a) and np.array_equal(rows[:, :, 1], a._r_a) and np.array_equal(rows[:, :, 2], a._rs_a), (what, "rows / mirror")
    pa, pb = _unpacked(torch, a), _unpacked(torch, b)
    ia, ib = a._page_ids_all.cpu().numpy(), b._page_ids_all.cpu().numpy()
    for l in range(a.layer_num):
        for s_ in range(a.bs):
            T = int(a._T_a[l, s_])
            ka, va = R.codes_of(pa, ia[l, s_], 0, T, a.M, a.C, False)
            kb, vb = R.codes_of(pb, ib[l, s_], 0, T, a.M, a.C, False)
            assert np.array_equal(ka, kb) and np.array_equal(va, vb), (what, l, s_, "codes")


MODES = ["host-lengths", "device-lengths", "on-demand", "spread", "graphs"]


@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("d,M,nbits,packed", CASES)
def test_encode_ahead_equals_the_inline_flush(d, M, nbits, packed, mode, env):
    torch, ops, L = env
    from million_amd import paged_turns
    s = Streams(d, M, nbits)
    use_dl = mode in ("device-lengths", "graphs", "on-demand")
    spread = 2 if mode == "spread" else 1
    ref, cache = (_cache(torch, s, nbits, packed, preallocate=mode != "on-demand") for _ in range(2))
    cache.encode_ahead_steps = spread      # the knob, not the default: the kinds below do not depend on the measured rule
    Kd, Vd, Qd = (R.to_dev(torch, X[:, :CBS]) for X in (s.K, s.V, s.Q))
    kn = [torch.empty(CBS, NHK, 1, d, device="cuda", dtype=torch.float16) for _ in range(CL)]
    vn = [torch.empty_like(kn[0]) for _ in range(CL)]
    qs = [torch.empty(CBS, NH, 1, d, device="cuda", dtype=torch.float16) for _ in range(CL)]
    outs = [torch.empty(CBS, NH, 1, d, device="cuda", dtype=torch.float16) for _ in range(CL)]

    def step():
        kind = paged_turns.begin_step(cache, use_dev_lengths=use_dl)
        for l in range(CL):
            paged_turns.decode(cache, qs[l], kn[l], vn[l], l, out=outs[l], use_dev_lengths=use_dl)
        return kind

    graphs = {}
    if mode == "graphs":
        st = cache.host_state()
        rows, win = cache._lengths_all.clone(), (cache._kres_all.clone(), cache._vres_all.clone())
        pools = (cache.key_page_pool.clone(), cache.value_page_pool.clone())
        for l in range(CL):
            kn[l].zero_(); vn[l].zero_(); qs[l].zero_()
        step()      # eager once: allocates the workspace (restored below)
        torch.cuda.synchronize()
        for name, state in cache.capture_states(st):
            cache.set_host_state(state)
            assert paged_turns.next_step_kind(cache) == name
            g = torch.cuda.CUDAGraph()
            with torch.cuda.graph(g):
                step()
            graphs[name] = g
        cache.set_host_state(st)
        cache._lengths_all.copy_(rows)
        cache._kres_all.copy_(win[0]); cache._vres_all.copy_(win[1])
        cache.key_page_pool.copy_(pools[0]); cache.value_page_pool.copy_(pools[1])
    kinds = []
    for i in range(N_DEC):
        t = N_PROMPT + i
        for l in range(CL):
            kn[l].copy_(Kd[l, :, :, t:t + 1]); vn[l].copy_(Vd[l, :, :, t:t + 1]); qs[l].copy_(Qd[l, :, :, t:t + 1])
        want = [paged_turns.decode(ref, qs[l], kn[l], vn[l], l, use_dev_lengths=use_dl).clone() for l in range(CL)]
        kind = paged_turns.next_step_kind(cache)
        assert cache.next_step_kind() in ("plain", "flush")
        kinds.append(kind)
        if graphs:
            graphs[kind].replay()
            paged_turns.note_replayed_step(cache, *(() if i % 2 else (kind,)))
        else:
            assert step() == kind
        torch.cuda.synchronize()
        for l in range(CL):
            assert torch.equal(outs[l].view(torch.int16).reshape(-1), want[l].view(torch.int16).reshape(-1)), f"step {i} ({kind}) layer {l}"
        _twins(torch, ref, cache, f"step {i} ({kind})", use_dl)
    pre = [i for i, k in enumerate(kinds) if k.startswith("pre")]
    assert len(pre) == 2 * spread and kinds.count("commit") == 2 and "flush" not in kinds
    assert pre[spread - 1] < kinds.index("commit") < pre[spread]
    assert [kinds[i] for i in pre] == (["pre0", "pre1"] if spread == 2 else ["pre"]) * 2
    assert int(ref._T_a[0, 0]) == N_PROMPT + 2 * PS and ops.tail_faults() == 0


def _decode_both(torch, paged_turns, s, caches, t, begin, use_dl=True, slots=None):
    """One step of the twins at stream position t[b] per slot: `begin` says which of them call begin_step.  Returns the kinds."""
    bs = caches[0].bs
    kinds = [paged_turns.begin_step(c, use_dev_lengths=use_dl) if on else None for c, on in zip(caches, begin)]
    for l in range(CL):
        q, k, v = (R.to_dev(torch, np.stack([X[l][b, :, t[b]:t[b] + 1] for b in range(bs)])) for X in (s.Q, s.K, s.V))
        outs = [paged_turns.decode(c, q, k, v, l, use_dev_lengths=use_dl) for c in caches]
        assert torch.equal(outs[0].view(torch.int16), outs[1].view(torch.int16)), (l, t)
    return kinds


@pytest.mark.parametrize("d,M,nbits,packed", [R.FORMATS[0] + (True,), R.FORMATS[1] + (False,), R.FORMATS[2] + (True,)])
def test_a_pre_step_then_verify_and_commit(d, M, nbits, packed, env):
    """The accepted rows overflow the window the 'pre' step encoded: the commit flushes it again, same codes, and clears the flags."""
    torch, ops, L = env
    from million_amd import paged_turns
    s = Streams(d, M, nbits)
    ref, cache = (_cache(torch, s, nbits, packed) for _ in range(2))
    cache.encode_ahead_steps = 1
    kinds = []
    for i in range(60):
        kinds.append(_decode_both(torch, paged_turns, s, (ref, cache), [N_PROMPT + i] * CBS, (False, True))[1])
    assert kinds.count("pre") == 1 and cache._pre_a.all() and int(cache._r_a[0, 0]) == 60
    t = N_PROMPT + 60
    for c in (ref, cache):
        for l in range(CL):
            paged_turns.verify(c, *(R.to_dev(torch, X[l][:CBS, :, t:t + 8]) for X in (s.Q, s.K, s.V)), l, n_draft=[8, 8])
        paged_turns.commit(c, [6, 6])      # 60 + 6 rows > 64: every request flushes inside the commit
    torch.cuda.synchronize()
    assert not cache._pre_a.any() and int(cache._T_a[0, 0]) == N_PROMPT + PS
    _twins(torch, ref, cache, "verify + commit", True)
    for i in range(6, 12):
        k = _decode_both(torch, paged_turns, s, (ref, cache), [N_PROMPT + 60 + i] * CBS, (False, True))[1]
        assert k in ("plain", "pre")
    torch.cuda.synchronize()
    _twins(torch, ref, cache, "steps after the commit", True)


@pytest.mark.parametrize("d,M,nbits,packed", [R.FORMATS[0] + (False,), R.FORMATS[1] + (True,)])
def test_a_pre_step_then_fork(d, M, nbits, packed, env):
    """Three requests in lockstep, a 'pre' step, then slot 2 is released and becomes a fork of slot 0's prompt (pages shared, the
    partly live tail page - which holds codes encoded ahead behind T - copied): the destination's flag is cleared and it holds
    no window, so the next full window is a 'flush' that encodes again, same codes."""
    torch, ops, L = env
    from million_amd import paged_turns
    s = Streams(d, M, nbits)
    ref, cache = (_cache(torch, s, nbits, packed, preallocate=False, bs=CBS + 1) for _ in range(2))
    cache.encode_ahead_steps = 1
    pos = [N_PROMPT] * (CBS + 1)
    kinds = []
    for i in range(R.CAP + 2):
        if i == 40:
            assert kinds.count("pre") == 1 and cache._pre_a.all()
            for c in (ref, cache):
                c.release(2)
                paged_turns.fork(c, 0, 2, n_tokens=N_PROMPT)
            assert not cache._pre_a[:, [0, 2]].any() and cache._pre_a[:, 1].all()      # the source was joined: its flag is cleared too
            pos[2] = N_PROMPT
        kinds.append(_decode_both(torch, paged_turns, s, (ref, cache), pos, (False, True))[1])
        pos = [p_ + 1 for p_ in pos]
    assert set(kinds[40:R.CAP]) == {"plain"} and kinds[R.CAP] == "flush" and "commit" not in kinds and kinds[R.CAP + 1] == "plain"
    torch.cuda.synchronize()
    _twins(torch, ref, cache, "fork", True)
    pa = _unpacked(torch, cache)
    ids = cache._page_ids_all.cpu().numpy()
    for l in range(CL):      # the fork and its source hold the same prompt codes
        a, b = R.codes_of(pa, ids[l, 0], 0, N_PROMPT, cache.M, cache.C, False), R.codes_of(pa, ids[l, 2], 0, N_PROMPT, cache.M, cache.C, False)
        assert np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1]), l
    assert ops.tail_faults() == 0


@pytest.mark.parametrize("d,M,nbits,packed", [R.FORMATS[0] + (True,), R.FORMATS[2] + (False,)])
def test_a_pre_step_then_release_and_a_shorter_prompt(d, M, nbits, packed, env):
    """The batch turns ragged: the kinds fall back to 'plain' / 'flush' and decoding with device lengths goes on."""
    torch, ops, L = env
    from million_amd import paged_turns
    s = Streams(d, M, nbits)
    ref, cache = (_cache(torch, s, nbits, packed) for _ in range(2))
    cache.encode_ahead_steps = 1
    pos = [N_PROMPT] * CBS
    kinds = []
    for i in range(40):
        kinds.append(_decode_both(torch, paged_turns, s, (ref, cache), pos, (False, True))[1])
        pos = [p + 1 for p in pos]
    assert kinds.count("pre") == 1 and cache._pre_a.all()
    for c in (ref, cache):
        c.release(1)
        for l in range(CL):
            c.prefill_request(1, *(R.to_dev(torch, X[l][1:2, :, :20]) for X in (s.Q, s.K, s.V)), l)
    pos[1] = 20
    assert not cache._pre_a[:, 1].any()
    kinds = []
    for i in range(R.CAP + 4):
        kinds.append(_decode_both(torch, paged_turns, s, (ref, cache), pos, (False, True))[1])
        pos = [p + 1 for p in pos]
    assert set(kinds) == {"plain", "flush"} and [i for i, k in enumerate(kinds) if k == "flush"] == [24, 56, 64]      # slot 0 twice, slot 1 at a step of its own
    torch.cuda.synchronize()
    _twins(torch, ref, cache, "release + prefill_request", True)
    assert ops.tail_faults() == 0
