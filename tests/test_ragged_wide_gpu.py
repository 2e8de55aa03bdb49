"""The ragged life of a wide PagedPQCache on the GPU (million_amd.paged_turns: prefill_ragged, decode, extend_ragged; DESIGN.md
4.19), per code format, uint16 and packed.

Prompts of 70 / 45 / 33 tokens arrive in one prefill_ragged call - on twin caches, device_store False and True, whose pools must
stay equal bit for bit; 70 decode steps with device lengths follow, slot 1 released after three of them and given a new prompt of
20, so that the windows fill at different steps (slots 0 and 2 at step 64, slot 1 at step 67: one flush launch serves each);
then extend_ragged with n_new = [5, 0, 9] and 3 more steps.  After every call the codes each slot reaches through its page
table are oracle.pq_encode of that request's own rows, bit for bit, its window ring rows are its last rows, and host mirror and
device rows are the per-request rule's integers.  Every decode output is within the suite's bar (finite, rel-L2 and mean-abs <
1e-3 per head: tests/test_attn_wide_gpu.py) of tests/wide_model.py's fp64 model, every extend output of tests/chunk_wide_model.py's,
rows past n_new[b] exact zeros.  A second test replays one captured `flush` step and one captured `plain` step, picked by
next_step_kind, beside an eager twin: the same outputs, pools, windows and lengths, bit for bit."""
import numpy as np
import pytest

from tests import chunk_wide_model as CM
from tests import ragged_wide_common as R
from tests import wide_model as W

pytestmark = pytest.mark.gpu

BS, NH, NHK, NL, PS, CAP = R.BS, R.NH, R.NHK, R.LAYERS, R.PS, R.CAP
PROMPTS, N_EXT, N_STREAM, SECOND = [70, 45, 33], [5, 0, 9], 200, 100      # SECOND: where slot 1's second request starts in its stream
TOL = 1e-3


@pytest.fixture(scope="module")
def env():
    import torch
    from million_amd import build, ops
    build.build()
    assert torch.cuda.is_available()
    return torch, ops


class Streams:
    """Every request's rows, seeded standard-normal fp16, and the oracle's codes of all of them - computed once per format."""
    _memo = {}

    def __new__(cls, oracle, d, M, nbits):
        key = (d, M, nbits)
        if key not in cls._memo:
            self = object.__new__(cls)
            rs = np.random.RandomState(1000 + nbits)
            h = lambda *s: rs.standard_normal(s).astype(np.float16)
            self.d, self.M, self.C = d, M, 2 ** nbits
            self.ck, self.cv = h(M, self.C, d // M), h(M, self.C, d // M)
            self.K, self.V, self.Q = h(NL, BS, NHK, N_STREAM, d), h(NL, BS, NHK, N_STREAM, d), h(NL, BS, NH, N_STREAM, d)
            self.Kc = [oracle.pq_encode(self.K[l], self.ck) for l in range(NL)]
            self.Vc = [oracle.pq_encode(self.V[l], self.cv) for l in range(NL)]
            assert self.Kc[0].dtype == np.uint16 and (self.Kc[0] >= 256).any() and (self.Vc[0] >= 256).any()
            cls._memo[key] = self
        return cls._memo[key]


def _cache(torch, s, nbits, packed):
    from million_amd.pq_cache import PagedPQCache
    c = PagedPQCache(bs=BS, nh=NH, num_key_value_heads=NHK, M=s.M, layer_num=NL, d=s.d, page_size=PS, extended_residual_size=CAP,
                     max_tokens=R.MAX_TOKENS, nbits=nbits, dtype=torch.uint16, packed=packed, device="cuda")
    c.set_cent(R.to_dev(torch, s.ck), R.to_dev(torch, s.cv))
    return c


class Rule:
    """The per-request integers: {T, r, start} and where the request's rows start in its stream."""

    def __init__(self):
        self.T, self.r, self.st, self.base = [0] * BS, [0] * BS, [0] * BS, [0] * BS

    def seen(self, b):
        return self.T[b] + self.r[b]

    def prefill(self, b, n, base=0):
        self.T[b], self.r[b], self.st[b], self.base[b] = n, 0, 0, base

    def flush_if_full(self, b):
        if self.r[b] >= CAP:
            self.T[b], self.r[b], self.st[b] = self.T[b] + PS, self.r[b] - PS, (self.st[b] + PS) % CAP
            return True
        return False

    def extend(self, b, n):
        self.T[b], self.r[b], self.st[b] = self.T[b] + self.r[b] + n, 0, 0


def _check_state(torch, s, cache, rule, what):
    pools = [R.to_np(torch, cache.key_page_pool), R.to_np(torch, cache.value_page_pool)]
    for l in range(NL):
        ids = cache.page_ids[l].cpu().numpy()
        dev = cache.lengths[l].cpu().numpy()
        kwin, vwin = cache.key_residual_cache[l].cpu().numpy(), cache.value_residual_cache[l].cpu().numpy()
        for b in range(BS):
            T, r, st, base = rule.T[b], rule.r[b], rule.st[b], rule.base[b]
            assert (int(cache._T_a[l, b]), int(cache._r_a[l, b]), int(cache._rs_a[l, b])) == (T, r, st), (what, l, b, "mirror")
            assert dev[b, :3].tolist() == [T, r, st], (what, l, b, "device row", dev[b].tolist())
            k, v = R.codes_of(pools, ids[b], 0, T, s.M, s.C, cache.packed)
            assert np.array_equal(k, s.Kc[l][b, :, base:base + T]) and np.array_equal(v, s.Vc[l][b, :, base:base + T]), (what, l, b, "codes")
            ring = (st + np.arange(r)) % CAP
            assert np.array_equal(kwin[b][:, ring].view(np.uint16), s.K[l][b, :, base + T:base + T + r].view(np.uint16)), (what, l, b, "K window")
            assert np.array_equal(vwin[b][:, ring].view(np.uint16), s.V[l][b, :, base + T:base + T + r].view(np.uint16)), (what, l, b, "V window")


def _window(s, X, l, b, rule):
    res = np.zeros((1, NHK, CAP, s.d), np.float16)
    t0 = rule.base[b] + rule.T[b]
    res[0, :, :rule.r[b]] = X[l][b, :, t0:t0 + rule.r[b]]
    return res


def _bar(got, ref, what):
    rel, mabs = W.head_errors(got, ref)
    assert np.isfinite(got).all(), f"{what}: non-finite output"
    assert np.isfinite(rel).all() and rel.max() < TOL and mabs.max() < TOL, f"{what}: worst rel-L2 {rel.max():.3e} mean-abs {mabs.max():.3e}"
    return float(rel.max()), float(mabs.max())


def _step_inputs(torch, s, l, rule):
    t = [rule.base[b] + rule.seen(b) for b in range(BS)]
    pick = lambda X: R.to_dev(torch, np.stack([X[l][b, :, t[b]:t[b] + 1] for b in range(BS)]))
    return pick(s.Q), pick(s.K), pick(s.V)


def _twins_equal(torch, a, b, what):
    for x, y in ((a.key_page_pool, b.key_page_pool), (a.value_page_pool, b.value_page_pool), (a._lengths_all, b._lengths_all),
                 (a._page_ids_all, b._page_ids_all)):
        assert np.array_equal(R.to_np(torch, x), R.to_np(torch, y)), what
    for x, y in zip(a.host_state(), b.host_state()):
        assert np.array_equal(x, y), what


@pytest.mark.parametrize("d,M,nbits,packed", [f + (p,) for f in R.FORMATS for p in (False, True)])
def test_a_ragged_life(env, oracle, d, M, nbits, packed):
    torch, ops = env
    from million_amd import paged_turns
    s = Streams(oracle, d, M, nbits)
    caches = [_cache(torch, s, nbits, packed) for _ in range(2)]      # device_store False / True
    rule = Rule()
    worst = [0.0, 0.0]

    # 1. three prompts, one attention launch
    n = max(PROMPTS)
    for l in range(NL):
        q, k, v = (R.to_dev(torch, X[l][:, :, :n]) for X in (s.Q, s.K, s.V))
        with pytest.raises(NotImplementedError, match="nbits"):
            caches[0].prefill_ragged(q, k, v, l, PROMPTS)
        outs = [paged_turns.prefill_ragged(c, q, k, v, l, PROMPTS, device_store=ds) for c, ds in zip(caches, (False, True))]
        assert torch.equal(outs[0].view(torch.int16), outs[1].view(torch.int16))
        for b, nb in enumerate(PROMPTS):
            assert not outs[0][b, :, nb:].any(), "rows past n_new are zeros"
    for b, nb in enumerate(PROMPTS):
        rule.prefill(b, nb)
    _check_state(torch, s, caches[0], rule, "prefill_ragged")
    _twins_equal(torch, *caches, "prefill_ragged")

    # 2. decode with device lengths; slot 1 recycled after three steps
    def decode_steps(first, count):
        for step in range(first, first + count):
            if step == 3:
                for c in caches:
                    c.release(1)
                    for l in range(NL):
                        q, k, v = (R.to_dev(torch, X[l][1:2, :, SECOND:SECOND + 20]) for X in (s.Q, s.K, s.V))
                        c.prefill_request(1, q, k, v, l)
                rule.prefill(1, 20, base=SECOND)
                _check_state(torch, s, caches[0], rule, "release + prefill_request")
            full = [rule.r[b] >= CAP for b in range(BS)]
            assert caches[0].next_step_kind() == ("flush" if any(full) else "plain")
            if any(full):
                flushes.append((step, [b for b in range(BS) if full[b]]))
                with pytest.raises(RuntimeError, match="lockstep"):      # the cache's own step still serves lockstep batches only
                    caches[0].decoding_with_pages(*_step_inputs(torch, s, 0, rule), 0, use_dev_lengths=True)
            for l in range(NL):
                q, k, v = _step_inputs(torch, s, l, rule)
                outs = [paged_turns.decode(c, q, k, v, l, use_dev_lengths=True) for c in caches]
                assert torch.equal(outs[0].view(torch.int16), outs[1].view(torch.int16))
                got = outs[0].float().cpu().numpy().reshape(BS, NH, 1, s.d)
                for b in range(BS):
                    after = Rule.__new__(Rule)
                    after.__dict__ = {k_: list(v_) for k_, v_ in rule.__dict__.items()}
                    after.flush_if_full(b)
                    t0, t = after.base[b], after.base[b] + after.seen(b)
                    ref = W.decode_attn(s.Q[l][b:b + 1, :, t:t + 1], s.Kc[l][b:b + 1, :, t0:t0 + after.T[b]], s.Vc[l][b:b + 1, :, t0:t0 + after.T[b]],
                                        s.ck, s.cv, _window(s, s.K, l, b, after), _window(s, s.V, l, b, after), after.r[b],
                                        k_new=s.K[l][b:b + 1, :, t:t + 1], v_new=s.V[l][b:b + 1, :, t:t + 1])[0]
                    e = _bar(got[b:b + 1], ref, f"decode step {step} layer {l} slot {b}")
                    worst[0], worst[1] = max(worst[0], e[0]), max(worst[1], e[1])
            for b in range(BS):
                rule.flush_if_full(b)
                rule.r[b] += 1
            _check_state(torch, s, caches[0], rule, f"decode step {step}")

    flushes = []
    decode_steps(0, 70)
    assert flushes == [(64, [0, 2]), (67, [1])], flushes      # every slot flushed once, slot 1 at a step of its own
    assert rule.T == [102, 52, 65] and rule.st == [PS] * BS
    _twins_equal(torch, *caches, "decode")

    # 3. extend_ragged, both stores
    n = max(N_EXT)
    for l in range(NL):
        t = [rule.base[b] + rule.seen(b) for b in range(BS)]
        pad = lambda X: np.stack([X[l][b, :, t[b]:t[b] + n] for b in range(BS)])
        qn, kn, vn = pad(s.Q), pad(s.K), pad(s.V)
        for b, nb in enumerate(N_EXT):      # rows past n_new hold NaN: never read by the attention launch nor by the store
            qn[b, :, nb:] = kn[b, :, nb:] = vn[b, :, nb:] = np.nan
        q, k, v = (R.to_dev(torch, x) for x in (qn, kn, vn))
        with pytest.raises(NotImplementedError, match="nbits"):
            caches[0].extend_ragged(q, k, v, l, N_EXT)
        outs = [paged_turns.extend_ragged(c, q, k, v, l, N_EXT, device_store=ds) for c, ds in zip(caches, (False, True))]
        assert torch.equal(outs[0].view(torch.int16), outs[1].view(torch.int16))
        got = outs[0].float().cpu().numpy()
        for b, nb in enumerate(N_EXT):
            assert not got[b, :, nb:].any(), "rows past n_new are zeros"
            if nb:
                t0 = rule.base[b]
                ref = CM.chunk_attn(s.Q[l][b:b + 1, :, t[b]:t[b] + nb], s.Kc[l][b:b + 1, :, t0:t0 + rule.T[b]], s.Vc[l][b:b + 1, :, t0:t0 + rule.T[b]],
                                    s.ck, s.cv, _window(s, s.K, l, b, rule), _window(s, s.V, l, b, rule), rule.r[b],
                                    k_chunk=s.K[l][b:b + 1, :, t[b]:t[b] + nb], v_chunk=s.V[l][b:b + 1, :, t[b]:t[b] + nb])[0]
                rel, mabs = CM.head_errors(got[b:b + 1, :, :nb], ref)
                assert np.isfinite(got[b]).all() and rel.max() < TOL and mabs.max() < TOL, (l, b, rel.max(), mabs.max())
    for b, nb in enumerate(N_EXT):
        if nb:
            rule.extend(b, nb)
    _check_state(torch, s, caches[0], rule, "extend_ragged")
    _twins_equal(torch, *caches, "extend_ragged")

    # 4. three more steps
    decode_steps(70, 3)
    _twins_equal(torch, *caches, "the end")
    assert ops.tail_faults() == 0
    print(f"worst decode head: rel-L2 {worst[0]:.3e}, mean-abs {worst[1]:.3e}")


@pytest.mark.parametrize("d,M,nbits,packed", [R.FORMATS[0] + (True,), R.FORMATS[1] + (False,)])
def test_captured_steps_follow_the_rows(env, oracle, d, M, nbits, packed):
    """One graph per step kind, captured once: the flush launch inside the `flush` graph is gated on the device, so the same graph
    serves the step at which slots 0 and 2 flush and the step at which slot 1 does."""
    torch, ops = env
    from million_amd import paged_turns
    s = Streams(oracle, d, M, nbits)
    eager, graph = _cache(torch, s, nbits, packed), _cache(torch, s, nbits, packed)
    rule = Rule()
    n = max(PROMPTS)
    for c in (eager, graph):
        for l in range(NL):
            q, k, v = (R.to_dev(torch, X[l][:, :, :n]) for X in (s.Q, s.K, s.V))
            paged_turns.prefill_ragged(c, q, k, v, l, PROMPTS, device_store=True)
    for b, nb in enumerate(PROMPTS):
        rule.prefill(b, nb)
    static = [[torch.zeros(BS, H, 1, s.d, dtype=torch.float16, device="cuda") for H in (NH, NHK, NHK)] for _ in range(NL)]
    outs = [torch.zeros(BS, NH, 1, s.d, dtype=torch.float16, device="cuda") for _ in range(NL)]

    def run_static(c):
        for l in range(NL):
            paged_turns.decode(c, *static[l], l, out=outs[l], use_dev_lengths=True)

    def load(rule):
        for l in range(NL):
            for dst, src in zip(static[l], _step_inputs(torch, s, l, rule)):
                dst.copy_(src)

    def advance(rule):
        for b in range(BS):
            rule.flush_if_full(b)
            rule.r[b] += 1

    graphs = {}
    for step in range(70):
        if step == 3:      # both caches are warm (workspace allocated, modules loaded): capture the two kinds, then recycle slot 1
            st = graph.host_state()
            dev_before = graph._lengths_all.clone()
            for kind, r_all in (("plain", 0), ("flush", CAP)):
                graph.set_host_state((st[0], np.full_like(st[1], r_all), st[2], st[3], st[4]))
                assert graph.next_step_kind() == kind
                g = torch.cuda.CUDAGraph()
                with torch.cuda.graph(g):
                    run_static(graph)
                graphs[kind] = g
            graph.set_host_state(st)
            torch.cuda.synchronize()
            assert torch.equal(graph._lengths_all, dev_before), "captured, not run"
            for c in (eager, graph):
                c.release(1)
                for l in range(NL):
                    q, k, v = (R.to_dev(torch, X[l][1:2, :, SECOND:SECOND + 20]) for X in (s.Q, s.K, s.V))
                    c.prefill_request(1, q, k, v, l)
            rule.prefill(1, 20, base=SECOND)
        load(rule)
        kind = eager.next_step_kind()
        assert kind == graph.next_step_kind() == ("flush" if any(r >= CAP for r in rule.r) else "plain")
        run_static(eager)
        want = [o.clone() for o in outs]
        if step < 3:
            run_static(graph)
        else:
            graphs[kind].replay()
            graph.note_replayed_step(kind)
        torch.cuda.synchronize()
        for l in range(NL):
            assert torch.equal(outs[l].view(torch.int16), want[l].view(torch.int16)), (step, l)
        advance(rule)
        if step in (2, 63, 64, 66, 67, 69):
            _check_state(torch, s, graph, rule, f"replayed step {step}")
            _twins_equal(torch, eager, graph, f"step {step}")
            for a, b_ in ((eager._kres_all, graph._kres_all), (eager._vres_all, graph._vres_all)):
                assert torch.equal(a.view(torch.int16), b_.view(torch.int16)), step
    assert rule.T == [102, 52, 65]
