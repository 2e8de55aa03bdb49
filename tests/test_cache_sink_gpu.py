"""PagedPQCache(sink_tokens=S) on the GPU: the first S tokens of a request stay exact fp16 rows beside the pages and every
attention call of the cache merges them in (ops.attn_sink_merge behind decode, extend and verify).

Two references.  The twin: a cache without sinks that was given the rows behind the sinks - same pages, same codes, same lengths,
and its outputs merged by hand with the sink rows are the cache's outputs bit for bit.  The model: tests/sink_model.py in fp64 over
[exact sink rows; dequantised codes; window; new rows], at the project's bars (rel-L2 and mean-abs < 1e-3, LSE_TOL on lse).

The smallest geometry that reaches every transition: 2 layers, 2 requests, 4 query heads on 2 kv heads, d = 128, M = 64, pages
and window of 64 rows, 4 sink rows."""
import numpy as np
import pytest

from tests import lse_ref as R
from tests import sink_model as SM

pytestmark = pytest.mark.gpu

GEOM = dict(bs=2, nh=4, num_key_value_heads=2, M=64, layer_num=2, d=128, page_size=64, extended_residual_size=64, max_tokens=1024)
BS, NH, NK, NL, D, M, C, S = 2, 4, 2, 2, 128, 64, 256, 4
REL, MABS = 1e-3, 1e-3


@pytest.fixture(scope="module")
def env():
    import torch
    assert torch.cuda.is_available(), "GPU tests need an MI355X"
    from million_amd import ops, _lib
    _lib.load()
    rs = np.random.RandomState(4242)
    cents = rs.standard_normal((M, C, D // M)).astype(np.float16), rs.standard_normal((M, C, D // M)).astype(np.float16)
    yield torch, ops, cents
    assert ops.tail_faults() == 0


def _cache(env, sinks, **over):
    torch, _, cents = env
    from million_amd.pq_cache import PagedPQCache
    c = PagedPQCache(**dict(GEOM, **over), sink_tokens=sinks)
    c.set_cent(torch.from_numpy(cents[0]).cuda(), torch.from_numpy(cents[1]).cuda())
    return c


def _rows(torch, rs, bs, n):
    """q (bs, nh, n, d), k, v (bs, nh_k, n, d): fp16 on the device."""
    mk = lambda h: torch.from_numpy(rs.standard_normal((bs, h, n, D)).astype(np.float16)).cuda()
    return mk(NH), mk(NK), mk(NK)


def _np(t):
    return t.detach().cpu().numpy()


def _bits(a, b):
    import torch
    v = lambda x: x.view(torch.int16) if x.dtype == torch.float16 else x.view(torch.int32) if x.dtype == torch.float32 else x
    return torch.equal(v(a), v(b))


def _same_store(A, B, what):
    """Pages, codes, windows, lengths on host and device: equal.  seen differs by the sink rows."""
    import torch
    for name in ("_page_ids_all", "key_page_pool", "value_page_pool", "_kres_all", "_vres_all", "_lengths_all"):
        assert torch.equal(getattr(A, name), getattr(B, name)), (what, name)
    for name in ("_T_a", "_r_a", "_rs_a", "_pages_a"):
        assert np.array_equal(getattr(A, name), getattr(B, name)), (what, name)
    assert np.array_equal(A._seen_a, B._seen_a + A._sink_a), what
    assert A._sink_all.cpu().numpy().tolist() == A._sink_a.tolist(), what


def _deq(env, cache, l):
    """Per request: the dequantised K and V codes (nh_k, T_b, d) of layer l, from the cache's own pages."""
    from oracle import oracle as O
    cents = env[2]
    Ts = [int(x) for x in cache._T_a[l]]
    if max(Ts) == 0:
        z = np.zeros((NK, 0, D))
        return [(z, z)] * cache.bs
    kc, vc = cache._codes_rowmajor(l, max(Ts))
    dk, dv = O.pq_decode_numpy(_np(kc), cents[0]), O.pq_decode_numpy(_np(vc), cents[1])
    return [(dk[b, :, :Ts[b]], dv[b, :, :Ts[b]]) for b in range(cache.bs)]


def _check(got_out, want_out, got_lse, want_lse, what):
    rel, mabs = SM.errors(got_out, want_out)
    dl = 0.0
    if got_lse is not None:
        fin = np.isfinite(want_lse)
        assert np.array_equal(np.isneginf(got_lse), np.isneginf(want_lse)), what
        dl = float(np.abs(got_lse[fin] - want_lse[fin]).max()) if fin.any() else 0.0
    print(f"{what}: rel-L2 {rel:.3e} mean-abs {mabs:.3e} lse {dl:.3e}")
    assert rel < REL and mabs < MABS and dl <= R.LSE_TOL, (what, rel, mabs, dl)


class Pair:
    """Cache A with sinks, its twin B without, and the model's requests of every (layer, slot); the same calls go to all three."""

    def __init__(self, env, seed, **over):
        self.env, self.torch, self.ops = env, env[0], env[1]
        self.rs = np.random.RandomState(seed)
        self.A, self.B = _cache(env, S, **over), _cache(env, 0, **over)
        self.req = [[SM.Request(S, NK, D) for _ in range(BS)] for _ in range(NL)]

    def prefill(self, b, n, full=None):
        """prefill_request of n rows into slot b, every layer; B gets the rows behind the sinks.  full: a cache without sinks
        that takes the whole prompt - its prompt attention is A's, bit for bit."""
        s = min(S, n)
        for l in range(NL):
            q, k, v = _rows(self.torch, self.rs, 1, n)
            out = self.A.prefill_request(b, q, k, v, l)
            if full is not None:
                assert _bits(out, full.prefill_request(b, q, k, v, l)), ("prefill", b, n, l)
            if n > s:
                self.B.prefill_request(b, q[:, :, s:].contiguous(), k[:, :, s:].contiguous(), v[:, :, s:].contiguous(), l)
            self.req[l][b].store(_np(k[0]), _np(v[0]))
        assert self.A._sink_a[:, b].tolist() == [s] * NL

    def hand(self, l, q, out, lse, dev_n=None, sel=slice(None)):
        """B's (out, lse) merged with A's sink rows by a hand call."""
        A = self.A
        return self.ops.attn_sink_merge(q, A._ksink_all[l][sel], A._vsink_all[l][sel], out, lse, dev_s=A._sink_all[l][sel], dev_n=dev_n,
                                        return_lse=True)

    def decode(self, what, with_lse=False, model=False):
        """One decode step of every layer: A equals the hand-merged twin bit for bit; model=True: and the model."""
        for l in range(NL):
            q, k, v = _rows(self.torch, self.rs, BS, 1)
            got = self.A.decoding_with_pages(q, k, v, l, use_dev_lengths=True, return_lse=with_lse)
            ob, lb = self.B.decoding_with_pages(q, k, v, l, use_dev_lengths=True, return_lse=True)
            ho, hl = self.hand(l, q, ob, lb)
            if with_lse:
                assert _bits(got[0], ho) and _bits(got[1], hl), (what, l)
                got, got_lse = got[0], _np(got[1]).astype(np.float64)
            else:
                assert _bits(got, ho), (what, l)
                got_lse = None
            for b in range(BS):
                self.req[l][b].append(_np(k[b]), _np(v[b]))
            if model:
                deq = _deq(self.env, self.A, l)
                for b in range(BS):
                    K, V = self.req[l][b].keys(*deq[b])
                    wo, wl = SM.attend_rows(_np(q[b]).astype(np.float64), K, V)
                    _check(_np(got[b].float()), wo, None if got_lse is None else got_lse[b], wl, f"{what} layer {l} slot {b}")

    def same(self, what):
        _same_store(self.A, self.B, what)


# ---------------------------------------------------------------- the twin ------------------------------------------------
@pytest.mark.parametrize("prompts", [(3, 70), (4, 200)])
def test_twin_bitwise_and_model_over_a_flush(env, prompts):
    p = Pair(env, 100 + prompts[1])
    full = _cache(env, 0)
    for b, n in enumerate(prompts):
        p.prefill(b, n, full=full)
    p.same("after prefill")
    assert p.A._T_a[0].tolist() == [n - min(S, n) for n in prompts] and p.A._seen_a[0].tolist() == list(prompts)
    T0 = p.A._T_a.copy()
    for t in range(70):
        p.decode(f"prompts {prompts} step {t}", with_lse=bool(t & 1), model=t in (0, 1, 64, 69))
    p.same("after 70 steps")
    assert (p.A._T_a == T0 + 64).all() and (p.A._r_a == 6).all()      # every window flushed once
    st = p.A.get_cache_stats()
    assert st["sink_rows_live"] == NL * sum(min(S, n) for n in prompts)
    assert st["memory_breakdown"]["sink_memory_mb"] == 2 * NL * BS * NK * S * D * 2 / 2 ** 20


# ---------------------------------------------------------------- extend, verify, commit ----------------------------------
def _extend_model(p, l, b, q, k, v, n):
    """The model's (out, lse) of n chunk rows of slot b: keys [sinks; codes; window; chunk], the chunk causally."""
    deq = _deq(p.env, p.A, l)[b]
    K, V = p.req[l][b].keys(*deq, extra_k=_np(k[:, :n]), extra_v=_np(v[:, :n]))
    return SM.attend_rows(_np(q[:, :n]).astype(np.float64), K, V, SM.causal_tail_mask(n, K.shape[1]))


def test_extend_verify_commit_against_the_model_and_the_twin(env):
    torch, ops, _ = env
    p = Pair(env, 7)
    A, B = p.A, p.B
    p.prefill(0, 70)
    p.prefill(1, 3)
    # a slot that holds nothing but sinks takes a chunk: chunk attention over the chunk, merged with the sinks
    for l in range(NL):
        q, k, v = _rows(torch, p.rs, 1, 5)
        want = _extend_model(p, l, 1, q[0], k[0], v[0], 5)
        out, lse = A.extend_request(1, q, k, v, l, return_lse=True)
        ob, lb = B.extend_request(1, q, k, v, l, return_lse=True)
        assert _bits(out, p.hand(l, q, ob, lb, sel=slice(1, 2))[0])
        _check(_np(out[0].float()), want[0], _np(lse[0]).astype(np.float64), want[1], f"extend_request sinks-only layer {l}")
        p.req[l][1].store(_np(k[0]), _np(v[0]))
    assert A._sink_a[:, 1].tolist() == [3, 3] and A._T_a[:, 1].tolist() == [5, 5] and A._seen_a[:, 1].tolist() == [8, 8]
    for t in range(5):
        p.decode(f"decode {t}")
    # extend_request on a slot with codes and a window
    for l in range(NL):
        q, k, v = _rows(torch, p.rs, 1, 5)
        want = _extend_model(p, l, 0, q[0], k[0], v[0], 5)
        out = A.extend_request(0, q, k, v, l)
        B.extend_request(0, q, k, v, l)
        _check(_np(out[0].float()), want[0], None, None, f"extend_request layer {l}")
        p.req[l][0].store(_np(k[0]), _np(v[0]))
    p.same("after extend_request")
    p.decode("decode behind extend_request", model=True)
    # extend_ragged: 40 and 5 rows in one launch; the rows past n_new[b] hold NaN and come back as zeros
    n_new = [40, 5]
    for l in range(NL):
        q, k, v = _rows(torch, p.rs, BS, 40)
        q[1, :, 5:], k[1, :, 5:], v[1, :, 5:] = float("nan"), float("nan"), float("nan")
        wants = [_extend_model(p, l, b, q[b], k[b], v[b], n_new[b]) for b in range(BS)]
        out = A.extend_ragged(q, k, v, l, n_new)
        B.extend_ragged(q, k, v, l, n_new)
        for b in range(BS):
            _check(_np(out[b, :, :n_new[b]].float()), wants[b][0], None, None, f"extend_ragged layer {l} slot {b}")
            assert (out[b, :, n_new[b]:] == 0).all()
            p.req[l][b].store(_np(k[b, :, :n_new[b]]), _np(v[b, :, :n_new[b]]))
    p.same("after extend_ragged")
    for t in range(3):
        p.decode(f"decode behind extend_ragged {t}", model=t == 2)

    # ---- verify: a chain of 4 and a tree of 6, both routes, against the model; nothing moves
    def verify_model(l, q, k, v, n_draft, parents):
        deq = _deq(env, A, l)
        res = []
        for b in range(BS):
            nb = n_draft[b]
            K, V = p.req[l][b].keys(*deq[b], extra_k=_np(k[b, :, :nb]), extra_v=_np(v[b, :, :nb]))
            mask = SM.causal_tail_mask(nb, K.shape[1]) if parents is None else SM.tree_tail_mask(list(parents[:nb]), K.shape[1])
            res.append(SM.attend_rows(_np(q[b, :, :nb]).astype(np.float64), K, V, mask))
        return res

    tree = [-1, 0, 0, 1, 1, 2]
    for n, n_draft, parents in ((4, [4, 2], None), (6, [6, 4], tree)):
        for route in ("heads", "chunk"):
            for l in range(NL):
                q, k, v = _rows(torch, p.rs, BS, n)
                wants = verify_model(l, q, k, v, n_draft, parents)
                out, lse = A.verify(q, k, v, l, n_draft=n_draft, route=route, return_lse=True, tree=parents)
                plain = A.verify(q, k, v, l, n_draft=n_draft, route=route, tree=parents)
                assert _bits(out, plain)
                for b in range(BS):
                    nb = n_draft[b]
                    _check(_np(out[b, :, :nb].float()), wants[b][0], _np(lse[b, :, :nb]).astype(np.float64), wants[b][1],
                           f"verify n={n} tree={parents is not None} route={route} layer {l} slot {b}")
                    assert (out[b, :, nb:] == 0).all() and torch.isneginf(lse[b, :, nb:]).all()
    p.same("after verify: pure")

    # ---- commit of a verified chain on both caches, then decode on: the twin's bits
    n_draft, n_accept = [4, 2], [3, 1]
    for l in range(NL):
        q, k, v = _rows(torch, p.rs, BS, 4)
        out = A.verify(q, k, v, l, n_draft=n_draft)
        ob, lb = B.verify(q, k, v, l, n_draft=n_draft, return_lse=True)
        assert _bits(out, p.hand(l, q, ob, lb, dev_n=torch.tensor(n_draft, dtype=torch.int32).cuda())[0])
        for b in range(BS):
            p.req[l][b].append(_np(k[b, :, :n_accept[b]]), _np(v[b, :, :n_accept[b]]))
    seen = A._seen_a.copy()
    A.commit(n_accept)
    B.commit(n_accept)
    assert np.array_equal(A._seen_a, seen + np.asarray(n_accept)[None, :])
    p.same("after commit")
    for t in range(2):
        p.decode(f"decode behind commit {t}", with_lse=True, model=True)
    p.same("at the end")


# ---------------------------------------------------------------- fork, release -------------------------------------------
@pytest.mark.parametrize("n_tokens", [None, 40])
@pytest.mark.parametrize("preallocate", [True, False], ids=["preallocated", "on-demand"])
def test_fork_decodes_the_sources_bits(env, preallocate, n_tokens):
    torch, ops, _ = env
    rs = np.random.RandomState(55)
    A = _cache(env, S, preallocate=preallocate)
    W = _cache(env, S, preallocate=preallocate)      # the slow way: slot 1 is given what the fork should leave there
    prompt = [_rows(torch, rs, 1, 70) for _ in range(NL)]
    for l in range(NL):
        A.prefill_request(0, *prompt[l], l)
        W.prefill_request(0, *prompt[l], l)
        if n_tokens is not None:
            q, k, v = (x[:, :, :S + n_tokens].contiguous() for x in prompt[l])
            W.prefill_request(1, q, k, v, l)
    steps = [[_rows(torch, rs, 1, 1) for _ in range(NL)] for _ in range(5)]
    both = lambda x: x.expand(BS, -1, -1, -1).contiguous()
    if n_tokens is None:      # the source with a window: three steps before the fork (slot 1 of A idles along and is released)
        for t in range(3):
            for l in range(NL):
                A.decoding_with_pages(*map(both, steps[t][l]), l, use_dev_lengths=True)
        A.release(1)
    A.fork(0, 1, n_tokens=n_tokens)
    assert A._sink_a.tolist() == [[S, S]] * NL and A._sink_all.cpu().numpy().tolist() == [[S, S]] * NL
    assert torch.equal(A._ksink_all[:, 1], A._ksink_all[:, 0]) and torch.equal(A._vsink_all[:, 1], A._vsink_all[:, 0])
    if n_tokens is None:
        assert A._seen_a[:, 1].tolist() == A._seen_a[:, 0].tolist() == [73] * NL
    else:
        assert A._T_a[:, 1].tolist() == [n_tokens] * NL and A._seen_a[:, 1].tolist() == [n_tokens + S] * NL
        assert torch.equal(A._sink_all, W._sink_all) and torch.equal(A._ksink_all, W._ksink_all)
    for t in range(3, 5):
        for l in range(NL):
            q, k, v = map(both, steps[t][l])
            out = A.decoding_with_pages(q, k, v, l, use_dev_lengths=True)
            if n_tokens is None:
                assert _bits(out[1], out[0]), (t, l)      # the fork decodes the source's bits
            else:
                assert _bits(out, W.decoding_with_pages(q, k, v, l, use_dev_lengths=True)), (t, l)
    # release, then a prompt of 2 rows: the slot keeps 2 sink rows
    A.release(1)
    assert A._sink_a[:, 1].tolist() == [0] * NL and A._sink_all[:, 1].cpu().tolist() == [0] * NL and A._sink_a[:, 0].tolist() == [S] * NL
    for l in range(NL):
        A.prefill_request(1, *_rows(torch, rs, 1, 2), l)
    assert A._sink_a[:, 1].tolist() == [2] * NL and A._sink_all[:, 1].cpu().tolist() == [2] * NL
    assert A._T_a[:, 1].tolist() == [0] * NL and A._seen_a[:, 1].tolist() == [2] * NL


# ---------------------------------------------------------------- a captured step -----------------------------------------
def test_captured_step_follows_release_and_a_new_prompt(env):
    """One graph of a two-layer decode step with device lengths (single stream, no side work).  The sink counts are read on the
    device: the same graph serves slot 1 before and after it was released and given a shorter prompt."""
    torch, ops, _ = env
    rs = np.random.RandomState(91)
    G, E = _cache(env, S), _cache(env, S)      # replayed, eager
    for b, n in ((0, 70), (1, 20)):
        for l in range(NL):
            rows = _rows(torch, rs, 1, n)
            G.prefill_request(b, *rows, l)
            E.prefill_request(b, *rows, l)
    qs, kn, vn = zip(*[_rows(torch, rs, BS, 1) for _ in range(NL)])
    outs = [torch.empty(BS, NH, 1, D, dtype=torch.float16, device="cuda") for _ in range(NL)]

    def step(c, outs=None):
        return [c.decoding_with_pages(qs[l], kn[l], vn[l], l, use_dev_lengths=True, **({} if outs is None else {"out": outs[l]}))
                for l in range(NL)]

    def fill():
        for l in range(NL):
            q, k, v = _rows(torch, rs, BS, 1)
            qs[l].copy_(q); kn[l].copy_(k); vn[l].copy_(v)

    step(G, outs)      # eager once: the workspace and the lse buffer exist before the capture
    step(E)
    torch.cuda.synchronize()
    st = G.host_state()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        step(G, outs)
    G.set_host_state(st)

    def replay_and_compare(what):
        fill()
        want = [w.clone() for w in step(E)]
        g.replay()
        G.note_replayed_step("plain")
        torch.cuda.synchronize()
        for l in range(NL):
            assert _bits(outs[l], want[l]), (what, l)
        assert torch.equal(G._lengths_all, E._lengths_all) and np.array_equal(G._r_a, E._r_a)

    replay_and_compare("first replay")
    for c in (G, E):
        c.release(1)
    for l in range(NL):
        rows = _rows(torch, rs, 1, 2)
        G.prefill_request(1, *rows, l)
        E.prefill_request(1, *rows, l)
    assert G._sink_all.cpu().numpy().tolist() == [[S, 2]] * NL
    replay_and_compare("replay after release and a 2-row prompt")
    replay_and_compare("and once more")


# ---------------------------------------------------------------- out of scope --------------------------------------------
def test_out_of_scope_calls_raise(env):
    torch, ops, _ = env
    from million_amd.pq_cache import DynamicPQCache
    from million_amd.shared_prefix import SharedPrefix
    rs = np.random.RandomState(3)
    A, plain = _cache(env, S), _cache(env, 0)
    for l in range(NL):
        A.prefill_request(0, *_rows(torch, rs, 1, 10), l)
    before = (A._T_a.copy(), A._seen_a.copy(), A._sink_a.copy(), A._lengths_all.clone())
    q, k, v = _rows(torch, rs, BS, 5)
    calls = {
        "swap_out": lambda: A.swap_out(0),
        "snapshot_request": lambda: A.snapshot_request(0),
        "swap_in": lambda: A.swap_in(1, plain.snapshot_request(0)),
        "prefill_ragged(device_store=True)": lambda: A.prefill_ragged(q, k, v, 0, [0, 5], device_store=True),
        "extend_ragged(device_store=True)": lambda: A.extend_ragged(q, k, v, 0, [5, 5], device_store=True),
        "SharedPrefix (prefix cache)": lambda: SharedPrefix(A, 0, plain),
        "SharedPrefix (continuations)": lambda: SharedPrefix(plain, 0, A),
        "DynamicPQCache": lambda: DynamicPQCache(bs=1, nh=NH, num_key_value_heads=NK, M=M, layer_num=1, sink_tokens=S),
    }
    for l in range(NL):
        plain.prefill_request(0, *_rows(torch, rs, 1, 10), l)
    for name, call in calls.items():
        with pytest.raises(NotImplementedError, match="sink_tokens"):
            call()
    assert np.array_equal(A._T_a, before[0]) and np.array_equal(A._seen_a, before[1]) and np.array_equal(A._sink_a, before[2])
    assert torch.equal(A._lengths_all, before[3])
    # without sinks the same calls run
    snap = plain.snapshot_request(0)
    plain.swap_in(1, snap)
    DynamicPQCache(bs=1, nh=NH, num_key_value_heads=NK, M=M, layer_num=1, sink_tokens=0)


# ---------------------------------------------------------------- what sinks are for --------------------------------------
SINK_SEED = 12      # chosen on the CPU (sink_demo_rows + the numpy oracle): the oracle alone shows far more than a factor 2


def sink_demo_rows(seed, n=100):
    """A prompt whose token 0 is an attention sink: its key carries two massive dims (30: no centroid of a codebook drawn from
    N(0, 1) is near it) that every query has a share in, so that it takes more than half of every later row's softmax mass.
    Returns q_prompt, k, v (1, heads, n, d), a decode row (q1, k1, v1) and the codebooks, fp16."""
    rs = np.random.RandomState(seed)
    cents = rs.standard_normal((M, C, D // M)).astype(np.float16), rs.standard_normal((M, C, D // M)).astype(np.float16)
    mk = lambda h, rows: rs.standard_normal((1, h, rows, D)).astype(np.float32)
    q, k, v, q1, k1, v1 = mk(NH, n), mk(NK, n), mk(NK, n), mk(NH, 1), mk(NK, 1), mk(NK, 1)
    for x in (q, q1):
        x[..., 5], x[..., 77] = 1.5, 1.5
    k[:, :, 0, :] *= 0.1
    k[:, :, 0, 5], k[:, :, 0, 77] = 30.0, 30.0
    v[:, :, 0, :] *= 4.0
    return tuple(x.astype(np.float16) for x in (q, k, v, q1, k1, v1)) + (cents,)


def sink_demo_oracle(seed, n=100):
    """(error without sinks, error with one sink, the sink's smallest share of a row's mass): numpy encode / decode of the
    oracle, attention in fp64, rel-L2 against attention over the exact rows."""
    from oracle import oracle as O
    q, k, v, q1, k1, v1, cents = sink_demo_rows(seed, n)
    dk = O.pq_decode_numpy(O.pq_encode_numpy(k, cents[0]), cents[0]).astype(np.float64)
    dv = O.pq_decode_numpy(O.pq_encode_numpy(v, cents[1]), cents[1]).astype(np.float64)
    cat = lambda *xs: np.concatenate([np.asarray(x, np.float64) for x in xs], axis=1)
    exact = SM.attend_rows(q1[0].astype(np.float64), cat(k[0], k1[0]), cat(v[0], v1[0]))[0]
    err = []
    for s in (0, 1):
        got = SM.attend_rows(q1[0].astype(np.float64), cat(k[0, :, :s], dk[0, :, s:], k1[0]), cat(v[0, :, :s], dv[0, :, s:], v1[0]))[0]
        err.append(SM.errors(got, exact)[0])
    K = cat(k[0], k1[0])
    share = min(float((lambda p: p[0] / p.sum())(np.exp((lambda s_: s_ - s_.max())(K[h // (NH // NK)] @ q1[0, h, 0].astype(np.float64) / np.sqrt(D)))))
                for h in range(NH))
    return err[0], err[1], share, exact


def test_what_sinks_are_for(env):
    """The decode output behind a prompt whose first token is a sink: its rel-L2 error against attention on the exact fp16 rows is
    strictly smaller with sink_tokens=1 than with 0 (profiles/attn_sink.txt keeps both figures)."""
    torch, ops, _ = env
    from million_amd.pq_cache import PagedPQCache
    e0, e1, share, exact = sink_demo_oracle(SINK_SEED)
    print(f"oracle: rel-L2 without sinks {e0:.4e}, with sink_tokens=1 {e1:.4e}, sink share of the mass >= {share:.3f}")
    assert share > 0.5 and e0 >= 2 * e1
    q, k, v, q1, k1, v1, cents = sink_demo_rows(SINK_SEED)
    dev = lambda x: torch.from_numpy(x).cuda()
    errs = []
    for sinks in (0, 1):
        c = PagedPQCache(**dict(GEOM, bs=1, layer_num=1), sink_tokens=sinks)
        c.set_cent(dev(cents[0]), dev(cents[1]))
        c.prefill_request(0, dev(q), dev(k), dev(v), 0)
        out = c.decoding_with_pages(dev(q1), dev(k1), dev(v1), 0, use_dev_lengths=True)
        errs.append(SM.errors(_np(out[0].float()), exact)[0])
    print(f"cache:  rel-L2 without sinks {errs[0]:.4e}, with sink_tokens=1 {errs[1]:.4e}")
    assert errs[1] < errs[0]
