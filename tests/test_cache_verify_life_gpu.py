"""GPU test of the random lifecycles with draft verification (tests/cache_verify_life.py): the first committed script of each
geometry on a real PagedPQCache with device-resident lengths, begin_step before every decode step where the geometry says so.

A verify_commit call: every free pool page is 0xFF and every dead window row NaN before the verifies and again before the
commit.  Every layer is verified with return_lse=True (twice with other rows for a `reverify` call; every set is checked) and

  * the cache is afterwards what it was before, byte for byte (tests/cache_life_model.snapshot): verify is pure;
  * out and lse of the rows below n_draft[b] are held against fp64 attention over the MODEL's codes, window rows and the draft
    rows causally (lse_ref.chunk_ref, as test_verify_gpu._verify_ref builds it from the device): per-row rel-L2 < 1e-3, lse
    within lse_ref.LSE_TOL, finite; the rows at or past n_draft[b] are exact zeros with lse -inf;
  * commit(n_accept), then the checks every call gets.  A refused commit raises with the word of its refusal and moves nothing.

After every public call (a decode burst is one call), as tests/test_cache_life_gpu.py and tests/test_cache_swap_life_gpu.py: the
device lengths rows and the host mirrors are the model's integers, the codes every slot reaches through its page table are the
oracle's codes of the request's own rows, the window's ring rows are the request's last rows, the allocator's invariants hold -
all bitwise.  Every decode step's output (every slot and layer) is compared with oracle.decode_attn on the model's codes and
window rows, every extend and prefill output with the fp64 chunk model, at the suite's bar (rel-L2 and mean-abs < 1e-3).  The
kind of step begin_step reports is the model's at every step, and the coverage condition holds on the reported kinds."""
import collections
import contextlib
import time

import numpy as np
import pytest

from tests import cache_life_model as LM
from tests import cache_verify_life as VL
from tests import lse_ref as R
from tests.test_cache_life_gpu import POOL, REL_TOL, _poison, _same, _Worst
from tests.test_chunk_attn_gpu import model as chunk_model
from tests.test_verify_gpu import _check_verify

pytestmark = pytest.mark.gpu

CASES = [(name, seeds[0]) for name, seeds in VL.SEEDS.items()]


@pytest.fixture(scope="module")
def env():
    import torch
    assert torch.cuda.is_available(), "GPU tests need an MI355X"
    from million_amd import ops, _lib
    _lib.load()
    yield torch, ops
    assert ops.tail_faults() == 0      # no split merge of the decode and verify launches of this file gave up


def drive(torch, oracle, geom, calls):
    """One script on a real cache, the model beside it, every check of the header.  -> the begin_step kinds in order, the worst
    errors against the oracle, the worst verify row error and the number of verified (layer, slot) blocks."""
    from million_amd.pq_cache import PagedPQCache
    ck, cv = LM.codebooks(geom)
    oracle.lib()
    t0 = time.perf_counter()
    VL.encode_rows(calls, geom, lambda x: oracle.pq_encode(x, ck), lambda x: oracle.pq_encode(x, cv), POOL)
    encode_s = time.perf_counter() - t0
    m = VL.Model(geom, rows=True)
    cache = PagedPQCache(**LM.cache_kwargs(geom), device="cuda")
    dev = lambda a: torch.from_numpy(np.ascontiguousarray(a)).cuda()
    cache.set_cent(dev(ck), dev(cv))
    nl, bs = m.nl, m.bs
    tables0 = cache._page_ids_all.cpu().numpy().copy()
    kinds, worst, snaps, ver = [], _Worst(), {}, dict(rel=0.0, n=0)
    secs = ver["secs"] = collections.Counter({"oracle codes": encode_s})      # where a script's seconds go: the host references, the snapshots and their checks
    _poison(torch, cache, m, geom)

    @contextlib.contextmanager
    def clock(name):
        t0 = time.perf_counter()
        yield
        secs[name] += time.perf_counter() - t0

    def chunk_golds(q, k, v, who):
        def gold(l, j, b, n):
            (kc, vc), (kw, vw) = m.codes(l, b), m.window(l, b)
            return chunk_model(oracle, q[l][j:j + 1, :, :n], kc, vc, ck, cv, kw, vw, k[l][j:j + 1, :, :n], v[l][j:j + 1, :, :n])
        keys = [(l, j, b, n) for l in range(nl) for j, b, n in who]
        with clock("references"):
            return {key[:2]: g for key, g in zip(keys, POOL.map(lambda key: gold(*key), keys))}

    def check_state(what):
        torch.cuda.synchronize()
        with clock("state checks"):
            snap = LM.snapshot(cache)
            LM.check_lengths(m, snap, what)
            LM.check_codes(m, snap, what)
            LM.check_window(m, snap, what)
            if geom["preallocate"]:
                LM.check_allocator_preallocated(snap, tables0, what)
            else:
                LM.check_allocator_on_demand(m, snap, what)
            _poison(torch, cache, m, geom)

    def verify(call, keys, what):
        """Every layer of call["layers"] with the rows call[keys], against fp64 over what the model holds."""
        q, k, v = (call[key] for key in keys)
        nd = call["n_draft"]
        got = [cache.verify(dev(q[l]), dev(k[l]), dev(v[l]), l, n_draft=nd, route=call["route"], return_lse=True) for l in call["layers"]]
        torch.cuda.synchronize()

        def ref(key):
            l, b = key
            if nd[b] == 0:      # no row to compare: zeros and -inf are asked of the output itself
                return np.zeros((1,) + q[l].shape[1:]), np.full((1,) + q[l].shape[1:3], -np.inf)
            (kc, vc), (kw, vw) = m.codes(l, b), m.window(l, b)
            st = dict(q=q[l][b:b + 1], k_res=kw, k_codes=kc, v_codes=vc, k_cents=ck, v_cents=cv, k_win=kw, v_win=vw,
                      k_ch=k[l][b:b + 1], v_ch=v[l][b:b + 1])
            return R.chunk_ref(oracle, st, [nd[b]])
        pairs = [(l, b) for l in call["layers"] for b in range(bs)]
        with clock("references"):
            refs = dict(zip(pairs, POOL.map(ref, pairs)))
        for l, g in zip(call["layers"], got):
            assert g[0].shape == (bs, geom["nh"], call["n"], geom["d"]) and g[1].shape == (bs, geom["nh"], call["n"])
            ro, rl = (np.concatenate([refs[l, b][i] for b in range(bs)]) for i in range(2))
            ver["rel"] = max(ver["rel"], _check_verify(g, (ro, rl), nd, f"{what}: verify of layer {l} (T={m.T.tolist()} r={m.r.tolist()})"))
            ver["n"] += sum(x > 0 for x in nd)

    def do(call, what):
        op = call["op"]
        if op == "decode":
            Q, K, V = dev(call["q"]), dev(call["k"]), dev(call["v"])
            outs, at = [], []
            for s in range(call["steps"]):
                kind = None
                if geom["begin_step"]:
                    want = m.next_kind()
                    kind = cache.begin_step(use_dev_lengths=True)
                    kind = "pre" if kind.startswith("pre") else kind
                    assert kind == want, f"{what}: step {s} is a {kind!r} step, the model expects {want!r}"
                    kinds.append(kind)
                for l in range(nl):
                    outs.append(cache.decoding_with_pages(Q[s, l], K[s, l], V[s, l], l, use_dev_lengths=True).clone())
                m.step(*[call[key][s] for key in ("k", "v", "kc", "vc")], kind=kind)
                at.append((m.T.copy(), m.r.copy()))      # the rows of a burst are only appended, so every step's view stays
            torch.cuda.synchronize()
            got = torch.stack(outs).float().cpu().numpy().reshape(call["steps"], nl, bs, geom["nh"], 1, geom["d"])

            def gold(key):
                s, l, b = key
                T, r = int(at[s][0][b]), int(at[s][1][b])
                return oracle.decode_attn(call["q"][s, l, b:b + 1], *m.codes(l, b, T), ck, cv, *m.window(l, b, T, r), r)
            keys = [(s, l, b) for s in range(call["steps"]) for l in range(nl) for b in range(bs)]
            with clock("references"):
                golds = list(POOL.map(gold, keys))
            for (s, l, b), g in zip(keys, golds):
                worst.check(got[s, l, b:b + 1], g, f"{what}: step {s} layer {l} slot {b} (T={at[s][0][b]} r={at[s][1][b]})")
            return
        if op == "verify_commit":
            if call["layers"]:
                with clock("state checks"):
                    before = LM.snapshot(cache)
                if call["reverify"]:
                    verify(call, ("q0", "k0", "v0"), what + " (first rows)")
                verify(call, ("q", "k", "v"), what)
                with clock("state checks"):
                    assert _same(before, LM.snapshot(cache)), f"{what}: verify moved lengths, pages or window bytes"
            if call.get("between"):
                m.verify(call["n"], call["n_draft"], call["layers"])
                do(call["between"], what + ": between")
                check_state(what + ": between")
                call = dict(call, layers=[], between=None)
            _poison(torch, cache, m, geom)
            if call.get("raises"):
                torch.cuda.synchronize()
                before = LM.snapshot(cache)
                with pytest.raises(RuntimeError, match=VL.REFUSALS[call["refusal"]]):
                    cache.commit(call["n_accept"])
                torch.cuda.synchronize()
                assert _same(before, LM.snapshot(cache)), f"{what}: a refused call moved something"
            else:
                cache.commit(call["n_accept"])
        elif op == "swap_out":
            snaps[call["snap"]] = cache.swap_out(call["b"])
        elif op == "swap_in":
            cache.swap_in(call["b"], snaps[call["snap"]])
        elif op == "release":
            cache.release(call["b"])
        elif op == "fork":
            cache.fork(call["src"], call["dst"], n_tokens=call["n_tokens"])
        elif op in ("prefill_request", "extend_request"):
            b, n = call["b"], call["n"]
            outs = [getattr(cache, op)(b, dev(call["q"][l]), dev(call["k"][l]), dev(call["v"][l]), l) for l in range(nl)]
            torch.cuda.synchronize()
            golds = chunk_golds(call["q"], call["k"], call["v"], [(0, b, n)])
            for l in range(nl):
                assert outs[l].shape == (1, geom["nh"], n, geom["d"])
                worst.check(outs[l].float().cpu().numpy(), golds[l, 0], f"{what}: layer {l} (T={m.T[b]} r={m.r[b]})")
        else:      # the ragged forms
            n_new = call["n_new"]
            outs = [getattr(cache, op)(dev(call["q"][l]), dev(call["k"][l]), dev(call["v"][l]), l, n_new, device_store=call["device_store"])
                    for l in range(nl)]
            torch.cuda.synchronize()
            golds = chunk_golds(call["q"], call["k"], call["v"], [(b, b, n) for b, n in enumerate(n_new) if n])
            for l in range(nl):
                out = outs[l].float().cpu().numpy()
                assert out.shape == (bs, geom["nh"], max(n_new), geom["d"])
                for b, n in enumerate(n_new):
                    assert not out[b, :, n:].any(), f"{what}: layer {l} slot {b}: rows past n_new={n} are not zeros"
                    if n:
                        worst.check(out[b:b + 1, :, :n], golds[l, b], f"{what}: layer {l} slot {b} (T={m.T[b]} r={m.r[b]})")
        m.apply(call)

    for i, call in enumerate(calls):
        what = f"call {i} ({VL.describe(call)})"
        do(call, what)
        check_state(what)
        assert np.array_equal(cache._pre_a, np.tile(m.pre, (nl, 1))), f"{what}: encoded-ahead flags {cache._pre_a.tolist()}, model {m.pre.tolist()}"
    torch.cuda.synchronize()
    LM.check_end(cache, m, geom, tables0)
    return kinds, worst, ver


@pytest.mark.parametrize("name,seed", CASES, ids=[f"{n}-{s}" for n, s in CASES])
def test_random_lifecycle_with_verify(env, oracle, name, seed):
    torch, ops = env
    geom = VL.GEOMS[name]
    t0 = time.perf_counter()
    kinds, worst, ver = drive(torch, oracle, geom, VL.script(seed, geom))
    seconds = time.perf_counter() - t0
    cnt = VL.coverage(VL.script(seed, geom, rows=False), geom, kinds=kinds if geom["begin_step"] else None)
    print(f"{name} seed {seed}: {worst.n} outputs against the oracle, worst rel-L2 {worst.rel:.3e} mean-abs {worst.mae:.3e} (bar {REL_TOL:.0e}); "
          f"{ver['n']} verified blocks, worst row rel-L2 {ver['rel']:.3e}; begin_step kinds "
          f"{ {k: kinds.count(k) for k in sorted(set(kinds))} }; {cnt['calls']} calls, {cnt['decode_steps']} decode steps, "
          f"{cnt['verify_rounds']} rounds; {seconds:.2f} s, of them " + ", ".join(f"{k} {v:.2f}" for k, v in ver["secs"].items()))
    assert worst.n > 0 and ver["n"] > 0 and ops.tail_faults() == 0
    assert not VL.missing(cnt, geom), f"{name} seed {seed} on the kinds the run reported lacks (have, need): {VL.missing(cnt, geom)}"
