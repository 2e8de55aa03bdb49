"""GPU tests of random request lifecycles on a PagedPQCache (tests/cache_life_model.py): every committed (geometry, seed)
script runs on a real cache with device-resident lengths, and after every public call (a decode burst is one call)

  * the device lengths rows and the host mirrors are the model's integers;
  * the codes every slot reaches through its page table are the oracle's codes of the request's own rows, byte for byte;
  * the window's ring rows are the request's last rows, bit for bit;
  * the allocator's invariants hold (reference counts, free list, device table rows, shared pages below every owner's T);
  * then every free pool page is filled with 0xFF (paging on demand) and every window row outside a ring span with NaN, so a
    later read of a freed page or a dead row shows as a non-finite output or a code mismatch.

Every decode step's output (every slot and layer) is compared with oracle.decode_attn on the model's codes and window rows,
every extend output with the fp64 chunk model of tests/test_chunk_attn_gpu.py, every prefill output with the same model
without a past (fp64 causal attention); rows past n_new[b] of a ragged call are exact zeros.  The bar is the suite's (finite,
rel-L2 and mean-abs < 1e-3, tests/test_gpu_parity.py); everything else is bitwise."""
import collections
import concurrent.futures
import time

import numpy as np
import pytest

from tests import cache_life_model as LM
from tests.test_chunk_attn_gpu import model as chunk_model

pytestmark = pytest.mark.gpu

REL_TOL = MEAN_ABS_TOL = 1e-3      # the oracle bar of tests/test_gpu_parity.py
CASES = [(name, seed) for name, seeds in LM.SEEDS.items() for seed in seeds]
# the references (oracle.pq_encode, oracle.decode_attn, the chunk model) are independent pieces of C and numpy work
POOL = concurrent.futures.ThreadPoolExecutor(8)


@pytest.fixture(scope="module")
def env():
    import torch
    assert torch.cuda.is_available(), "GPU tests need an MI355X"
    from million_amd import ops, _lib
    _lib.load()
    yield torch, ops
    assert ops.tail_faults() == 0      # no split merge of the decode steps of this file gave up


class _Worst:
    """The largest errors seen, and the bar."""

    def __init__(self):
        self.rel = self.mae = 0.0
        self.n = 0

    def check(self, out, gold, what):
        out = np.asarray(out, np.float64)
        assert np.isfinite(out).all(), f"{what}: non-finite output"
        rel = np.linalg.norm(out - gold) / max(np.linalg.norm(gold), 1e-30)
        mae = np.abs(out - gold).mean()
        self.rel, self.mae, self.n = max(self.rel, rel), max(self.mae, mae), self.n + 1
        assert rel < REL_TOL and mae < MEAN_ABS_TOL, f"{what}: rel-L2 {rel:.3e} mean-abs {mae:.3e}"


def _poison(torch, cache, m, geom):
    """0xFF in every free pool page (paging on demand), NaN in every window row outside its slot's ring span."""
    if not geom["preallocate"]:
        free = torch.tensor(sorted(cache.page_manager.free_pages), dtype=torch.long).cuda()
        cache.key_page_pool[free] = 0xFF
        cache.value_page_pool[free] = 0xFF
    dead = np.ones((m.bs, m.cap), bool)
    for b in range(m.bs):
        dead[b, (int(m.rs[b]) + np.arange(int(m.r[b]))) % m.cap] = False
    mask = torch.from_numpy(dead).cuda()[None, :, None, :].expand(m.nl, m.bs, m.nhk, m.cap)
    cache._kres_all[mask] = float("nan")
    cache._vres_all[mask] = float("nan")


def _same(before, after):
    return all(np.array_equal(before[k], after[k]) if isinstance(before[k], np.ndarray) else before[k] == after[k] for k in before)


def drive(torch, oracle, geom, calls):
    """One script on a real cache, the model beside it, every check of the header.  -> the begin_step kinds seen, the worst
    errors against the oracle."""
    from million_amd.pq_cache import PagedPQCache
    ck, cv = LM.codebooks(geom)
    oracle.lib()
    LM.encode_rows(calls, geom, lambda x: oracle.pq_encode(x, ck), lambda x: oracle.pq_encode(x, cv), POOL)
    m = LM.Model(geom, rows=True)
    cache = PagedPQCache(**LM.cache_kwargs(geom), device="cuda")
    dev = lambda a: torch.from_numpy(np.ascontiguousarray(a)).cuda()
    cache.set_cent(dev(ck), dev(cv))
    nl, bs = m.nl, m.bs
    tables0 = cache._page_ids_all.cpu().numpy().copy()
    kinds, worst = collections.Counter(), _Worst()
    _poison(torch, cache, m, geom)

    def chunk_golds(q, k, v, who):
        """fp64 outputs of the chunks q / k / v (layers, slots, heads, n, d) of the slots `who` = [(index, slot, rows)] over what
        each slot holds now: {(layer, index): (1, nh, rows, d)}."""
        def gold(l, j, b, n):
            (kc, vc), (kw, vw) = m.codes(l, b), m.window(l, b)
            return chunk_model(oracle, q[l][j:j + 1, :, :n], kc, vc, ck, cv, kw, vw, k[l][j:j + 1, :, :n], v[l][j:j + 1, :, :n])
        keys = [(l, j, b, n) for l in range(nl) for j, b, n in who]
        return {key[:2]: g for key, g in zip(keys, POOL.map(lambda key: gold(*key), keys))}

    for i, call in enumerate(calls):
        op, what = call["op"], f"call {i} ({LM.describe(call)})"
        if op == "decode":
            Q, K, V = dev(call["q"]), dev(call["k"]), dev(call["v"])
            outs = []
            for s in range(call["steps"]):
                if geom["begin_step"]:
                    kind = cache.begin_step(use_dev_lengths=True)
                    kinds["pre" if kind.startswith("pre") else kind] += 1
                for l in range(nl):
                    outs.append(cache.decoding_with_pages(Q[s, l], K[s, l], V[s, l], l, use_dev_lengths=True).clone())
            torch.cuda.synchronize()
            got = torch.stack(outs).float().cpu().numpy().reshape(call["steps"], nl, bs, geom["nh"], 1, geom["d"])
            at = []      # (T, r) of every slot behind each step; the rows of a burst are only appended, so every step's view stays
            for s in range(call["steps"]):
                m.step(*[call[key][s] for key in ("k", "v", "kc", "vc")])
                at.append((m.T.copy(), m.r.copy()))

            def gold(key):
                s, l, b = key
                T, r = int(at[s][0][b]), int(at[s][1][b])
                return oracle.decode_attn(call["q"][s, l, b:b + 1], *m.codes(l, b, T), ck, cv, *m.window(l, b, T, r), r)
            keys = [(s, l, b) for s in range(call["steps"]) for l in range(nl) for b in range(bs)]
            for (s, l, b), g in zip(keys, POOL.map(gold, keys)):
                worst.check(got[s, l, b:b + 1], g, f"{what}: step {s} layer {l} slot {b} (T={at[s][0][b]} r={at[s][1][b]})")
        elif call.get("raises"):
            before = LM.snapshot(cache)
            for l in range(1 if op == "fork" else nl):
                with pytest.raises(RuntimeError):
                    if op == "fork":
                        cache.fork(call["src"], call["dst"], n_tokens=call["n_tokens"])
                    else:
                        cache.extend_request(call["b"], dev(call["q"][l]), dev(call["k"][l]), dev(call["v"][l]), l)
            torch.cuda.synchronize()
            assert _same(before, LM.snapshot(cache)), f"{what}: a refused call moved something"
            m.apply(call)
        elif op == "release":
            cache.release(call["b"])
            m.apply(call)
        elif op == "fork":
            cache.fork(call["src"], call["dst"], n_tokens=call["n_tokens"])
            m.apply(call)
        elif op in ("prefill_request", "extend_request"):
            b, n = call["b"], call["n"]
            outs = [getattr(cache, op)(b, dev(call["q"][l]), dev(call["k"][l]), dev(call["v"][l]), l) for l in range(nl)]
            torch.cuda.synchronize()
            golds = chunk_golds(call["q"], call["k"], call["v"], [(0, b, n)])
            for l in range(nl):
                assert outs[l].shape == (1, geom["nh"], n, geom["d"])
                worst.check(outs[l].float().cpu().numpy(), golds[l, 0], f"{what}: layer {l} (T={m.T[b]} r={m.r[b]})")
            m.apply(call)
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
        torch.cuda.synchronize()
        snap = LM.snapshot(cache)
        LM.check_lengths(m, snap, what)
        LM.check_codes(m, snap, what)
        LM.check_window(m, snap, what)
        if geom["preallocate"]:
            LM.check_allocator_preallocated(snap, tables0, what)
        else:
            LM.check_allocator_on_demand(m, snap, what)
        _poison(torch, cache, m, geom)
    torch.cuda.synchronize()
    LM.check_end(cache, m, geom, tables0)
    return kinds, worst


_RUNS = {}      # (geometry, seed) -> result or the exception: the kinds test reads the script tests' runs, or makes its own


def _run(env, oracle, name, seed):
    if (name, seed) not in _RUNS:
        torch, _ = env
        geom = LM.GEOMS[name]
        t0 = time.perf_counter()
        try:
            kinds, worst = drive(torch, oracle, geom, LM.script(seed, geom))
            _RUNS[name, seed] = (kinds, worst, time.perf_counter() - t0)
        except BaseException as e:
            _RUNS[name, seed] = e
    if isinstance(_RUNS[name, seed], BaseException):
        raise _RUNS[name, seed]
    return _RUNS[name, seed]


@pytest.mark.parametrize("name,seed", CASES, ids=[f"{n}-{s}" for n, s in CASES])
def test_random_lifecycle(env, oracle, name, seed):
    _, ops = env
    kinds, worst, seconds = _run(env, oracle, name, seed)
    print(f"{name} seed {seed}: {worst.n} outputs against the oracle, worst rel-L2 {worst.rel:.3e} mean-abs {worst.mae:.3e} "
          f"(bar {REL_TOL:.0e}); begin_step kinds {dict(kinds)}; {seconds:.1f} s")
    assert worst.n > 0 and ops.tail_faults() == 0


@pytest.mark.parametrize("name", [n for n, g in LM.GEOMS.items() if g["begin_step"]])
def test_encode_ahead_geometries_see_every_kind_of_step(env, oracle, name):
    """pre and commit need the whole batch in lockstep (a fork into every other slot), flush is what a step falls back to when a
    slot of a full batch was not encoded ahead (a fork's destinations, a recycled slot)."""
    kinds = sum((_run(env, oracle, name, seed)[0] for seed in LM.SEEDS[name]), collections.Counter())
    print(f"{name}: {dict(kinds)}")
    assert all(kinds[k] >= 1 for k in ("pre", "commit", "flush", "plain")), dict(kinds)
