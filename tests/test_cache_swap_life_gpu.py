"""GPU test of the random lifecycles with swaps (tests/cache_swap_life.py): one script per geometry on a real PagedPQCache with
device-resident lengths.  After every public call (a decode burst is one call) the invariant checks of
tests/test_cache_life_gpu.py: the device lengths rows and the host mirrors are the model's integers, the codes every slot
reaches through its page table are the oracle's codes of the request's own rows, the window's ring rows are the request's last
rows, the allocator's invariants hold; then every free pool page is filled with 0xFF and every dead window row with NaN.  Every
decode step's output (every slot and layer) is compared with oracle.decode_attn on the model's codes and window rows - a slot
restored by swap_in included - at the suite's bar.  The outputs of prefill_request and extend_request are the other file's."""
import time

import numpy as np
import pytest

from tests import cache_life_model as LM
from tests import cache_swap_life as SL
from tests.test_cache_life_gpu import POOL, _Worst, _poison, _same

pytestmark = pytest.mark.gpu

CASES = [(name, seeds[0]) for name, seeds in SL.SEEDS.items()]


@pytest.fixture(scope="module")
def env():
    import torch
    assert torch.cuda.is_available(), "GPU tests need an MI355X"
    from million_amd import ops, _lib
    _lib.load()
    yield torch, ops
    assert ops.tail_faults() == 0


def drive(torch, oracle, geom, calls):
    from million_amd.pq_cache import PagedPQCache
    ck, cv = LM.codebooks(geom)
    oracle.lib()
    LM.encode_rows(calls, geom, lambda x: oracle.pq_encode(x, ck), lambda x: oracle.pq_encode(x, cv), POOL)
    m = SL.Model(geom, rows=True)
    cache = PagedPQCache(**LM.cache_kwargs(geom), device="cuda")
    dev = lambda a: torch.from_numpy(np.ascontiguousarray(a)).cuda()
    cache.set_cent(dev(ck), dev(cv))
    nl, bs = m.nl, m.bs
    tables0 = cache._page_ids_all.cpu().numpy().copy()
    worst, snaps = _Worst(), {}
    _poison(torch, cache, m, geom)
    for i, call in enumerate(calls):
        op, what = call["op"], f"call {i} ({LM.describe(call)})"
        if op == "decode":
            Q, K, V = dev(call["q"]), dev(call["k"]), dev(call["v"])
            outs = [cache.decoding_with_pages(Q[s, l], K[s, l], V[s, l], l, use_dev_lengths=True).clone()
                    for s in range(call["steps"]) for l in range(nl)]
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
            with pytest.raises(RuntimeError):
                cache.swap_in(call["b"], snaps[call["snap"]])
            torch.cuda.synchronize()
            assert _same(before, LM.snapshot(cache)), f"{what}: a refused call moved something"
            m.apply(call)
        else:
            if op == "swap_out":
                snaps[call["snap"]] = cache.swap_out(call["b"])
            elif op == "swap_in":
                cache.swap_in(call["b"], snaps[call["snap"]])
            elif op == "release":
                cache.release(call["b"])
            elif op == "fork":
                cache.fork(call["src"], call["dst"], n_tokens=call["n_tokens"])
            else:
                for l in range(nl):
                    getattr(cache, op)(call["b"], dev(call["q"][l]), dev(call["k"][l]), dev(call["v"][l]), l)
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
    return worst


@pytest.mark.parametrize("name,seed", CASES, ids=[f"{n}-{s}" for n, s in CASES])
def test_random_lifecycle_with_swaps(env, oracle, name, seed):
    torch, ops = env
    geom = SL.GEOMS[name]
    t0 = time.perf_counter()
    worst = drive(torch, oracle, geom, SL.script(seed, geom))
    print(f"{name} seed {seed}: {worst.n} outputs against the oracle, worst rel-L2 {worst.rel:.3e} mean-abs {worst.mae:.3e}; "
          f"{time.perf_counter() - t0:.1f} s")
    assert worst.n > 0 and ops.tail_faults() == 0
