"""CPU tests of the random lifecycles with swaps (tests/cache_swap_life.py): the coverage condition of every committed script,
and the scripts on a CPU PagedPQCache whose launches are the numpy stand-ins of tests/test_cache_life_host.py plus the swap
model (tests/cache_swap_model.py) - lengths (device rows and host mirrors) and the allocator's invariants after every call,
and every restored slot's live data against what left at swap_out."""
import numpy as np
import pytest
import torch

from tests import cache_life_model as LM
from tests import cache_swap_life as SL
from tests import cache_swap_model as SM
from tests.test_cache_life_host import _cpu_cache, _stand_ins

CASES = [(name, seed) for name, seeds in SL.SEEDS.items() for seed in seeds]


@pytest.mark.parametrize("name,seed", CASES, ids=[f"{n}-{s}" for n, s in CASES])
def test_committed_scripts_meet_the_coverage_condition(name, seed):
    geom = SL.GEOMS[name]
    cnt = SL.coverage(SL.script(seed, geom, rows=False), geom)
    print(f"{name} seed {seed}: {cnt}")
    assert not SL.missing(cnt, geom), f"{name} seed {seed} lacks (have, need): {SL.missing(cnt, geom)}"
    assert SL.N_CALLS <= cnt["calls"] <= SL.N_CALLS + 5 and cnt["decode_steps"] <= SL.DECODE_BUDGET + 2 * geom["extended_residual_size"]
    assert sorted(SL.GEOMS[n]["preallocate"] for n in SL.GEOMS) == [False, True]


def _live(cache, b):
    view16 = lambda t: t.view(torch.int16).numpy()
    T, r, st = (int(a[0, b]) for a in (cache._T_a, cache._r_a, cache._rs_a))
    return [x.copy() for x in SM.live_data(cache._page_ids_all.numpy(), cache.key_page_pool.numpy(), cache.value_page_pool.numpy(),
                                          view16(cache._kres_all), view16(cache._vres_all), b, T, r, st)]


@pytest.mark.parametrize("name,seed", CASES, ids=[f"{n}-{s}" for n, s in CASES])
def test_script_on_a_cpu_cache(monkeypatch, name, seed):
    from million_amd import ops
    geom = SL.GEOMS[name]
    _stand_ins(monkeypatch)
    monkeypatch.setattr(ops, "cache_swap", SM.as_ops_stub())
    cache, m = _cpu_cache(geom), SL.Model(geom)
    # the stand-ins encode nothing: give every pool page and window row bytes of its own, so that a restored slot shows its request
    g = torch.Generator().manual_seed(seed)
    cache.key_page_pool.copy_(torch.randint(0, 256, cache.key_page_pool.shape, generator=g, dtype=torch.uint8))
    cache.value_page_pool.copy_(torch.randint(0, 256, cache.value_page_pool.shape, generator=g, dtype=torch.uint8))
    cache._kres_all.copy_(torch.randn(cache._kres_all.shape, generator=g).half())
    cache._vres_all.copy_(torch.randn(cache._vres_all.shape, generator=g).half())
    nl, bs, nh, nhk, d = geom["layer_num"], geom["bs"], geom["nh"], geom["num_key_value_heads"], geom["d"]
    z = lambda *s: torch.zeros(*s, dtype=torch.float16)
    tables0 = cache._page_ids_all.numpy().copy()
    snaps, left = {}, {}
    for i, call in enumerate(SL.script(seed, geom, rows=False)):
        op, what = call["op"], f"call {i} ({LM.describe(call)})"
        if op == "decode":
            for _ in range(call["steps"]):
                for l in range(nl):
                    cache.decoding_with_pages(z(bs, nh, 1, d), z(bs, nhk, 1, d), z(bs, nhk, 1, d), l, use_dev_lengths=True)
                m.step()
            continue
        if call.get("raises"):
            before = LM.snapshot(cache)
            with pytest.raises(RuntimeError):
                cache.swap_in(call["b"], snaps[call["snap"]])
            after = LM.snapshot(cache)
            assert all(np.array_equal(before[k], after[k]) if isinstance(before[k], np.ndarray) else before[k] == after[k]
                       for k in before), f"{what}: a refused call moved something"
        elif op == "swap_out":
            left[call["snap"]] = _live(cache, call["b"])
            snaps[call["snap"]] = cache.swap_out(call["b"])
            assert snaps[call["snap"]].meta["T"] == m.T[call["b"]] and snaps[call["snap"]].meta["start"] == m.rs[call["b"]]
        elif op == "swap_in":
            cache.swap_in(call["b"], snaps[call["snap"]])
            for a, b in zip(left[call["snap"]], _live(cache, call["b"])):
                assert np.array_equal(a, b), f"{what}: the restored slot does not hold what left"
        elif op == "release":
            cache.release(call["b"])
        elif op == "fork":
            cache.fork(call["src"], call["dst"], n_tokens=call["n_tokens"])
        else:
            for l in range(nl):
                getattr(cache, op)(call["b"], z(1, nh, call["n"], d), z(1, nhk, call["n"], d), z(1, nhk, call["n"], d), l)
        m.apply(call)
        snap = LM.snapshot(cache)
        LM.check_lengths(m, snap, what)
        if geom["preallocate"]:
            LM.check_allocator_preallocated(snap, tables0, what)
        else:
            LM.check_allocator_on_demand(m, snap, what)
    LM.check_end(cache, m, geom, tables0)
