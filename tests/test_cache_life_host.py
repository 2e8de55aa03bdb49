"""CPU tests of the random request lifecycles (tests/cache_life_model.py): the coverage condition of every committed script,
the model's decode rule against the oracle's paging policy, and every script on a CPU PagedPQCache (tests/cache_life_driver.py
says what is checked), the two begin_step geometries included."""
import numpy as np
import pytest

from tests import cache_life_driver as D
from tests import cache_life_model as LM

CASES = [(name, seed) for name, seeds in LM.SEEDS.items() for seed in seeds]


@pytest.mark.parametrize("name,seed", CASES, ids=[f"{n}-{s}" for n, s in CASES])
def test_committed_scripts_meet_the_coverage_condition(name, seed):
    geom = LM.GEOMS[name]
    cnt = LM.coverage(LM.script(seed, geom, rows=False), geom)
    print(f"{name} seed {seed}: {cnt}")
    assert not LM.missing(cnt, geom), f"{name} seed {seed} lacks (have, need): {LM.missing(cnt, geom)}"
    assert 70 <= cnt["calls"] <= 100 and cnt["decode_steps"] <= LM.DECODE_BUDGET + 2 * geom["extended_residual_size"]


def test_two_distinct_seeds_per_geometry():
    assert set(LM.SEEDS) == set(LM.GEOMS) and all(len(set(s)) == 2 for s in LM.SEEDS.values())


def test_script_rows_are_reproducible_and_padded_with_nan():
    geom = LM.GEOMS["share-32"]
    a, b = (LM.script(LM.SEEDS["share-32"][0], geom) for _ in range(2))
    strip = lambda calls: [{k: v for k, v in c.items() if k not in "qkv"} for c in calls]
    assert strip(a) == strip(b) == LM.plan(LM.SEEDS["share-32"][0], geom)
    for ca, cb in zip(a, b):
        for key in "qkv":
            if key in ca:
                assert ca[key].dtype == np.float16 and np.array_equal(ca[key].view(np.int16), cb[key].view(np.int16))
        if ca["op"].endswith("ragged"):
            for s, n in enumerate(ca["n_new"]):
                assert np.isfinite(ca["k"][:, s, :, :n]).all() and np.isnan(ca["k"][:, s, :, n:]).all() and np.isnan(ca["q"][:, s, :, n:]).all()


@pytest.mark.parametrize("ps,cap", [(32, 64), (64, 128), (128, 128)])
@pytest.mark.parametrize("prompt", [0, 5, 70])
def test_decode_rule_is_the_oracles_paging_policy(oracle, ps, cap, prompt):
    m = LM.Model(dict(LM.BASE, page_size=ps, extended_residual_size=cap))
    if prompt:
        m.prefill(1, prompt)
    pol = oracle.PagedPolicy(page_size=ps, residual=cap, prefill=prompt)
    idle = oracle.PagedPolicy(page_size=ps, residual=cap, prefill=0)
    for i in range(300):
        m.step()
        assert (m.T[1], m.r[1]) == pol.step() and (m.T[0], m.r[0]) == idle.step(), f"step {i}"
        assert m.rs[1] == (m.T[1] - prompt) % cap and m.n(1) == prompt + i + 1


@pytest.mark.parametrize("name,seed", CASES, ids=[f"{n}-{s}" for n, s in CASES])
def test_script_on_a_cpu_cache(monkeypatch, name, seed):
    geom = LM.GEOMS[name]
    D.run_on_cpu(monkeypatch, geom, LM.script(seed, geom, rows=False), seed)
