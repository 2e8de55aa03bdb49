"""CPU tests of the random lifecycles with swaps (tests/cache_swap_life.py): the coverage condition of every committed script,
and every script on a CPU PagedPQCache (tests/cache_life_driver.py says what is checked)."""
import pytest

from tests import cache_life_driver as D
from tests import cache_swap_life as SL

CASES = [(name, seed) for name, seeds in SL.SEEDS.items() for seed in seeds]


@pytest.mark.parametrize("name,seed", CASES, ids=[f"{n}-{s}" for n, s in CASES])
def test_committed_scripts_meet_the_coverage_condition(name, seed):
    geom = SL.GEOMS[name]
    cnt = SL.coverage(SL.script(seed, geom, rows=False), geom)
    print(f"{name} seed {seed}: {cnt}")
    assert not SL.missing(cnt, geom), f"{name} seed {seed} lacks (have, need): {SL.missing(cnt, geom)}"
    assert SL.N_CALLS <= cnt["calls"] <= SL.N_CALLS + 5 and cnt["decode_steps"] <= SL.DECODE_BUDGET + 2 * geom["extended_residual_size"]
    assert sorted(SL.GEOMS[n]["preallocate"] for n in SL.GEOMS) == [False, True]


@pytest.mark.parametrize("name,seed", CASES, ids=[f"{n}-{s}" for n, s in CASES])
def test_script_on_a_cpu_cache(monkeypatch, name, seed):
    geom = SL.GEOMS[name]
    D.run_on_cpu(monkeypatch, geom, SL.script(seed, geom, rows=False), seed)
