"""GPU tests of random request lifecycles on a PagedPQCache (tests/cache_life_model.py): every committed (geometry, seed)
script on a real cache with device-resident lengths, begin_step before every decode step where the geometry says so
(tests/cache_life_driver.py says what is checked), and every kind of step on the encode-ahead geometries."""
import collections
import time

import pytest

from tests import cache_life_driver as D
from tests import cache_life_model as LM

pytestmark = pytest.mark.gpu

CASES = [(name, seed) for name, seeds in LM.SEEDS.items() for seed in seeds]


@pytest.fixture(scope="module")
def env():
    yield from D.gpu_env()


_RUNS = {}      # (geometry, seed) -> result or the exception: the kinds test reads the script tests' runs, or makes its own


def _run(env, oracle, name, seed):
    if (name, seed) not in _RUNS:
        geom = LM.GEOMS[name]
        t0 = time.perf_counter()
        try:
            run = D.GpuDriver(oracle, geom, LM.script(seed, geom)).run()
            _RUNS[name, seed] = (collections.Counter(run.kinds), run.worst, time.perf_counter() - t0)
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
          f"(bar {D.REL_TOL:.0e}); begin_step kinds {dict(kinds)}; {seconds:.1f} s")
    assert worst.n > 0 and ops.tail_faults() == 0


@pytest.mark.parametrize("name", [n for n, g in LM.GEOMS.items() if g["begin_step"]])
def test_encode_ahead_geometries_see_every_kind_of_step(env, oracle, name):
    """pre and commit need the whole batch in lockstep (a fork into every other slot), flush is what a step falls back to when a
    slot of a full batch was not encoded ahead (a fork's destinations, a recycled slot)."""
    kinds = sum((_run(env, oracle, name, seed)[0] for seed in LM.SEEDS[name]), collections.Counter())
    print(f"{name}: {dict(kinds)}")
    assert all(kinds[k] >= 1 for k in ("pre", "commit", "flush", "plain")), dict(kinds)
