"""GPU test of the random lifecycles with draft verification (tests/cache_verify_life.py): the first committed script of each
geometry on a real PagedPQCache with device-resident lengths, begin_step before every decode step where the geometry says so
(tests/cache_life_driver.py says what is checked), and the coverage condition on the kinds of step the run reported."""
import time

import pytest

from tests import cache_life_driver as D
from tests import cache_verify_life as VL

pytestmark = pytest.mark.gpu

CASES = [(name, seeds[0]) for name, seeds in VL.SEEDS.items()]


@pytest.fixture(scope="module")
def env():
    yield from D.gpu_env()


@pytest.mark.parametrize("name,seed", CASES, ids=[f"{n}-{s}" for n, s in CASES])
def test_random_lifecycle_with_verify(env, oracle, name, seed):
    _, ops = env
    geom = VL.GEOMS[name]
    t0 = time.perf_counter()
    run = D.GpuDriver(oracle, geom, VL.script(seed, geom)).run()
    kinds, worst, ver = run.kinds, run.worst, run.ver
    seconds = time.perf_counter() - t0
    cnt = VL.coverage(VL.script(seed, geom, rows=False), geom, kinds=kinds if geom["begin_step"] else None)
    print(f"{name} seed {seed}: {worst.n} outputs against the oracle, worst rel-L2 {worst.rel:.3e} mean-abs {worst.mae:.3e} (bar {D.REL_TOL:.0e}); "
          f"{ver['n']} verified blocks, worst row rel-L2 {ver['rel']:.3e}; begin_step kinds "
          f"{ {k: kinds.count(k) for k in sorted(set(kinds))} }; {cnt['calls']} calls, {cnt['decode_steps']} decode steps, "
          f"{cnt['verify_rounds']} rounds; {seconds:.2f} s, of them " + ", ".join(f"{k} {v:.2f}" for k, v in run.secs.items()))
    assert worst.n > 0 and ver["n"] > 0 and ops.tail_faults() == 0
    assert not VL.missing(cnt, geom), f"{name} seed {seed} on the kinds the run reported lacks (have, need): {VL.missing(cnt, geom)}"
