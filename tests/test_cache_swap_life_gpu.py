"""GPU test of the random lifecycles with swaps (tests/cache_swap_life.py): one script per geometry on a real PagedPQCache with
device-resident lengths (tests/cache_life_driver.py says what is checked) - a slot restored by swap_in is read by decode steps,
extends and the byte checks as any other."""
import time

import pytest

from tests import cache_life_driver as D
from tests import cache_swap_life as SL

pytestmark = pytest.mark.gpu

CASES = [(name, seeds[0]) for name, seeds in SL.SEEDS.items()]


@pytest.fixture(scope="module")
def env():
    yield from D.gpu_env()


@pytest.mark.parametrize("name,seed", CASES, ids=[f"{n}-{s}" for n, s in CASES])
def test_random_lifecycle_with_swaps(env, oracle, name, seed):
    _, ops = env
    geom = SL.GEOMS[name]
    t0 = time.perf_counter()
    run = D.GpuDriver(oracle, geom, SL.script(seed, geom)).run()
    worst = run.worst
    print(f"{name} seed {seed}: {worst.n} outputs against the oracle, worst rel-L2 {worst.rel:.3e} mean-abs {worst.mae:.3e}; "
          f"{time.perf_counter() - t0:.1f} s, of them " + ", ".join(f"{k} {v:.2f}" for k, v in run.secs.items()))
    assert worst.n > 0 and ops.tail_faults() == 0
