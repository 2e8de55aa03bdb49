"""The lean decode kernel's block loop and query image (csrc/attn_lean.h): a wave's last block requests nothing (BLOCK_LAST) and
the workgroup's query rows reach LDS once (kQOff), read back by every wave behind the codebook barrier.

Shapes.  32 (b, kv head) pairs - bs 4, nh 32, nh_k 8, d 128, M 64, C 256, pages of 64 - get 8 splits on a 256-CU chip: page p goes
to split p % 8, wave (p / 8) % 8, round p / 64, so a wave has T / 4096 units and 64 k more tokens give k waves one more.  The
sweep walks the unit count through every form of the loop:
    3776 waves with 0 and 1 units | 4096 one unit everywhere | 4160 one wave runs BLOCK_LAST<0> | 8185 partial last unit |
    8192 two units everywhere (the flagship's path) | 8256, 8768 BLOCK<0> BLOCK_LAST<1> in 1 and 9 waves | 12288 three units |
    16384 four: BLOCK<0> BLOCK<1> BLOCK_LAST<0> | 16448 loop pair + both tails
Every case runs through tests/decode_poison.py's runner over the C ABI: the clean copy against the fp64 oracle (whole tensor
and every head, REL_TOL / MEAN_ABS_TOL = 1e-3 as in tests/test_gpu_parity.py) and the poisoned copy bitwise equal to the
clean one - a unit that is never requested would read 0xFF codes or stale ring registers there."""
import numpy as np
import pytest

from tests import decode_poison as P

pytestmark = pytest.mark.gpu

SWEEP_T = [3776, 4096, 4160, 8185, 8192, 8256, 8768, 12288, 16384, 16448]


def _case(name, d=128, M=64, C=256, G=4, kind=1, **kw):
    kw.setdefault("bs", 4)
    kw.setdefault("nhk", 8)
    return P.Case(name, d, M, C, G, kind, **kw)


SWEEP = [_case(f"units-T{T}-r{r}", T=T, r=r, rs=120 if r else 0) for T in SWEEP_T for r in (17, 0)]
FORMS = [      # T = 8256: BLOCK<0> BLOCK_LAST<1> in one wave per split, BLOCK_LAST<0> in the others
    _case("M32", M=32, T=8256),
    _case("d64-M64-padded", d=64, T=8256),
    _case("d64-M32", d=64, M=32, T=8256),
    _case("C128", C=128, T=8256),
    _case("rowmajor-10arg", kind=2, kl="row", vl="row", T=8256),
]
QUERY = [
    # G < 4: the idle head columns of the 4 x 4 x 4 products must stay exact zeros (a NaN there would reach every head)
    _case("G1", G=1, T=8256),
    _case("G2", G=2, T=8256, r=100, rs=90, dev=True, gap=64, append=True),
    _case("G3", G=3, T=8256),
    _case("d64-G8-parts", d=64, M=32, G=8, T=8256, r=40, rs=100),
    _case("d64-M64-G3-padded", d=64, G=3, T=4160),
    # 2 splits of 64 window rows each: waves 0 - 3 of a workgroup carry a residual tile (and read qb from the image)
    _case("window-rows-in-four-waves", bs=2, nhk=2, T=1000, r=128, rs=50),
]


@pytest.fixture(scope="module")
def env():
    import torch
    assert torch.cuda.is_available(), "GPU tests need an MI355X"
    from million_amd import ops, _lib
    return torch, ops, _lib.load(), _lib


def test_planner_kind_and_splits(env):
    """The flagship shape (1 request, 32 / 8 heads, T = 32768, M = 64) is planned onto the MFMA kernels (kind 1), and so is the
    sweep's; on a 256-CU chip the sweep's launch is 32 pairs x 8 splits (tests/test_decode_advance.py restates the split rule)."""
    torch, ops, lib, L = env
    from tests.test_decode_advance import _mfma_grid
    assert P.kernel_kind(_case("flagship", bs=1, T=32768, r=100), lib, L) == 1
    assert P.kernel_kind(_case("flagship-step", bs=1, T=32768, r=100, dev=True, append=True), lib, L) == 1
    cus = torch.cuda.get_device_properties(0).multi_processor_count
    if cus == 256:
        for T in SWEEP_T:
            assert _mfma_grid(cus, 4, 8, T, 128) == 32 * 8, T


@pytest.mark.parametrize("case", SWEEP + FORMS + QUERY, ids=[c.name for c in SWEEP + FORMS + QUERY])
def test_block_forms_clean_and_poisoned(case, env, oracle):
    torch, ops, lib, L = env
    res = P.check_case(case, torch, ops, lib, L, oracle)
    print(f"{case.name}: rel {res['rel']:.3e} mean_abs {res['mean_abs']:.3e} worst head {res['worst_head']:.3e}")


def test_lse_instance(env, oracle):
    """The LSE instances share the loop: `out` bitwise the plain entry's, lse within lse_ref.LSE_TOL of the fp64 reference."""
    torch, ops, lib, L = env
    from tests import lse_ref as R
    from tests.test_attn_lse_gpu import run_lse
    c = _case("lse-T8256", T=8256)
    built = P.build(c)
    plain = P.run(c, built["clean"], torch, ops, lib, L)
    clean = run_lse(c, built["clean"], torch, ops, lib, L)
    pois = run_lse(c, built["poisoned"], torch, ops, lib, L)
    assert np.array_equal(clean["out"].view(np.uint16), plain["out"].view(np.uint16))
    g, ref = R.decode_ref(c, built, oracle)
    e = P.head_err(clean["out"], g)
    err = np.abs(clean["lse"].astype(np.float64) - ref)
    print(f"lse-T8256: worst head {e.max():.3e}, lse max abs error {err.max():.3e}")
    assert e.max() < P.REL_TOL
    assert np.isfinite(clean["lse"]).all() and err.max() < R.LSE_TOL
    assert np.array_equal(pois["out"].view(np.uint16), clean["out"].view(np.uint16))
    assert np.array_equal(pois["lse"].view(np.uint32), clean["lse"].view(np.uint32))
    assert ops.tail_faults() == 0


def test_step_form_ragged_back_to_back(env, oracle):
    """Device-resident lengths plus the fused append, four requests with 1, 2, 2 (+ one wave with 3) and 3 (+ one wave with 4)
    units per wave in ONE launch, two launches back to back on one workspace: every output against the oracle for its own window,
    the appended rows and the device lengths (tests/test_decode_advance.py's driver)."""
    torch, ops, lib, L = env
    from tests.test_decode_advance import _Steps
    ops.tail_faults()
    s = _Steps(torch, ops, oracle, 5100, 4, 32, 8, 128, 64, [4096, 8192, 8256, 12352], [17, 0, 100, 41])
    assert s.kind() == 1
    s.run_and_check(2, "ragged step form")
