"""The lean decode kernel's read-once instances (csrc/attn_lean.h, `once`: fully paged codes, 64-token pages, one part per kv
head): every wave request takes 1 KiB of its unit whole, K turns into the lane = token form by row swaps where a ring slot is
first consumed, V picks the register of the lane's parity in the gather.  tests/test_decode_code_requests_host.py restates the
two lane -> address maps; here the kernels run, through tests/decode_poison.py's runner over the C ABI: the clean copy against
the fp64 oracle (whole tensor and every head, REL_TOL / MEAN_ABS_TOL = 1e-3) and the poisoned copy bitwise equal to the clean
one - a lane that took a neighbour's bytes, or a request based one unit off, reads other tokens' codes or 0xFF there.

Shapes: bs 4, nh_k 8 - 32 (b, kv head) pairs, 8 splits on a 256-CU chip, T / 4096 units per wave (test_decode_lastblock_gpu.py):
    page ids     scattered (the builder's shuffle) and descending, under device lengths with a host bound beyond them (gap)
    unit counts  8185 partial last unit | 4160 one wave swaps a second slot | 8256 BLOCK + BLOCK_LAST | 16448 the loop's swaps in both slots
    forms        M 32 (one half swap), d 64 / M 32, d 64 / M 64 padded, C 128 (its instance serves every layout: present requests)
    heads        G 1 .. 3
    step form    device lengths + the fused append
    present form 128-token pages and row-major K must stay on the lane = token requests (the planner's rule)
    pool end     the last request's partial last unit sits in the LAST page of the pool: the requests read the unit's own bytes only"""
import numpy as np
import pytest

from tests import decode_poison as P

pytestmark = pytest.mark.gpu


def _case(name, d=128, M=64, C=256, G=4, kind=1, **kw):
    kw.setdefault("bs", 4)
    kw.setdefault("nhk", 8)
    return P.Case(name, d, M, C, G, kind, **kw)


# (case, page order: None = the builder's shuffle, "desc" = logical page L at pool page n_pool - 1 - L, "last" = the live pages in
#  order at the END of the pool, the spare pages in front)
CASES = [
    (_case("ids-scattered-gap", T=8256, r=40, rs=100, dev=True, gap=200), None),
    (_case("ids-descending-gap", T=8256, r=40, rs=100, dev=True, gap=200), "desc"),
    (_case("T8185-partial-last-unit", T=8185), None),
    (_case("T4160", T=4160, r=0), None),
    (_case("T8256", T=8256), "desc"),
    (_case("T16448", T=16448, r=5), None),
    (_case("M32", M=32, T=8256), None),
    (_case("M32-T16448", M=32, T=16448, r=0), "desc"),
    (_case("d64-M32", d=64, M=32, T=8256), None),
    (_case("d64-M64-padded", d=64, T=8256), None),
    (_case("d64-M16", d=64, M=16, T=8256), None),
    (_case("C128", C=128, T=8256), None),
    (_case("G1", G=1, T=8256), None),
    (_case("G2", G=2, T=4160), "desc"),
    (_case("G3", G=3, T=8185), None),
    (_case("dev-append", T=8256, r=100, rs=90, dev=True, gap=64, append=True), None),
    (_case("dev-append-M32-G2", M=32, G=2, T=8185, r=17, rs=120, dev=True, gap=130, append=True), "desc"),
    (_case("present-form-ps128", ps=128, T=8256), None),
    (_case("present-form-rowmajor-K", kl="row", T=8256), None),
    (_case("last-unit-in-last-pool-page", T=8185), "last"),
]


def _reorder(c, built, order):
    """The same case with its pool pages in another order: pools, live masks and page tables move together."""
    n_lp = c.bs * c.nhk * c.n_live
    inv = np.argsort(np.random.RandomState(7 + n_lp).permutation(c.n_pool))      # decode_poison.build: inv[logical] = pool page
    logical = np.arange(c.n_pool)
    new = c.n_pool - 1 - logical if order == "desc" else np.where(logical < n_lp, P.EXTRA_PAGES + logical, logical - n_lp)
    m = np.empty(c.n_pool, np.int64)
    m[inv] = new
    for side in ("clean", "poisoned", "live"):
        for nm in ("k_codes", "v_codes"):
            moved = np.empty_like(built[side][nm])
            moved[m] = built[side][nm]
            built[side][nm] = moved
    for side in ("clean", "poisoned"):
        built[side]["ids"] = m[built[side]["ids"]].astype(built[side]["ids"].dtype)
    live_ids = built["clean"]["ids"][built["live"]["ids"]]
    if order == "desc":
        assert (np.diff(live_ids.astype(np.int64)) == -1).all()
    else:
        assert int(live_ids[-1]) == c.n_pool - 1 and (np.diff(live_ids.astype(np.int64)) == 1).all()
    return built


@pytest.fixture(scope="module")
def env():
    import torch
    assert torch.cuda.is_available(), "GPU tests need an MI355X"
    from million_amd import ops, _lib
    return torch, ops, _lib.load(), _lib


@pytest.mark.parametrize("case,order", CASES, ids=[c.name for c, _ in CASES])
def test_code_requests_clean_and_poisoned(case, order, env, oracle, monkeypatch):
    torch, ops, lib, L = env
    if order is not None:
        build = P.build
        monkeypatch.setattr(P, "build", lambda c, src=None: _reorder(c, build(c, src), order))
    res = P.check_case(case, torch, ops, lib, L, oracle)
    print(f"{case.name}: rel {res['rel']:.3e} mean_abs {res['mean_abs']:.3e} worst head {res['worst_head']:.3e}")
