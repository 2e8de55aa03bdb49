"""CPU side of the poisoned-memory matrix (tests/decode_poison.py): every row still plans the kernel it is meant to test, and
the builders really poison something in every row - so a planner change cannot move the table onto another kernel, and a
builder change cannot turn the matrix into clean-memory parity, without a failure here."""
import numpy as np
import pytest

from tests import decode_poison as P


@pytest.fixture(scope="module")
def lib():
    from million_amd import build, _lib
    build.build()
    return _lib.load()


@pytest.mark.parametrize("case", P.CASES, ids=[c.name for c in P.CASES])
def test_poison_case_plans_its_kernel(case, lib):
    from million_amd import _lib
    assert P.kernel_kind(case, lib, _lib) == case.kind


def test_poison_matrix_covers_the_issue():
    kinds = {(c.kind, c.policy) for c in P.CASES}
    assert {(1, 0), (1, 16), (2, 0), (3, 0), (0, 1)} <= kinds
    lean = {(c.d, c.M, c.C) for c in P.CASES if c.kind == 1 and c.policy == 0 and c.G <= 4}
    for d, M in ((128, 64), (128, 32), (64, 64), (64, 32), (64, 16)):
        assert {(d, M, 256), (d, M, 128)} <= lean, (d, M)
    assert {c.ps for c in P.CASES if c.kind == 1 and c.policy == 0 and c.d == 128 and c.kl == "paged"} >= {64, 128}
    stream = {(c.M, c.C) for c in P.CASES if c.policy == 16}
    assert {(M, C) for M in (64, 32, 16) for C in (256, 128)} <= stream
    parts = {(c.d, c.M, c.G) for c in P.CASES if c.dev and c.append and 4 < c.G <= 16}
    assert {(64, 7), (64, 8), (128, 8)} <= {(d, G) for d, _, G in parts}
    assert any(c.G > 16 and c.dev and c.append for c in P.CASES)
    assert any(c.kind == 3 and c.ps == 32 and c.d == 64 for c in P.CASES)
    assert any(c.kind == 3 and c.T == 0 for c in P.CASES)
    assert {c.vl for c in P.CASES if c.kl == "row"} >= {"row", "paged", "dense"}
    assert any(c.i64 for c in P.CASES) and any(not c.i64 and c.paged for c in P.CASES)
    assert any(c.rs + c.r > c.cap for c in P.CASES if c.append) and any(c.rs + c.r > c.cap for c in P.CASES if not c.append)


def _differ_everywhere(a, b):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    if a.dtype == np.float16:
        a, b = a.view(np.uint16), b.view(np.uint16)
    return bool(np.all(a != b))


@pytest.mark.parametrize("case", P.CASES, ids=[c.name for c in P.CASES])
def test_poison_builders_poison(case):
    c = case
    built = P.build(c)
    cl, po, live = built["clean"], built["poisoned"], built["live"]
    if c.T:
        assert c.T % 64 and c.T % c.ps, "the last live page must be partial"
    assert c.r < c.cap, "window rows outside the span must exist"
    if c.kl == "paged" or c.vl == "paged":
        assert c.n_pages_cap > c.n_live and (~live["ids"]).any(), "page-table entries past the live pages must exist"
        assert ((po["ids"] >= 0) & (po["ids"] < c.n_pool)).all(), "poisoned ids must stay inside the pool"
    if c.dev:
        assert c.T_host > c.T and -(-c.T_host // c.ps) > c.n_live or c.kl == "row", "pages between the device and host lengths"
    for nm in ("k_codes", "v_codes", "k_res", "v_res", "ids"):
        if cl.get(nm) is None:
            continue
        lv = live[nm]
        a, b = np.ascontiguousarray(cl[nm]), np.ascontiguousarray(po[nm])
        if a.dtype == np.float16:
            a, b = a.view(np.uint16), b.view(np.uint16)
        assert np.array_equal(a[lv], b[lv]), f"{nm}: live bytes differ between the copies"
        assert (~lv).any(), f"{nm}: nothing outside the live data"
        assert _differ_everywhere(a[~lv], b[~lv]), f"{nm}: the copies agree somewhere outside the live data"
        if nm.endswith("codes"):
            assert (b[~lv] == 0xFF).all() and (a[~lv] == 0).all()
        if nm.endswith("res"):
            assert np.isnan(po[nm][~lv]).all() and (cl[nm][~lv] == 0).all()
    # pool pages that no live entry names exist and are 0xFF
    if c.kl == "paged":
        named = set(np.asarray(built["clean"]["ids"])[live["ids"]].ravel().tolist())
        unused = [p for p in range(c.n_pool) if p not in named]
        assert len(unused) >= P.EXTRA_PAGES and all((po["k_codes"][p] == 0xFF).all() for p in unused)
    if c.append:
        row = (c.rs + c.r) % c.cap
        assert not live["k_res"][0, 0, row, 0] and np.isnan(po["k_res"][:, :, row]).all()
