"""The lean decode kernel's code requests (csrc/attn_lean.h: UNIT_REQ_K, UNIT_REQ_V, LEAN_K_LANE_IS_TOKEN, VG), restated in
numpy: which bytes of a 64-token unit every lane of every wave request takes, in the present lane = token layout and in the
read-once instances' whole-line layout, and what the row swaps (K) and the parity select (V) leave in every lane.

A byte is modelled by its offset from the page's base (pages are 64 M or 128 M bytes, so a page base is line-aligned):
    K page [token][M]:         token t, byte m     at (tin + t) M + m
    V page [subspace][ps]:     subspace s, token t at s ps + tin + t
tin is the unit's first token inside its page: 0 at 64-token pages, 0 or 64 at 128-token pages.

For every lean (M, d) form and both page-relative unit offsets the tests assert that
  * every whole-line wave request covers whole 128-byte lines,
  * every line of the unit is touched by exactly one request per side,
  * after the modelled swaps / select every lane holds exactly the bytes of the present layout,
and, for the record the planner's rule rests on, that the present layout touches a K line from NQ requests and a d_m = 2 V
line from two, and that at 128-token pages a V line belongs to two units (no whole-line form exists there)."""
import numpy as np
import pytest

LINE = 128
# (M, d, d_m = 2 value form): d = 64 / M = 64 runs as the zero-padded d_m = 2 form of d = 128 / M = 64 - the codes are the same
FORMS = [(64, 128, True), (32, 128, False), (32, 64, True), (16, 64, False), (64, 64, True)]
IDS = ["d128-M64", "d128-M32", "d64-M32", "d64-M16", "d64-M64-padded"]
UNITS = [(64, 0), (128, 0), (128, 64)]      # (page size, tin)

LANE = np.arange(64)
B16 = np.arange(16)


# ---- the present layout (what the products expect) ----
def k_present(M, tin):
    """[q][lane][16]: lane = token, register q = bytes [16 q, 16 q + 16) of its code row."""
    nq = M // 16
    return np.stack([(tin + LANE)[:, None] * M + 16 * q + B16[None, :] for q in range(nq)])


def v_present(M, dm2, ps, tin):
    """[x][lane (kg, n)][16]: d_m = 2: subspace 32 (x >> 1) + 16 ((x & 1) ^ (kg & 1)) + n; d_m = 4: subspace n + 16 x;
    tokens 16 kg .. 16 kg + 15."""
    nq, kg, n = M // 16, LANE >> 4, LANE & 15
    rows = [32 * (x >> 1) + 16 * ((x & 1) ^ (kg & 1)) + n if dm2 else n + 16 * x for x in range(nq)]
    return np.stack([(r * ps + tin + 16 * kg)[:, None] + B16[None, :] for r in rows])


# ---- the whole-line requests ----
def k_whole_requests(M, tin):
    """[q][lane][16]: request q takes tokens (64 / NQ) q .. whole: lane (j, a) bytes [16 j, 16 j + 16) of token (64 / NQ) q + a."""
    nq = M // 16
    rpq = 64 // nq
    a, j = LANE % rpq, LANE // rpq
    return np.stack([(tin * M + 1024 * q + a * M + 16 * j)[:, None] + B16[None, :] for q in range(nq)])


def v_whole_requests(M, dm2, ps, tin):
    """[x][lane (kg, n)][16]: subspace row n + 16 x (d_m = 2: n + 16 (x & 1) + 32 (x >> 1) - the same number), tokens 16 kg .."""
    nq, kg, n = M // 16, LANE >> 4, LANE & 15
    return np.stack([((n + 16 * x) * ps + tin + 16 * kg)[:, None] + B16[None, :] for x in range(nq)])


def permlane32_swap(a, b):
    """v_permlane32_swap a, b: lanes 32-63 of a <-> lanes 0-31 of b."""
    a2, b2 = a.copy(), b.copy()
    a2[32:], b2[:32] = b[:32], a[32:]
    return a2, b2


def permlane16_swap(a, b):
    """v_permlane16_swap a, b: rows 1, 3 of a <-> rows 0, 2 of b (rows of 16 lanes)."""
    a2, b2 = a.copy(), b.copy()
    for r in (0, 2):
        a2[16 * (r + 1):16 * (r + 2)], b2[16 * r:16 * (r + 1)] = b[16 * r:16 * (r + 1)], a[16 * (r + 1):16 * (r + 2)]
    return a2, b2


def k_lane_is_token(k):
    """LEAN_K_LANE_IS_TOKEN: per dword, registers (q, q + NQ / 2) by halves, then (at NQ = 4) registers (q, q + 1), q even, by
    rows.  A swap moves whole dwords; a register is modelled as its 16 bytes, four dwords swapped alike."""
    k = [x.copy() for x in k]
    nq = len(k)
    if nq == 1:
        return np.stack(k)
    for q in range(nq // 2):
        k[q], k[q + nq // 2] = permlane32_swap(k[q], k[q + nq // 2])
    if nq == 4:
        for q in (0, 2):
            k[q], k[q + 1] = permlane16_swap(k[q], k[q + 1])
    return np.stack(k)


def v_select(v, dm2):
    """VG: a lane of an odd token group takes the pair's other register."""
    if not dm2:
        return v
    odd = ((LANE >> 4) & 1).astype(bool)[None, :, None]
    other = v[np.arange(len(v)) ^ 1]
    return np.where(odd, other, v)


def lines_per_request(req):
    """For every request: {line: number of its bytes the request takes}."""
    out = []
    for r in req:
        ln, cnt = np.unique(r.ravel() // LINE, return_counts=True)
        assert len(np.unique(r.ravel())) == r.size, "a request takes a byte twice"
        out.append(dict(zip(ln.tolist(), cnt.tolist())))
    return out


def assert_whole_lines_once(req, unit_bytes):
    per = lines_per_request(req)
    for i, d in enumerate(per):
        assert all(c == LINE for c in d.values()), f"request {i} takes part of a line: {d}"
        assert len(d) == 8, f"request {i}: {len(d)} lines, not 1 KiB"
    unit_lines = sorted(set((np.asarray(unit_bytes) // LINE).tolist()))
    touched = sorted(l for d in per for l in d)
    assert touched == unit_lines, "the requests do not touch every line of the unit exactly once"
    assert sorted(np.concatenate([r.ravel() for r in req]).tolist()) == sorted(np.asarray(unit_bytes).tolist())


@pytest.mark.parametrize("ps,tin", UNITS, ids=[f"ps{p}-tin{t}" for p, t in UNITS])
@pytest.mark.parametrize("M,d,dm2", FORMS, ids=IDS)
def test_k_requests_whole_lines_and_lane_is_token(M, d, dm2, ps, tin):
    """K pages are token-major: a unit is 64 M contiguous bytes at either offset, so the K map holds at both page sizes (the
    planner still keeps 128-token pages on the present form: their V lines are shared, below)."""
    req = k_whole_requests(M, tin)
    unit = np.arange(tin * M, (tin + 64) * M)
    assert_whole_lines_once(req, unit)
    assert np.array_equal(k_lane_is_token(req), k_present(M, tin))


@pytest.mark.parametrize("M,d,dm2", FORMS, ids=IDS)
def test_v_requests_whole_lines_and_select(M, d, dm2):
    """64-token pages (tin = 0): the unit is the whole V page."""
    req = v_whole_requests(M, dm2, 64, 0)
    assert_whole_lines_once(req, np.arange(64 * M))
    assert np.array_equal(v_select(req, dm2), v_present(M, dm2, 64, 0))
    if not dm2:      # d_m = 4: the present requests are whole rows already
        assert np.array_equal(req, v_present(M, dm2, 64, 0))


@pytest.mark.parametrize("M,d,dm2", FORMS, ids=IDS)
def test_present_layout_shares_lines_between_requests(M, d, dm2):
    """What the L1 merges today and would reach L2 as separate requests without it: every K line is touched by all NQ requests
    of its unit, every d_m = 2 V line by two."""
    nq = M // 16
    per = lines_per_request(k_present(M, 0))
    lines = sorted(set(l for d_ in per for l in d_))
    assert len(lines) == 64 * M // LINE
    if nq > 1:      # M = 16: a row is one request's 16 bytes - eight tokens per line, one request
        assert all(sum(l in d_ for d_ in per) == nq for l in lines)
        assert all(c == LINE // nq for d_ in per for c in d_.values())
    per = lines_per_request(v_present(M, dm2, 64, 0))
    lines = sorted(set(l for d_ in per for l in d_))
    assert all(sum(l in d_ for d_ in per) == (2 if dm2 else 1) for l in lines)


@pytest.mark.parametrize("tin", [0, 64])
@pytest.mark.parametrize("M,d,dm2", FORMS, ids=IDS)
def test_v_lines_of_128_token_pages_belong_to_two_units(M, d, dm2, tin):
    """A subspace row of a 128-token page is one line, half of it this unit's: no request of one wave can take it whole, and the
    select still reproduces the present layout (the maps do not depend on the page size; the planner does)."""
    req = v_whole_requests(M, dm2, 128, tin)
    per = lines_per_request(req)
    assert all(c == LINE // 2 for d_ in per for c in d_.values())
    assert np.array_equal(v_select(req, dm2), v_present(M, dm2, 128, tin))
