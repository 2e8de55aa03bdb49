"""CPU side of the decode numerics tests: the inputs of tests/decode_inputs.py are well posed for a per-head bar, and the
arithmetic of the lean and streaming decode kernels, restated in numpy (decode_inputs.model_workgroups), meets that bar on them.

Well posed is a condition, not a measurement: on every (family or peak, shape) pair that test_decode_numerics_gpu.py runs, the
fp64 result rounded to fp16 (the best any kernel can do) and the model are within 0.5 x REL_TOL on their worst head, so a GPU
kernel that misses REL_TOL on a head is wrong by at least as much again as its number formats explain.  The model runs on the
workgroups that hold the first head of the first request and the last head of the last one.

test_flushed_subnormal_probabilities_miss_the_bar shows that the many-pairs case of the GPU file can fail: the same arithmetic
with fp16-subnormal probabilities read as zero misses the bar twice over on every sampled head.
test_whole_tensor_norm_is_blind_to_one_head keeps the reason for the per-head bar in the suite."""
import dataclasses
import hashlib

import numpy as np
import pytest

from tests import decode_inputs as D
from tests import decode_poison as P
from tests import flash_inputs as F

CAP = 0.5 * F.REL_TOL


def _worst(out, gold):
    return float(F.row_err(out, gold).max())


def _well_posed(oracle, c, src, what, requests=None):
    """ideal and model within CAP: the ideal on every head of the sampled requests, the model on the first head of the first and
    the last head of the last."""
    bs = src["q"].shape[0]
    for b, h in ((0, 0), (bs - 1, c.nh - 1)) if requests is None else requests:
        g = D.gold(oracle, c, D.request(src, b))[0]
        assert np.isfinite(g).all() and np.linalg.norm(g[h]) > 0
        ideal = _worst(F.ideal(g), g)
        assert ideal <= CAP, f"{what}: request {b}: ideal worst head {ideal:.2e}"
        m = D.model_heads(oracle, c, src, [h], b=b)[h]
        e = _worst(m[None], g[h])
        assert e <= CAP, f"{what}: request {b} head {h}: model {e:.2e}"


# ---------------------------------------------------------------- the generator --------------------------------------------
def test_decode_gold_is_the_chunk_gold_at_one_query_row(oracle):
    """The family code's own fp64 reference (flash_inputs.chunk_gold, one chunk row = the appended row) and the project's oracle
    (oracle.decode_attn over codes + ring + appended row) agree to 1e-12."""
    for cname, name in (("lean-d128-M64-ps64-C128", "sink_local"), ("lean-d64-M32-C256", "stair5")):
        c = P.BY_NAME[cname]
        src = D.for_case(name, c)
        g = D.gold(oracle, c, src)
        cg = F.chunk_gold(oracle, src["st"])
        assert g.shape == cg.shape == (c.bs, c.nh, 1, c.d)
        assert np.abs(g - cg).max() <= 1e-12 * np.abs(g).max()
        built = P.build(c, src)
        assert np.array_equal(P.gold(c, built, oracle), g)      # and through the case builder


def test_build_with_a_source_keeps_its_arrays():
    """build(c, src) lays out the source's arrays, and nothing else, as it lays out its own draws."""
    c = P.BY_NAME["lean-d128-M64-ps64-C128"]
    src = D.for_case("peak:appended", c)
    own, b = P.build(c), P.build(c, src)
    for nm in ("q", "k_cents", "v_cents", "k_new", "v_new"):
        assert b["clean"][nm] is src[nm] and b["poisoned"][nm] is src[nm]
    assert b["k_codes"] is src["k_codes"] and b["v_codes"] is src["v_codes"]
    for nm in ("k_codes", "v_codes", "k_res", "v_res", "ids"):
        assert np.array_equal(b["live"][nm], own["live"][nm])
        lv = b["live"][nm]
        if nm != "ids":
            assert np.array_equal(b["poisoned"][nm].view(np.uint16 if nm.endswith("res") else np.uint8)[~lv],
                                  own["poisoned"][nm].view(np.uint16 if nm.endswith("res") else np.uint8)[~lv])
    assert np.array_equal(b["clean"]["ids"], own["clean"]["ids"]) and np.array_equal(b["poisoned"]["ids"], own["poisoned"]["ids"])
    ring = (c.rs + np.arange(c.r)) % c.cap
    assert np.array_equal(b["clean"]["k_res"][:, :, ring], src["k_res"][:, :, ring])
    at = src["peak_at"]
    assert at == c.T + c.r      # the dominating key is the row the launch appends


# sha256 over every array of both copies and the live masks, computed with build() as it was before it took a source
BUILD_HASHES = {
    "lean-d128-M64-ps64-C128": "8ba39b01e9dc15affee68f371d9a899c2df16009e19304c94b0e952994f9c5eb",
    "parts-d64-M32-G7-C128": "a037a0599f9d6a73dab26d21fa0f18096b0997f29c7a2b7f9b7b04c38b896253",
    "rowkv-d64-M16-C128": "4b3dfc6b3314efd34ee9cdac0993463d345850fcf99ec5d743e3218049100e44",
    "scalar-pagedK-rowV-d128-M64-C256": "47d4274d5628c4a4f48c1f4048a50381fe132118dfad7edee068c4afa29d8adb",
    "tile-T0-d128-M64-C256": "07c8c32350005c2c3b7025478f5d6edca12cbcc8428cae2770198d81b12342f9",
}


def build_hash(built):
    h = hashlib.sha256()
    for part in ("clean", "poisoned", "live"):
        for nm in sorted(built[part]):
            a = built[part][nm]
            h.update(nm.encode())
            if a is not None:
                a = np.ascontiguousarray(a)
                h.update(repr((a.dtype.str, a.shape)).encode())
                h.update(a.tobytes())
    for nm in ("k_codes", "v_codes"):
        h.update(np.ascontiguousarray(built[nm]).tobytes())
    return h.hexdigest()


@pytest.mark.parametrize("cname", list(BUILD_HASHES))
def test_build_without_a_source_is_unchanged(cname):
    assert build_hash(P.build(P.BY_NAME[cname])) == BUILD_HASHES[cname]


# ---------------------------------------------------------------- the cases plan the kernels they are meant for ------------
@pytest.fixture(scope="module")
def lib():
    from million_amd import build, _lib
    build.build()
    return _lib.load()


def test_generated_cases_plan_the_mfma_kernels(lib):
    from million_amd import _lib
    cases = [D.many_pairs_case(pol) for pol in (0, 16)]
    cases += [D.group_case(*form, G) for form in D.GROUP_FORMS for G in D.GROUPINGS]
    cases += [D.ragged_case(i, pol) for i in range(len(D.RAGGED_T)) for pol in (0, 16)]
    for c in cases:
        assert P.kernel_kind(c, lib, _lib) == 1, c.name
    assert {c.name for c in map(P.BY_NAME.get, D.SECTION_A)} == set(D.SECTION_A)
    kinds = {(c.kind, c.policy) for c in map(P.BY_NAME.get, D.SECTION_A)}
    assert {(1, 0), (1, 16), (3, 0), (0, 1)} <= kinds


def test_model_dealing_matches_the_launch_front():
    """Every token belongs to exactly one (split, wave, round), for both unit sizes and page sizes, whatever the split count."""
    for unit, ps in ((64, 64), (64, 128), (32, 32), (32, 64), (32, 128)):
        for ns in (1, 3, 7):
            T = 2500
            upp = ps // unit
            seen = np.zeros(T, int)
            for s in range(ns):
                for w in range(8):
                    t0 = ((w // upp) * ns + s) * ps + (w % upp) * unit
                    for tu in range(t0, T, ns * (8 // upp) * ps):
                        seen[tu:tu + unit] += 1
            assert (seen == 1).all(), (unit, ps, ns)
    assert D.mfma_splits(4096, 256, 128) == 1 and D.mfma_splits(1000, 4, 128) == 2 and D.mfma_splits(3333, 2, 128) == 7
    assert D.mfma_splits(40, 2, 256) == 2 and D.mfma_splits(100000, 1, 128) == 64


# ---------------------------------------------------------------- well-posedness, section by section of the GPU file -------
A_PAIRS = [(cn, n) for cn in D.SECTION_A for n in D.NAMES if D.has_peak(P.BY_NAME[cn], D.split_name(n)[1])]
B_PAIRS = [(c.name, n) for c in P.CASES for n in D.SECTION_B_NAMES]


@pytest.mark.parametrize("cname,name", A_PAIRS + [p for p in B_PAIRS if p not in A_PAIRS], ids=lambda x: x)
def test_families_are_well_posed_on_the_case_matrix(cname, name, oracle):
    c = P.BY_NAME[cname]
    src = D.for_case(name, c)
    _well_posed(oracle, c, src, f"{cname} {name}")
    peak = D.split_name(name)[1]
    if peak is not None:      # the dominating key holds nearly all of the mass
        K, _ = D.keys(oracle, c, src)
        s = F.logits(src["q"][:1], K[None])[0, :, 0]
        at = src["peak_at"]
        assert np.all(s[:, at] - np.delete(s, at, axis=1).max(axis=1) > 0.5 * F.PEAK_NATS)


@pytest.fixture(scope="module")
def many_pairs():
    cache = {}

    def get(name):
        if name not in cache:
            cache.clear()
            cache[name] = D.for_case(name, D.many_pairs_case(0))
        return cache[name]
    return get


@pytest.mark.parametrize("policy", [0, 16], ids=["lean", "stream"])
@pytest.mark.parametrize("name", D.MANY_PAIRS_NAMES)
def test_families_are_well_posed_at_one_split_per_pair(name, policy, many_pairs, oracle):
    c = D.many_pairs_case(policy)
    assert D.mfma_splits(c.T_host, c.bs * c.nhk, c.cap) == 1
    _well_posed(oracle, c, many_pairs(name), f"{c.name} {name}")


def test_flushed_subnormal_probabilities_miss_the_bar(many_pairs, oracle):
    """descending at T = 4096 with one split per (request, kv head): key 0 is the maximum, wave 0 of the workgroup streams
    T / 8 = 512 keys under its reference, and their probabilities 2^-10 .. 2^-20 are partly fp16-subnormal.  Read as zero, the
    share they carry is lost from O but not from l: at least two bars on every sampled head, on both kernels; read as they are,
    half a bar at most."""
    src = many_pairs("descending")
    for policy in (0, 16):
        c = D.many_pairs_case(policy)
        for b, heads in ((0, [0, 5, 14, 31]), (c.bs - 1, [0, 17, c.nh - 1])):
            g = D.gold(oracle, c, D.request(src, b))[0]
            flushed = D.model_heads(oracle, c, src, heads, b=b, flush=True)
            plain = D.model_heads(oracle, c, src, heads, b=b)
            for h in heads:
                ef, ep = _worst(flushed[h][None], g[h]), _worst(plain[h][None], g[h])
                print(f"{c.name} request {b} head {h}: flushed {ef:.2e} plain {ep:.2e}")
                assert ef >= 2 * F.REL_TOL, f"{c.name} request {b} head {h}: flushed model {ef:.2e}"
                assert ep <= CAP, f"{c.name} request {b} head {h}: model {ep:.2e}"


G_PAIRS = [(form, G, n) for form in D.GROUP_FORMS for G in D.GROUPINGS for n in D.GROUP_NAMES]


@pytest.mark.parametrize("form,G,name", G_PAIRS, ids=[f"{f[0]}-G{G}-{n}" for f, G, n in G_PAIRS])
def test_families_are_well_posed_for_every_head_grouping(form, G, name, oracle):
    c = D.group_case(*form, G)
    src = D.group_inputs(name, c)
    _well_posed(oracle, c, src, f"{c.name} {name}")
    if name.startswith("peak:"):      # one head of every group sees the peak, the others do not
        K, _ = D.keys(oracle, c, src)
        s = F.logits(src["q"][:1], K[None])[0, :, 0]
        at, keep = src["peak_at"], (G - 1 if name == "peak:last_head" else 0)
        lead = s[:, at] - np.delete(s, at, axis=1).max(axis=1)
        for h in range(c.nh):
            assert (lead[h] > 0.5 * F.PEAK_NATS) == (h % G == keep), (h, lead[h])


@pytest.fixture(scope="module")
def ragged():
    return D.ragged_inputs()


@pytest.mark.parametrize("policy", [0, 16], ids=["lean", "stream"])
@pytest.mark.parametrize("i", range(len(D.RAGGED_T)), ids=[f"T{t}-r{r}" for t, r in zip(D.RAGGED_T, D.RAGGED_R)])
def test_families_are_well_posed_at_the_ragged_lengths(i, policy, ragged, oracle):
    c, src = D.ragged_request(ragged, i, policy)
    assert c.T + c.r > 0
    _well_posed(oracle, c, src, c.name, requests=[(i, 0), (i, c.nh - 1)])


# ---------------------------------------------------------------- why the bar is per head ---------------------------------
def test_whole_tensor_norm_is_blind_to_one_head(oracle):
    """32 heads; one of them is gold x (1 + 4e-3), the others the fp16 rounding of gold: the whole-tensor check passes, the
    per-head check fails (and passes without the bad head)."""
    c = dataclasses.replace(P.BY_NAME["lean-d128-M64-ps64-C256"], bs=1, nhk=8)
    src = D.for_case("gauss4", c)
    g = D.gold(oracle, c, src)
    out = F.ideal(g).astype(np.float64)
    D.check_heads(out, g, "ideal", "gauss4")
    out[0, 13] = g[0, 13] * (1 + 4e-3)
    assert D.whole_tensor_ok(out, g)
    with pytest.raises(AssertionError, match=r"worst head \(b=0, h=13, i=0\)"):
        D.check_heads(out, g, "one head off", "gauss4")
    assert abs(P.head_err(out, g)[0, 13] - 4e-3) < 1e-6
