"""CPU tests of the random lifecycles with draft verification (tests/cache_verify_life.py): the coverage condition of every
committed script, the model's per-slot append rule against both forms of tests/verify_model.py, and every script on a CPU
PagedPQCache (tests/cache_life_driver.py says what is checked); on the begin_step geometries the coverage condition is held
against the kinds of decode step the cache reported too."""
import numpy as np
import pytest

from tests import cache_life_driver as D
from tests import cache_life_model as LM
from tests import cache_verify_life as VL
from tests import verify_model as VM

CASES = [(name, seed) for name, seeds in VL.SEEDS.items() for seed in seeds]


@pytest.mark.parametrize("name,seed", CASES, ids=[f"{n}-{s}" for n, s in CASES])
def test_committed_scripts_meet_the_coverage_condition(name, seed):
    geom = VL.GEOMS[name]
    calls = VL.script(seed, geom, rows=False)
    cnt = VL.coverage(calls, geom)
    print(f"{name} seed {seed}: {cnt}")
    assert not VL.missing(cnt, geom), f"{name} seed {seed} lacks (have, need): {VL.missing(cnt, geom)}"
    verifies = sum(c["op"] == "verify_commit" and bool(c["layers"]) for c in calls)
    assert VL.N_CALLS <= cnt["calls"] <= 2 * VL.N_CALLS and verifies <= VL.MAX_ROUNDS
    assert cnt["decode_steps"] <= VL.DECODE_BUDGET[geom["extended_residual_size"]] + 8


def test_two_distinct_seeds_per_geometry():
    assert set(VL.SEEDS) == set(VL.GEOMS) == set(LM.GEOMS) and all(len(set(s)) == 2 for s in VL.SEEDS.values())
    assert sorted(g["begin_step"] for g in VL.GEOMS.values()) == [False, False, True, True]


def test_script_rows_are_reproducible_and_padded_with_nan():
    name = "share-32"
    geom = VL.GEOMS[name]
    a, b = (VL.script(VL.SEEDS[name][0], geom) for _ in range(2))
    strip = lambda calls: [{k: ({x: y for x, y in v.items() if x not in VL.ROW_KEYS} if isinstance(v, dict) else v)
                            for k, v in c.items() if k not in VL.ROW_KEYS} for c in calls]
    assert strip(a) == strip(b) == strip(VL.plan(VL.SEEDS[name][0], geom))
    seen = 0
    for ca, cb in zip(a, b):
        for key in VL.ROW_KEYS:
            if key in ca:
                assert ca[key].dtype == np.float16 and np.array_equal(ca[key].view(np.int16), cb[key].view(np.int16))
        if ca["op"] == "verify_commit":
            seen += 1
            nl, bs, nh, nhk, d = geom["layer_num"], geom["bs"], geom["nh"], geom["num_key_value_heads"], geom["d"]
            assert ca["q"].shape == (nl, bs, nh, ca["n"], d) and ca["k"].shape == ca["v"].shape == (nl, bs, nhk, ca["n"], d)
            assert ("q0" in ca) == bool(ca["reverify"])
            for s, n in enumerate(ca["n_draft"]):
                for key in ("q", "k", "v") + (("q0", "k0", "v0") if ca["reverify"] else ()):
                    assert np.isfinite(ca[key][:, s, :, :n]).all() and np.isnan(ca[key][:, s, :, n:]).all()
            if ca["reverify"]:
                assert not np.array_equal(ca["k"].view(np.int16), ca["k0"].view(np.int16))
    assert seen >= 12


def test_encode_rows_gives_the_model_the_accepted_rows_only():
    geom = VL.GEOMS["share-32"]
    call = dict(op="verify_commit", n=4, n_draft=[4, 3, 0, 2], n_accept=[2, 3, 0, 0], route=None, reverify=False, layers=[0, 1])
    rs = np.random.RandomState(3)
    shape = (geom["layer_num"], geom["bs"], geom["num_key_value_heads"], 4, geom["d"])
    call["k"], call["v"] = rs.standard_normal(shape).astype(np.float16), rs.standard_normal(shape).astype(np.float16)
    for b, nd in enumerate(call["n_draft"]):
        call["k"][:, b, :, nd:] = call["v"][:, b, :, nd:] = np.nan
    seen = []

    def enc(x):
        assert np.isfinite(x).all()      # a NaN row past n_draft never reaches the encoder
        seen.append(x.shape[2])
        return np.full(x.shape[:3] + (geom["M"],), 7, np.uint8)
    refused = dict(call, raises=True, refusal="over_accept", between=None)
    VL.encode_rows([call, refused], geom, enc, enc, type("Serial", (), {"map": staticmethod(map)}))
    rows = geom["layer_num"] * geom["num_key_value_heads"]
    assert sorted(seen) == sorted([2 * rows, 3 * rows] * 2) and "kc" not in refused
    for b, a in enumerate(call["n_accept"]):
        assert (call["kc"][:, b, :, :a] == 7).all() and not call["kc"][:, b, :, a:].any() and (call["vc"][:, b, :, :a] == 7).all()


@pytest.mark.parametrize("name", ["share-32", "copy-128"])
def test_append_rule_is_both_forms_of_the_commit(name):
    """Model.append, a times, against verify_model.commit_sequential and commit_closed for every window fill r, ring start rs
    and accepted count a of a geometry: the integers, and how many rows became codes."""
    geom = VL.GEOMS[name]
    ps, cap = geom["page_size"], geom["extended_residual_size"]
    for r in range(cap + 1):
        for rs in range(0, cap, max(1, ps // 4)) if r else (0,):
            for a in range(17):
                m = VL.Model(geom)
                m.T[:], m.r[:], m.rs[:] = 5, 9, 0
                m.T[1], m.r[1], m.rs[1] = 3 * ps, r, rs
                flushed = m.commit([0, a, 0, 0])
                got = (int(m.T[1]), int(m.r[1]), int(m.rs[1]))
                seq, closed = VM.commit_sequential(3 * ps, r, rs, a, ps, cap), VM.commit_closed(3 * ps, r, rs, a, ps, cap)
                assert got == seq[:3] == closed[:3], f"r={r} rs={rs} a={a}: the rule {got}, sequential {seq[:3]}, closed {closed[:3]}"
                assert len(seq[3]) == len(closed[3]) == got[0] - 3 * ps and flushed == [1] * (len(seq[3]) // ps)
                assert (m.T[0], m.r[0], m.rs[0]) == (5, 9, 0) and m.n(1) == 3 * ps + r + a      # that slot only; no row is lost


@pytest.mark.parametrize("name,seed", CASES, ids=[f"{n}-{s}" for n, s in CASES])
def test_script_on_a_cpu_cache(monkeypatch, name, seed):
    geom = VL.GEOMS[name]
    calls = VL.script(seed, geom, rows=False)
    kinds = D.run_on_cpu(monkeypatch, geom, calls, seed).kinds
    if geom["begin_step"]:      # the coverage condition on the kinds the cache reported
        cnt = VL.coverage(calls, geom, kinds=kinds)
        assert not VL.missing(cnt, geom), f"{name} seed {seed} on the reported kinds lacks (have, need): {VL.missing(cnt, geom)}"
