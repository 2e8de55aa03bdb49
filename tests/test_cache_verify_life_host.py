"""CPU tests of the random lifecycles with draft verification (tests/cache_verify_life.py): the coverage condition of every
committed script, the model's per-slot append rule against both forms of tests/verify_model.py, and the scripts on a CPU
PagedPQCache whose launches are the numpy stand-ins of the life and swap host tests plus three of this file's - ops.window_commit
advances the length rows by verify_model.commit_closed, the verify launches return zeros - with lengths (device rows and host
mirrors) and the allocator's invariants checked after every call, every refusal moving nothing, and every restored slot's live
data against what left at swap_out.

All four geometries run here: begin_step's side stream and events are replaced by objects that do nothing (a CPU cache's
launches are the stand-ins, in program order), so the kind of every decode step the cache reports is held against the model's
(Model.next_kind), which the coverage condition is computed on."""
import contextlib

import numpy as np
import pytest
import torch

from tests import cache_life_model as LM
from tests import cache_swap_model as SWM
from tests import cache_verify_life as VL
from tests import verify_model as VM
from tests.test_cache_life_host import _cpu_cache, _stand_ins
from tests.test_cache_swap_life_host import _live

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


# ---------------------------------------------------------------- the scripts on a CPU cache --------------------------------
class _Nothing:
    """A stream or an event of a cache whose launches are host functions."""

    def __init__(self, *a, **k):
        pass

    wait_stream = wait_event = record = synchronize = lambda self, *a, **k: None


def verify_stand_ins(monkeypatch):
    """Stand-ins of the launches verify and commit add to those of the life and swap host tests, and of the side stream."""
    from million_amd import ops
    step_attn = ops.pq_decode_attn      # (the life test's: the fused append advances r)

    def decode_attn(q, *a, k_new=None, return_lse=False, **k):
        if k_new is not None:
            return step_attn(q, *a, **k)
        out = torch.zeros_like(q)      # a verify launch appends nothing
        return (out, torch.zeros(q.shape[:3])) if return_lse else out

    def block_merge(q, k_blk, v_blk, out_a, lse_a, dev_n=None, out=None, lse_out=None, return_lse=False, k_stage=None, v_stage=None):
        out = torch.zeros_like(q) if out is None else out
        return (out, torch.zeros(q.shape[:3])) if return_lse else out

    def window_commit(k_new, v_new, k_res, v_res, k_prep, v_prep, k_pool, v_pool, page_ids, dev_lengths, dev_n, *, M, C, n_bound=None):
        rows, ps, cap = dev_lengths.numpy(), k_pool.shape[1], k_res.shape[3]
        assert rows.shape[:2] == (k_res.shape[0], len(dev_n)) and int(dev_n.max()) <= n_bound <= k_new.shape[3]
        for l in range(rows.shape[0]):
            for b, a in enumerate(dev_n.tolist()):
                T, r, st = VM.commit_closed(*(int(x) for x in rows[l, b, :3]), a, ps, cap)[:3]
                assert T <= page_ids.shape[3] * ps, "a flush past the page table"
                rows[l, b, :3] = (T, r, st)

    monkeypatch.setattr(ops, "pq_decode_attn", decode_attn)
    monkeypatch.setattr(ops, "attn_block_merge", block_merge)
    monkeypatch.setattr(ops, "window_commit", window_commit)
    monkeypatch.setattr(ops, "decode_workspace_bytes", lambda *a, **k: 16)
    monkeypatch.setattr(ops, "cache_swap", SWM.as_ops_stub())
    monkeypatch.setattr(torch.cuda, "Stream", _Nothing)
    monkeypatch.setattr(torch.cuda, "Event", _Nothing)
    monkeypatch.setattr(torch.cuda, "current_stream", lambda *a, **k: _Nothing())
    monkeypatch.setattr(torch.cuda, "stream", lambda s: contextlib.nullcontext())
    monkeypatch.setattr(torch.cuda, "is_current_stream_capturing", lambda: False)


def _same(before, after):
    return all(np.array_equal(before[k], after[k]) if isinstance(before[k], np.ndarray) else before[k] == after[k] for k in before)


def run_on_cpu(cache, calls, geom):
    """Drives the cache through a script (rows of zeros: nothing reads them), the model beside it; the checks after every call.
    -> the kinds begin_step reported."""
    m = VL.Model(geom)
    nl, bs, nh, nhk, d = geom["layer_num"], geom["bs"], geom["nh"], geom["num_key_value_heads"], geom["d"]
    z = lambda *s: torch.zeros(*s, dtype=torch.float16)
    tables0 = cache._page_ids_all.numpy().copy()
    snaps, left, kinds = {}, {}, []

    def check(what):
        snap = LM.snapshot(cache)
        LM.check_lengths(m, snap, what)
        if geom["preallocate"]:
            LM.check_allocator_preallocated(snap, tables0, what)
        else:
            LM.check_allocator_on_demand(m, snap, what)

    def verify(call, layers):
        for _ in range(2 if call["reverify"] else 1):
            for l in layers:
                cache.verify(z(bs, nh, call["n"], d), z(bs, nhk, call["n"], d), z(bs, nhk, call["n"], d), l, n_draft=call["n_draft"],
                             route=call["route"])

    def do(call, what):
        op = call["op"]
        if op == "decode":
            for s in range(call["steps"]):
                kind = None
                if geom["begin_step"]:
                    want = m.next_kind()
                    kind = cache.begin_step(use_dev_lengths=True)
                    kind = "pre" if kind.startswith("pre") else kind
                    assert kind == want, f"{what}: step {s} is a {kind!r} step, the model expects {want!r}"
                    kinds.append(kind)
                for l in range(nl):
                    cache.decoding_with_pages(z(bs, nh, 1, d), z(bs, nhk, 1, d), z(bs, nhk, 1, d), l, use_dev_lengths=True)
                m.step(kind=kind)
                assert np.array_equal(cache._pre_a, np.tile(m.pre, (nl, 1))), f"{what}: step {s}: encoded-ahead flags {cache._pre_a.tolist()}, model {m.pre.tolist()}"
            return
        if op == "verify_commit":
            before = LM.snapshot(cache)
            verify(call, call["layers"])
            assert _same(before, LM.snapshot(cache)), f"{what}: verify moved something"
            if call.get("between"):
                m.verify(call["n"], call["n_draft"], call["layers"])
                do(call["between"], what + ": between")
                check(what + ": between")
                call = dict(call, layers=[], between=None)
            if call.get("raises"):
                before = LM.snapshot(cache)
                with pytest.raises(RuntimeError, match=VL.REFUSALS[call["refusal"]]):
                    cache.commit(call["n_accept"])
                assert _same(before, LM.snapshot(cache)), f"{what}: a refused call moved something"
            else:
                cache.commit(call["n_accept"])
            m.apply(call)
            return
        if op == "swap_out":
            left[call["snap"]] = _live(cache, call["b"])
            snaps[call["snap"]] = cache.swap_out(call["b"])
        elif op == "swap_in":
            cache.swap_in(call["b"], snaps[call["snap"]])
            for a, b in zip(left[call["snap"]], _live(cache, call["b"])):
                assert np.array_equal(a, b), f"{what}: the restored slot does not hold what left"
        elif op == "release":
            cache.release(call["b"])
        elif op == "fork":
            cache.fork(call["src"], call["dst"], n_tokens=call["n_tokens"])
        elif op in ("prefill_request", "extend_request"):
            for l in range(nl):
                getattr(cache, op)(call["b"], z(1, nh, call["n"], d), z(1, nhk, call["n"], d), z(1, nhk, call["n"], d), l)
        else:
            n = max(call["n_new"])
            for l in range(nl):
                getattr(cache, op)(z(bs, nh, n, d), z(bs, nhk, n, d), z(bs, nhk, n, d), l, call["n_new"], device_store=call["device_store"])
        m.apply(call)

    for i, call in enumerate(calls):
        what = f"call {i} ({VL.describe(call)})"
        do(call, what)
        check(what)
        assert np.array_equal(cache._pre_a, np.tile(m.pre, (nl, 1))), f"{what}: encoded-ahead flags {cache._pre_a.tolist()}, model {m.pre.tolist()}"
    LM.check_end(cache, m, geom, tables0)
    return kinds


@pytest.mark.parametrize("name,seed", CASES, ids=[f"{n}-{s}" for n, s in CASES])
def test_script_on_a_cpu_cache(monkeypatch, name, seed):
    geom = VL.GEOMS[name]
    _stand_ins(monkeypatch)
    verify_stand_ins(monkeypatch)
    cache = _cpu_cache(geom)
    # the stand-ins encode nothing: give every pool page and window row bytes of its own, so that a restored slot shows its request
    g = torch.Generator().manual_seed(seed)
    cache.key_page_pool.copy_(torch.randint(0, 256, cache.key_page_pool.shape, generator=g, dtype=torch.uint8))
    cache.value_page_pool.copy_(torch.randint(0, 256, cache.value_page_pool.shape, generator=g, dtype=torch.uint8))
    cache._kres_all.copy_(torch.randn(cache._kres_all.shape, generator=g).half())
    cache._vres_all.copy_(torch.randn(cache._vres_all.shape, generator=g).half())
    calls = VL.script(seed, geom, rows=False)
    kinds = run_on_cpu(cache, calls, geom)
    if geom["begin_step"]:      # the coverage condition on the kinds the cache reported
        cnt = VL.coverage(calls, geom, kinds=kinds)
        assert not VL.missing(cnt, geom), f"{name} seed {seed} on the reported kinds lacks (have, need): {VL.missing(cnt, geom)}"
