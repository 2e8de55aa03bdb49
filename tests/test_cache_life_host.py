"""CPU tests of the random request lifecycles (tests/cache_life_model.py): the coverage condition of every committed script,
the model's decode rule against the oracle's paging policy, and the scripts themselves on a CPU PagedPQCache whose launches are
numpy stand-ins that move the device rows the way each call's contract says - lengths (device rows and host mirrors) and the
allocator's invariants after every call.  Codes, windows and attention outputs are the GPU file's (tests/test_cache_life_gpu.py).

Only the two geometries without begin_step run here: begin_step opens a torch.cuda.Stream on its `pre` and `flush` kinds and
cannot run without a GPU."""
import numpy as np
import pytest
import torch

from tests import cache_fork_model as FM
from tests import cache_life_model as LM
from tests import store_ragged_model as SM

CASES = [(name, seed) for name, seeds in LM.SEEDS.items() for seed in seeds]


@pytest.mark.parametrize("name,seed", CASES, ids=[f"{n}-{s}" for n, s in CASES])
def test_committed_scripts_meet_the_coverage_condition(name, seed):
    geom = LM.GEOMS[name]
    cnt = LM.coverage(LM.script(seed, geom, rows=False), geom)
    print(f"{name} seed {seed}: {cnt}")
    assert not LM.missing(cnt, geom), f"{name} seed {seed} lacks (have, need): {LM.missing(cnt, geom)}"
    assert 70 <= cnt["calls"] <= 100 and cnt["decode_steps"] <= LM.DECODE_BUDGET + 2 * geom["extended_residual_size"]


def test_two_distinct_seeds_per_geometry():
    assert set(LM.SEEDS) == set(LM.GEOMS) and all(len(set(s)) == 2 for s in LM.SEEDS.values())


def test_script_rows_are_reproducible_and_padded_with_nan():
    geom = LM.GEOMS["share-32"]
    a, b = (LM.script(LM.SEEDS["share-32"][0], geom) for _ in range(2))
    strip = lambda calls: [{k: v for k, v in c.items() if k not in "qkv"} for c in calls]
    assert strip(a) == strip(b) == LM.plan(LM.SEEDS["share-32"][0], geom)
    for ca, cb in zip(a, b):
        for key in "qkv":
            if key in ca:
                assert ca[key].dtype == np.float16 and np.array_equal(ca[key].view(np.int16), cb[key].view(np.int16))
        if ca["op"].endswith("ragged"):
            for s, n in enumerate(ca["n_new"]):
                assert np.isfinite(ca["k"][:, s, :, :n]).all() and np.isnan(ca["k"][:, s, :, n:]).all() and np.isnan(ca["q"][:, s, :, n:]).all()


@pytest.mark.parametrize("ps,cap", [(32, 64), (64, 128), (128, 128)])
@pytest.mark.parametrize("prompt", [0, 5, 70])
def test_decode_rule_is_the_oracles_paging_policy(oracle, ps, cap, prompt):
    m = LM.Model(dict(LM.BASE, page_size=ps, extended_residual_size=cap))
    if prompt:
        m.prefill(1, prompt)
    pol = oracle.PagedPolicy(page_size=ps, residual=cap, prefill=prompt)
    idle = oracle.PagedPolicy(page_size=ps, residual=cap, prefill=0)
    for i in range(300):
        m.step()
        assert (m.T[1], m.r[1]) == pol.step() and (m.T[0], m.r[0]) == idle.step(), f"step {i}"
        assert m.rs[1] == (m.T[1] - prompt) % cap and m.n(1) == prompt + i + 1


# ---------------------------------------------------------------- the scripts on a CPU cache --------------------------------
def _advance(rows, who, n, cap):
    """The flush advance of the lengths rows `who` (a mask over (rows, 4) int32), in place."""
    rows[who, 0] += n
    rows[who, 1] -= n
    rows[who, 2] = (rows[who, 2] + n) % cap


def _stand_ins(monkeypatch):
    from million_amd import ops

    def decode_attn(q, *a, dev_lengths=None, **k):
        dev_lengths[:, 1] += 1      # the fused append
        return torch.zeros_like(q)

    def flush(k_rows, v_rows, k_cents, v_cents, k_pool, v_pool, page_ids, *, n, page_size, token_start=0, x_row_start=0,
              dev_lengths=None, min_r=0, advance=True):
        if dev_lengths is not None and advance:
            rows = dev_lengths.view(-1, 4).numpy()
            _advance(rows, rows[:, 1] >= min_r, n, k_rows.shape[-2])

    def lengths_advance(dev_lengths, n_flushed, resid_cap):
        rows = dev_lengths.numpy()
        _advance(rows, np.ones(len(rows), bool), n_flushed, resid_cap)

    def store_ragged(k_new, v_new, k_res, v_res, k_prep, v_prep, k_pool, v_pool, page_ids, dev_lengths, dev_n, *, M, C, page_size):
        dev_lengths.copy_(torch.from_numpy(SM.advance(dev_lengths.numpy(), dev_n.numpy(), page_size=page_size, n_pages_cap=page_ids.shape[2],
                                                      resid_cap=k_res.shape[2], n_bound=k_new.shape[2])))

    monkeypatch.setattr(ops, "pq_encode_into", lambda *a, **k: None)
    monkeypatch.setattr(ops, "prefill_attn", lambda q, k, v, **kw: torch.zeros_like(q))
    monkeypatch.setattr(ops, "pq_chunk_attn", lambda q, *a, **k: torch.zeros_like(q))
    monkeypatch.setattr(ops, "pq_decode_attn", decode_attn)
    monkeypatch.setattr(ops, "pq_flush", flush)
    monkeypatch.setattr(ops, "lengths_advance", lengths_advance)
    monkeypatch.setattr(ops, "pq_store_ragged", store_ragged)
    monkeypatch.setattr(ops, "cache_fork", FM.as_ops_stub())


def _cpu_cache(geom):
    """As tests/cache_trace_scenario.py sets up its CPU cache: codebooks, prepared images and workspace by hand."""
    from million_amd.pq_cache import PagedPQCache
    cache = PagedPQCache(**LM.cache_kwargs(geom), device="cpu")
    cache.key_cent = cache.value_cent = torch.zeros(geom["M"], LM.C, geom["d"] // geom["M"], dtype=torch.float16)
    cache._kprep = cache._vprep = torch.zeros(1, dtype=torch.float16)
    cache._ws = torch.zeros(1, dtype=torch.uint8)
    return cache


def run_on_cpu(cache, calls, geom, check=True):
    """Drives the cache through a script (rows of zeros: nothing reads them), the model beside it; the checks after every call."""
    m = LM.Model(geom)
    nl, bs, nh, nhk, d = geom["layer_num"], geom["bs"], geom["nh"], geom["num_key_value_heads"], geom["d"]
    z = lambda *s: torch.zeros(*s, dtype=torch.float16)
    tables0 = cache._page_ids_all.numpy().copy()
    for i, call in enumerate(calls):
        op, what = call["op"], f"call {i} ({LM.describe(call)})"
        if op == "decode":
            for _ in range(call["steps"]):
                for l in range(nl):
                    cache.decoding_with_pages(z(bs, nh, 1, d), z(bs, nhk, 1, d), z(bs, nhk, 1, d), l, use_dev_lengths=True)
                m.step()
        else:
            if op == "release":
                do = lambda l: cache.release(call["b"])
            elif op == "fork":
                do = lambda l: cache.fork(call["src"], call["dst"], n_tokens=call["n_tokens"])
            elif op in ("prefill_request", "extend_request"):
                do = lambda l: getattr(cache, op)(call["b"], z(1, nh, call["n"], d), z(1, nhk, call["n"], d), z(1, nhk, call["n"], d), l)
            else:
                n = max(call["n_new"])
                do = lambda l: getattr(cache, op)(z(bs, nh, n, d), z(bs, nhk, n, d), z(bs, nhk, n, d), l, call["n_new"],
                                                  device_store=call["device_store"])
            for l in range(1 if op in ("release", "fork") else nl):      # (one call serves every layer)
                if call.get("raises"):
                    before = LM.snapshot(cache)
                    with pytest.raises(RuntimeError):
                        do(l)
                    after = LM.snapshot(cache)
                    assert all(np.array_equal(before[k], after[k]) if isinstance(before[k], np.ndarray) else before[k] == after[k]
                               for k in before), f"{what}: a refused call moved something"
                else:
                    do(l)
            m.apply(call)
        if check:
            snap = LM.snapshot(cache)
            LM.check_lengths(m, snap, what)
            if geom["preallocate"]:
                LM.check_allocator_preallocated(snap, tables0, what)
            else:
                LM.check_allocator_on_demand(m, snap, what)
    LM.check_end(cache, m, geom, tables0)


HOST_CASES = [(n, s) for n, s in CASES if not LM.GEOMS[n]["begin_step"]]


@pytest.mark.parametrize("name,seed", HOST_CASES, ids=[f"{n}-{s}" for n, s in HOST_CASES])
def test_script_on_a_cpu_cache(monkeypatch, name, seed):
    geom = LM.GEOMS[name]
    assert not geom["begin_step"]
    _stand_ins(monkeypatch)
    run_on_cpu(_cpu_cache(geom), LM.script(seed, geom, rows=False), geom)
