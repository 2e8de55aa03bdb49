"""GPU tests of ragged prompt attention: million_prefill_desc.dev_spans (the RAGGED instances of csrc/prefill.hip),
ops.prefill_attn(dev_spans=...) and PagedPQCache.prefill_ragged.  The bar is the project's - rel-L2 < 1e-3 per output row against
fp64 (flash_inputs.check_rows) - and everything the contract calls equal is compared bit for bit: a ragged launch against the
lockstep launch with the same values, a request's live rows against the batch-1 lockstep call, data surrounded by NaN against
data surrounded by zeros, a replayed capture against the eager call.  tests/test_prefill_ragged_host.py shows on the CPU that
the inputs leave a correct kernel half the bar of room."""
import numpy as np
import pytest

from tests import flash_inputs as F
from tests import prefill_ragged_cases as R
from tests.test_chunk_attn_gpu import _check, _decode_gold, _paged_cache
from tests.test_flash_numerics_gpu import _embed, _out_buffer, _sentinels_untouched

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def env():
    import torch
    assert torch.cuda.is_available(), "GPU tests need an MI355X"
    from million_amd import ops, _lib
    _lib.load()
    return torch, ops


def _cu(torch, a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def _bits(a):
    return np.ascontiguousarray(a).view(np.uint16)


def _run(env, q, k, v, causal, policy, rows=None, q_pos0=0):
    """One call under `policy` (0: pipelined at d = 128; 64: the plain tile loop); rows: the (bs, 4) device rows, or None for the
    lockstep call.  -> fp16 numpy (bs, nh, n_q, d); `out` holds NaN before the call."""
    torch, ops = env
    out = torch.full(q.shape, float("nan"), dtype=torch.float16, device="cuda")
    try:
        ops.set_force_generic(policy)
        ops.prefill_attn(_cu(torch, q), _cu(torch, k), _cu(torch, v), causal=causal, q_pos0=q_pos0, out=out,
                         dev_spans=None if rows is None else _cu(torch, rows))
        torch.cuda.synchronize()
    finally:
        ops.set_force_generic(0)
    return out.cpu().numpy()


# ---------------------------------------------------------------- 1. equal rows: the lockstep call, bit for bit --------------
@pytest.mark.parametrize("mode", ["causal", "noncausal", "causal-at-80"])
@pytest.mark.parametrize("G,bound", R.GROUPS, ids=R.GROUP_IDS)
@pytest.mark.parametrize("d,policy", R.FORMS, ids=R.FORM_IDS)
def test_equal_rows_are_the_lockstep_call(d, policy, G, bound, mode, env):
    """Every request's row equal to the host values: the ragged instance's output is the lockstep instance's."""
    n_q, n_kv, q_pos0, causal = {"causal": (bound, bound, 0, True), "noncausal": (bound - 23, bound, 0, False),
                                 "causal-at-80": (bound - 80, bound, 80, True)}[mode]
    q, k, v = R.inputs(R.BASE, 3, G, bound, d)
    q = q[:, :, :n_q]
    lock = _run(env, q, k, v, causal, policy, q_pos0=q_pos0)
    rag = _run(env, q, k, v, causal, policy, rows=R.spans([(n_q, n_kv, q_pos0)] * 3, word3=0x7EADBEEF), q_pos0=5)
    assert np.isfinite(lock).all()
    assert np.array_equal(_bits(lock), _bits(rag))


# ---------------------------------------------------------------- 2. ragged batches against fp64 ----------------------------
@pytest.mark.parametrize("batch", ["edges", "offsets", "noncausal"])
@pytest.mark.parametrize("G,bound", R.GROUPS, ids=R.GROUP_IDS)
@pytest.mark.parametrize("name", R.FAMILIES)
def test_ragged_rows_against_fp64(name, G, bound, batch, env):
    """Each request's live rows within the bar of its own fp64 attention; rows past n_q_b and requests without keys exact zeros."""
    causal, reqs = R.requests(batch, bound)
    for d, policies in ((128, (0, 64)), (64, (0,))):
        q, k, v = R.inputs(name, len(reqs), G, bound, d)
        gold = R.gold(name, batch, G, bound, d)
        for pol in policies:
            out = _run(env, q, k, v, causal, pol, rows=R.spans(reqs))
            assert np.isfinite(out).all(), "non-finite output"
            for b, (n_q, n_kv, _) in enumerate(reqs):
                what = f"ragged {R.FORM_NAME[d, pol]} {name} {batch} G{G} request {b} {reqs[b]}"
                if R.live(reqs[b]):
                    F.check_rows(out[b:b + 1, :, :n_q], gold[b], what, unit=F.v_unit(name))
                    assert not _bits(out[b, :, n_q:]).any(), f"{what}: rows past n_q are not zeros"
                else:
                    assert not _bits(out[b]).any(), f"{what}: a request without rows or keys is not zeros"


# ---------------------------------------------------------------- 3. a request alone, bit for bit ----------------------------
@pytest.mark.parametrize("batch", ["edges", "offsets", "noncausal"])
@pytest.mark.parametrize("G,bound", R.GROUPS, ids=R.GROUP_IDS)
@pytest.mark.parametrize("d,policy", R.FORMS, ids=R.FORM_IDS)
def test_live_rows_are_the_batch_1_lockstep_call(d, policy, G, bound, batch, env):
    causal, reqs = R.requests(batch, bound)
    q, k, v = R.inputs(R.BASE, len(reqs), G, bound, d)
    out = _run(env, q, k, v, causal, policy, rows=R.spans(reqs))
    for b, req in enumerate(reqs):
        if not R.live(req):
            continue
        alone = _run(env, *R.request_inputs(q, k, v, b, req), causal, policy, q_pos0=req[2])
        assert np.array_equal(_bits(out[b:b + 1, :, :req[0]]), _bits(alone)), f"request {b} {req}"


# ---------------------------------------------------------------- 4. poisoned surroundings -----------------------------------
@pytest.mark.parametrize("G,bound", R.GROUPS, ids=R.GROUP_IDS)
@pytest.mark.parametrize("d,policy", R.FORMS, ids=R.FORM_IDS)
def test_nothing_past_a_requests_lengths_is_read(d, policy, G, bound, env):
    """The same live data twice: zeros, then NaN, in the q rows at or past n_q_b, the K / V rows at or past n_kv_b, the gaps
    behind every row and whole pad tiles before and after the tensors; `out` full of NaN inside a sentinel-filled allocation.
    The outputs are equal bit for bit, match fp64, and no sentinel outside out has moved."""
    torch, ops = env
    causal, reqs = R.requests("poison", bound)
    q, k, v = R.inputs(R.BASE, len(reqs), G, bound, d)
    gold = R.gold(R.BASE, "poison", G, bound, d)
    got = []
    try:
        ops.set_force_generic(policy)
        for fill in (0.0, float("nan")):
            qq, kk, vv = (a.copy() for a in (q, k, v))
            for b, (n_q, n_kv, _) in enumerate(reqs):
                qq[b, :, n_q:] = fill
                kk[b, :, n_kv:] = fill
                vv[b, :, n_kv:] = fill
            views = [_embed(torch, _cu(torch, a), fill)[1] for a in (qq, kk, vv)]
            obuf, out = _out_buffer(torch, q.shape)
            out.fill_(float("nan"))
            ops.prefill_attn(*views, causal=causal, out=out, dev_spans=_cu(torch, R.spans(reqs)))
            torch.cuda.synchronize()
            assert _sentinels_untouched(torch, obuf, q.shape), "a sentinel outside out moved"
            got.append(out.contiguous().cpu().numpy())
    finally:
        ops.set_force_generic(0)
    assert np.array_equal(_bits(got[0]), _bits(got[1])), "NaN past the requests' lengths changed the output"
    for b, req in enumerate(reqs):
        if R.live(req):
            F.check_rows(got[1][b:b + 1, :, :req[0]], gold[b], f"ragged poisoned {R.FORM_NAME[d, policy]} G{G} request {b} {req}")
            assert not _bits(got[1][b, :, req[0]:]).any()
        else:
            assert not _bits(got[1][b]).any()


# ---------------------------------------------------------------- 5. untrusted rows ------------------------------------------
@pytest.mark.parametrize("G,bound", [(4, 200), (1, 300)], ids=["G4-bound200", "G1-bound300"])
@pytest.mark.parametrize("d,policy", R.FORMS, ids=R.FORM_IDS)
def test_untrusted_rows_are_clamped(d, policy, G, bound, env):
    """n_q_b into [0, n_q], n_kv_b and q_pos0_b into [0, n_kv]; word 3 is not read, the array is not written."""
    torch, ops = env
    big = 2 ** 31 - 1
    wild = [(bound + 300, 5 * bound, -7), (-3, 50, 0), (100, -1, 5), (150, 150, 900), (big, big, big), (70, 90, -big - 1)]
    tame = [(bound, bound, 0), (0, 50, 0), (100, 0, 5), (150, 150, bound), (bound, bound, bound), (70, 90, 0)]
    q, k, v = R.inputs(R.BASE, len(wild), G, bound, d)
    rows = _cu(torch, R.spans(wild, word3=0x7EADBEEF))
    keep = rows.clone()
    out = torch.full(q.shape, float("nan"), dtype=torch.float16, device="cuda")
    try:
        ops.set_force_generic(policy)
        ops.prefill_attn(_cu(torch, q), _cu(torch, k), _cu(torch, v), out=out, dev_spans=rows)
        torch.cuda.synchronize()
    finally:
        ops.set_force_generic(0)
    assert torch.equal(rows, keep), "the device rows were written"
    want = _run(env, q, k, v, True, policy, rows=R.spans(tame))
    assert np.isfinite(want).all()
    assert np.array_equal(_bits(out.cpu().numpy()), _bits(want))


# ---------------------------------------------------------------- 6. one captured launch, moving rows ------------------------
@pytest.mark.parametrize("d,policy", R.FORMS, ids=R.FORM_IDS)
def test_graph_replay_follows_the_rows(d, policy, env):
    """One launch captured on a single stream (no parallel branch); the device rows are rewritten between replays."""
    torch, ops = env
    G, bound = 4, 200
    states = [R.requests(b, bound)[1][:4] for b in ("edges", "offsets")] + [[(0, 0, 0), (200, 200, 0), (1, 200, 199), (130, 64, 0)]]
    q, k, v = R.inputs(R.BASE, 4, G, bound, d)
    tq, tk, tv = (_cu(torch, a) for a in (q, k, v))
    rows = _cu(torch, R.spans(states[0]))
    out = torch.zeros(q.shape, dtype=torch.float16, device="cuda")
    try:
        ops.set_force_generic(policy)
        ops.prefill_attn(tq, tk, tv, out=out, dev_spans=rows)      # eager once: module load, kernel attributes
        torch.cuda.synchronize()
        g = torch.cuda.CUDAGraph()
        with torch.cuda.graph(g):
            ops.prefill_attn(tq, tk, tv, out=out, dev_spans=rows)
    finally:
        ops.set_force_generic(0)
    for st in states[1:] + states[:1]:
        rows.copy_(_cu(torch, R.spans(st)))
        out.fill_(float("nan"))
        g.replay()
        torch.cuda.synchronize()
        assert np.array_equal(_bits(out.cpu().numpy()), _bits(_run(env, q, k, v, True, policy, rows=R.spans(st)))), st


# ---------------------------------------------------------------- 7. PagedPQCache.prefill_ragged -----------------------------
def test_prefill_ragged_matches_prefill_request(env, oracle):
    """bs = 4, prompts of 130 / - / 64 / 5 tokens into the empty slots 0, 2, 3 while slot 1 is mid-sequence (codes and window
    rows): the slots are left as prefill_request leaves them, slot 1 is not touched, and a decode step over the batch follows."""
    torch, ops = env
    bs, nhk, d, ps, cap, G = 4, 2, 128, 32, 64, 4
    cu = lambda a: _cu(torch, a)
    rs_ = np.random.RandomState(23)
    n_new, n = [130, 0, 64, 5], 130
    K = rs_.standard_normal((bs, nhk, n + 1, d)).astype(np.float16)      # the prompts' rows and one decode row behind them
    V = rs_.standard_normal((bs, nhk, n + 1, d)).astype(np.float16)
    Q = rs_.standard_normal((bs, G * nhk, n, d)).astype(np.float16)
    K1 = rs_.standard_normal((1, nhk, 47, d)).astype(np.float16)         # slot 1: a prompt of 40, 6 decode steps, this test's step
    V1 = rs_.standard_normal((1, nhk, 47, d)).astype(np.float16)
    q1 = rs_.standard_normal((bs, G * nhk, 1, d)).astype(np.float16)
    caches, outs, decs = [], [], []
    for ragged in (True, False):
        cache, kc, vc = _paged_cache(torch, np.random.RandomState(3), bs, nhk, d, 64, ps, cap)
        cache.prefill_request(1, cu(np.zeros((1, G * nhk, 40, d), np.float16)), cu(K1[:, :, :40]), cu(V1[:, :, :40]), 0)
        for i in range(6):      # decode steps of the whole batch put window rows into slot 1; the other slots are then released
            k1, v1 = np.repeat(K1[:, :, 40 + i:41 + i], bs, axis=0), np.repeat(V1[:, :, 40 + i:41 + i], bs, axis=0)
            cache.decoding_with_pages(cu(q1), cu(k1), cu(v1), 0, use_dev_lengths=True)
        for b in (0, 2, 3):
            cache.release(b)
        assert (cache._T_a[0, 1], cache._r_a[0, 1]) == (40, 6) and not cache._T_a[0, [0, 2, 3]].any()
        before = (cache.lengths[0][1].clone(), cache.page_ids[0][1].clone(), cache.key_residual_cache[0][1].clone(),
                  cache.value_residual_cache[0][1].clone(), [a[0, 1] for a in cache.host_state()])
        pages1 = [p.clone() for p in (cache.key_page_pool[cache.page_ids[0][1].long()], cache.value_page_pool[cache.page_ids[0][1].long()])]
        if ragged:
            # rows past a slot's n_new - q, K and V - hold NaN
            Qp, Kp, Vp = Q.copy(), K[:, :, :n].copy(), V[:, :, :n].copy()
            for b in range(bs):
                Qp[b, :, n_new[b]:] = Kp[b, :, n_new[b]:] = Vp[b, :, n_new[b]:] = np.nan
            with pytest.raises(RuntimeError, match="extend_ragged"):
                cache.prefill_ragged(cu(Qp), cu(Kp), cu(Vp), 0, [130, 3, 64, 5])      # slot 1 holds tokens
            with pytest.raises(RuntimeError):
                cache.prefill_ragged(cu(Qp[:3]), cu(Kp[:3]), cu(Vp[:3]), 0, n_new[:3])   # wrong batch size
            with pytest.raises(RuntimeError):
                cache.prefill_ragged(cu(Qp), cu(Kp), cu(Vp), 0, [131, 0, 64, 5])      # more rows than the tensors hold
            with pytest.raises(RuntimeError):
                cache.prefill_ragged(cu(Qp), cu(Kp), cu(Vp), 0, [130, 0, -1, 5])
            assert not cache._T_a[0, [0, 2, 3]].any()                                 # nothing happened
            out = cache.prefill_ragged(cu(Qp), cu(Kp), cu(Vp), 0, n_new).cpu().numpy()
        else:
            out = np.zeros((bs, G * nhk, n, d), np.float16)
            for b in (0, 2, 3):
                x = n_new[b]
                out[b, :, :x] = cache.prefill_request(b, cu(Q[b:b + 1, :, :x]), cu(K[b:b + 1, :, :x]), cu(V[b:b + 1, :, :x]), 0).cpu().numpy()
        torch.cuda.synchronize()
        # slot 1: device row, page ids, page contents, window and host lengths untouched
        assert torch.equal(cache.lengths[0][1], before[0]) and torch.equal(cache.page_ids[0][1], before[1])
        assert torch.equal(cache.key_residual_cache[0][1].view(torch.int16), before[2].view(torch.int16))
        assert torch.equal(cache.value_residual_cache[0][1].view(torch.int16), before[3].view(torch.int16))
        assert [a[0, 1] for a in cache.host_state()] == before[4]
        assert torch.equal(cache.key_page_pool[cache.page_ids[0][1].long()], pages1[0])
        assert torch.equal(cache.value_page_pool[cache.page_ids[0][1].long()], pages1[1])
        assert cache.lengths[0].tolist() == [[130, 0, 0, 0], [40, 6, 0, 0], [64, 0, 0, 0], [5, 0, 0, 0]]
        caches.append(cache)
        outs.append(out)
        # one decode step over the batch, each slot against the oracle
        kd = np.concatenate([K[:1, :, 130:131], K1[:, :, 46:47], K[2:3, :, 64:65], K[3:4, :, 5:6]])
        vd = np.concatenate([V[:1, :, 130:131], V1[:, :, 46:47], V[2:3, :, 64:65], V[3:4, :, 5:6]])
        dec = cache.decoding_with_pages(cu(q1), cu(kd), cu(vd), 0, use_dev_lengths=True).cpu().numpy()
        torch.cuda.synchronize()
        for b, (T, r) in enumerate([(130, 1), (40, 7), (64, 1), (5, 1)]):
            Kall, Vall = (K1, V1) if b == 1 else (K[b:b + 1], V[b:b + 1])
            _check(dec[b:b + 1], _decode_gold(oracle, q1[b:b + 1], Kall, Vall, kc, vc, T, r, cap), f"decode after prefill_ragged, slot {b}")
        decs.append(dec)
    a, b_ = caches
    assert all((x == y).all() for x, y in zip(a.host_state(), b_.host_state()))
    assert torch.equal(a.lengths[0], b_.lengths[0]) and torch.equal(a.page_ids[0], b_.page_ids[0])
    ids = a.page_ids[0].cpu().numpy()
    for pool in ("key_page_pool", "value_page_pool"):
        back = oracle.pool_to_k_rowmajor if pool == "key_page_pool" else oracle.pool_to_v_rowmajor
        ga, gb = back(getattr(a, pool).cpu().numpy(), ids, 130), back(getattr(b_, pool).cpu().numpy(), ids, 130)
        for s in (0, 2, 3):
            assert np.array_equal(ga[s, :, :n_new[s]], gb[s, :, :n_new[s]]), (pool, s)
    # the output rows: bit for bit those of prefill_request, zeros past n_new and in the slot that took no part
    assert np.array_equal(_bits(outs[0]), _bits(outs[1]))
    assert np.array_equal(_bits(decs[0]), _bits(decs[1]))
    for b in (0, 2, 3):
        F.check_rows(outs[0][b:b + 1, :, :n_new[b]], F.prefill_gold(Q[b:b + 1, :, :n_new[b]], K[b:b + 1, :, :n_new[b]], V[b:b + 1, :, :n_new[b]]),
                     f"prefill_ragged slot {b}")
