"""GPU tests of million_prefill_attn_lse (ops.prefill_attn(return_lse=True)): prompt attention that returns every row's
log-sum-exp.  `out` of an LSE call is compared bit for bit with the call without it, in all three kernels (pipelined and plain
at d = 128, plain at d = 64) and in both forms (lockstep, dev_spans); lse is compared with fp64 within lse_ref.LSE_TOL, on
gaussian inputs and on the flash_inputs families that make the pipelined kernel's lazy reference move; rows and requests
without a key give out 0 and lse -inf; and the intended use - a key range split in two, merged by attn_merge - meets the
attention bar against the whole call."""
import functools

import numpy as np
import pytest

from tests import chunk_blocks_model as B
from tests import flash_inputs as F
from tests.lse_ref import LSE_TOL

pytestmark = pytest.mark.gpu

BS, NH_K = 2, 2
FORMS = [(128, 0), (128, 64), (64, 0)]      # (d, million_set_force_generic value): pipelined, plain, plain
FORM_IDS = ["d128-pipelined", "d128-plain", "d64-plain"]
# (n_q, n_kv, q_pos0, causal)
CASES = [(70, 200, 130, True), (70, 200, 0, False), (33, 64, 31, True), (1, 65, 64, True)]
CASE_IDS = ["70x200-causal-at-130", "70x200-noncausal", "33x64-causal-at-31", "1x65-causal-at-64"]
PEAKED = ["stair9", "descending", "sink_local", "gauss8"]      # the reference climbs by steps, is set by key 0, climbs at the end, spreads


@pytest.fixture(scope="module")
def env():
    import torch
    assert torch.cuda.is_available(), "GPU tests need an MI355X"
    from million_amd import ops, _lib
    _lib.load()
    return torch, ops


@functools.lru_cache(maxsize=None)
def _case(name, G, d, n_q, n_kv, q_pos0, causal, bs=BS):
    """(q, k, v, fp64 out, fp64 lse) of a case: computed once, shared, never written."""
    q, k, v = F.prefill_inputs(name, bs, G * NH_K, NH_K, n_q, n_kv, d)
    out, lse = B.prefill_ref(q, k, v, q_pos0, causal)
    for a in (q, k, v, out, lse):
        a.setflags(write=False)
    return q, k, v, out, lse


def _cu(torch, a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def _bits(a):
    a = np.ascontiguousarray(a)
    return a.view(np.uint16 if a.dtype == np.float16 else np.uint32)


def _run(env, q, k, v, causal, policy, q_pos0=0, spans=None, want_lse=True):
    """One call under `policy`; out and lse hold NaN before it.  -> (out fp16, lse fp32 or None) as numpy."""
    torch, ops = env
    out = torch.full(q.shape, float("nan"), dtype=torch.float16, device="cuda")
    lse = torch.full(q.shape[:3], float("nan"), dtype=torch.float32, device="cuda") if want_lse else None
    try:
        ops.set_force_generic(policy)
        res = ops.prefill_attn(_cu(torch, q), _cu(torch, k), _cu(torch, v), causal=causal, q_pos0=q_pos0, out=out, lse=lse,
                               dev_spans=None if spans is None else _cu(torch, np.asarray(spans, np.int32)))
        torch.cuda.synchronize()
    finally:
        ops.set_force_generic(0)
    if want_lse:
        assert isinstance(res, tuple) and res[0] is out and res[1] is lse
    else:
        assert res is out
    return out.cpu().numpy(), None if lse is None else lse.cpu().numpy()


def _check(out, lse, gold_out, gold_lse, what, unit=1.0):
    """The attention bar on out (whole tensor, mean-abs in units of V's scale) and LSE_TOL on lse."""
    B.check_bar(out, gold_out, what, mae_tol=F.MEAN_ABS_TOL * unit)
    B.check_lse(lse, gold_lse, what, LSE_TOL)


@pytest.mark.parametrize("case", CASES, ids=CASE_IDS)
@pytest.mark.parametrize("d,policy", FORMS, ids=FORM_IDS)
def test_lse_against_fp64_and_out_bitwise(d, policy, case, env):
    n_q, n_kv, q_pos0, causal = case
    q, k, v, gold_out, gold_lse = _case("gauss1", 4, d, *case)
    out, lse = _run(env, q, k, v, causal, policy, q_pos0)
    plain, _ = _run(env, q, k, v, causal, policy, q_pos0, want_lse=False)
    assert np.array_equal(_bits(out), _bits(plain)), "out of the LSE call is not bitwise the call without it"
    _check(out, lse, gold_out, gold_lse, f"{d}/{policy} {case}")


@pytest.mark.parametrize("G", [1, 8])
def test_group_sizes(G, env):
    case = CASES[0]
    for d, policy in FORMS:
        q, k, v, gold_out, gold_lse = _case("gauss1", G, d, *case)
        out, lse = _run(env, q, k, v, case[3], policy, case[2])
        plain, _ = _run(env, q, k, v, case[3], policy, case[2], want_lse=False)
        assert np.array_equal(_bits(out), _bits(plain))
        _check(out, lse, gold_out, gold_lse, f"G{G} {d}/{policy}")


@pytest.mark.parametrize("name", PEAKED)
@pytest.mark.parametrize("d,policy", FORMS, ids=FORM_IDS)
def test_peaked_inputs_move_the_reference(d, policy, name, env):
    """The lse comes from the reference in force at the end, not from the row maximum: families whose maximum arrives late
    (stair9: 9 log2 units per 32 keys, past the 2^8 a probability may reach), first (descending, sink_local) or anywhere."""
    for case in (CASES[0], CASES[1]):
        q, k, v, gold_out, gold_lse = _case(name, 4, d, *case)
        out, lse = _run(env, q, k, v, case[3], policy, case[2])
        plain, _ = _run(env, q, k, v, case[3], policy, case[2], want_lse=False)
        assert np.array_equal(_bits(out), _bits(plain))
        _check(out, lse, gold_out, gold_lse, f"{name} {d}/{policy} {case}", unit=F.v_unit(name))


REQS = [(70, 200, 130), (0, 0, 0), (20, 0, 0), (5, 64, 59)]      # (n_q, n_kv, q_pos0) per request; bounds 70 x 200


@pytest.mark.parametrize("d,policy", FORMS, ids=FORM_IDS)
def test_ragged_rows(d, policy, env):
    """dev_spans: dead rows and key-less requests give out 0 and lse -inf; live rows are bitwise the batch-1 lockstep call;
    out is bitwise the ragged call without lse."""
    q, k, v, _, _ = _case("gauss1", 4, d, 70, 200, 0, True, bs=len(REQS))
    spans = [(a, b, c, 0) for a, b, c in REQS]
    out, lse = _run(env, q, k, v, True, policy, spans=spans)
    plain, _ = _run(env, q, k, v, True, policy, spans=spans, want_lse=False)
    assert np.array_equal(_bits(out), _bits(plain))
    for b, (n_q, n_kv, q_pos0) in enumerate(REQS):
        live = n_q if n_kv else 0
        assert not _bits(out[b, :, live:]).any(), f"request {b}: dead rows are not zeros"
        assert np.isneginf(lse[b, :, live:]).all(), f"request {b}: dead rows' lse is not -inf"
        if live:
            o1, l1 = _run(env, q[b:b + 1, :, :n_q], k[b:b + 1, :, :n_kv], v[b:b + 1, :, :n_kv], True, policy, q_pos0)
            assert np.array_equal(_bits(out[b:b + 1, :, :n_q]), _bits(o1)), f"request {b}: out"
            assert np.array_equal(_bits(lse[b:b + 1, :, :n_q]), _bits(l1)), f"request {b}: lse"
            go, gl = B.prefill_ref(q[b:b + 1, :, :n_q], k[b:b + 1, :, :n_kv], v[b:b + 1, :, :n_kv], q_pos0, True)
            _check(o1, l1, go, gl, f"ragged {d}/{policy} request {b}")


@pytest.mark.parametrize("d,policy", FORMS, ids=FORM_IDS)
def test_nan_past_the_lengths_changes_nothing(d, policy, env):
    q, k, v, _, _ = _case("gauss1", 4, d, 70, 200, 0, True, bs=len(REQS))
    spans = [(a, b, c, 0) for a, b, c in REQS]
    got = []
    for fill in (0.0, np.nan):
        qq, kk, vv = q.copy(), k.copy(), v.copy()
        for b, (n_q, n_kv, _) in enumerate(REQS):
            qq[b, :, n_q:] = fill
            kk[b, :, n_kv:] = fill
            vv[b, :, n_kv:] = fill
        got.append(_run(env, qq, kk, vv, True, policy, spans=spans))
    assert np.array_equal(_bits(got[0][0]), _bits(got[1][0])), "NaN past the requests' lengths changed out"
    assert np.array_equal(_bits(got[0][1]), _bits(got[1][1])), "NaN past the requests' lengths changed lse"
    assert np.isfinite(got[1][0]).all() and not np.isnan(got[1][1]).any()


@pytest.mark.parametrize("d,policy", FORMS, ids=FORM_IDS)
def test_split_keys_merge_to_the_whole_call(d, policy, env):
    """The intended use: keys [0, 96) non-causally, keys [96, 200) causally with q_pos0 - 96, one attn_merge."""
    torch, ops = env
    n_q, n_kv, q_pos0, a = 70, 200, 130, 96
    q, k, v, gold_out, gold_lse = _case("gauss1", 4, d, n_q, n_kv, q_pos0, True)
    whole_o, whole_l = _run(env, q, k, v, True, policy, q_pos0)
    o1, l1 = _run(env, q, k[:, :, :a], v[:, :, :a], False, policy)
    o2, l2 = _run(env, q, k[:, :, a:], v[:, :, a:], True, policy, q_pos0 - a)
    mo, ml = ops.attn_merge([_cu(torch, o1), _cu(torch, o2)], [_cu(torch, l1), _cu(torch, l2)], return_lse=True)
    torch.cuda.synchronize()
    mo, ml = mo.cpu().numpy(), ml.cpu().numpy()
    B.check_bar(mo, whole_o.astype(np.float64), f"split/merged vs whole {d}/{policy}")
    B.check_lse(ml, whole_l, f"split/merged vs whole {d}/{policy}", LSE_TOL)
    _check(mo, ml, gold_out, gold_lse, f"split/merged vs fp64 {d}/{policy}")
