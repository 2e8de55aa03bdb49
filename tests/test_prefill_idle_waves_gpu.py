"""GPU tests of prompt attention (csrc/prefill.hip) in workgroups where only some of the eight waves hold query rows.  A wave
without rows computes nothing, but it issues its piece of every K / V request and joins every barrier, so it runs ahead of its
neighbours: a request that no barrier separates from another wave's read of the same LDS region overwrites what that wave is
still multiplying against.  The pipelined kernel had such a hole between the prologue's scores of K half 0 and the first
burst's K half 4, both in quarter 0 (profiles/prefill_prologue_race.txt; tests/test_prefill_schedule_host.py states the rule).

1. Volume: one launch with more than a thousand partly idle workgroups whose requests are all the SAME request - K, V and Q
   of request 0 expanded over the batch with stride 0 - so every request must return request 0's bits, and the rows of the
   partial query blocks must lie within the project's bar of fp64.  No luck is needed to notice a wrong row, only to produce one.
   (Measured: the kernel without the barrier passed these in 5 of 5 fresh processes - on the MI355X the strike is far rarer than one
   in a thousand such workgroups; the development switch of profiles/prefill_prologue_race.txt is the proof of the cause, the host
   test the guard of the schedule, these the guard against a strike in place.)
2. Sweep: every way a workgroup can be partly idle - heads per workgroup, rows in the last query block, key tiles of that
   workgroup on both sides of the fifth half, causal at two offsets and at the end of the keys, every key - per row against fp64,
   lockstep and ragged, bit for bit over two calls and between the ragged and the lockstep instance.

Inputs are the sink_local family: the fp32 models of both loops stay at or below half the bar on it
(tests/test_prefill_ragged_host.py), and keys 0 .. 31 hold the sink, so a corrupted first half cannot hide."""
import functools

import numpy as np
import pytest

from tests import flash_inputs as F
from tests import prefill_ragged_cases as R

pytestmark = pytest.mark.gpu

NAME = R.BASE      # sink_local


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


def _launch(env, q, k, v, causal, q_pos0, policy, rows=None):
    """One call on device tensors (views are passed as they are) under `policy` (0: pipelined at d = 128; 64: the plain tile
    loop); rows: the (bs, 4) int32 rows of a ragged call.  -> the device tensor `out`, NaN before the call."""
    torch, ops = env
    out = torch.full(tuple(q.shape), float("nan"), dtype=torch.float16, device="cuda")
    try:
        ops.set_force_generic(policy)
        ops.prefill_attn(q, k, v, causal=causal, q_pos0=q_pos0, out=out, dev_spans=None if rows is None else _cu(torch, rows))
        torch.cuda.synchronize()
    finally:
        ops.set_force_generic(0)
    return out


# ---------------------------------------------------------------- 1. volume -------------------------------------------------
# name -> (causal, n_q, n_kv, nh, nh_k, bs, requests of the ragged variants by name)
#   mixed: the recorded shape (n = 257, G = 2: query blocks of 128 rows) scaled out - per request 8 workgroups hold row 256 of two
#     heads (2 live waves of 8, 5 key tiles) and are dispatched among 16 full ones: 128 requests x 8 = 1024 of them.  The
#     alternating variant gives every other request 129 rows behind 128 cached keys: its block 1 holds the one row at position 256.
#   homogeneous: one query row over 320 keys, no mask, G = 1: each of the 64 x 32 = 2048 workgroups has 1 live wave and 7 idle
#     ones and walks all 5 tiles.
VOLUME = {
    "mixed": (True, 257, 257, 16, 8, 128, {"dev_spans": [(257, 257, 0)], "dev_spans-alternating": [(257, 257, 0), (129, 257, 128)]}),
    "homogeneous": (False, 1, 320, 32, 32, 64, {"dev_spans": [(1, 320, 0)]}),
}
VOLUME_CASES = [(form, spans) for form, c in VOLUME.items() for spans in ["lockstep"] + list(c[6])]


def _partial_rows(n_q, G):
    """The query rows of the last, partly filled query block (256 / hpw rows per head and workgroup)."""
    hpw = max(c for c in (8, 4, 2, 1) if G % c == 0)
    QB = 256 // hpw
    return list(range((n_q - 1) // QB * QB, n_q))


@functools.lru_cache(maxsize=None)
def _volume_data(form, d):
    """fp16 inputs of the one request and, per distinct request (n_q, n_kv, q_pos0), (its partial-block rows, their fp64 output)."""
    causal, n_q, n_kv, nh, nh_k, _, variants = VOLUME[form]
    q, k, v = F.prefill_inputs(NAME, 1, nh, nh_k, n_q, n_kv, d)
    gold = {}
    for req in {r for reqs in variants.values() for r in reqs}:
        rows = _partial_rows(req[0], nh // nh_k)
        gold[req] = (rows, F.prefill_gold(q[:, :, :req[0]], k[:, :, :req[1]], v[:, :, :req[1]], req[2], causal, rows=rows))
    return q, k, v, gold


@pytest.mark.parametrize("form,spans", VOLUME_CASES, ids=[f"{f}-{s}" for f, s in VOLUME_CASES])
@pytest.mark.parametrize("d,policy", R.FORMS, ids=R.FORM_IDS)
def test_identical_requests_return_identical_bits(d, policy, form, spans, env):
    """Every request of the launch is request 0 (or, alternating, request 0 or 1): same bits out, and the rows of the partly
    idle workgroups within the bar of fp64.  The plain loop and d = 64 do not have the pipelined form's schedule: they show the
    oracle sound on a kernel without the hazard."""
    torch, _ = env
    causal, n_q, n_kv, nh, nh_k, bs, variants = VOLUME[form]
    q1, k1, v1, gold = _volume_data(form, d)
    q, k, v = (_cu(torch, a).expand(bs, -1, -1, -1) for a in (q1, k1, v1))
    assert q.stride(0) == 0 and k.stride(0) == 0 and v.stride(0) == 0
    reqs = [(n_q, n_kv, 0)] if spans == "lockstep" else variants[spans]
    rows = None if spans == "lockstep" else R.spans([reqs[b % len(reqs)] for b in range(bs)])
    out = _launch(env, q, k, v, causal, 0, policy, rows)
    what = f"volume {form} {R.FORM_NAME[d, policy]} {spans}"
    for j, req in enumerate(reqs):      # requests j, j + len(reqs), ... are the same request
        mine = out[j::len(reqs)]
        differ = (mine.view(torch.int16) != mine[:1].view(torch.int16)).any(dim=-1)      # (requests, nh, n_q)
        n_rows = int(differ.sum().item())
        where = [tuple(int(x) for x in i) for i in differ.nonzero()[:4].cpu()]
        first = mine[0].cpu().numpy()[None]
        prows, g = gold[req]
        F.check_rows(first[:, :, prows], g, f"{what} request {j} {req}", rows=prows, tag="IDLEWAVES")
        assert not _bits(first[:, :, req[0]:]).any(), f"{what}: rows past n_q are not zeros"
        assert np.isfinite(first[:, :, :req[0]]).all(), f"{what}: non-finite output"
        assert n_rows == 0, (f"{what}: {n_rows} rows in {int(differ.any(dim=2).any(dim=1).sum().item())} of {mine.shape[0]} requests equal to "
                             f"request {j} differ from it, first (request, head, row): {where}")


# ---------------------------------------------------------------- 2. sweep --------------------------------------------------
NH_K = 2
SWEEP_G = [1, 3, 2, 4, 12]                       # hpw 1, 1, 2, 4, 4: query blocks of 256, 256, 128, 64, 64 rows
EXTRA_ROWS = [1, 31, 32, 33]                     # rows in the last query block: one lane, a wave less one row, a wave, a wave and a lane
N_KV = [127, 129, 256, 290]                      # 2, 3, 4, 5 key tiles: four halves; a fifth half of one key; whole tiles; a tenth half of two keys
MODES = ["causal-at-0", "causal-at-130", "causal-at-end", "noncausal"]


def _mode(mode, n_q, n_kv):
    """-> (causal, q_pos0).  causal-at-end: the rows are the last n_q positions of the keys, so the last workgroup walks every
    tile (at 0 and at 130 the diagonal ends its walk earlier)."""
    if mode == "noncausal":
        return False, 0
    return True, {"causal-at-0": 0, "causal-at-130": 130, "causal-at-end": max(0, n_kv - n_q)}[mode]


def _tiles_of_last_block(G, n_q, n_kv, causal, q_pos0):
    """prefill_rows restated: key tiles of the workgroup that holds the last query row."""
    end = min(q_pos0 + n_q, n_kv) if causal else n_kv
    return -(-end // 64)


@functools.lru_cache(maxsize=None)
def _sweep_inputs(G, n_q_max, n_kv, d):
    q, k, v = F.prefill_inputs(NAME, 1, G * NH_K, NH_K, n_q_max, n_kv, d)
    for a in (q, k, v):
        a.setflags(write=False)
    return q, k, v


@functools.lru_cache(maxsize=None)
def _sweep_gold(G, n_q_max, n_kv, d, causal, q_pos0, n_rows):
    """fp64 over the first n_rows query rows at q_pos0: a call with fewer rows at the same offset returns the first of them, so
    the modes with one offset share the reference over n_q_max rows."""
    return F.prefill_gold(*_sweep_inputs(G, n_q_max, n_kv, d), q_pos0, causal, rows=np.arange(n_rows))


def _sweep(env, G, mode, d, policy):
    torch, _ = env
    hpw = max(c for c in (8, 4, 2, 1) if G % c == 0)
    QB = 256 // hpw
    counts = [kb * QB + e for kb in (0, 1) for e in EXTRA_ROWS]
    n_q_max = max(counts)
    reached = set()
    for n_kv in N_KV:
        q1, k1, v1 = _sweep_inputs(G, n_q_max, n_kv, d)
        q, k, v = (_cu(torch, a) for a in (q1, k1, v1))
        reqs = []
        for n_q in counts:
            causal, q_pos0 = _mode(mode, n_q, n_kv)
            reqs.append((n_q, n_kv, q_pos0))
            reached.add(_tiles_of_last_block(G, n_q, n_kv, causal, q_pos0))
        # the eight row counts as eight requests of one ragged launch (the same Q, K, V for each), twice
        bs = len(reqs)
        rag = [_launch(env, *(a.expand(bs, -1, -1, -1) for a in (q, k, v)), causal, 5, policy, R.spans(reqs)).cpu().numpy() for _ in range(2)]
        assert np.array_equal(_bits(rag[0]), _bits(rag[1])), f"ragged n_kv {n_kv}: two calls differ"
        for b, (n_q, _, q_pos0) in enumerate(reqs):
            what = f"sweep {R.FORM_NAME[d, policy]} G{G} {mode} n_q {n_q} n_kv {n_kv} at {q_pos0}"
            lock = [_launch(env, q[:, :, :n_q], k, v, causal, q_pos0, policy).cpu().numpy() for _ in range(2)]
            assert np.array_equal(_bits(lock[0]), _bits(lock[1])), f"{what}: two lockstep calls differ"
            gold = _sweep_gold(G, n_q_max, n_kv, d, causal, q_pos0, n_q if mode == "causal-at-end" else n_q_max)
            F.check_rows(lock[0], gold[:, :, :n_q], what, tag="IDLEWAVES")
            assert np.array_equal(_bits(rag[0][b:b + 1, :, :n_q]), _bits(lock[0])), f"{what}: the ragged instance differs from the lockstep one"
            assert not _bits(rag[0][b, :, n_q:]).any(), f"{what}: rows past n_q are not zeros"
    return reached


@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("G", SWEEP_G)
@pytest.mark.parametrize("d,policy", R.FORMS, ids=R.FORM_IDS)
def test_partly_idle_workgroups_against_fp64(d, policy, G, mode, env):
    """n_q = k QB + {1, 31, 32, 33}, k in {0, 1}: the last query block holds one to two waves' rows per head, the other waves
    of its workgroup are idle.  The key counts give that workgroup 2 .. 5 tiles wherever the mask lets it walk them all - both
    sides of the fifth half (the first request of the loop's first burst) and both parities of the loop's unroll."""
    reached = _sweep(env, G, mode, d, policy)
    hi = {"causal-at-0": {1: 5, 3: 5, 2: 3, 4: 2, 12: 2}, "causal-at-130": {4: 4, 12: 4}}.get(mode, {}).get(G, 5)
    # at offsets 0 and 130 the diagonal of the last row ends the walk after (q_pos0 + n_q) / 64 tiles: blocks of 64 and 128 rows stop short of 5
    assert reached == set(range(1 if mode == "causal-at-0" else 2, hi + 1))


@pytest.mark.parametrize("d,policy", R.FORMS, ids=R.FORM_IDS)
def test_control_eight_heads_per_workgroup_has_no_idle_wave(d, policy, env):
    """The control: at G = 8 (hpw = 8) each wave of a workgroup serves another head over the SAME 32 rows, all eight share
    q_lo, so a workgroup with rows has no idle wave: the same sweep on the one grouping that cannot be partly idle."""
    assert _sweep(env, 8, "noncausal", d, policy) == {2, 3, 4, 5}
