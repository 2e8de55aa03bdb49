"""CPU side of the flash-family numerics tests: the input families of tests/flash_inputs.py are well posed and are what they
claim to be, and the arithmetic of the d = 128 prompt-attention kernels, restated in numpy, meets the per-row bar on them.

Well posed is a condition, not a measurement: on every family and shape that test_flash_numerics_gpu.py runs, the fp64 result
rounded to fp16 (the best any kernel can do) and the plain kernel's arithmetic model are within 0.5 x REL_TOL on their worst
row, so a GPU kernel that misses REL_TOL on a row is wrong by at least as much again as its number formats explain.  The models
run on sampled heads of each shape (rows of different heads are independent draws of the same family).

The last test keeps the reason for the pipelined kernel's arithmetic in the suite: with the softmax scale folded into an fp16 Q
(the form it had) the score error grows with the score and the worst row crosses the bar from logit standard deviation 4 on."""
import numpy as np
import pytest

from tests import flash_inputs as F

CAP = 0.5 * F.REL_TOL

# (n_q, n_kv, q_pos0, causal): the shapes of test_flash_numerics_gpu.py
SHAPES = [(1024, 1024, 0, True), (333, 1500, 1167, True), (200, 777, 0, False)]
GQA = [(32, 8), (8, 8)]
# (d, M, C, G, n_q, T, r, cap, rstart, chunk): chunk-attention shapes of the GPU file: one code tile, many, d = 64 without the chunk
CHUNK_SHAPES = [(128, 64, 256, 4, 96, 64, 100, 128, 90, True), (128, 32, 256, 4, 96, 1000, 100, 128, 90, True),
                (64, 32, 128, 4, 96, 1000, 100, 128, 90, False)]


def _heads(nh):
    return [0, nh - 1] if nh > 1 else [0]


def _worst(out, gold):
    return float(F.row_err(out, gold).max())


@pytest.mark.parametrize("nh,nh_k", GQA, ids=["gqa32-8", "gqa8-8"])
@pytest.mark.parametrize("shape", SHAPES, ids=["1024sq", "333at1167", "200x777-noncausal"])
@pytest.mark.parametrize("name", list(F.FAMILIES))
def test_families_are_well_posed_for_prefill(name, shape, nh, nh_k):
    n_q, n_kv, q_pos0, causal = shape
    for d in (128, 64):
        q, k, v = F.prefill_inputs(name, 1, nh, nh_k, n_q, n_kv, d)
        hs = _heads(nh)
        gold = F.prefill_gold(q[:, hs], k[:, [h * nh_k // nh for h in hs]], v[:, [h * nh_k // nh for h in hs]], q_pos0, causal)[0]
        vis = F.visible(n_q, n_kv, q_pos0, causal)
        assert _worst(F.ideal(gold), gold) <= CAP, f"{name} d={d}: ideal worst row {_worst(F.ideal(gold), gold):.2e}"
        plain = F.model_heads(F.model_plain, q, k, v, vis, hs, F.prefill_tiles(n_kv))
        assert _worst(plain, gold) <= CAP, f"{name} d={d}: plain model worst row {_worst(plain, gold):.2e}"
        if d == 128:
            pipe = F.model_heads(F.model_pipelined, q, k, v, vis, hs)
            assert _worst(pipe, gold) < F.REL_TOL, f"{name}: pipelined model worst row {_worst(pipe, gold):.2e}"


CHUNK_CASES = [(n, s) for s in CHUNK_SHAPES for n in list(F.FAMILIES) + ["peak:" + p for p in F.PEAKS]
               if s[-1] or n != "peak:chunk_row"]


@pytest.mark.parametrize("name,shape", CHUNK_CASES, ids=[n + "-" + "-".join(map(str, s)) for n, s in CHUNK_CASES])
def test_families_are_well_posed_for_chunk_attention(name, shape, oracle):
    d, M, C, G, n_q, T, r, cap, rstart, chunk = shape
    peak = name[5:] if name.startswith("peak:") else None
    nh_k = 2
    st = F.chunk_inputs(name, 1, G * nh_k, nh_k, d, M, C, n_q, T, r, cap, rstart, chunk, peak=peak)
    K, V, n_past = F.chunk_keys(oracle, st)
    hs = _heads(G * nh_k)
    gold = F.chunk_gold(oracle, st)[0, hs]
    n_c = n_q if chunk else 0
    vis = np.ones((n_q, n_past + n_c), bool)
    if chunk:
        vis[:, n_past:] = np.arange(n_c)[None, :] <= np.arange(n_q)[:, None]
    assert _worst(F.ideal(gold), gold) <= CAP
    plain = F.model_heads(F.model_plain, st["q"], K, V, vis, hs, F.chunk_tiles(T, r, n_c))
    assert _worst(plain, gold) <= CAP, f"{name}: plain model worst row {_worst(plain, gold):.2e}"
    if peak is not None:      # the dominating key holds nearly all of the mass of every row that sees it
        at = st["peak_at"]
        s = F.logits(st["q"], K)[0, 0]
        sees = vis[:, at]
        others = np.where(vis & (np.arange(vis.shape[1]) != at)[None, :], s, -np.inf).max(axis=1)
        assert sees.any() and np.all(s[sees, at] - others[sees] > 0.5 * F.PEAK_NATS)


@pytest.mark.parametrize("d", [128, 64])
@pytest.mark.parametrize("name,L", [("gauss1", 1), ("gauss2", 2), ("gauss4", 4), ("gauss8", 8), ("outlier4", 4)])
def test_logit_spread_is_nominal(name, L, d):
    q, k, _ = F.prefill_inputs(name, 1, 8, 8, 1024, 1024, d)
    s = F.logits(q, k)
    assert abs(s.std() / L - 1) < 0.1, f"{name}: logit standard deviation {s.std():.3f}, nominal {L}"
    if name == "outlier4":      # two channels carry most of q . k
        hot = [5, d - 3]
        part = np.einsum("bhid,bhjd->bhij", q[..., hot].astype(np.float64), k[..., hot].astype(np.float64)) / np.sqrt(d)
        assert part.var() / s.var() > 0.8


@pytest.mark.parametrize("d", [128, 64])
@pytest.mark.parametrize("step", [5, 9])
def test_staircase_step(step, d):
    q, k, _ = F.prefill_inputs(f"stair{step}", 1, 8, 8, 256, 1024, d)
    s = F.logits(q, k)[0] * F.LOG2E                                        # (heads, rows, keys) in log2 units
    halves = s.reshape(s.shape[0], s.shape[1], -1, 32).mean(axis=3)
    rise = np.diff(halves, axis=2)
    assert abs(np.median(rise) / step - 1) < 0.02, f"median rise {np.median(rise):.3f} log2 units per half, nominal {step}"
    assert abs(rise.mean(axis=1) / step - 1).max() < 0.05                  # every half, averaged over the rows of a head


def test_sink_and_ramp():
    q, k, _ = F.prefill_inputs("sink_local", 1, 8, 8, 256, 1024, 128)
    s = F.logits(q, k)[0]
    body = s[:, :, 100:900].mean()
    assert abs((s[:, :, 0].mean() - body) / F.SINK_NATS - 1) < 0.1
    ramp = s[:, :, -64:].mean(axis=(0, 1)) - body
    assert np.all(np.diff(ramp) > 0) and abs(ramp[-1] / F.SINK_NATS - 1) < 0.1


@pytest.mark.parametrize("d", [128, 64])
def test_descending_mass_below_fp16_normal_range(d):
    """Key 0 is the row maximum and every later key lies 10 .. 20 log2 units below it; in rows with at least 512 visible keys at
    least 0.4 % of the softmax mass belongs to keys whose P = 2^(s - max) is below 2^-14, the smallest normal fp16 number: a
    kernel that flushed those operands (while l counts them in fp32) is wrong by that share, four bars."""
    q, k, _ = F.prefill_inputs("descending", 1, 8, 8, 1024, 1024, d)
    s = F.logits(q, k)[0] * F.LOG2E
    below = s[:, :, :1] - s[:, :, 1:]
    assert below.min() > 10 and below.max() < 20, f"later keys lie {below.min():.2f} .. {below.max():.2f} log2 units below key 0"
    p = np.exp2(s - s[:, :, :1])
    for n_vis in (512, 1024):
        pr = p[:, n_vis - 1, :n_vis]
        share = np.where(pr < 2.0 ** -14, pr, 0).sum(axis=1) / pr.sum(axis=1)
        assert share.min() >= 0.004, f"{n_vis} keys: share below 2^-14 {share.min():.4f}"
    # and the arithmetic the kernels are meant to have is hurt by a flush as the docstring says
    qv, kv, vv = F.prefill_inputs("descending", 1, 1, 1, 64, 1024, d)
    gold = F.prefill_gold(qv, kv, vv, 960, True)[0, 0]
    mass = np.exp2((F.logits(qv, kv)[0, 0] - F.logits(qv, kv)[0, 0][:, :1]) * F.LOG2E)
    keep = np.where(mass >= 2.0 ** -14, mass, 0)
    flushed = (keep @ vv[0, 0].astype(np.float64)) / mass.sum(axis=1, keepdims=True)
    assert F.row_err(flushed, gold).min() > 2 * F.REL_TOL


def test_scaled_fp16_q_misses_the_row_bar():
    """Why prefill_attn_pipe_kernel keeps Q unscaled.  Worst row of the retired form (qf = fp16(q * scale * log2 e)) against fp64 at
    n = 1024, d = 128, causal: within the bar at logit standard deviation 1, past it at 4, further at 8, while the whole-tensor
    norm stays under the bar throughout - the reason the bar is per row.  The present form stays within the bar, near half of it (its lazy
    reference rounds the dominating P of a peaked row to fp16 where the plain kernel's is exactly 1)."""
    seen = {}
    for name in ("gauss1", "gauss4", "gauss8"):
        q, k, v = F.prefill_inputs(name, 1, 8, 8, 1024, 1024, 128)
        hs = [0, 7]
        gold = F.prefill_gold(q[:, hs], k[:, hs], v[:, hs])[0]
        vis = F.visible(1024, 1024)
        old = F.model_heads(F.model_pipelined, q, k, v, vis, hs, scaled_q=True)
        new = F.model_heads(F.model_pipelined, q, k, v, vis, hs)
        whole = np.linalg.norm(old.astype(np.float64) - gold) / np.linalg.norm(gold)
        seen[name] = (_worst(old, gold), whole, _worst(new, gold))
    print(seen)
    assert seen["gauss1"][0] < F.REL_TOL
    assert seen["gauss4"][0] > F.REL_TOL
    assert seen["gauss8"][0] > 2 * F.REL_TOL and seen["gauss8"][0] > seen["gauss4"][0]
    assert all(w < F.REL_TOL for _, w, _ in seen.values())
    assert all(n < F.REL_TOL for _, _, n in seen.values())
