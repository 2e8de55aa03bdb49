"""million_attn_sink_merge on the GPU (ops.attn_sink_merge) against the fp64 model of tests/sink_model.py, at the project's bars -
rel-L2 < 1e-3 and mean-abs < 1e-3 on out, LSE_TOL absolute on lse - and bit for bit where the contract says so: no sink rows is
the identity, out may alias out_a, views cost nothing, a host count is a device count, poisoned memory is never looked at.
Both instances are covered everywhere: n <= 4 (lane = sink row) and n > 4 (lane = (row, quarter of d)), with the 16 / 17 edge."""
import numpy as np
import pytest

from tests import lse_ref as R
from tests import sink_model as SM

pytestmark = pytest.mark.gpu

BS, NHK = 2, 2
REL, MABS = 1e-3, 1e-3


def _case(seed, n, d, s_cap, G=4, lse_loc=0.0):
    """fp16 / fp32 numpy inputs: q, sink rows, (out_a, lse_a)."""
    rs = np.random.RandomState(seed)
    nh = G * NHK
    return dict(q=rs.standard_normal((BS, nh, n, d)).astype(np.float16),
                ks=rs.standard_normal((BS, NHK, s_cap, d)).astype(np.float16),
                vs=rs.standard_normal((BS, NHK, s_cap, d)).astype(np.float16),
                out_a=rs.standard_normal((BS, nh, n, d)).astype(np.float16),
                lse_a=(rs.standard_normal((BS, nh, n)) * 2 + lse_loc).astype(np.float32))


def _dev(c):
    import torch
    return {k: torch.from_numpy(v).cuda() for k, v in c.items()}


def _i32(xs):
    import torch
    return torch.tensor(list(xs), dtype=torch.int32).cuda()


def _run(t, **kw):
    from million_amd import ops
    out, lse = ops.attn_sink_merge(t["q"], t["ks"], t["vs"], t["out_a"], t["lse_a"], return_lse=True, **kw)
    return out, lse


def _check(got, want, what):
    out, lse = got[0].float().cpu().numpy().astype(np.float64), got[1].cpu().numpy().astype(np.float64)
    wo, wl = want
    rel, mabs = SM.errors(out, wo)
    fin = np.isfinite(wl)
    assert np.array_equal(np.isneginf(lse), np.isneginf(wl)), what
    dl = float(np.abs(lse[fin] - wl[fin]).max()) if fin.any() else 0.0
    print(f"{what}: rel-L2 {rel:.3e} mean-abs {mabs:.3e} lse {dl:.3e}")
    assert rel < REL and mabs < MABS and dl <= R.LSE_TOL, (what, rel, mabs, dl)


def _same(a, b):
    import torch
    return all(torch.equal(x.view(torch.int16) if x.dtype == torch.float16 else x.view(torch.int32), y.view(torch.int16) if y.dtype == torch.float16 else y.view(torch.int32))
               for x, y in zip(a, b))


@pytest.mark.parametrize("s_cap", [4, 64])
@pytest.mark.parametrize("n", [1, 3, 16, 17, 40])
@pytest.mark.parametrize("G", [1, 4, 7])
@pytest.mark.parametrize("d", [64, 128])
def test_against_the_model(d, G, n, s_cap):
    c = _case(1000 + d + 7 * G + 31 * n + s_cap, n, d, s_cap, G)
    t = _dev(c)
    # the two requests at different counts: {0, s_cap} and {1, s_cap - 1}; the second call with fewer live query rows
    for s_valid, n_valid in (([0, s_cap], None), ([1, s_cap - 1], [n - 1, max(n - 3, 0)] if n > 1 else [1, 0])):
        got = _run(t, dev_s=_i32(s_valid), dev_n=None if n_valid is None else _i32(n_valid))
        want = SM.sink_merge(c["q"], c["ks"], c["vs"], c["out_a"], c["lse_a"], s_valid=s_valid, n_valid=n_valid)
        _check(got, want, f"d={d} G={G} n={n} s_cap={s_cap} s={s_valid} n_b={n_valid}")


@pytest.mark.parametrize("n,d,s_cap", [(1, 128, 64), (4, 64, 4), (17, 128, 4), (40, 64, 64)])
def test_bitwise_contracts(n, d, s_cap):
    import torch
    from million_amd import ops
    c = _case(77 + n, n, d, s_cap)
    t = _dev(c)
    # no sink rows: the identity on (out_a, lse_a), from a device count and from a host count
    for kw in (dict(dev_s=_i32([0, 0])), dict(n_sink=0)):
        assert _same(_run(t, **kw), (t["out_a"], t["lse_a"])), kw
    s_valid = [s_cap - 1, 1]
    ref = _run(t, dev_s=_i32(s_valid))
    # out aliasing out_a (and lse_out aliasing lse_a: a row's lse is read by the one wave that writes it)
    oa, la = t["out_a"].clone(), t["lse_a"].clone()
    got = ops.attn_sink_merge(t["q"], t["ks"], t["vs"], oa, la, dev_s=_i32(s_valid), out=oa, lse_out=la)
    assert got[0] is oa and got[1] is la and _same(got, ref)
    # a transposed view of out_a (and of q, and of out) costs nothing and changes nothing
    tr = lambda x: x.transpose(1, 2).contiguous().transpose(1, 2)
    out_t = torch.empty_like(tr(t["out_a"]).transpose(1, 2)).transpose(1, 2)
    assert not tr(t["out_a"]).is_contiguous() or n == 1
    got = ops.attn_sink_merge(tr(t["q"]), t["ks"], t["vs"], tr(t["out_a"]), t["lse_a"], dev_s=_i32(s_valid), out=out_t, return_lse=True)
    assert _same(got, ref)
    # a host count is the same count on the device
    for s in (1, s_cap):
        assert _same(_run(t, n_sink=s), _run(t, dev_s=_i32([s, s]))), s
    # sink views with strides of their own (a layer of a cache's buffer)
    big_k = torch.zeros(3, BS, NHK, s_cap, d, dtype=torch.float16, device="cuda")
    big_v = torch.zeros_like(big_k)
    big_k[1], big_v[1] = t["ks"], t["vs"]
    got = ops.attn_sink_merge(t["q"], big_k[1, :, :, :], big_v[1], t["out_a"], t["lse_a"], dev_s=_i32(s_valid), return_lse=True)
    assert _same(got, ref)


@pytest.mark.parametrize("n,d,s_cap", [(2, 128, 4), (3, 64, 64), (17, 128, 64), (20, 64, 4)])
def test_poison_and_garbage_counts(n, d, s_cap):
    """NaN in sink rows at or past s_b, in q / out_a rows at or past n_b and in `out` beforehand: the same bits as zeros there.
    Counts outside their range: the bits of the clamped counts."""
    import torch
    c = _case(300 + n + s_cap, n, d, s_cap)
    s_valid, n_valid = [s_cap - 1, 1], [n - 1, 1]
    clean = {k: v.copy() for k, v in c.items()}
    dirty = {k: v.copy() for k, v in c.items()}
    for b in range(BS):
        for x, val in ((clean, 0), (dirty, np.nan)):
            x["ks"][b, :, s_valid[b]:], x["vs"][b, :, s_valid[b]:] = val, val
            x["q"][b, :, n_valid[b]:], x["out_a"][b, :, n_valid[b]:] = val, val
            x["lse_a"][b, :, n_valid[b]:] = val
    tc, td = _dev(clean), _dev(dirty)
    from million_amd import ops
    outs = []
    for t, fill in ((tc, 0.0), (td, float("nan"))):
        out = torch.full((BS, t["q"].shape[1], n, d), fill, dtype=torch.float16, device="cuda")
        lse = torch.full((BS, t["q"].shape[1], n), fill, dtype=torch.float32, device="cuda")
        outs.append(ops.attn_sink_merge(t["q"], t["ks"], t["vs"], t["out_a"], t["lse_a"], dev_s=_i32(s_valid), dev_n=_i32(n_valid),
                                        out=out, lse_out=lse))
    assert _same(outs[0], outs[1])
    o, l = outs[1]
    assert torch.isfinite(o).all() and not torch.isnan(l).any()
    for b in range(BS):
        assert (o[b, :, n_valid[b]:] == 0).all() and torch.isneginf(l[b, :, n_valid[b]:]).all()
        assert torch.isfinite(l[b, :, :n_valid[b]]).all()
    _check(outs[1], SM.sink_merge(clean["q"], clean["ks"], clean["vs"], clean["out_a"], np.nan_to_num(clean["lse_a"]), s_valid, n_valid), "poison")
    t = _dev(c)
    assert _same(_run(t, dev_s=_i32([-5, 1000]), dev_n=_i32([1000, -5])), _run(t, dev_s=_i32([0, s_cap]), dev_n=_i32([n, 0])))


@pytest.mark.parametrize("n,d,s_cap", [(1, 128, 4), (4, 64, 64), (17, 128, 64), (16, 64, 4)])
def test_lse_edges(n, d, s_cap):
    import torch
    c = _case(500 + n + s_cap, n, d, s_cap)
    nh = c["q"].shape[1]
    # lse_a = -inf: pure sink attention, whatever out_a holds; with no sink row either: zeros, -inf
    c["lse_a"][0] = -np.inf
    c["out_a"][0] = np.float16(6e4)
    # lse_a = NaN: that row is NaN, no other
    c["lse_a"][1, nh - 1, n - 1] = np.nan
    t = _dev(c)
    s_valid = [s_cap, s_cap - 1]
    got = _run(t, dev_s=_i32(s_valid))
    assert torch.isnan(got[0][1, nh - 1, n - 1]).all() and torch.isnan(got[1][1, nh - 1, n - 1])
    keep = torch.ones(BS, nh, n, dtype=torch.bool, device="cuda")
    keep[1, nh - 1, n - 1] = False
    assert torch.isfinite(got[0][keep]).all() and torch.isfinite(got[1][keep]).all()
    want = SM.sink_merge(c["q"], c["ks"], c["vs"], c["out_a"], c["lse_a"], s_valid=s_valid)
    own = R.attend(c["q"][:1].astype(np.float64), c["ks"][:1].astype(np.float64), c["vs"][:1].astype(np.float64))
    assert np.abs(want[0][0] - own[0][0]).max() <= 1e-12
    g = (got[0].float().cpu().numpy().astype(np.float64), got[1].cpu().numpy().astype(np.float64))
    g[0][1, nh - 1, n - 1], g[1][1, nh - 1, n - 1] = 0, 0
    want[0][1, nh - 1, n - 1], want[1][1, nh - 1, n - 1] = 0, 0
    _check((torch.from_numpy(g[0]), torch.from_numpy(g[1])), want, "edges")
    none = _run(t, dev_s=_i32([0, 0]))
    assert (none[0][0] == 0).all() and torch.isneginf(none[1][0]).all()


@pytest.mark.parametrize("n,d,s_cap", [(1, 128, 64), (3, 64, 4), (17, 64, 64), (40, 128, 4)])
def test_peaked_both_ways(n, d, s_cap):
    """A sink score far above lse_a (the past's weight underflows to 0: the row is the sink attention) and lse_a far above every
    sink score (the sinks' weights underflow: the row is out_a)."""
    import torch
    c = _case(700 + n + s_cap, n, d, s_cap)
    c["lse_a"][0] = -200.0      # sink scores are O(1): w = exp(-200 - L) = 0 in fp32
    c["lse_a"][1] = 200.0       # p_j = exp(s_j - 200) = 0 in fp32
    t = _dev(c)
    got = _run(t, n_sink=s_cap)
    want = SM.sink_merge(c["q"], c["ks"], c["vs"], c["out_a"], c["lse_a"])
    _check(got, want, "peaked")
    own = R.attend(c["q"][:1].astype(np.float64), c["ks"][:1].astype(np.float64), c["vs"][:1].astype(np.float64))
    rel, mabs = SM.errors(got[0][0].float().cpu().numpy(), own[0][0])
    assert rel < REL and mabs < MABS
    assert torch.equal(got[0][1], t["out_a"][1]) and torch.equal(got[1][1], t["lse_a"][1])
    # and a sink row that dominates: one key scaled so that its score is ~ 40 above the rest
    c2 = _case(701 + n, n, d, s_cap, lse_loc=3.0)
    c2["ks"][:, :, 0] = (c2["q"][:, ::c2["q"].shape[1] // NHK, 0] * np.float16(40.0 / np.sqrt(d))).astype(np.float16)
    got = _run(_dev(c2), n_sink=s_cap)
    _check(got, SM.sink_merge(c2["q"], c2["ks"], c2["vs"], c2["out_a"], c2["lse_a"]), "dominant sink")


def test_python_binding_refuses():
    import torch
    from million_amd import ops
    t = _dev(_case(1, 3, 128, 4))
    with pytest.raises(RuntimeError, match="not both"):
        ops.attn_sink_merge(t["q"], t["ks"], t["vs"], t["out_a"], t["lse_a"], n_sink=1, dev_s=_i32([1, 1]))
    with pytest.raises(RuntimeError, match="n_sink"):
        ops.attn_sink_merge(t["q"], t["ks"], t["vs"], t["out_a"], t["lse_a"], n_sink=5)
    with pytest.raises(RuntimeError, match="s_cap"):
        big = torch.zeros(BS, NHK, 65, 128, dtype=torch.float16, device="cuda")
        ops.attn_sink_merge(t["q"], big, big, t["out_a"], t["lse_a"])
    with pytest.raises(RuntimeError, match="dense rows"):
        wide = torch.zeros(BS, NHK, 4, 256, dtype=torch.float16, device="cuda")[..., :128]
        ops.attn_sink_merge(t["q"], wide, wide, t["out_a"], t["lse_a"])
    with pytest.raises(RuntimeError, match="device tensors"):
        ops.attn_sink_merge(t["q"].cpu(), t["ks"], t["vs"], t["out_a"], t["lse_a"])
