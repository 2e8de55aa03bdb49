"""PagedPQCache(nbits 9 .. 12, dtype=torch.uint16) on the GPU: prefill, decode across flushes with host lengths, with device
lengths and with one captured plain step, release + a new prompt - against tests/wide_model.py (attention, fp64) and
oracle.pq_encode (the codes in the pages, bit for bit).  The bar: rel-L2 < 1e-3 and mean-abs < 1e-3 per head."""
import numpy as np
import pytest

from tests import wide_model as W

pytestmark = pytest.mark.gpu
REL_TOL = MEAN_ABS_TOL = 1e-3
BS, NH, NHK, D, LAYERS, WINDOW, PROMPT, MORE = 2, 8, 2, 128, 2, 64, 70, 5
STEPS = 2 * WINDOW + 3
CONFIGS = {"nbits10-M64-page32": dict(nbits=10, M=64, page=32), "nbits12-M32-page64": dict(nbits=12, M=32, page=64)}


@pytest.fixture(scope="module")
def env():
    import torch
    from million_amd import build
    build.build()
    assert torch.cuda.is_available()
    return torch


_data = {}


def data(oracle, name):
    """The inputs of a configuration and the codes of every row, drawn and encoded once for all its tests: rows (layer, bs, nh_k,
    token, d) of the first request lives (prompt, then one row per step) and of the prompt slot 0 gets after its release."""
    if name not in _data:
        cfg = CONFIGS[name]
        rs = np.random.RandomState(cfg["nbits"])
        n = PROMPT + STEPS + MORE
        h = lambda *s: rs.standard_normal(s).astype(np.float16)
        x = dict(cfg, C=2 ** cfg["nbits"], k_cents=h(cfg["M"], 2 ** cfg["nbits"], D // cfg["M"]), v_cents=h(cfg["M"], 2 ** cfg["nbits"], D // cfg["M"]),
                 K=h(LAYERS, BS, NHK, n, D), V=h(LAYERS, BS, NHK, n, D), Q=h(LAYERS, n, BS, NH, 1, D),
                 K2=h(LAYERS, 1, NHK, 45, D), V2=h(LAYERS, 1, NHK, 45, D))
        for nm, cents in (("K", "k_cents"), ("V", "v_cents")):
            x[nm + "c"] = np.stack([oracle.pq_encode(x[nm][l], x[cents]) for l in range(LAYERS)])
            x[nm + "2c"] = np.stack([oracle.pq_encode(x[nm + "2"][l], x[cents]) for l in range(LAYERS)])
            assert x[nm + "c"].dtype == np.uint16 and x[nm + "c"].max() >= 256
        _data[name] = x
    return _data[name]


def make_cache(torch, x):
    from million_amd.pq_cache import PagedPQCache
    cache = PagedPQCache(bs=BS, nh=NH, num_key_value_heads=NHK, M=x["M"], layer_num=LAYERS, nbits=x["nbits"], dtype=torch.uint16, d=D,
                         page_size=x["page"], extended_residual_size=WINDOW, max_tokens=512)
    cache.set_cent(torch.from_numpy(x["k_cents"]).cuda(), torch.from_numpy(x["v_cents"]).cuda())
    assert cache.key_page_pool.dtype == torch.uint16
    return cache


def within_bar(got, ref, what):
    rel, mabs = W.head_errors(got.float().cpu().numpy(), ref)
    assert np.isfinite(rel).all() and rel.max() < REL_TOL and mabs.max() < MEAN_ABS_TOL, \
        f"{what}: worst head rel-L2 {rel.max():.3e} mean-abs {mabs.max():.3e}"
    return rel.max()


def pages_hold(cache, l, b, k_codes, v_codes, T):
    """The codes read back from the pools through the page table of (layer l, request b) are k_codes / v_codes[:, :T], bit for bit."""
    ps = cache.page_size
    npg = -(-T // ps)
    if not npg:
        return True
    ids = cache.page_ids[l][b, :, :npg].long()
    i16 = __import__("torch").int16      # (gathered as int16: the same bits)
    kc = cache.key_page_pool.view(i16)[ids].reshape(NHK, npg * ps, cache.M)[:, :T].cpu().numpy().view(np.uint16)
    vc = cache.value_page_pool.view(i16)[ids].permute(0, 1, 3, 2).reshape(NHK, npg * ps, cache.M)[:, :T].cpu().numpy().view(np.uint16)
    return np.array_equal(kc, k_codes[:, :T]) and np.array_equal(vc, v_codes[:, :T])


def check_step(cache, x, l, out, q, policy, seen, lens_on_device, what):
    """Layer l after a step: the output within the bar of the model over the rows the policy says are coded (as oracle.pq_encode
    codes them) and windowed, the pages hold those codes, host (and device) lengths are the policy's."""
    T, r = policy
    assert cache._T_a[l].tolist() == [T] * BS and cache._r_a[l].tolist() == [r] * BS and T + r == seen, what
    if not lens_on_device:      # a host-length step moves the mirror alone; the device rows follow when somebody asks for them
        cache._refresh_device_rows()
    rows = cache.lengths[l].cpu().numpy()
    assert rows[:, 0].tolist() == [T] * BS and rows[:, 1].tolist() == [r] * BS and rows[:, 2].tolist() == cache._rs_a[l].tolist(), what
    ref, _ = W.decode_attn(q, x["Kc"][l][:, :, :T], x["Vc"][l][:, :, :T], x["k_cents"], x["v_cents"], x["K"][l][:, :, T:seen],
                           x["V"][l][:, :, T:seen], r)
    worst = within_bar(out, ref, what)
    for b in range(BS):
        assert pages_hold(cache, l, b, x["Kc"][l][b], x["Vc"][l][b], T), what
    return worst


def drive(torch, oracle, x, cache, mode, check=True, graph_at=10):
    """Prefill PROMPT rows, then STEPS decode steps; mode "host" / "dev" / "graph" (device lengths, step graph_at captured and
    replayed).  Returns the steps' flush count."""
    dev = mode != "host"
    g = lambda a: torch.from_numpy(np.ascontiguousarray(a)).cuda()
    for l in range(LAYERS):
        cache.prefill(g(np.zeros((BS, NH, PROMPT, D), np.float16)), g(x["K"][l][:, :, :PROMPT]), g(x["V"][l][:, :, :PROMPT]), l)
    pol = oracle.PagedPolicy(page_size=x["page"], residual=WINDOW, prefill=PROMPT)
    worst = 0.0
    for step in range(STEPS):
        t = PROMPT + step
        qs = [g(x["Q"][l][t]) for l in range(LAYERS)]
        ks = [g(x["K"][l][:, :, t:t + 1]) for l in range(LAYERS)]
        vs = [g(x["V"][l][:, :, t:t + 1]) for l in range(LAYERS)]
        flushing = cache.next_step_flushes()
        assert cache.begin_step(use_dev_lengths=dev) == ("flush" if flushing else "plain")
        if mode == "graph" and step == graph_at:
            assert not flushing
            torch.cuda.synchronize()
            graph = torch.cuda.CUDAGraph()
            with torch.cuda.graph(graph):      # the Python runs once (the mirror moves), the launches are recorded: one stream
                outs = [cache.decoding_with_pages(qs[l], ks[l], vs[l], l, use_dev_lengths=True) for l in range(LAYERS)]
            graph.replay()
        else:
            outs = [cache.decoding_with_pages(qs[l], ks[l], vs[l], l, use_dev_lengths=dev) for l in range(LAYERS)]
        state = pol.step()
        if check:
            for l in range(LAYERS):
                worst = max(worst, check_step(cache, x, l, outs[l], x["Q"][l][t], state, t + 1, dev, f"{mode} step {step} layer {l}"))
    if check:
        print(f"{mode}: worst head rel-L2 over {STEPS} steps x {LAYERS} layers {worst:.3e}, {pol.flushes} flushes")
    return pol


@pytest.mark.parametrize("mode", ["host", "dev", "graph"])
@pytest.mark.parametrize("name", list(CONFIGS))
def test_decode_across_flushes(env, oracle, name, mode):
    torch = env
    x = data(oracle, name)
    cache = make_cache(torch, x)
    pol = drive(torch, oracle, x, cache, mode)
    assert pol.flushes >= 2
    cache._refresh_device_rows()      # host lengths: the device rows follow when somebody needs them
    for l in range(LAYERS):
        rows = cache.lengths[l].cpu().numpy()
        assert rows[:, 0].tolist() == cache._T_a[l].tolist() and rows[:, 1].tolist() == cache._r_a[l].tolist()
        assert rows[:, 2].tolist() == cache._rs_a[l].tolist()
    st = cache.get_cache_stats()
    assert st["layer_stats"][0]["key_cache_tokens"] == pol.T and st["layer_stats"][1]["residual_tokens"] == pol.r


def _more_steps(torch, x, cache, n_done):
    outs = []
    g = lambda a: torch.from_numpy(np.ascontiguousarray(a)).cuda()
    for i in range(MORE):
        t = n_done + i
        outs.append([cache.decoding_with_pages(g(x["Q"][l][t]), g(x["K"][l][:, :, t:t + 1]), g(x["V"][l][:, :, t:t + 1]), l, use_dev_lengths=True)
                     for l in range(LAYERS)])
    return outs


@pytest.mark.parametrize("name", list(CONFIGS))
def test_release_and_a_new_prompt(env, oracle, name):
    torch = env
    x = data(oracle, name)
    g = lambda a: torch.from_numpy(np.ascontiguousarray(a)).cuda()
    kept = make_cache(torch, x)
    pol = drive(torch, oracle, x, kept, "dev", check=False)
    base = _more_steps(torch, x, kept, PROMPT + STEPS)
    cache = make_cache(torch, x)
    drive(torch, oracle, x, cache, "dev", check=False)
    cache.release(0)
    assert not cache._T_a[:, 0].any() and not cache.lengths[0][0].any()
    for l in range(LAYERS):
        cache.prefill_request(0, g(np.zeros((1, NH, 45, D), np.float16)), g(x["K2"][l]), g(x["V2"][l]), l)
    outs = _more_steps(torch, x, cache, PROMPT + STEPS)
    T1, r1 = pol.T, pol.r
    for i in range(MORE):
        t = PROMPT + STEPS + i
        for l in range(LAYERS):
            # slot 1: the bits of the run in which slot 0 was never recycled; slot 0: its new prompt's codes, then the rows of the steps
            assert torch.equal(outs[i][l][1], base[i][l][1]), (i, l)
            ref, _ = W.decode_attn(x["Q"][l][t][:1], x["K2c"][l], x["V2c"][l], x["k_cents"], x["v_cents"],
                                   x["K"][l][:1, :, PROMPT + STEPS:t + 1], x["V"][l][:1, :, PROMPT + STEPS:t + 1], i + 1)
            within_bar(outs[i][l][:1], ref, f"recycled slot, step {i} layer {l}")
            ref1, _ = W.decode_attn(x["Q"][l][t][1:], x["Kc"][l][1:, :, :T1], x["Vc"][l][1:, :, :T1], x["k_cents"], x["v_cents"],
                                    x["K"][l][1:, :, T1:t + 1], x["V"][l][1:, :, T1:t + 1], r1 + i + 1)
            within_bar(outs[i][l][1:], ref1, f"kept slot, step {i} layer {l}")
    for l in range(LAYERS):
        assert pages_hold(cache, l, 0, x["K2c"][l][0], x["V2c"][l][0], 45) and pages_hold(cache, l, 1, x["Kc"][l][1], x["Vc"][l][1], T1)
        assert cache.lengths[l].cpu().tolist() == [[45, MORE, 0, 0], [T1, r1 + MORE, int(cache._rs_a[l, 1]), 0]]
