"""GPU tests of the block route of chunk attention (ops.pq_chunk_attn_blocks) and of route="blocks" on the
caches' extend(): the past dequantised block by block into a bounded scratch (ops.pq_gather_rows), each block and the chunk
attended by the prompt kernel with lse, the parts merged.  Against the fp64 model of the unsplit attention: the attention bar
(rel-L2 < 1e-3, mean-abs < 1e-3) and lse_ref.LSE_TOL; against ops.pq_chunk_attn on the same inputs: rel-L2 < 2e-3 (two results
each inside 1e-3).  tests/test_chunk_blocks_host.py shows on the CPU that the route's own roundings leave the bar."""
import numpy as np
import pytest

from tests import chunk_blocks_model as B
from tests import lse_ref
from tests.test_chunk_attn_gpu import _state

pytestmark = pytest.mark.gpu

BS, NH, NH_K, CAP = 2, 8, 2, 64
# name -> (T, block_tokens, r, resid_start, n_q, chunk)
CASES = {
    "3-blocks-window-chunk": (300, 128, 37, 50, 70, True),      # the last block partial, the ring wraps
    "3-blocks-window-past-only": (300, 128, 37, 50, 70, False),
    "window-and-chunk": (0, 128, 37, 50, 70, True),
    "chunk-alone": (0, 128, 0, 0, 70, True),
    "11-parts-two-levels": (700, 64, 0, 0, 70, False),
}


@pytest.fixture(scope="module")
def env():
    import torch
    assert torch.cuda.is_available(), "GPU tests need an MI355X"
    from million_amd import ops, _lib
    _lib.load()
    return torch, ops


def _cu(torch, a):
    return None if a is None else torch.from_numpy(np.ascontiguousarray(a)).cuda()


def _wide_state(rs_, d, M, C, n_q, T, r, rstart, chunk):
    st = _state(rs_, BS, NH, NH_K, d, M, 256, n_q, T, r, CAP, rstart, chunk)
    f = lambda *s: rs_.standard_normal(s).astype(np.float16)
    st["k_cents"], st["v_cents"] = f(M, C, d // M), f(M, C, d // M)
    st["k_codes"] = rs_.randint(0, C, (BS, NH_K, T, M)).astype(np.uint16)
    st["v_codes"] = rs_.randint(0, C, (BS, NH_K, T, M)).astype(np.uint16)
    return st


def _args(torch, ops, st, M, C, layout, ps=64):
    """(positional arguments, keyword arguments) shared by ops.pq_chunk_attn / pq_chunk_attn_wide / pq_chunk_attn_blocks."""
    cu = lambda a: _cu(torch, a)
    T = st["k_codes"].shape[2]
    wide = st["k_codes"].dtype == np.uint16
    kp, vp = (cu(st["k_cents"]), cu(st["v_cents"])) if wide else (ops.prepare_cents(cu(st["k_cents"]), cache=False),
                                                                  ops.prepare_cents(cu(st["v_cents"]), cache=False))
    kw = dict(M=M, C=C, n_tokens=T, resid_start=st["rs"])
    if layout == "paged":
        kpool, vpool, ids = B.to_pools(st["k_codes"], st["v_codes"], ps, fill=np.iinfo(st["k_codes"].dtype).max)
        ids_t = cu(ids)
        k_codes, v_codes = cu(kpool), cu(vpool)
        kw.update(k_page_ids=ids_t, v_page_ids=ids_t, page_size=ps)
    else:
        k_codes, v_codes = cu(st["k_codes"]), cu(st["v_codes"])
    return (cu(st["q"]), cu(st["k_ch"]), cu(st["v_ch"]), k_codes, v_codes, kp, vp, cu(st["k_res"]), cu(st["v_res"]), st["r"]), kw


def _check_route(torch, ops, oracle, st, M, C, layout, bt, what, against_chunk=True):
    args, kw = _args(torch, ops, st, M, C, layout)
    out, lse = ops.pq_chunk_attn_blocks(*args, block_tokens=bt, return_lse=True, **kw)
    only = ops.pq_chunk_attn_blocks(*args, block_tokens=bt, **kw)
    torch.cuda.synchronize()
    assert tuple(out.shape) == st["q"].shape and tuple(lse.shape) == st["q"].shape[:3]
    assert torch.equal(out.contiguous().view(torch.int16), only.contiguous().view(torch.int16)), f"{what}: out with lse differs from out without"
    gold_out, gold_lse = B.route_ref(oracle, st)
    o, l = out.float().cpu().numpy(), lse.cpu().numpy()
    B.check_bar(o, gold_out, f"{what} vs fp64")
    B.check_lse(l, gold_lse, f"{what} vs fp64", lse_ref.LSE_TOL)
    if against_chunk:
        ref = (ops.pq_chunk_attn_wide if st["k_codes"].dtype == np.uint16 else ops.pq_chunk_attn)(*args, **kw)
        torch.cuda.synchronize()
        B.check_bar(o, ref.float().cpu().numpy(), f"{what} vs the chunk route", rel_tol=2e-3, mae_tol=2e-3)
    return out, lse


@pytest.mark.parametrize("name", list(CASES))
def test_block_route_paged(name, env, oracle):
    torch, ops = env
    T, bt, r, rstart, n_q, chunk = CASES[name]
    st = _state(np.random.RandomState(len(name)), BS, NH, NH_K, 128, 64, 256, n_q, T, r, CAP, rstart, chunk)
    n_parts = len(ops.chunk_blocks_plan(T, r, chunk, bt)["parts"])
    assert n_parts == {"3-blocks-window-chunk": 4, "3-blocks-window-past-only": 3, "window-and-chunk": 2, "chunk-alone": 1, "11-parts-two-levels": 11}[name]
    _check_route(torch, ops, oracle, st, 64, 256, "paged", bt, name)


def test_block_route_rowmajor(env, oracle):
    torch, ops = env
    T, bt, r, rstart, n_q, chunk = CASES["3-blocks-window-chunk"]
    st = _state(np.random.RandomState(31), BS, NH, NH_K, 128, 64, 256, n_q, T, r, CAP, rstart, chunk)
    _check_route(torch, ops, oracle, st, 64, 256, "rowmajor", bt, "row-major")


def test_block_route_d64(env, oracle):
    torch, ops = env
    T, bt, r, rstart, n_q, chunk = CASES["3-blocks-window-chunk"]
    st = _state(np.random.RandomState(32), BS, NH, NH_K, 64, 32, 256, n_q, T, r, CAP, rstart, chunk)
    _check_route(torch, ops, oracle, st, 32, 256, "paged", bt, "d64 M32")


def test_nothing_to_attend_to(env):
    torch, ops = env
    st = _state(np.random.RandomState(33), BS, NH, NH_K, 128, 64, 256, 5, 0, 0, CAP, 0, False)
    args, kw = _args(torch, ops, st, 64, 256, "rowmajor")
    out = torch.full(st["q"].shape, float("nan"), dtype=torch.float16, device="cuda")
    lse = torch.full(st["q"].shape[:3], float("nan"), dtype=torch.float32, device="cuda")
    ops.pq_chunk_attn_blocks(*args, out=out, lse=lse, **kw)
    torch.cuda.synchronize()
    assert not out.view(torch.int16).any() and torch.isneginf(lse).all()


@pytest.mark.parametrize("layout", ["paged", "rowmajor"])
def test_block_route_uint16(layout, env, oracle):
    torch, ops = env
    T, bt, r, rstart, n_q, chunk = CASES["3-blocks-window-chunk"]
    st = _wide_state(np.random.RandomState(34), 128, 64, 1024, n_q, T, r, rstart, chunk)
    _check_route(torch, ops, oracle, st, 64, 1024, layout, bt, f"uint16 {layout}")


def test_dev_lengths_are_refused_by_name(env):
    torch, ops = env
    st = _state(np.random.RandomState(35), BS, NH, NH_K, 128, 64, 256, 5, 64, 0, CAP, 0, True)
    args, kw = _args(torch, ops, st, 64, 256, "rowmajor")
    with pytest.raises(RuntimeError, match="dev_lengths"):
        ops.pq_chunk_attn_blocks(*args, dev_lengths=torch.zeros(BS, 4, dtype=torch.int32, device="cuda"), **kw)
    with pytest.raises(RuntimeError, match="dev_n_q"):
        ops.pq_chunk_attn_blocks(*args, dev_n_q=torch.zeros(BS, dtype=torch.int32, device="cuda"), **kw)


def test_captured_route_replays_bitwise(env, oracle):
    """out=, workspace=, lse=: nothing is allocated and the route is a chain on one stream; two replays are bitwise the eager run."""
    torch, ops = env
    T, bt, r, rstart, n_q, chunk = CASES["3-blocks-window-chunk"]
    st = _state(np.random.RandomState(36), BS, NH, NH_K, 128, 64, 256, n_q, T, r, CAP, rstart, chunk)
    args, kw = _args(torch, ops, st, 64, 256, "paged")
    need = ops.chunk_blocks_workspace_bytes(BS, NH, NH_K, n_q, 128, CAP, bt)
    assert need == ops.chunk_blocks_workspace_bytes(BS, NH, NH_K, n_q, 128, CAP, bt)
    ws = torch.empty(need, dtype=torch.uint8, device="cuda")
    out = torch.empty(BS, NH, n_q, 128, dtype=torch.float16, device="cuda")
    lse = torch.empty(BS, NH, n_q, dtype=torch.float32, device="cuda")
    run = lambda: ops.pq_chunk_attn_blocks(*args, block_tokens=bt, out=out, lse=lse, workspace=ws, **kw)
    run()      # eager once: module load, kernel attributes
    torch.cuda.synchronize()
    eager_o, eager_l = out.clone(), lse.clone()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        run()
    for _ in range(2):
        out.fill_(float("nan"))
        lse.fill_(float("nan"))
        ws.fill_(0xFF)
        g.replay()
        torch.cuda.synchronize()
        assert torch.equal(out.view(torch.int16), eager_o.view(torch.int16)) and torch.equal(lse.view(torch.int32), eager_l.view(torch.int32))
    gold_out, gold_lse = B.route_ref(oracle, st)
    B.check_bar(out.float().cpu().numpy(), gold_out, "captured vs fp64")
    B.check_lse(lse.cpu().numpy(), gold_lse, "captured vs fp64")


# ---------------------------------------------------------------- caches ------------------------------------------------
def _paged_state(cache, oracle, q, k_ch, v_ch, kc, vc, b=None):
    """The chunk state a PagedPQCache holds for layer 0 (request b, or all in lockstep), read back through its table, and its
    live sink rows (or None)."""
    sel = slice(None) if b is None else slice(b, b + 1)
    i = 0 if b is None else b
    T, r, rs = int(cache._T_a[0, i]), int(cache._r_a[0, i]), int(cache._rs_a[0, i])
    k_codes, v_codes = B.from_pools(cache.key_page_pool.cpu().numpy(), cache.value_page_pool.cpu().numpy(), cache.page_ids[0].cpu().numpy()[sel], T)
    k_res, v_res = cache.key_residual_cache[0][sel].cpu().numpy(), cache.value_residual_cache[0][sel].cpu().numpy()
    ring = (rs + np.arange(r)) % k_res.shape[2]
    st = dict(q=q, k_codes=k_codes, v_codes=v_codes, k_cents=kc, v_cents=vc, k_res=k_res, v_res=v_res, r=r, rs=rs,
              k_win=k_res[:, :, ring], v_win=v_res[:, :, ring], k_ch=k_ch, v_ch=v_ch)
    s = int(cache._sink_a[0, i])
    sinks = (cache._ksink_all[0][sel, :, :s].cpu().numpy(), cache._vsink_all[0][sel, :, :s].cpu().numpy()) if s else None
    return st, sinks


def _gold_with_sinks(oracle, st, sinks):
    out, lse = B.route_ref(oracle, st)
    if sinks is None:
        return out, lse
    so, sl = lse_ref.attend(st["q"], sinks[0].astype(np.float64), sinks[1].astype(np.float64))
    return lse_ref.merge([out, so], [lse, sl])


def _same_cache_state(torch, a, b):
    assert all((x == y).all() for x, y in zip(a.host_state(), b.host_state()))
    for name in ("key_page_pool", "value_page_pool"):
        assert torch.equal(getattr(a, name), getattr(b, name)), name
    for name in ("page_ids", "lengths", "key_residual_cache", "value_residual_cache"):
        x, y = getattr(a, name)[0], getattr(b, name)[0]
        assert torch.equal(x.view(torch.int16) if x.dtype == torch.float16 else x, y.view(torch.int16) if y.dtype == torch.float16 else y), name
    if a.sink_tokens:
        assert torch.equal(a._sink_all, b._sink_all) and torch.equal(a._ksink_all.view(torch.int16), b._ksink_all.view(torch.int16))


@pytest.mark.parametrize("sink_tokens", [0, 4])
def test_paged_cache_extend_by_blocks(sink_tokens, env, oracle):
    """extend(route="blocks") and extend_request(b, ..., route="blocks"): outputs within the bar of the model of what the cache
    holds; pages, window, host and device lengths bit-identical to a twin driven with route=None."""
    torch, ops = env
    from million_amd.pq_cache import PagedPQCache
    cu = lambda a: _cu(torch, a)
    d, M, ps, n_a, n_dec, n_b, n_dec2, n_c = 128, 64, 64, 100, CAP + 6, 40, 5, 24
    rs_ = np.random.RandomState(41)
    kc, vc = (rs_.standard_normal((M, 256, d // M)).astype(np.float16) for _ in range(2))
    f = lambda *s: rs_.standard_normal(s).astype(np.float16)
    K, V = f(BS, NH_K, n_a + n_dec + n_b + n_dec2, d), f(BS, NH_K, n_a + n_dec + n_b + n_dec2, d)
    qa, q1s, qb, q2s = f(BS, NH, n_a, d), f(n_dec, BS, NH, 1, d), f(BS, NH, n_b, d), f(n_dec2, BS, NH, 1, d)
    qc, Kc, Vc = f(1, NH, n_c, d), f(1, NH_K, n_c, d), f(1, NH_K, n_c, d)
    twins, outs = [], []
    for route in (None, "blocks"):
        cache = PagedPQCache(bs=BS, nh=NH, num_key_value_heads=NH_K, M=M, layer_num=1, d=d, page_size=ps, extended_residual_size=CAP,
                             max_tokens=2048, device="cuda", sink_tokens=sink_tokens)
        cache.set_cent(cu(kc), cu(vc))
        cache.prefill(cu(qa), cu(K[:, :, :n_a]), cu(V[:, :, :n_a]), 0)
        for i in range(n_dec):
            cache.decoding_with_pages(cu(q1s[i]), cu(K[:, :, n_a + i:n_a + i + 1]), cu(V[:, :, n_a + i:n_a + i + 1]), 0)
        assert cache._r_a[0, 0] > 0 and cache._T_a[0, 0] > 0
        t0 = n_a + n_dec
        st, sinks = _paged_state(cache, oracle, qb, K[:, :, t0:t0 + n_b], V[:, :, t0:t0 + n_b], kc, vc)
        out = cache.extend(cu(qb), cu(K[:, :, t0:t0 + n_b]), cu(V[:, :, t0:t0 + n_b]), 0, route=route)
        torch.cuda.synchronize()
        B.check_bar(out.float().cpu().numpy(), _gold_with_sinks(oracle, st, sinks)[0], f"extend route={route} sinks={sink_tokens}")
        for i in range(n_dec2):
            t = t0 + n_b + i
            cache.decoding_with_pages(cu(q2s[i]), cu(K[:, :, t:t + 1]), cu(V[:, :, t:t + 1]), 0)
        st, sinks = _paged_state(cache, oracle, qc, Kc, Vc, kc, vc, b=1)
        assert st["r"] == n_dec2
        o2, l2 = cache.extend_request(1, cu(qc), cu(Kc), cu(Vc), 0, return_lse=True, route=route)
        torch.cuda.synchronize()
        g_out, g_lse = _gold_with_sinks(oracle, st, sinks)
        B.check_bar(o2.float().cpu().numpy(), g_out, f"extend_request route={route} sinks={sink_tokens}")
        B.check_lse(l2.cpu().numpy(), g_lse, f"extend_request route={route} sinks={sink_tokens}")
        twins.append(cache)
        outs.append((out.float().cpu().numpy(), o2.float().cpu().numpy()))
    _same_cache_state(torch, *twins)
    B.check_bar(outs[1][0], outs[0][0], "extend: blocks vs chunk route", rel_tol=2e-3, mae_tol=2e-3)
    B.check_bar(outs[1][1], outs[0][1], "extend_request: blocks vs chunk route", rel_tol=2e-3, mae_tol=2e-3)
    with pytest.raises(ValueError, match="route"):
        twins[0].extend(cu(qb), cu(K[:, :, :n_b]), cu(V[:, :, :n_b]), 0, route="torch")


@pytest.mark.parametrize("nbits", [8, 10])
def test_dynamic_cache_extend_by_blocks(nbits, env, oracle):
    torch, ops = env
    from million_amd.pq_cache import DynamicPQCache
    cu = lambda a: _cu(torch, a)
    d, M, C, n_a, n_dec, n_b = 128, 64, 2 ** nbits, 200, 6 if nbits == 8 else 0, 50
    rs_ = np.random.RandomState(42 + nbits)
    f = lambda *s: rs_.standard_normal(s).astype(np.float16)
    kc, vc = f(M, C, d // M), f(M, C, d // M)
    K, V = f(1, NH_K, n_a + n_dec + n_b, d), f(1, NH_K, n_a + n_dec + n_b, d)
    qa, q1s, qb = f(1, NH, n_a, d), f(max(n_dec, 1), 1, NH, 1, d), f(1, NH, n_b, d)
    twins, outs = [], []
    for route in (None, "blocks"):
        cache = DynamicPQCache(bs=1, nh=NH, num_key_value_heads=NH_K, M=M, layer_num=1, d=d, nbits=nbits, max_tokens=1024, device="cuda")
        cache.set_cent(cu(kc), cu(vc))
        cache.prefill(cu(qa), cu(K[:, :, :n_a]), cu(V[:, :, :n_a]), 0)
        for i in range(n_dec):      # (the fused decode kernels are uint8-only: the uint16 cache extends straight behind its prompt)
            cache.decoding(cu(q1s[i]), cu(K[:, :, n_a + i:n_a + i + 1]), cu(V[:, :, n_a + i:n_a + i + 1]), 0)
        T, r = cache._T[0], cache.residualed_tokens[0]
        assert (T, r) == (n_a, n_dec)
        k_res, v_res = cache.key_residual_cache[0].cpu().numpy(), cache.value_residual_cache[0].cpu().numpy()
        t0 = n_a + n_dec
        st = dict(q=qb, k_codes=cache._k_store[0][:, :, :T].cpu().numpy(), v_codes=cache._v_store[0][:, :, :T].cpu().numpy(), k_cents=kc,
                  v_cents=vc, k_res=k_res, v_res=v_res, r=r, rs=0, k_win=k_res[:, :, :r], v_win=v_res[:, :, :r],
                  k_ch=K[:, :, t0:t0 + n_b], v_ch=V[:, :, t0:t0 + n_b])
        out = cache.extend(cu(qb), cu(K[:, :, t0:t0 + n_b]), cu(V[:, :, t0:t0 + n_b]), 0, route=route)
        torch.cuda.synchronize()
        B.check_bar(out.float().cpu().numpy(), B.route_ref(oracle, st)[0], f"dynamic nbits={nbits} route={route}")
        assert (cache._T[0], cache.residualed_tokens[0], cache.seen_tokens[0]) == (t0 + n_b, 0, t0 + n_b)
        twins.append(cache)
        outs.append(out.float().cpu().numpy())
    a, b = twins
    assert torch.equal(a._k_store[0], b._k_store[0]) and torch.equal(a._v_store[0], b._v_store[0])
    B.check_bar(outs[1], outs[0], f"dynamic nbits={nbits}: blocks vs chunk route", rel_tol=2e-3, mae_tol=2e-3)
