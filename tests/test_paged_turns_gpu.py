"""million_amd.paged_turns on the GPU: extend / extend_request for a PagedPQCache with nbits 9 .. 12, packed beside its unpacked twin.

One life - prefill, decode across a flush, extend, decode, extend_request of every slot (one by blocks), extend of one row.  Every
output of the packed cache is bitwise its twin's; the twin's is within the project's bar (tests/test_chunk_wide_gpu.py) of the fp64
model over oracle.pq_encode's codes of all earlier coded rows and the fp16 window rows.  At the end the pools hold
oracle.pq_encode of the whole sequence and every length is what prefill() of the whole sequence leaves."""
import numpy as np
import pytest

from tests import chunk_wide_model as CM
from tests import packed_model as P
from tests.test_chunk_wide_gpu import same_bits, within_bar

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def env():
    import torch
    from million_amd import build, ops
    build.build()
    assert torch.cuda.is_available()
    return torch, ops


@pytest.mark.parametrize("nbits,M", [(10, 64), (12, 32)])
def test_a_life_beside_the_unpacked_twin(env, oracle, nbits, M):
    torch, ops = env
    from million_amd import paged_turns
    from million_amd.pq_cache import PagedPQCache
    bs, nh, nhk, d, ps, cap, nl = 2, 8, 2, 128, 32, 64, 2
    C = 2 ** nbits
    n_prompt, n_dec1, n_ext1, n_dec2, n_req, n_last = 50, cap + 2, 5, 3, 70, 1
    n_all = n_prompt + n_dec1 + n_ext1 + n_dec2 + n_req + n_last
    rs = np.random.RandomState(nbits)
    h = lambda *s: rs.standard_normal(s).astype(np.float16)
    g = lambda a: torch.from_numpy(np.ascontiguousarray(a)).cuda()
    ck, cv = h(M, C, d // M), h(M, C, d // M)
    K, V, Q = h(nl, bs, nhk, n_all, d), h(nl, bs, nhk, n_all, d), h(nl, bs, nh, n_all, d)
    Kc, Vc = [oracle.pq_encode(K[l], ck) for l in range(nl)], [oracle.pq_encode(V[l], cv) for l in range(nl)]
    assert Kc[0].dtype == np.uint16 and Kc[0].max() >= 256 and Vc[0].max() >= 256
    geom = dict(bs=bs, nh=nh, num_key_value_heads=nhk, M=M, layer_num=nl, d=d, page_size=ps, extended_residual_size=cap, max_tokens=512,
                nbits=nbits, dtype=torch.uint16, device="cuda")
    packed, twin = PagedPQCache(**geom, packed=True), PagedPQCache(**geom)
    for c in (packed, twin):
        c.set_cent(g(ck), g(cv))
    assert packed.key_page_pool.dtype == torch.uint8 and twin.key_page_pool.dtype == torch.uint16

    def model(l, sl, t0, n, decode=False):
        """fp64 attention of the rows [t0, t0 + n) of layer l (requests sl) over the twin's state BEFORE they are stored: the codes of
        its T tokens, its window rows (tokens T .. T + r, in ring order from row 0 of the model's ring), the rows themselves.  A
        decode step on a full window first flushes its oldest page of rows into codes (oracle.PagedPolicy)."""
        b0 = sl.start or 0
        T, r = int(twin._T_a[l, b0]), int(twin._r_a[l, b0])
        assert T + r == t0
        if decode and r >= cap:
            T, r = T + ps, r - ps
        k_res, v_res = np.zeros((bs, nhk, cap, d), np.float16)[sl], np.zeros((bs, nhk, cap, d), np.float16)[sl]
        k_res[:, :, :r], v_res[:, :, :r] = K[l][sl, :, T:t0], V[l][sl, :, T:t0]
        return CM.chunk_attn(Q[l][sl, :, t0:t0 + n], Kc[l][sl, :, :T], Vc[l][sl, :, :T], ck, cv, k_res, v_res, r,
                             k_chunk=K[l][sl, :, t0:t0 + n], v_chunk=V[l][sl, :, t0:t0 + n])[0]

    def both(what, l, sl, t0, n, fn, decode=False):
        """fn(cache) on the packed cache and on its twin: the same bits, and the twin within the bar of the model."""
        ref = model(l, sl, t0, n, decode)
        outs = [fn(c) for c in (packed, twin)]
        torch.cuda.synchronize()
        if isinstance(outs[0], tuple):
            assert same_bits(outs[0][1], outs[1][1]), what
            outs = [o[0] for o in outs]
        assert same_bits(outs[0], outs[1]), what
        within_bar(outs[1], ref, what)

    every = slice(None)
    rows = lambda a, l, sl, t0, n: g(a[l][sl, :, t0:t0 + n])

    def decode(t0, n):
        for t in range(t0, t0 + n):
            for l in range(nl):
                both(f"decode {t} layer {l}", l, every, t, 1,
                     lambda c: c.decoding_with_pages(rows(Q, l, every, t, 1), rows(K, l, every, t, 1), rows(V, l, every, t, 1), l, return_lse=True),
                     decode=True)

    t = 0
    for l in range(nl):      # 1. the prompt
        both(f"prefill layer {l}", l, every, 0, n_prompt,
             lambda c: paged_turns.extend(c, rows(Q, l, every, 0, n_prompt), rows(K, l, every, 0, n_prompt), rows(V, l, every, 0, n_prompt), l))
    t += n_prompt
    decode(t, n_dec1)        # 2. decode across a flush
    t += n_dec1
    assert int(twin._T_a[0, 0]) == n_prompt + ps and int(twin._r_a[0, 0]) == n_dec1 - ps and int(twin._rs_a[0, 0]) == ps      # flushed once
    for l in range(nl):      # 3. extend 5: codes, a window that does not start at row 0, the chunk
        with pytest.raises(NotImplementedError, match="nbits"):
            packed.extend(rows(Q, l, every, t, n_ext1), rows(K, l, every, t, n_ext1), rows(V, l, every, t, n_ext1), l)
        with pytest.raises(NotImplementedError, match="nbits"):
            twin.extend_request(0, rows(Q, l, slice(0, 1), t, n_ext1), rows(K, l, slice(0, 1), t, n_ext1), rows(V, l, slice(0, 1), t, n_ext1), l)
        both(f"extend {n_ext1} layer {l}", l, every, t, n_ext1,
             lambda c: paged_turns.extend(c, rows(Q, l, every, t, n_ext1), rows(K, l, every, t, n_ext1), rows(V, l, every, t, n_ext1), l))
    t += n_ext1
    assert int(twin._T_a[0, 0]) == t and int(twin._r_a[0, 0]) == 0
    decode(t, n_dec2)        # 4. decode behind it
    t += n_dec2
    for l in range(nl):      # 5. every slot on its own: slot 0 by the chunk route with lse, slot 1 by blocks
        for b, kw in ((0, dict(return_lse=True)), (1, dict(route="blocks"))):
            sl = slice(b, b + 1)
            both(f"extend_request slot {b} layer {l} {kw}", l, sl, t, n_req,
                 lambda c: paged_turns.extend_request(c, b, rows(Q, l, sl, t, n_req), rows(K, l, sl, t, n_req), rows(V, l, sl, t, n_req), l, **kw))
    t += n_req
    for l in range(nl):      # 6. one more row, in lockstep again, by blocks
        both(f"extend 1 layer {l}", l, every, t, n_last,
             lambda c: paged_turns.extend(c, rows(Q, l, every, t, 1), rows(K, l, every, t, 1), rows(V, l, every, t, 1), l, route="blocks"))
    t += n_last
    assert t == n_all
    torch.cuda.synchronize()

    # ---- the state: what prefill of the whole sequence leaves ----
    whole = PagedPQCache(**geom, packed=True)
    whole.set_cent(g(ck), g(cv))
    for l in range(nl):
        whole.prefill(g(Q[l]), g(K[l]), g(V[l]), l)
    torch.cuda.synchronize()
    for a, b_, w in zip(packed.host_state(), twin.host_state(), whole.host_state()):
        assert np.array_equal(a, b_) and np.array_equal(a, w)
    live = -(-n_all // ps)
    for l in range(nl):
        assert packed.lengths[l].cpu().tolist() == twin.lengths[l].cpu().tolist() == whole.lengths[l].cpu().tolist() == [[n_all, 0, 0, 0]] * bs
        ids = packed.page_ids[l].cpu().numpy()
        assert np.array_equal(ids, twin.page_ids[l].cpu().numpy())
        tok = np.arange(n_all)
        for side, pp, tp, want in (("k", packed.key_page_pool, twin.key_page_pool, Kc[l]), ("v", packed.value_page_pool, twin.value_page_pool, Vc[l])):
            got = P.unpack(pp.cpu().numpy(), side, ps, M, C)
            tw = tp.view(torch.int16).cpu().numpy().view(np.uint16)
            for b in range(bs):
                for hk in range(nhk):
                    assert len(set(ids[b, hk, :live].tolist())) == live
                    pages, off = ids[b, hk, tok // ps], tok % ps
                    a, b_ = (got[pages, off], tw[pages, off]) if side == "k" else (got[pages, :, off], tw[pages, :, off])
                    assert np.array_equal(a, b_) and np.array_equal(a, want[b, hk]), (l, side, b, hk)
    assert ops.tail_faults() == 0
