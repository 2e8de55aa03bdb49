"""Packed code pages on the GPU (include/million_hip.h, "Packed code pages"): the encoder's packed store and the
repack launch against the numpy model of tests/packed_model.py, byte for byte; ops.pq_decode_attn_packed against
ops.pq_decode_attn_wide over uint16 pools that hold the same codes, bit for bit, and against the fp64 model at the project's bar;
poisoned memory; a packed PagedPQCache beside its unpacked twin; page ids on both sides of byte 2^32 of a packed pool.
Shapes, inputs and bar are those of tests/test_attn_wide_gpu.py."""
import numpy as np
import pytest

from tests import lse_ref as R
from tests import packed_model as P
from tests.test_attn_wide_gpu import MAIN, M32, SHAPES, Store, bits, within_bar

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def env():
    import torch
    from million_amd import build, ops
    build.build()
    assert torch.cuda.is_available()
    return torch, ops


def packed_pools(s, fill=0):
    """The store's uint16 pools (Store.pools) packed by the model, on the device."""
    kp, vp = s.pools(fill)
    if fill:      # every byte of both planes outside the live tokens: the poison of a packed pool is 0xFF bytes
        pk, pv = np.full((s.n_pool, P.page_bytes(s.ps, s.M, s.C)), 0xFF, np.uint8), np.full((s.n_pool, P.page_bytes(s.ps, s.M, s.C)), 0xFF, np.uint8)
        for b in range(s.bs):
            for h in range(s.nhk):
                P.store(pk, "k", s.ids[b, h], 0, s.k_codes[b, h], s.ps, s.M, s.C)
                P.store(pv, "v", s.ids[b, h], 0, s.v_codes[b, h], s.ps, s.M, s.C)
    else:
        pk, pv = P.pack(kp, "k", s.C), P.pack(vp, "v", s.C)
    return s.torch.from_numpy(pk).cuda(), s.torch.from_numpy(pv).cuda()


def run_packed(s, ops, pools, T, r, start=0, *, append=False, n_tokens=None, dev=None, **kw):
    """Store.run through ops.pq_decode_attn_packed over the packed pools."""
    g = s.g
    if append:
        kw.update(k_new=g["k_new"], v_new=g["v_new"])
    return ops.pq_decode_attn_packed(g["q"], pools[0], pools[1], g["k_cents"], g["v_cents"], g["k_res"], g["v_res"], r,
                                     n_tokens=T if n_tokens is None else n_tokens, page_ids=g["ids"], page_size=s.ps, resid_start=start,
                                     dev_lengths=dev, **kw)


def splits(s, ops, pools, T, r, packed):
    g = s.g
    desc = ops.wide_attn_desc("test", g["q"], pools[0], pools[1], g["k_cents"], g["v_cents"], g["k_res"], g["v_res"], r, T, g["ids"], s.ps, 0,
                              None, packed)
    return ops.attn_wide_splits(desc)


# --------------------------------------------------------------------------------------------------------------- 1. encode ---
class EncCase:
    """X rows, a codebook, the oracle's codes of the rows (once per shape), shuffled page ids over a pool with spare pages."""

    def __init__(self, torch, oracle, d, M, C, ps, bs=2, nhk=2, rows=130, tok_max=64 + 130):
        rs = np.random.RandomState(d + M + C + ps)
        self.d, self.M, self.C, self.ps, self.bs, self.nhk = d, M, C, ps, bs, nhk
        self.X = rs.standard_normal((bs, nhk, rows, d)).astype(np.float16)
        self.cents = rs.standard_normal((M, C, d // M)).astype(np.float16)
        self.codes = oracle.pq_encode(self.X, self.cents)
        assert self.codes.dtype == np.uint16 and self.codes.max() >= 256
        self.npc = -(-tok_max // ps) + 1
        self.n_pool = bs * nhk * self.npc + 3
        self.ids = rs.permutation(self.n_pool)[:bs * nhk * self.npc].reshape(bs, nhk, self.npc).astype(np.int32)
        self.pb = P.page_bytes(ps, M, C)
        self.gX, self.gcents, self.gids = (torch.from_numpy(a).cuda() for a in (self.X, self.cents, self.ids))
        self.pool = torch.empty(self.n_pool, self.pb, dtype=torch.uint8, device="cuda")

    def want(self, side, tok0, rows):
        """The model: the same 0xA5 pool with the oracle's codes of source rows `rows[b]` stored from token tok0[b] on."""
        pool = np.full((self.n_pool, self.pb), 0xA5, np.uint8)
        for b in range(self.bs):
            for h in range(self.nhk):
                P.store(pool, side, self.ids[b, h], tok0[b], self.codes[b, h][rows[b]], self.ps, self.M, self.C)
        return pool


@pytest.mark.parametrize("d,M,C,ps,G,cap", SHAPES)
def test_encode_packed_whole_pool(env, oracle, d, M, C, ps, G, cap):
    torch, ops = env
    from million_amd import _lib as L
    c = EncCase(torch, oracle, d, M, C, ps)
    for n in (1, 3, 64, 130):
        for tok0 in (0, 1, 41, 63, 64):
            for side, layout in (("k", L.MILLION_CODES_KPAGES), ("v", L.MILLION_CODES_VPAGES)):
                c.pool.fill_(0xA5)
                ops.pq_encode_into_packed(c.gX, c.gcents, c.pool, layout=layout, token_start=tok0, n=n, page_ids=c.gids, page_size=ps)
                want = c.want(side, [tok0] * c.bs, [np.arange(n)] * c.bs)
                assert np.array_equal(c.pool.cpu().numpy(), want), (side, n, tok0)


@pytest.mark.parametrize("d,M,C,ps,G,cap", [MAIN, M32, SHAPES[4]])
def test_encode_packed_ring_source_and_device_lengths(env, oracle, d, M, C, ps, G, cap):
    """The source as a ring of 130 rows read from row 100 on (the flush's form), then the destination token and the ring start
    of every request read from its device row: request 0 and request 1 at different tokens and ring starts."""
    torch, ops = env
    from million_amd import _lib as L
    c = EncCase(torch, oracle, d, M, C, ps)
    ring, n = 130, 64
    for side, layout in (("k", L.MILLION_CODES_KPAGES), ("v", L.MILLION_CODES_VPAGES)):
        c.pool.fill_(0xA5)
        ops.pq_encode_into_packed(c.gX, c.gcents, c.pool, layout=layout, token_start=41, n=n, page_ids=c.gids, page_size=ps, x_row_start=100, x_row_mod=ring)
        rows = (100 + np.arange(n)) % ring
        assert np.array_equal(c.pool.cpu().numpy(), c.want(side, [41, 41], [rows, rows])), side
        dev = torch.tensor([[63, 64, 7, 0], [1, 64, 129, 0]], dtype=torch.int32, device="cuda")
        c.pool.fill_(0xA5)
        ops.pq_encode_into_packed(c.gX, c.gcents, c.pool, layout=layout, token_start=0, n=n, page_ids=c.gids, page_size=ps, x_row_mod=ring, dev_lengths=dev)
        assert np.array_equal(c.pool.cpu().numpy(), c.want(side, [63, 1], [(7 + np.arange(n)) % ring, (129 + np.arange(n)) % ring])), side
        assert dev.cpu().tolist() == [[63, 64, 7, 0], [1, 64, 129, 0]]      # read, not advanced
        # a destination past the page table drops its stores (the clamp of million_pq_encode), and nothing else is touched
        cap_tok = c.npc * ps
        dev2 = torch.tensor([[cap_tok - 3, 0, 0, 0], [2 ** 31 - 1, 0, 0, 0]], dtype=torch.int32, device="cuda")
        c.pool.fill_(0xA5)
        ops.pq_encode_into_packed(c.gX, c.gcents, c.pool, layout=layout, token_start=0, n=n, page_ids=c.gids, page_size=ps, dev_lengths=dev2)
        want = np.full((c.n_pool, c.pb), 0xA5, np.uint8)
        for h in range(c.nhk):
            P.store(want, side, c.ids[0, h], cap_tok - 3, c.codes[0, h][:3], ps, M, C)
        assert np.array_equal(c.pool.cpu().numpy(), want), side


# --------------------------------------------------------------------------------------------------------------- 2. repack ---
@pytest.mark.parametrize("d,M,C,ps,G,cap", SHAPES)
def test_repack(env, d, M, C, ps, G, cap):
    torch, ops = env
    rs = np.random.RandomState(C + ps)
    for side, shape in (("k", (37, ps, M)), ("v", (37, M, ps))):
        pages = rs.randint(0, C, shape).astype(np.uint16)
        pages.reshape(-1)[:2] = (C - 1, 0)
        g = torch.from_numpy(pages).cuda()
        packed = ops.pq_pack_pages(g, side=side, C=C)
        assert packed.dtype == torch.uint8 and tuple(packed.shape) == (37, ops.packed_page_bytes(ps, M, C))
        assert np.array_equal(packed.cpu().numpy(), P.pack(pages, side, C)), side
        back = ops.pq_unpack_pages(packed, side=side, page_size=ps, M=M, C=C)
        assert back.dtype == torch.uint16 and np.array_equal(back.cpu().numpy(), pages), side
        # into a caller's buffer, which holds something else before
        out = torch.full_like(packed, 0xA5)
        assert ops.pq_pack_pages(g, side=side, C=C, out=out) is out and torch.equal(out, packed)


# --------------------------------------------------------------------------------------------------------------- 3. decode ---
@pytest.mark.parametrize("d,M,C,ps,G,cap", SHAPES)
def test_matrix_bitwise_against_the_uint16_pools(env, d, M, C, ps, G, cap):
    torch, ops = env
    s = Store(torch, d, M, C, ps, G, cap=cap)
    pk = packed_pools(s)
    n = 0
    for T in (0, 1, ps - 1, ps, ps + 1, 1029):
        for r in (0, 1, 17, cap):
            start = cap - 5 if r > 5 else (3 if r else 0)
            assert s.live_codes_are_wide(T)
            assert splits(s, ops, pk, T, r, True) == splits(s, ops, (s.g["k_pool"], s.g["v_pool"]), T, r, False) >= 1
            wide, wide_l = s.run(ops, T, r, start, return_lse=True)
            out, lse = run_packed(s, ops, pk, T, r, start, return_lse=True)
            assert np.array_equal(bits(out), bits(wide)) and torch.equal(lse, wide_l), (T, r)
            if T == 0 and r == 0:
                assert not out.any() and torch.isneginf(lse).all()
                continue
            ref, ref_l = s.model(T, r, start)
            within_bar(out, ref, f"packed d{d} M{M} C{C} ps{ps} G{G} T{T} r{r}")
            assert np.abs(lse.cpu().numpy()[:, :, 0] - ref_l).max() < R.LSE_TOL
            n += 1
    assert n == 23


@pytest.mark.parametrize("d,M,C,ps,G,cap", [MAIN, M32])
def test_splits_bitwise(env, d, M, C, ps, G, cap):
    torch, ops = env
    T = 4133
    s = Store(torch, d, M, C, ps, G, bs=1, T_max=T, cap=cap, seed=2)
    pk = packed_pools(s)
    assert splits(s, ops, pk, T, 33, True) == splits(s, ops, (s.g["k_pool"], s.g["v_pool"]), T, 33, False) >= 2
    a, b = run_packed(s, ops, pk, T, 33, 7), s.run(ops, T, 33, 7)
    assert np.array_equal(bits(a), bits(b))
    within_bar(a, s.model(T, 33, 7)[0], f"packed splits d{d} M{M} C{C}")


@pytest.mark.parametrize("use_dev", [False, True])
@pytest.mark.parametrize("d,M,C,ps,G,cap", [MAIN, SHAPES[4]])
def test_fused_append_bitwise(env, d, M, C, ps, G, cap, use_dev):
    torch, ops = env
    s = Store(torch, d, M, C, ps, G, cap=cap, seed=4)
    pk = packed_pools(s)
    T, r, st = 333, 17, cap - 5
    row = (st + r) % cap
    before = {nm: s.g[nm].clone() for nm in ("k_res", "v_res")}
    mk_dev = lambda: torch.tensor([[T, r, st, 0]] * s.bs, dtype=torch.int32, device="cuda") if use_dev else None
    kw = lambda dev: dict(n_tokens=512, dev=dev) if use_dev else {}
    dev_w = mk_dev()
    wide, wide_l = s.run(ops, T, r, st, append=True, return_lse=True, **kw(dev_w))
    after_wide = {nm: s.g[nm].clone() for nm in ("k_res", "v_res")}
    for nm in before:
        s.g[nm].copy_(before[nm])
    dev_p = mk_dev()
    out, lse = run_packed(s, ops, pk, T, r, st, append=True, return_lse=True, **kw(dev_p))
    assert np.array_equal(bits(out), bits(wide)) and torch.equal(lse, wide_l)
    for nm in before:
        assert torch.equal(s.g[nm], after_wide[nm])
    assert torch.equal(s.g["k_res"][:, :, row], s.g["k_new"][:, :, 0]) and torch.equal(s.g["v_res"][:, :, row], s.g["v_new"][:, :, 0])
    if use_dev:
        assert dev_p.cpu().tolist() == dev_w.cpu().tolist() == [[T, r + 1, st, 0]] * s.bs
    ref, ref_l = s.model(T, r, st, append=True)
    within_bar(out, ref, "packed fused append")
    assert np.abs(lse.cpu().numpy()[:, :, 0] - ref_l).max() < R.LSE_TOL


def test_captured_launch_follows_the_lengths(env):
    """One launch with the fused append and device lengths, captured; replayed after the lengths moved (a longer context, another
    ring position): bitwise the eager wide call at the same lengths."""
    torch, ops = env
    d, M, C, ps, G, cap = MAIN
    s = Store(torch, d, M, C, ps, G, cap=cap, seed=9)
    pk = packed_pools(s)
    bound = 1088
    dev = torch.tensor([[333, 17, 3, 0], [64, 0, 0, 0]], dtype=torch.int32, device="cuda")
    ws = torch.zeros(ops.decode_wide_workspace_bytes(s.g["q"], s.g["k_res"], M=M, C=C, page_size=ps), dtype=torch.uint8, device="cuda")
    out, lse = torch.empty_like(s.g["q"]), torch.empty(s.bs, s.nh, 1, dtype=torch.float32, device="cuda")
    res0 = {nm: s.g[nm].clone() for nm in ("k_res", "v_res")}      # (the warm-up and every replay append a row)
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        run_packed(s, ops, pk, 0, 0, 0, append=True, n_tokens=bound, dev=dev, out=out, lse=lse, workspace=ws)      # warm-up, eager
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        run_packed(s, ops, pk, 0, 0, 0, append=True, n_tokens=bound, dev=dev, out=out, lse=lse, workspace=ws)
    for rows in ([[1029, 40, 100, 0], [ps + 1, cap - 1, 5, 0]], [[0, 0, 0, 0], [1029, 17, cap - 5, 0]]):
        for nm in res0:
            s.g[nm].copy_(res0[nm])
        dev.copy_(torch.tensor(rows, dtype=torch.int32))
        graph.replay()
        torch.cuda.synchronize()
        assert dev.cpu().tolist() == [[T, r + 1, st, 0] for T, r, st, _ in rows]
        got, got_l = out.clone(), lse.clone()
        for nm in res0:
            s.g[nm].copy_(res0[nm])
        dev_w = torch.tensor(rows, dtype=torch.int32, device="cuda")
        wide, wide_l = s.run(ops, 0, 0, 0, append=True, n_tokens=bound, dev=dev_w, return_lse=True)
        assert np.array_equal(bits(got), bits(wide)) and torch.equal(got_l, wide_l), rows
        ref, _ = s.model([x[0] for x in rows], [x[1] for x in rows], [x[2] for x in rows], append=True)
        within_bar(got, ref, f"packed, replayed at {rows}")


@pytest.mark.parametrize("d,M,C,ps,G,cap", [MAIN, SHAPES[3]])
def test_out_with_lse_is_out_without(env, d, M, C, ps, G, cap):
    torch, ops = env
    s = Store(torch, d, M, C, ps, G, cap=cap, seed=6)
    pk = packed_pools(s)
    for T, r in ((1029, 17), (0, 5), (ps + 1, 0)):
        out = run_packed(s, ops, pk, T, r, 2)
        out2, lse = run_packed(s, ops, pk, T, r, 2, return_lse=True)
        assert np.array_equal(bits(out), bits(out2)) and np.array_equal(bits(out), bits(s.run(ops, T, r, 2)))
        assert np.abs(lse.cpu().numpy()[:, :, 0] - s.model(T, r, 2)[1]).max() < R.LSE_TOL


# --------------------------------------------------------------------------------------------------------------- 4. poison ---
@pytest.mark.parametrize("d,M,C,ps,G,cap", [MAIN, M32, SHAPES[4], SHAPES[2]])
def test_poison(env, d, M, C, ps, G, cap):
    """tests/test_attn_wide_gpu.py::test_poison over packed pools: 0xFF in both planes past T, in the pages nobody names and in
    the pages named past the live ones, NaN window rows outside the ring, codebooks at the front of NaN-tailed allocations of
    65536 entries: bitwise the clean result.  C = 512 and 2048 leave the top bit of a field unused: 0xFF sets it, the mask drops it."""
    torch, ops = env
    T, r, st = 2 * ps + 5, 17, cap - 5
    s = Store(torch, d, M, C, ps, G, T_max=T, cap=cap, seed=8, cents_alloc=65536)
    assert s.live_codes_are_wide(T) and s.npc == 4
    ring = [(st + i) % cap for i in range(r)]
    dead = [i for i in range(cap) if i not in ring]
    for nm in ("k_res", "v_res"):
        getattr(s, nm)[:, :, dead] = 0
    s.upload(fill=0)
    clean, clean_l = run_packed(s, ops, packed_pools(s), T, r, st, return_lse=True)
    wide, wide_l = s.run(ops, T, r, st, return_lse=True)
    assert np.array_equal(bits(clean), bits(wide)) and torch.equal(clean_l, wide_l)
    within_bar(clean, s.model(T, r, st)[0], f"packed poison (clean) d{d} M{M} C{C}")
    for nm in ("k_res", "v_res"):
        getattr(s, nm)[:, :, dead] = np.nan
    s.upload(fill=0)
    dirty_pools = packed_pools(s, fill=0xFF)
    assert int((dirty_pools[0] == 0xFF).all(dim=1).sum()) >= s.bs * s.nhk + 3      # pages nobody wrote, named past the context
    live_k = dirty_pools[0][int(s.ids[0, 0, 2])].cpu().numpy()      # the last live page: 5 tokens, both planes 0xFF behind them
    h = P.hi_bits(C)
    assert (live_k[5 * M:ps * M] == 0xFF).all() and (live_k[ps * M + 5 * M * h // 8:] == 0xFF).all() and not (live_k[:5 * M] == 0xFF).all()
    dirty, dirty_l = run_packed(s, ops, dirty_pools, T, r, st, return_lse=True)
    assert np.array_equal(bits(clean), bits(dirty)) and torch.equal(clean_l, dirty_l)


# ---------------------------------------------------------------------------------------------------------------- 5. cache ---
@pytest.mark.parametrize("use_dev", [False, True])
@pytest.mark.parametrize("nbits,M", [(10, 64), (12, 32)])
def test_cache_beside_its_unpacked_twin(env, oracle, nbits, M, use_dev):
    torch, ops = env
    from million_amd.pq_cache import PagedPQCache
    # 140 steps behind a prompt of 200 cross the flush at step 129 (the window fills from empty); 60 more cross the one at step 193
    bs, nh, nhk, d, ps, cap, n_prompt, n_dec, nl = 2, 8, 2, 128, 64, 128, 200, 140 + 60, 2
    C = 2 ** nbits
    rs = np.random.RandomState(nbits)
    f = lambda *sh: torch.from_numpy(rs.standard_normal(sh).astype(np.float16)).cuda()
    kc, vc = f(M, C, d // M), f(M, C, d // M)
    K, V, Q = f(nl, bs, nhk, n_prompt + n_dec, d), f(nl, bs, nhk, n_prompt + n_dec, d), f(n_dec, nl, bs, nh, 1, d)
    geom = dict(bs=bs, nh=nh, num_key_value_heads=nhk, M=M, layer_num=nl, d=d, page_size=ps, extended_residual_size=cap, max_tokens=512,
                nbits=nbits, dtype=torch.uint16, device="cuda")
    packed, twin = PagedPQCache(**geom, packed=True), PagedPQCache(**geom)
    h = ops.packed_hi_bits(C)
    for c in (packed, twin):
        c.set_cent(kc, vc)
    for a, b in ((packed.key_page_pool, twin.key_page_pool), (packed.value_page_pool, twin.value_page_pool)):
        assert a.numel() * a.element_size() * 16 == b.numel() * b.element_size() * (8 + h)      # exactly (8 + h) / 16 of the bytes
    qp = f(bs, nh, n_prompt, d)
    for l in range(nl):
        outs = [c.prefill(qp, K[l][:, :, :n_prompt].contiguous(), V[l][:, :, :n_prompt].contiguous(), l) for c in (packed, twin)]
        assert torch.equal(outs[0], outs[1])
    pol = oracle.PagedPolicy(page_size=ps, residual=cap, prefill=n_prompt)
    for i in range(n_dec):
        t = n_prompt + i
        for l in range(nl):
            res = [c.decoding_with_pages(Q[i, l], K[l][:, :, t:t + 1].contiguous(), V[l][:, :, t:t + 1].contiguous(), l, use_dev_lengths=use_dev,
                                         return_lse=True) for c in (packed, twin)]
            assert np.array_equal(bits(res[0][0]), bits(res[1][0])) and torch.equal(res[0][1], res[1][1]), (i, l)
        assert (int(packed._T_a[0, 0]), int(packed._r_a[0, 0])) == pol.step()
    print(f"packed cache: {pol.flushes} flushes in {n_dec} steps")
    assert pol.flushes == 2
    torch.cuda.synchronize()
    for a, b in zip(packed.host_state(), twin.host_state()):
        assert np.array_equal(a, b)
    T = int(packed._T_a[0, 0])
    assert T == n_prompt + pol.flushes * ps and packed._r_a[0, 0] == n_dec - pol.flushes * ps
    live = -(-T // ps)
    for l in range(nl):
        assert torch.equal(packed.lengths[l], twin.lengths[l]) and torch.equal(packed.page_ids[l], twin.page_ids[l])
        assert torch.equal(packed.key_residual_cache[l], twin.key_residual_cache[l]) and torch.equal(packed.value_residual_cache[l], twin.value_residual_cache[l])
        ids = packed.page_ids[l][:, :, :live].reshape(bs * nhk, live).cpu().numpy()
        full = ids[:, :T // ps].reshape(-1)      # the pages every token of which is live
        pools = [(side, pp.cpu().numpy(), tp.cpu().numpy()) for side, pp, tp in (("k", packed.key_page_pool, twin.key_page_pool),
                                                                                  ("v", packed.value_page_pool, twin.value_page_pool))]
        for side, pp, tp in pools:
            assert np.array_equal(pp[full], P.pack(tp[full], side, C)), (l, side)
            # the partial last page: its live tokens are the twin's; the bytes behind them belong to nobody
            last = ids[:, -1]
            got = P.unpack(pp[last], side, ps, M, C)
            want = tp[last]
            n_last = T - (live - 1) * ps
            assert np.array_equal(got[:, :n_last] if side == "k" else got[:, :, :n_last], want[:, :n_last] if side == "k" else want[:, :, :n_last])
    assert packed.pq_cache_size() * 16 == twin.pq_cache_size() * (8 + h)
    assert packed.get_cache_stats()["memory_breakdown"]["cache_memory_mb"] * 16 == twin.get_cache_stats()["memory_breakdown"]["cache_memory_mb"] * (8 + h)
    assert ops.tail_faults() == 0


# -------------------------------------------------------------------------------------------------------- 6. far addresses ---
@pytest.mark.parametrize("d,M,C,ps,G,cap", [MAIN, M32])
def test_decode_far_pages(env, d, M, C, ps, G, cap):
    """One decode through page ids on both sides of byte 2^31 and byte 2^32 of packed pools past 4 GiB, against the compact twin,
    bitwise.  A packed page is no power of two, so the page's offset is a 64-bit multiply: an offset kept in 32 bits wraps to a
    page of 0xA5 bytes - valid, wrong codes.  The free-memory skip is tests/test_big_address_gpu.py's."""
    torch, ops = env
    from tests.test_big_address_gpu import NEED_FREE
    free = torch.cuda.mem_get_info()[0]
    if free < NEED_FREE:
        pytest.skip(f"{free / 2 ** 30:.1f} GiB of device memory free, the far pools want {NEED_FREE >> 30} GiB")
    T = 9 * ps + 5
    s = Store(torch, d, M, C, ps, G, T_max=T, cap=cap, seed=12, spare_pages=0)
    pb = P.page_bytes(ps, M, C)
    compact = packed_pools(s)
    lo_id, hi_id = 2 ** 31 // pb, 2 ** 32 // pb
    n_far = hi_id + 48
    rows = s.bs * s.nhk
    assert s.npc == 11
    # every row: a page below byte 2^31, the pages that straddle or follow both boundaries, pages past byte 2^32
    rs = np.random.RandomState(5)
    far_ids = np.zeros((rows, s.npc), np.int64)
    for i in range(rows):
        picks = [3 + i, lo_id - 1 - i, lo_id + i, lo_id + 8 + i, hi_id - 1 - i, hi_id + i, hi_id + 8 + i, hi_id + 16 + i, hi_id + 24 + i, hi_id + 32 + i, hi_id + 40 + i]
        far_ids[i] = rs.permutation(picks[:s.npc])
    assert len(set(far_ids.reshape(-1).tolist())) == far_ids.size and far_ids.max() < n_far
    assert ((far_ids * pb) % 2 ** 32 // pb != far_ids).any(axis=1).all()      # every row has a page a 32-bit offset would miss
    tab = torch.from_numpy(far_ids.reshape(s.bs, s.nhk, s.npc).astype(np.int32)).cuda()
    big = [torch.full((n_far, pb), 0xA5, dtype=torch.uint8, device="cuda") for _ in range(2)]
    assert big[0].numel() > 2 ** 32
    src = torch.from_numpy(s.ids.reshape(-1).astype(np.int64)).cuda()
    for b_, c_ in zip(big, compact):
        b_[torch.from_numpy(far_ids.reshape(-1)).cuda()] = c_[src]
    r, st = 17, cap - 5
    twin, twin_l = run_packed(s, ops, compact, T, r, st, return_lse=True)
    twin2, _ = run_packed(s, ops, compact, T, r, st, return_lse=True)
    g = s.g
    got, got_l = ops.pq_decode_attn_packed(g["q"], big[0], big[1], g["k_cents"], g["v_cents"], g["k_res"], g["v_res"], r, n_tokens=T, page_ids=tab,
                                           page_size=ps, resid_start=st, return_lse=True)
    torch.cuda.synchronize()
    within_bar(twin, s.model(T, r, st)[0], f"packed far pages twin d{d} M{M} C{C}")
    assert np.array_equal(bits(twin), bits(twin2))
    assert np.array_equal(bits(got), bits(twin)) and torch.equal(got_l, twin_l)
    assert ops.tail_faults() == 0
    del big
    torch.cuda.empty_cache()
