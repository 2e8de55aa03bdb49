"""ops.pq_chunk_attn_packed (csrc/chunk_attn_wide.hip, million_pq_chunk_attn_packed) on the GPU: chunk attention over packed 10- /
12-bit code pages, against ops.pq_chunk_attn_wide over uint16 pools that hold the same codes - bit for bit, out and lse - and the
uint16 result against the fp64 model of tests/chunk_wide_model.py at the project's bar (tests/test_chunk_wide_gpu.py).

The packed pools are built on the host by the numpy model of the format (tests/packed_model.py) from the uint16 pools
Case.tensors makes: P.pack of the whole pools, or - poison - P.store of the live tokens into pools of 0xFF bytes."""
import numpy as np
import pytest

from tests import chunk_wide_model as CM
from tests import packed_model as P
from tests.test_chunk_wide_gpu import ALONE, RAGGED_ROWS, Case, same_bits, splits, within_bar

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def env():
    import torch
    from million_amd import build, ops
    build.build()
    assert torch.cuda.is_available()
    return torch, ops


def u16(t):
    import torch
    return t.view(torch.int16).cpu().numpy().view(np.uint16)


def packed(torch, c, t, poison=False):
    """Case.tensors(k="paged", v="paged") -> the same tensors with k_codes / v_codes the packed pools of the same codes.  poison:
    every byte of both planes that is not a live token's is 0xFF (page tails, pages nobody names, pages named past the live ones)."""
    ps = t["kw"]["page_size"]
    kp, vp = u16(t["k_codes"]), u16(t["v_codes"])          # (n, ps, M), (n, M, ps)
    if not poison:
        pk, pv = P.pack(kp, "k", c.C), P.pack(vp, "v", c.C)
    else:
        ids = t["kw"]["k_page_ids"].cpu().numpy()
        Ts = t["lengths"].cpu().numpy()[:, 0]
        pk = np.full((kp.shape[0], P.page_bytes(ps, c.M, c.C)), 0xFF, np.uint8)
        pv = pk.copy()
        for b, T in enumerate(Ts):
            for h in range(c.nhk):
                tok = np.arange(T)
                pages, off = ids[b, h, tok // ps], tok % ps
                P.store(pk, "k", ids[b, h], 0, kp[pages, off], ps, c.M, c.C)
                P.store(pv, "v", ids[b, h], 0, vp[pages, :, off], ps, c.M, c.C)
    tp = dict(t)
    tp["k_codes"], tp["v_codes"] = torch.from_numpy(pk).cuda(), torch.from_numpy(pv).cuda()
    return tp


class _PackedOps:
    """Case.run calls ops.pq_chunk_attn_wide: this hands it the packed entry."""

    def __init__(self, ops):
        self.pq_chunk_attn_wide = ops.pq_chunk_attn_packed


# ---------------------------------------------------------------- 1. the matrix ---------------------------------------------
# (d, M, C, G, n_q, T, window, chunk, page size, int64 ids): all eight (d, d / M, h) combinations; every row on an edge - T = 0, 1, a
# tile edge (63, 65), a page tail (1000), S > 1 (4097) - one / two query blocks, an empty / plain / wrapped window, with / without chunk
MATRIX = [
    (128, 64, 1024, 4, 3, 1000, "17", True, 64, False),
    (128, 64, 4096, 8, 1, 4097, "wrap", False, 32, True),
    (128, 32, 512, 1, 65, 63, "0", True, 32, False),
    (128, 32, 2048, 8, 257, 1, "17", True, 128, True),
    (64, 32, 1024, 4, 65, 65, "wrap", True, 64, False),
    (64, 32, 2048, 4, 257, 1000, "wrap", False, 128, False),
    (64, 16, 512, 1, 1, 0, "17", True, 64, True),
    (64, 16, 4096, 8, 3, 4097, "0", True, 128, False),
]
ROW_IDS = [f"d{r[0]}-M{r[1]}-C{r[2]}-G{r[3]}-nq{r[4]}-T{r[5]}-w{r[6]}-{'chunk' if r[7] else 'past'}-ps{r[8]}" for r in MATRIX]
_cases = {}


def matrix_case(i):
    if i not in _cases:
        d, M, C, G, n_q, T, win, chunk = MATRIX[i][:8]
        c = Case(d, M, C, G, [(T, win, n_q)] * (2 if n_q <= 3 else 1), chunk, seed=40 + i)
        _cases[i] = (c, c.model())
    return _cases[i]


@pytest.mark.parametrize("i", range(len(MATRIX)), ids=ROW_IDS)
def test_matrix_bitwise_against_the_uint16_launch(env, i):
    torch, ops = env
    c, (ref, ref_l) = matrix_case(i)
    assert c.live_codes_are_wide()
    ps, i64 = MATRIX[i][8:]
    t = c.tensors(torch, ops, k="paged", v="paged", ps=ps, i64=i64)
    wide, wide_l = c.run(torch, ops, t)
    out, lse = c.run(torch, _PackedOps(ops), packed(torch, c, t))
    assert same_bits(out, wide) and same_bits(lse, wide_l)
    within_bar(wide, ref, ROW_IDS[i])
    CM.lse_error(wide_l.cpu().numpy(), ref_l)
    if MATRIX[i][5] or MATRIX[i][6] != "0" or MATRIX[i][7]:
        assert out.any()


@pytest.mark.parametrize("i", [1, 4], ids=[ROW_IDS[1], ROW_IDS[4]])
def test_out_with_lse_is_out_without(env, i):
    torch, ops = env
    c, _ = matrix_case(i)
    ps, i64 = MATRIX[i][8:]
    t = packed(torch, c, c.tensors(torch, ops, k="paged", v="paged", ps=ps, i64=i64))
    with_lse, _ = c.run(torch, _PackedOps(ops), t)
    without, none = c.run(torch, _PackedOps(ops), t, lse=False)
    assert none is None and same_bits(with_lse, without) and with_lse.any()


# ---------------------------------------------------------------- 2. poison --------------------------------------------------
@pytest.mark.parametrize("C", [1024, 2048])
@pytest.mark.parametrize("form", ["lockstep", "ragged"])
def test_poison_moves_no_bit(env, form, C):
    """The same live data inside zeros and inside poison: 0xFF in every byte of both planes outside the live tokens (page tails,
    unused pages, table entries past the live pages naming such pages), NaN window rows outside the ring span, NaN q and chunk
    rows past dev_n_q[b], the codebooks at the front of 65536-entry NaN allocations, NaN out / lse and a 0xFF workspace.  At
    C = 2048 the top bit of a 4-bit field is no part of a code: 0xFF sets it in dead bytes only."""
    torch, ops = env
    rows = RAGGED_ROWS if form == "ragged" else [(1000, "wrap", 5)] * 2
    c = Case(128, 64, C, 4, rows, True, seed=51)
    assert c.live_codes_are_wide()
    ragged = form == "ragged"
    lay = dict(k="paged", v="paged", ps=32, big_cents=True)
    pops = _PackedOps(ops)
    t_clean = c.tensors(torch, ops, **lay)
    clean = c.run(torch, pops, packed(torch, c, t_clean), ragged=ragged)
    t_dirty = packed(torch, c, c.tensors(torch, ops, poison=True, **lay), poison=True)
    pool = t_dirty["k_codes"]
    assert int((pool == 0xFF).all(dim=1).sum()) >= 3      # the spare pages, named past the live ones
    dirty = c.run(torch, pops, t_dirty, ragged=ragged, poison=True)
    assert torch.isfinite(dirty[0]).all() and not torch.isnan(dirty[1]).any(), "poison reached the output"
    assert same_bits(clean[0], dirty[0]) and same_bits(clean[1], dirty[1])
    wide = c.run(torch, ops, t_clean, ragged=ragged)
    assert same_bits(clean[0], wide[0]) and same_bits(clean[1], wide[1])
    within_bar(wide[0], c.model()[0], f"{form} clean")


# ---------------------------------------------------------------- 3. ragged equals alone -------------------------------------
@pytest.mark.parametrize("form", list(ALONE))
def test_ragged_equals_alone(env, form):
    """tests/test_chunk_wide_gpu.py's rows (the split count of each request alone is the ragged launch's): three and more requests
    at different (T, window, n_q) in one launch; each request's rows are bitwise its batch-1 call, the rows past dev_n_q zeros / -inf."""
    torch, ops = env
    rows = ALONE[form]
    c = Case(128, 32, 2048, 4, rows, True, seed=53)
    for b, (T, _, _) in enumerate(rows):
        assert splits(1, 2, 5, 4, T) == splits(len(rows), 2, 5, 4, c.Tb) or rows[b][2] == 0
    lay = dict(k="paged", v="paged", ps=32)
    pops = _PackedOps(ops)
    out, lse = c.run(torch, pops, packed(torch, c, c.tensors(torch, ops, poison=True, **lay), poison=True), ragged=True, poison=True)
    for b, (T, win, nq) in enumerate(rows):
        assert not out[b, :, nq:].any() and torch.isneginf(lse[b, :, nq:]).all(), b
        if nq == 0:
            continue
        one = Case.__new__(Case)
        one.__dict__.update(c.__dict__)
        one.n_q = nq
        one.q, one.k_ch, one.v_ch = c.q[:, :, :nq], c.k_ch[:, :, :nq], c.v_ch[:, :, :nq]
        o1, l1 = one.run(torch, pops, packed(torch, one, one.tensors(torch, ops, only=b, **lay)))
        assert same_bits(out[b:b + 1, :, :nq], o1) and same_bits(lse[b:b + 1, :, :nq], l1), b
        assert o1.any()


def test_graph_replay_follows_the_lengths(env):
    """One captured ragged call replayed after dev_lengths / dev_n_q changed: bitwise a fresh packed call and a fresh uint16 call
    at the same rows."""
    torch, ops = env
    c = Case(128, 32, 4096, 4, [(1000, "full", 5)] * 2, True, seed=57)
    t = c.tensors(torch, ops, k="paged", v="paged", ps=64)
    tp = packed(torch, c, t)
    states = [[(63, 5, 0, 5), (1000, 0, 0, 3)], [(65, 64, 40, 2), (1000, 17, 3, 5)], [(128, 0, 0, 0), (936, 64, 63, 5)]]
    S = splits(2, 2, 5, 4, 1000)
    ws = torch.empty(2 * 2 * S * 5 * 4 * (128 + 2) * 4, dtype=torch.uint8, device="cuda")
    out = torch.zeros(2, 5, c.nh, 128, dtype=torch.float16, device="cuda").transpose(1, 2)
    lse = torch.zeros(2, c.nh, 5, dtype=torch.float32, device="cuda")
    lengths, n_q = t["lengths"].clone(), t["n_q"].clone()

    def call(fn, src, **kw):
        return fn(t["q"], t["k_ch"], t["v_ch"], src["k_codes"], src["v_codes"], t["k_tab"], t["v_tab"], t["k_res"], t["v_res"], 0,
                  M=c.M, C=c.C, n_tokens=1000, dev_lengths=lengths, dev_n_q=n_q, **kw, **t["kw"])

    call(ops.pq_chunk_attn_packed, tp, workspace=ws, out=out, lse=lse)      # eager once: module load
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        call(ops.pq_chunk_attn_packed, tp, workspace=ws, out=out, lse=lse)
    for rows in states:
        lengths.copy_(torch.tensor([[T, r, s, 0] for T, r, s, _ in rows], dtype=torch.int32))
        n_q.copy_(torch.tensor([r[3] for r in rows], dtype=torch.int32))
        out.fill_(float("nan"))
        lse.fill_(float("nan"))
        g.replay()
        torch.cuda.synchronize()
        fresh = call(ops.pq_chunk_attn_packed, tp, return_lse=True)
        wide = call(ops.pq_chunk_attn_wide, t, return_lse=True)
        torch.cuda.synchronize()
        assert same_bits(out, fresh[0]) and same_bits(lse, fresh[1]), rows
        assert same_bits(out, wide[0]) and same_bits(lse, wide[1]), rows
        ref, _ = CM.chunk_attn(c.q, c.k_codes, c.v_codes, c.k_cents, c.v_cents, c.k_res, c.v_res, [r[1] for r in rows],
                               T=[r[0] for r in rows], start=[r[2] for r in rows], k_chunk=c.k_ch, v_chunk=c.v_ch, n_q=[r[3] for r in rows])
        within_bar(out, ref, f"replay {rows}")
        for b, r in enumerate(rows):
            assert not out[b, :, r[3]:].any()


# ---------------------------------------------------------------- 4. far pages -----------------------------------------------
def test_far_pages(env):
    """Page ids on both sides of byte 2^32 of packed pools past 4 GiB, bitwise against the compact twin.  A packed page is no
    power of two bytes: a page offset kept in 32 bits wraps to a page of 0xA5 bytes - valid memory, wrong codes.  The free-memory
    skip is tests/test_packed_gpu.py::test_decode_far_pages'."""
    torch, ops = env
    from tests.test_big_address_gpu import NEED_FREE
    free = torch.cuda.mem_get_info()[0]
    if free < NEED_FREE:
        pytest.skip(f"{free / 2 ** 30:.1f} GiB of device memory free, the far pools want {NEED_FREE >> 30} GiB")
    ps, T = 64, 5 * 64 + 9
    c = Case(128, 64, 1024, 4, [(T, "17", 3)], True, seed=59)
    t = c.tensors(torch, ops, k="paged", v="paged", ps=ps)
    tp = packed(torch, c, t)
    pb = P.page_bytes(ps, c.M, c.C)
    ids = t["kw"]["k_page_ids"].cpu().numpy()                # (1, nhk, 7): 6 live pages and one entry behind them
    hi_id = 2 ** 32 // pb
    n_far = hi_id + 16
    far = np.zeros_like(ids)
    for h in range(c.nhk):      # below byte 2^32, the page that straddles it, pages past it
        far[0, h] = [3 + h, hi_id - 2 - h, hi_id + h, hi_id + 4 + h, hi_id + 8 + h, hi_id + 12 + h, 1]
    assert len(set(far[0, :, :6].reshape(-1).tolist())) == 2 * 6 and far.max() < n_far
    big = [torch.full((n_far, pb), 0xA5, dtype=torch.uint8, device="cuda") for _ in range(2)]
    assert big[0].numel() > 2 ** 32
    src, dst = torch.from_numpy(ids[0, :, :6].reshape(-1).astype(np.int64)).cuda(), torch.from_numpy(far[0, :, :6].reshape(-1).astype(np.int64)).cuda()
    for b_, c_ in zip(big, (tp["k_codes"], tp["v_codes"])):
        b_[dst] = c_[src]
    twin, twin_l = c.run(torch, _PackedOps(ops), tp)
    tf = dict(tp)
    tf["k_codes"], tf["v_codes"] = big
    tab = torch.from_numpy(far.astype(np.int32)).cuda()
    tf["kw"] = dict(tp["kw"], k_page_ids=tab, v_page_ids=tab)
    got, got_l = c.run(torch, _PackedOps(ops), tf)
    assert same_bits(got, twin) and same_bits(got_l, twin_l)
    within_bar(twin, c.model()[0], "far pages twin")
    del big, tf
    torch.cuda.empty_cache()
