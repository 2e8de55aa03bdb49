"""GPU tests of the one-launch flush and ragged store of wide code pages, at op level: million_pq_flush_wide through
ops.pq_flush_wide and million_pq_store_ragged_wide through ops.pq_store_ragged_wide, uint16 pages and packed pages.

Everything is compared bit for bit.  The pages of the written tokens hold oracle.pq_encode of the very source rows, in the order
of the numpy rule (tests/ragged_wide_common.py FlushPlan, tests/store_ragged_model.py Plan); every other pool byte still holds the
0xA5 it was filled with (packed pools: byte for byte against tests/packed_model.py's stores, and through ops.pq_unpack_pages);
window rows and new rows the rule does not read hold NaN; lengths rows are the rule's integers with word 3 untouched.
Geometry: 3 requests, 2 kv heads, pages of 32 tokens, a window of 64 rows, tables of 512 tokens; (d, M, nbits) = (128, 64, 10),
(128, 32, 12), (64, 32, 9), each as uint16 and packed: d_m 2 / 4, 2 / 4 high bits."""
import numpy as np
import pytest

from tests import ragged_wide_common as R
from tests import store_ragged_model as SM

pytestmark = pytest.mark.gpu

BS, NHK, PS, CAP, NPC = R.BS, R.NHK, R.PS, R.CAP, R.NPC
FLUSH_ROWS = [(45, 64, 40), (70, 64, 0), (33, 17, 5)]      # {T, r, start}: 0 wraps its ring and straddles pages 1 / 2, 2 takes no part
N_NEW, N_BOUND = [5, 0, 40], 40
CASES = [f + (p,) for f in R.FORMATS for p in (False, True)]
WORD3 = 0x7EADBEEF


@pytest.fixture(scope="module")
def env():
    import torch
    assert torch.cuda.is_available(), "GPU tests need an MI355X"
    from million_amd import build, ops, _lib
    build.build()
    _lib.load()
    return torch, ops, _lib


class Scene:
    """Windows, new rows, codebooks and a shuffled page table over a pool with three pages no entry names."""

    def __init__(self, seed, d, M, nbits, packed):
        rs = np.random.RandomState(seed)
        f = lambda *s: rs.standard_normal(s).astype(np.float16)
        self.d, self.M, self.C, self.packed = d, M, 2 ** nbits, packed
        self.k_win, self.v_win, self.k_new, self.v_new = f(BS, NHK, CAP, d), f(BS, NHK, CAP, d), f(BS, NHK, N_BOUND, d), f(BS, NHK, N_BOUND, d)
        self.k_cents, self.v_cents = f(M, self.C, d // M), f(M, self.C, d // M)
        self.n_pool = BS * NHK * NPC + 3
        self.ids = rs.permutation(self.n_pool)[:BS * NHK * NPC].reshape(BS, NHK, NPC).astype(np.int32)

    def tensors(self, torch, win_read, new_read=None):
        """Device tensors.  win_read[b]: the window rows of request b the call may read (the others hold NaN); new_read[b]: how
        many of its new rows (the others hold NaN)."""
        k_win, v_win, k_new, v_new = self.k_win.copy(), self.v_win.copy(), self.k_new.copy(), self.v_new.copy()
        for b in range(BS):
            dead = np.setdiff1d(np.arange(CAP), np.asarray(win_read[b], dtype=np.int64))
            k_win[b, :, dead] = v_win[b, :, dead] = np.float16("nan")
            if new_read is not None:
                k_new[b, :, new_read[b]:] = v_new[b, :, new_read[b]:] = np.float16("nan")
        pools = R.fill_pools(self.n_pool, self.M, self.C, self.packed)
        dev = lambda a: R.to_dev(torch, a)
        return dict(k_win=dev(k_win), v_win=dev(v_win), k_new=dev(k_new), v_new=dev(v_new), kc=dev(self.k_cents), vc=dev(self.v_cents),
                    k_pool=dev(pools[0]), v_pool=dev(pools[1]), ids=dev(self.ids))

    def encode(self, oracle, k_rows, v_rows):
        """oracle.pq_encode of one request's source rows (nh_k, rows, d), with codes >= 256 on both sides."""
        kc, vc = oracle.pq_encode(k_rows[None], self.k_cents)[0], oracle.pq_encode(v_rows[None], self.v_cents)[0]
        assert kc.dtype == np.uint16 and (kc >= 256).any() and (vc >= 256).any()
        return kc, vc

    def check_pools(self, torch, ops, t, want, what):
        """The device pools against the numpy pools `want`, byte for byte; packed pools also through ops.pq_unpack_pages."""
        for side, got, exp in (("k", t["k_pool"], want[0]), ("v", t["v_pool"], want[1])):
            g = R.to_np(torch, got)
            assert np.array_equal(g, exp), f"{what}: {side} pool differs in {int((g != exp).sum())} places"
            if self.packed:
                from tests import packed_model as P
                un = R.to_np(torch, ops.pq_unpack_pages(got, side=side, page_size=PS, M=self.M, C=self.C))
                assert np.array_equal(un, P.unpack(exp, side, PS, self.M, self.C)), f"{what}: {side} pool, unpacked"


def _flush_expect(sc, oracle, rows, n, min_r):
    plans = [R.FlushPlan(row, n, min_r) for row in rows]
    want = R.fill_pools(sc.n_pool, sc.M, sc.C, sc.packed)
    for b, p in enumerate(plans):
        if p.live:
            kc, vc = sc.encode(oracle, sc.k_win[b][:, p.ring], sc.v_win[b][:, p.ring])
            R.put(want, sc.ids[b], p.tokens, p.kept, kc, vc, sc.M, sc.C, sc.packed)
    return plans, want


def _flush(torch, ops, sc, t, rows, n, min_r):
    lengths = torch.tensor([list(r) + [WORD3] for r in rows], dtype=torch.int32).cuda()
    ops.pq_flush_wide(t["k_win"], t["v_win"], t["kc"], t["vc"], t["k_pool"], t["v_pool"], t["ids"], n=n, page_size=PS,
                      dev_lengths=lengths, min_r=min_r, packed=sc.packed)
    torch.cuda.synchronize()
    return lengths.cpu().numpy()


@pytest.mark.parametrize("d,M,nbits,packed", CASES)
def test_flush_of_a_ragged_batch(d, M, nbits, packed, env, oracle):
    """One launch over the three requests, min_r = 64, 32 rows: requests 0 and 1 flush (0 out of a wrapped ring into pages 1 and
    2), request 2 takes no part - its window is NaN from end to end, its row and pages stay."""
    torch, ops, L = env
    sc = Scene(d + M + nbits, d, M, nbits, packed)
    plans, want = _flush_expect(sc, oracle, FLUSH_ROWS, PS, CAP)
    assert [p.live for p in plans] == [True, True, False] and plans[0].ring[-1] < plans[0].ring[0] and plans[0].tokens[0] // PS != plans[0].tokens[-1] // PS
    t = sc.tensors(torch, [p.ring if p.live else [] for p in plans])
    lengths = _flush(torch, ops, sc, t, FLUSH_ROWS, PS, CAP)
    sc.check_pools(torch, ops, t, want, "flush")
    for b, p in enumerate(plans[:2]):      # the codes each request reaches through its table
        got = R.codes_of([R.to_np(torch, t["k_pool"]), R.to_np(torch, t["v_pool"])], sc.ids[b], p.T, p.T + PS, M, sc.C, packed)
        exp = sc.encode(oracle, sc.k_win[b][:, p.ring], sc.v_win[b][:, p.ring])
        assert np.array_equal(got[0], exp[0]) and np.array_equal(got[1], exp[1]), b
    assert lengths.tolist() == [[77, 32, 8, WORD3], [102, 32, 32, WORD3], [33, 17, 5, WORD3]]


@pytest.mark.parametrize("d,M,nbits,packed", CASES)
def test_host_length_form_writes_what_two_encode_launches_write(d, M, nbits, packed, env, oracle):
    """dev_lengths=None: every request flushes 32 rows from ring row 40 on to tokens [45, 77) - the pages of two
    pq_encode_into[_packed] launches from the same start, and the oracle's."""
    torch, ops, L = env
    sc = Scene(3 * d + M + nbits, d, M, nbits, packed)
    rows = [(45, CAP, 40)] * BS
    plans, want = _flush_expect(sc, oracle, rows, PS, 0)
    t = sc.tensors(torch, [p.ring for p in plans])
    ref_k, ref_v = t["k_pool"].clone(), t["v_pool"].clone()
    kw = dict(token_start=45, n=PS, page_ids=t["ids"], page_size=PS, x_row_start=40, x_row_mod=CAP)
    enc = ops.pq_encode_into_packed if packed else ops.pq_encode_into
    enc(t["k_win"], t["kc"], ref_k, layout=L.MILLION_CODES_KPAGES, **kw)
    enc(t["v_win"], t["vc"], ref_v, layout=L.MILLION_CODES_VPAGES, **kw)
    ops.pq_flush_wide(t["k_win"], t["v_win"], t["kc"], t["vc"], t["k_pool"], t["v_pool"], t["ids"], n=PS, page_size=PS,
                      token_start=45, x_row_start=40, packed=packed)
    torch.cuda.synchronize()
    assert np.array_equal(R.to_np(torch, t["k_pool"]), R.to_np(torch, ref_k)) and np.array_equal(R.to_np(torch, t["v_pool"]), R.to_np(torch, ref_v))
    sc.check_pools(torch, ops, t, want, "host-length flush")


HOSTILE = [[(R.INT_MAX, 64, 0), (100, -5, 3), (50, 64, 70)],       # T far past the table; r < 0: no part; start >= cap reads as 0
           [(R.CAP_TOK - 10, 64, 0), (R.CAP_TOK, 64, 0), (-7, 100, -1)]]      # the last 22 tokens past the table; all of them; T < 0, r > cap, start < 0
HOSTILE_AFTER = [[[512, 32, 32], [100, -5, 3], [82, 32, 32]], [[512, 32, 32], [512, 32, 32], [32, 32, 32]]]


@pytest.mark.parametrize("which", [0, 1])
@pytest.mark.parametrize("packed", [False, True])
def test_flush_device_lengths_are_clamped_not_trusted(which, packed, env, oracle):
    """Rows no cache would write: they are clamped as load_len_row clamps them, a token past the table drops its store, and
    nothing outside the table is written - the whole pool is the rule's, the 0xA5 bytes included."""
    torch, ops, L = env
    d, M, nbits = R.FORMATS[which]
    sc = Scene(17 + which, d, M, nbits, packed)
    rows = HOSTILE[which]
    plans, want = _flush_expect(sc, oracle, rows, PS, CAP)
    assert [p.live for p in plans] == ([True, False, True] if which == 0 else [True, True, True])
    assert [int(p.kept.sum()) for p in plans if p.live] == ([0, 32] if which == 0 else [10, 0, 32])
    t = sc.tensors(torch, [p.ring if p.live else [] for p in plans])
    lengths = _flush(torch, ops, sc, t, rows, PS, CAP)
    sc.check_pools(torch, ops, t, want, "hostile flush")
    assert lengths[:, :3].tolist() == HOSTILE_AFTER[which] == [list(p.after) for p in plans] and (lengths[:, 3] == WORD3).all()


# ---------------------------------------------------------------- the ragged store ---------------------------------------------
GEOM = dict(page_size=PS, n_pages_cap=NPC, resid_cap=CAP, n_bound=N_BOUND)


def _store_expect(sc, oracle, rows):
    plans = SM.plans(rows, **GEOM)
    want = R.fill_pools(sc.n_pool, sc.M, sc.C, sc.packed)
    for b, p in enumerate(plans):
        if p.live:
            kc, vc = sc.encode(oracle, p.rows_of(sc.k_win[b], sc.k_new[b]), p.rows_of(sc.v_win[b], sc.v_new[b]))
            R.put(want, sc.ids[b], p.tokens, p.kept, kc, vc, sc.M, sc.C, sc.packed)
    return plans, want


def _store(torch, ops, sc, plans, rows):
    t = sc.tensors(torch, [[(p.start + j) % CAP for j in range(p.r)] if p.live else [] for p in plans], [p.n if p.live else 0 for p in plans])
    lengths = torch.tensor([list(r[:3]) + [WORD3] for r in rows], dtype=torch.int32).cuda()
    dev_n = torch.tensor([r[3] for r in rows], dtype=torch.int32).cuda()
    ops.pq_store_ragged_wide(t["k_new"], t["v_new"], t["k_win"], t["v_win"], t["kc"], t["vc"], t["k_pool"], t["v_pool"], t["ids"],
                             lengths, dev_n, M=sc.M, C=sc.C, page_size=PS, packed=sc.packed)
    torch.cuda.synchronize()
    assert dev_n.tolist() == [r[3] for r in rows], "dev_n is read, never written"
    return t, lengths.cpu().numpy()


@pytest.mark.parametrize("d,M,nbits,packed", CASES)
def test_store_ragged_wide_against_the_rule(d, M, nbits, packed, env, oracle):
    """The three requests with n_new = [5, 0, 40]: 0 stores its wrapped window and 5 rows behind T = 45, 1 takes no part, 2 its
    17 window rows and 40 new rows behind T = 33."""
    torch, ops, L = env
    sc = Scene(5 * d + M + nbits, d, M, nbits, packed)
    rows = [r + (n,) for r, n in zip(FLUSH_ROWS, N_NEW)]
    plans, want = _store_expect(sc, oracle, rows)
    assert [(p.live, len(p.src)) for p in plans] == [(True, 69), (False, 0), (True, 57)]
    t, lengths = _store(torch, ops, sc, plans, rows)
    sc.check_pools(torch, ops, t, want, "store")
    assert np.array_equal(lengths, SM.advance([list(r[:3]) + [WORD3] for r in rows], N_NEW, **GEOM))
    assert lengths.tolist() == [[114, 0, 0, WORD3], [70, 64, 0, WORD3], [90, 0, 0, WORD3]]


@pytest.mark.parametrize("packed", [False, True])
def test_store_ragged_wide_untrusted_values_are_clamped(packed, env, oracle):
    """Every clamp at once; a T far past the table; a request whose last rows lie past it."""
    torch, ops, L = env
    d, M, nbits = R.FORMATS[1]
    sc = Scene(23, d, M, nbits, packed)
    rows = [(-5, 1000, 64, 1000), (10 ** 9, -3, -1, 5), (R.CAP_TOK - 12, 0, 0, 20)]
    plans, want = _store_expect(sc, oracle, rows)
    assert [(p.T, p.r, p.start, p.n) for p in plans] == [(0, 64, 0, 40), (512, 0, 0, 5), (500, 0, 0, 20)]
    assert [int(p.kept.sum()) for p in plans] == [104, 0, 12]
    t, lengths = _store(torch, ops, sc, plans, rows)
    sc.check_pools(torch, ops, t, want, "hostile store")
    assert lengths.tolist() == [[104, 0, 0, WORD3], [512, 0, 0, WORD3], [512, 0, 0, WORD3]]


# ---------------------------------------------------------------- every writer of wide pages ----------------------------------
WRITER_SHAPES = [(64, 16, 10), (64, 32, 12)]      # d_m 4 with 2 high bits, d_m 2 with 4: the two combinations R.FORMATS does not hold


@pytest.mark.parametrize("packed", [False, True])
@pytest.mark.parametrize("d,M,nbits", WRITER_SHAPES)
def test_four_writers_one_page_image(d, M, nbits, packed, env, oracle):
    """The token store of wide pages is written once (csrc/code_pages.h) and has four users.  The same 32 source rows - ring rows
    40 .. 7 of every request's window - go to tokens [45, 77), across pages 1 and 2, through each: two pq_encode_into[_packed]
    launches, pq_flush_wide in its host-length form, pq_store_ragged_wide with r = 0 (the rows handed in as new rows) and, for packed
    pools, pq_pack_pages of the uint16 pools a flush wrote.  Every pool is the oracle's codes inside 0xA5 fill, byte for byte."""
    torch, ops, L = env
    sc = Scene(7 * d + M + nbits, d, M, nbits, packed)
    plans, want = _flush_expect(sc, oracle, [(45, CAP, 40)] * BS, PS, 0)
    ring = plans[0].ring
    assert ring[0] == 40 and ring[-1] == 7 and plans[0].tokens[0] // PS == 1 and plans[0].tokens[-1] // PS == 2
    t = sc.tensors(torch, [ring] * BS)
    fresh = lambda: [R.to_dev(torch, a) for a in R.fill_pools(sc.n_pool, M, sc.C, packed)]
    images = {}

    k, v = images["encode"] = fresh()
    kw = dict(token_start=45, n=PS, page_ids=t["ids"], page_size=PS, x_row_start=40, x_row_mod=CAP)
    enc = ops.pq_encode_into_packed if packed else ops.pq_encode_into
    enc(t["k_win"], t["kc"], k, layout=L.MILLION_CODES_KPAGES, **kw)
    enc(t["v_win"], t["vc"], v, layout=L.MILLION_CODES_VPAGES, **kw)

    k, v = images["flush"] = fresh()
    flush = dict(n=PS, page_size=PS, token_start=45, x_row_start=40)
    ops.pq_flush_wide(t["k_win"], t["v_win"], t["kc"], t["vc"], k, v, t["ids"], packed=packed, **flush)

    k, v = images["ragged store"] = fresh()
    lengths = torch.tensor([[45, 0, 0, WORD3]] * BS, dtype=torch.int32).cuda()
    dev_n = torch.full((BS,), PS, dtype=torch.int32).cuda()
    ops.pq_store_ragged_wide(R.to_dev(torch, sc.k_win[:, :, ring]), R.to_dev(torch, sc.v_win[:, :, ring]), None, None, t["kc"], t["vc"],
                             k, v, t["ids"], lengths, dev_n, M=M, C=sc.C, page_size=PS, packed=packed)

    if packed:
        # uint16 pools whose packed image is the 0xA5 fill, flushed into, then packed
        from tests import packed_model as P
        k, v = (R.to_dev(torch, P.unpack(a, side, PS, M, sc.C)) for a, side in zip(R.fill_pools(sc.n_pool, M, sc.C, True), "kv"))
        ops.pq_flush_wide(t["k_win"], t["v_win"], t["kc"], t["vc"], k, v, t["ids"], packed=False, **flush)
        images["pack"] = [ops.pq_pack_pages(k, side="k", C=sc.C), ops.pq_pack_pages(v, side="v", C=sc.C)]
    torch.cuda.synchronize()
    assert lengths.tolist() == [[77, 0, 0, WORD3]] * BS
    for who, (k, v) in images.items():
        for side, got, exp in (("k", k, want[0]), ("v", v, want[1])):
            g = R.to_np(torch, got)
            assert g.shape == exp.shape and np.array_equal(g, exp), f"{who}: {side} pool differs in {int((g != exp).sum())} places"
