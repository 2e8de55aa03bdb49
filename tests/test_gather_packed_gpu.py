"""ops.pq_gather_rows(packed=True) (csrc/gather_rows.hip, million_pq_gather_rows_packed) on the GPU: a token range dequantised
straight from packed 10- / 12-bit pages, then the window rows in ring order.  Everything is bit for bit: against ops.pq_gather_rows
over the uint16 pools of the same codes, against oracle.pq_decode of the live codes followed by the ring rows, and against a
poisoned twin in which every byte of both planes that belongs to no token of [t0, t1) is 0xFF.  The rows of the destination behind
the written ones keep their NaN pre-fill.  Packed pools are built by the numpy model of the format (tests/packed_model.py)."""
import numpy as np
import pytest

from tests import chunk_blocks_model as B
from tests import packed_model as P

pytestmark = pytest.mark.gpu

BS, NH_K, T, CAP = 2, 2, 300, 64
ROWS_CAP = T + CAP + 5
# (d, M, C, page size): all eight (d, d / M, h) combinations, one page size each
FORMS = [(128, 64, 1024, 64), (128, 64, 4096, 32), (128, 32, 512, 128), (128, 32, 2048, 64),
         (64, 32, 1024, 32), (64, 32, 2048, 128), (64, 16, 512, 64), (64, 16, 4096, 32)]
FORM_IDS = [f"d{d}-M{M}-C{C}-ps{ps}" for d, M, C, ps in FORMS]
# [t0, t1): unaligned to pages and to the 64-row tile; nothing coded (window rows only); a whole store
RANGES = [(37, 167), (120, 120), (0, 300)]
RINGS = [(50, 37), (0, 0)]      # (resid_start, r): a ring of 64 that wraps, and no window


@pytest.fixture(scope="module")
def env():
    import torch
    from million_amd import build, ops
    build.build()
    assert torch.cuda.is_available()
    return torch, ops


def _inputs(d, M, C):
    rs = np.random.RandomState(M * 1000 + C + d)
    f = lambda *s: rs.standard_normal(s).astype(np.float16)
    return dict(k_codes=rs.randint(0, C, (BS, NH_K, T, M)).astype(np.uint16), v_codes=rs.randint(0, C, (BS, NH_K, T, M)).astype(np.uint16),
                k_cents=f(M, C, d // M), v_cents=f(M, C, d // M), k_res=f(BS, NH_K, CAP, d), v_res=f(BS, NH_K, CAP, d))


def _poisoned(inp, ids, n_pool, ps, M, C, t0, t1):
    """Packed pools of 0xFF bytes holding the tokens [t0, t1) of every (request, kv head) only."""
    pools = []
    for side, codes in (("k", inp["k_codes"]), ("v", inp["v_codes"])):
        pool = np.full((n_pool, P.page_bytes(ps, M, C)), 0xFF, np.uint8)
        for b in range(BS):
            for h in range(NH_K):
                P.store(pool, side, ids[b, h], t0, codes[b, h, t0:t1], ps, M, C)
        pools.append(pool)
    return pools


def _nan_out(torch, d, rows=ROWS_CAP, bs=BS):
    return torch.full((bs, NH_K, rows, d), float("nan"), dtype=torch.float16, device="cuda")


def _bits(t):
    import torch
    return t.view(torch.int16).cpu().numpy().view(np.uint16)


@pytest.mark.parametrize("d,M,C,ps", FORMS, ids=FORM_IDS)
def test_packed_gather_is_the_uint16_gather(env, oracle, d, M, C, ps):
    torch, ops = env
    cu = lambda a: torch.from_numpy(np.ascontiguousarray(a)).cuda()
    inp = _inputs(d, M, C)
    assert inp["k_codes"].max() >= 256 and inp["v_codes"].max() >= 256
    k_cents, v_cents = cu(inp["k_cents"]), cu(inp["v_cents"])
    kpool, vpool, ids = B.to_pools(inp["k_codes"], inp["v_codes"], ps)
    g_ids = cu(ids)
    wide_pools = cu(kpool), cu(vpool)
    clean_pools = cu(P.pack(kpool, "k", C)), cu(P.pack(vpool, "v", C))
    for t0, t1 in RANGES:
        for rs, r in RINGS:
            n = (t1 - t0) + r
            want = [B.gather_ref(oracle, inp[s + "_codes"], inp[s + "_cents"], inp[s + "_res"], t0, t1, r, rs).view(np.uint16) for s in ("k", "v")]
            k_res, v_res = inp["k_res"].copy(), inp["v_res"].copy()
            dead = np.setdiff1d(np.arange(CAP), (rs + np.arange(r)) % CAP)
            k_res[:, :, dead] = v_res[:, :, dead] = np.nan      # window rows outside the ring span
            kw = dict(t0=t0, t1=t1, k_res=cu(k_res), v_res=cu(v_res), r=r, resid_start=rs, k_page_ids=g_ids, v_page_ids=g_ids, page_size=ps)
            got = {}
            dirty_ids = ids.copy()
            dirty_ids[:, :, (t1 + ps - 1) // ps:] = ids[0, 0, -1]      # entries past the range name an unused page: 0xFF
            runs = (("wide", wide_pools, {}, kw), ("clean", clean_pools, {"packed": True}, kw),
                    ("dirty", tuple(cu(p) for p in _poisoned(inp, ids, kpool.shape[0], ps, M, C, t0, t1)), {"packed": True},
                     dict(kw, k_page_ids=cu(dirty_ids), v_page_ids=cu(dirty_ids))))
            for name, pools, flag, kws in runs:
                k_out, v_out = _nan_out(torch, d), _nan_out(torch, d)
                assert ops.pq_gather_rows(pools[0], pools[1], k_cents, v_cents, k_out, v_out, **kws, **flag) == n
                torch.cuda.synchronize()
                assert torch.isnan(k_out[:, :, n:]).all() and torch.isnan(v_out[:, :, n:]).all(), f"{name}: rows past {n} were written"
                got[name] = (_bits(k_out)[:, :, :n], _bits(v_out)[:, :, :n])
            what = f"[{t0}, {t1}) ring ({rs}, {r})"
            for i, side in enumerate("KV"):
                assert np.array_equal(got["wide"][i], want[i]), f"{side} {what}: the uint16 gather is not pq_decode, then the ring"
                assert np.array_equal(got["clean"][i], got["wide"][i]), f"{side} {what}: packed differs from uint16"
                assert np.array_equal(got["dirty"][i], got["clean"][i]), f"{side} {what}: bytes outside [t0, t1) reached the rows"


def test_the_index_rule_on_the_raw_field(env):
    """C = 512 keeps one unused bit in a 2-bit field, C = 2048 one in a 4-bit field: a raw field >= C indexes entry 0, as
    million_pq_gather_rows does with the uint16 word the unpack launch makes of it."""
    torch, ops = env
    for d, M, C, ps in ((128, 64, 512, 64), (64, 16, 2048, 32)):
        rs = np.random.RandomState(C)
        n_pool, npg = 5, 4
        raw = rs.randint(0, 2 * C, (n_pool, ps, M)).astype(np.uint16)      # every field value of 8 + h bits
        assert raw.max() >= C
        pk, pv = P.pack(raw, "k", C), P.pack(np.ascontiguousarray(raw.transpose(0, 2, 1)), "v", C)
        cents = torch.from_numpy(rs.standard_normal((M, C, d // M)).astype(np.float16)).cuda()
        ids = torch.from_numpy(rs.permutation(n_pool)[:npg].astype(np.int32).reshape(1, 1, npg)).cuda()
        gk, gv = torch.from_numpy(pk).cuda(), torch.from_numpy(pv).cuda()
        outs = []
        for pools, flag in (((gk, gv), {"packed": True}),
                            ((ops.pq_unpack_pages(gk, side="k", page_size=ps, M=M, C=C), ops.pq_unpack_pages(gv, side="v", page_size=ps, M=M, C=C)), {})):
            k_out = torch.zeros(1, 1, npg * ps, d, dtype=torch.float16, device="cuda")
            v_out = torch.zeros_like(k_out)
            ops.pq_gather_rows(pools[0], pools[1], cents, cents, k_out, v_out, t0=0, t1=npg * ps, k_page_ids=ids, v_page_ids=ids, page_size=ps, **flag)
            outs.append((k_out, v_out))
        torch.cuda.synchronize()
        assert torch.equal(outs[0][0].view(torch.int16), outs[1][0].view(torch.int16)) and torch.equal(outs[0][1].view(torch.int16), outs[1][1].view(torch.int16))
        assert torch.equal(outs[0][0].view(torch.int16), outs[0][1].view(torch.int16)) and outs[0][0].any()


def test_far_pages(env, oracle):
    """Page ids on both sides of byte 2^32 of packed pools past 4 GiB: the rows of the compact twin, bit for bit (the skip is
    tests/test_packed_gpu.py::test_decode_far_pages')."""
    torch, ops = env
    from tests.test_big_address_gpu import NEED_FREE
    free = torch.cuda.mem_get_info()[0]
    if free < NEED_FREE:
        pytest.skip(f"{free / 2 ** 30:.1f} GiB of device memory free, the far pools want {NEED_FREE >> 30} GiB")
    d, M, C, ps = 128, 64, 1024, 64
    cu = lambda a: torch.from_numpy(np.ascontiguousarray(a)).cuda()
    inp = _inputs(d, M, C)
    kpool, vpool, ids = B.to_pools(inp["k_codes"], inp["v_codes"], ps)
    compact = cu(P.pack(kpool, "k", C)), cu(P.pack(vpool, "v", C))
    pb = P.page_bytes(ps, M, C)
    hi_id = 2 ** 32 // pb
    npg = ids.shape[2]                                       # 5 live pages and one entry behind them
    far = np.zeros_like(ids)
    for i in range(BS * NH_K):      # every row: pages below byte 2^32, the one that straddles it, pages past it
        far.reshape(-1, npg)[i] = [7 + i, hi_id - 1 - i, hi_id + i, hi_id + 8 + i, hi_id + 16 + i, 2][:npg]
    n_far = hi_id + 32
    live = npg - 1
    assert len(set(far[:, :, :live].reshape(-1).tolist())) == BS * NH_K * live and far.max() < n_far
    big = [torch.full((n_far, pb), 0xA5, dtype=torch.uint8, device="cuda") for _ in range(2)]
    assert big[0].numel() > 2 ** 32
    src, dst = cu(ids[:, :, :live].reshape(-1).astype(np.int64)), cu(far[:, :, :live].reshape(-1).astype(np.int64))
    for b_, c_ in zip(big, compact):
        b_[dst] = c_[src]
    k_cents, v_cents = cu(inp["k_cents"]), cu(inp["v_cents"])
    t0, t1 = 37, 300
    got = []
    for pools, tab in ((compact, cu(ids)), (big, cu(far))):
        k_out, v_out = _nan_out(torch, d), _nan_out(torch, d)
        ops.pq_gather_rows(pools[0], pools[1], k_cents, v_cents, k_out, v_out, t0=t0, t1=t1, k_page_ids=tab, v_page_ids=tab, page_size=ps, packed=True)
        torch.cuda.synchronize()
        got.append((_bits(k_out), _bits(v_out)))
    assert np.array_equal(got[0][0], got[1][0]) and np.array_equal(got[0][1], got[1][1])
    want = B.gather_ref(oracle, inp["k_codes"], inp["k_cents"], inp["k_res"], t0, t1, 0, 0).view(np.uint16)
    assert np.array_equal(got[0][0][:, :, :t1 - t0], want)
    del big
    torch.cuda.empty_cache()
