"""GPU tests of million_pq_gather_rows (ops.pq_gather_rows): a token range of every request dequantised straight from its code
store - row-major or paged, per side - followed by its window rows in ring order.  Everything is compared bit for bit: against
oracle.pq_decode of the codes read back through the page table followed by the ring rows, and against a poisoned twin (0xFF
code words past t1, in page tails and in unused pages, table entries past the range naming a poisoned page, NaN window rows
outside the ring); the rows of the destination behind the gathered ones keep their sentinel."""
import numpy as np
import pytest

from tests import chunk_blocks_model as B

pytestmark = pytest.mark.gpu

BS, NH_K, T, T_CAP, CAP = 2, 2, 300, 320, 64
ROWS_CAP = T + CAP + 5
SENTINEL = 0x7BCD      # fp16 bits of the destination before a call
# (code dtype, M, C, d)
FORMS = [(np.uint8, 64, 256, 128), (np.uint8, 32, 128, 64), (np.uint8, 16, 256, 128), (np.uint16, 64, 1024, 128)]
FORM_IDS = ["u8-M64-C256-d128", "u8-M32-C128-d64", "u8-M16-C256-d128", "u16-M64-C1024-d128"]
# (K paged, V paged, page size)
LAYOUTS = [(False, False, 0), (True, True, 32), (True, True, 64), (True, True, 128), (True, False, 64), (False, True, 32)]
LAYOUT_IDS = ["rowmajor", "paged32", "paged64", "paged128", "k-paged64", "v-paged32"]
RANGES = [(0, 0), (37, 171), (64, 128), (0, 300)]
RINGS = [(50, 37), (0, 0)]      # (resid_start, r): a ring of 64 that wraps, and no window


@pytest.fixture(scope="module")
def env():
    import torch
    assert torch.cuda.is_available(), "GPU tests need an MI355X"
    from million_amd import ops, _lib
    _lib.load()
    return torch, ops


def _inputs(dt, M, C, d):
    rs_ = np.random.RandomState(M * 1000 + C + d)
    f = lambda *s: rs_.standard_normal(s).astype(np.float16)
    return dict(k_codes=rs_.randint(0, C, (BS, NH_K, T, M)).astype(dt), v_codes=rs_.randint(0, C, (BS, NH_K, T, M)).astype(dt),
                k_cents=f(M, C, d // M), v_cents=f(M, C, d // M), k_res=f(BS, NH_K, CAP, d), v_res=f(BS, NH_K, CAP, d))


def _stores(inp, k_paged, v_paged, ps, t1, poison):
    """The code stores of one call (numpy): row-major tensors of T_CAP tokens and / or pools with their table.  poison: every
    code word at or past t1, page tails, unused pages hold all-ones; table entries past ceil(t1 / ps) name an unused page."""
    dt = inp["k_codes"].dtype
    ones = np.iinfo(dt).max
    kc, vc = inp["k_codes"].copy(), inp["v_codes"].copy()
    if poison:
        kc[:, :, t1:] = ones
        vc[:, :, t1:] = ones
    st = {}
    if k_paged or v_paged:
        kpool, vpool, ids = B.to_pools(kc, vc, ps, fill=ones if poison else 0)
        if poison:
            ids[:, :, (t1 + ps - 1) // ps:] = ids[0, 0, -1]      # an unused page: all ones
        st.update(kpool=kpool, vpool=vpool, ids=ids)
    pad = np.full((BS, NH_K, T_CAP - T, kc.shape[3]), ones if poison else 0, dt)
    st["k_rm"], st["v_rm"] = np.concatenate([kc, pad], axis=2), np.concatenate([vc, pad], axis=2)
    return st


@pytest.mark.parametrize("k_paged,v_paged,ps", LAYOUTS, ids=LAYOUT_IDS)
@pytest.mark.parametrize("dt,M,C,d", FORMS, ids=FORM_IDS)
def test_gather_is_pq_decode_then_the_ring(dt, M, C, d, k_paged, v_paged, ps, env, oracle):
    torch, ops = env
    cu = lambda a: torch.from_numpy(np.ascontiguousarray(a)).cuda()
    inp = _inputs(dt, M, C, d)
    k_cents, v_cents = cu(inp["k_cents"]), cu(inp["v_cents"])
    clean = _stores(inp, k_paged, v_paged, ps, T, False)
    # what the table says the store holds (the paged sides: read back through it)
    kc, vc = inp["k_codes"], inp["v_codes"]
    if k_paged or v_paged:
        kb, vb = B.from_pools(clean["kpool"], clean["vpool"], clean["ids"], T)
        kc, vc = (kb if k_paged else kc), (vb if v_paged else vc)
        assert np.array_equal(kc, inp["k_codes"]) and np.array_equal(vc, inp["v_codes"])
    for t0, t1 in RANGES:
        for rs, r in RINGS:
            want_k = B.gather_ref(oracle, kc, inp["k_cents"], inp["k_res"], t0, t1, r, rs)
            want_v = B.gather_ref(oracle, vc, inp["v_cents"], inp["v_res"], t0, t1, r, rs)
            n = (t1 - t0) + r
            got = []
            for poison in (False, True):
                st = _stores(inp, k_paged, v_paged, ps, t1, poison)
                k_res, v_res = inp["k_res"].copy(), inp["v_res"].copy()
                if poison:
                    dead = np.setdiff1d(np.arange(CAP), (rs + np.arange(r)) % CAP)
                    k_res[:, :, dead] = np.nan
                    v_res[:, :, dead] = np.nan
                ids = cu(st["ids"]) if (k_paged or v_paged) else None
                k_out = torch.full((BS, NH_K, ROWS_CAP, d), SENTINEL, dtype=torch.int16, device="cuda").view(torch.float16)
                v_out = k_out.clone()
                wrote = ops.pq_gather_rows(cu(st["kpool"] if k_paged else st["k_rm"]), cu(st["vpool"] if v_paged else st["v_rm"]),
                                           k_cents, v_cents, k_out, v_out, t0=t0, t1=t1, k_res=cu(k_res), v_res=cu(v_res), r=r,
                                           resid_start=rs, k_page_ids=ids if k_paged else None, v_page_ids=ids if v_paged else None,
                                           page_size=ps or None)
                torch.cuda.synchronize()
                assert wrote == n
                got.append((k_out.view(torch.int16).cpu().numpy().view(np.uint16), v_out.view(torch.int16).cpu().numpy().view(np.uint16)))
            what = f"[{t0}, {t1}) ring ({rs}, {r})"
            for side, want, (g_clean, g_poison) in (("K", want_k, (got[0][0], got[1][0])), ("V", want_v, (got[0][1], got[1][1]))):
                assert np.array_equal(g_clean[:, :, :n], want.view(np.uint16)), f"{side} {what}: not pq_decode of the codes, then the ring rows"
                assert (g_clean[:, :, n:] == SENTINEL).all(), f"{side} {what}: rows past {n} were written"
                assert np.array_equal(g_clean, g_poison), f"{side} {what}: poison outside the range reached the result"


def test_uint8_block_is_pq_decode_of_the_op(env):
    """Against ops.pq_decode itself (the kernel the contract names), every code value of a C < 256 table included: an index is
    c < C ? c : 0."""
    torch, ops = env
    M, C, d = 64, 200, 128
    rs_ = np.random.RandomState(9)
    codes = torch.from_numpy(rs_.randint(0, 256, (BS, NH_K, T, M)).astype(np.uint8)).cuda()      # codes >= C too
    cents = torch.from_numpy(rs_.standard_normal((M, C, d // M)).astype(np.float16)).cuda()
    k_out = torch.zeros(BS, NH_K, T, d, dtype=torch.float16, device="cuda")
    v_out = torch.zeros_like(k_out)
    ops.pq_gather_rows(codes, codes, cents, cents, k_out, v_out, t0=0, t1=T)
    want = ops.pq_decode(codes, cents)
    torch.cuda.synchronize()
    assert torch.equal(k_out.view(torch.int16), want.view(torch.int16)) and torch.equal(v_out.view(torch.int16), want.view(torch.int16))
