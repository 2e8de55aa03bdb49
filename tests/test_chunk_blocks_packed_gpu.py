"""ops.pq_chunk_attn_blocks(packed=True) on the GPU: the block route with its gather reading packed 10- / 12-bit pages.  Nothing
else in the route changes, so out and lse are bitwise those of the route over uint16 pools holding the same codes; that result
is held to the project's bar against the fp64 model (tests/chunk_blocks_model.py), as tests/test_chunk_blocks_gpu.py does."""
import numpy as np
import pytest

from tests import chunk_blocks_model as B
from tests import lse_ref
from tests import packed_model as P
from tests.test_chunk_blocks_gpu import BS, CAP, NH, NH_K, _args, _wide_state

pytestmark = pytest.mark.gpu
BT = 64
# name -> (d, M, C, T, r, resid_start, n_q, chunk, parts): one merge; two merge levels; a wrapped window and the chunk
CASES = {
    "T200-one-merge": (128, 64, 1024, 200, 0, 0, 70, False, 4),
    "T600-two-levels": (128, 32, 4096, 600, 0, 0, 5, False, 10),
    "T200-wrapped-window-chunk": (64, 32, 2048, 200, 37, 50, 70, True, 5),
    "T600-window-chunk-two-levels": (128, 64, 512, 600, 37, 50, 5, True, 11),
}


@pytest.fixture(scope="module")
def env():
    import torch
    from million_amd import build, ops
    build.build()
    assert torch.cuda.is_available()
    return torch, ops


def _both(torch, ops, name):
    """(state, uint16 arguments, packed arguments, keyword arguments) of a case: the same codes behind the same page table."""
    d, M, C, T, r, rstart, n_q, chunk, parts = CASES[name]
    st = _wide_state(np.random.RandomState(len(name) + C), d, M, C, n_q, T, r, rstart, chunk)
    assert st["k_codes"].max() >= 256 and st["v_codes"].max() >= 256
    plan = ops.chunk_blocks_plan(T, r, chunk, BT)
    assert len(plan["parts"]) == parts and (len(plan["groups"]) > 1) == (parts > 8)
    args, kw = _args(torch, ops, st, M, C, "paged", ps=32)
    u16 = lambda t: t.view(torch.int16).cpu().numpy().view(np.uint16)
    pk = torch.from_numpy(P.pack(u16(args[3]), "k", C)).cuda()
    pv = torch.from_numpy(P.pack(u16(args[4]), "v", C)).cuda()
    return st, args, args[:3] + (pk, pv) + args[5:], kw


@pytest.mark.parametrize("name", list(CASES))
def test_packed_route_is_the_uint16_route(name, env, oracle):
    torch, ops = env
    st, args, pargs, kw = _both(torch, ops, name)
    wide, wide_l = ops.pq_chunk_attn_blocks(*args, block_tokens=BT, return_lse=True, **kw)
    out, lse = ops.pq_chunk_attn_blocks(*pargs, block_tokens=BT, return_lse=True, packed=True, **kw)
    only = ops.pq_chunk_attn_blocks(*pargs, block_tokens=BT, packed=True, **kw)
    torch.cuda.synchronize()
    bits = lambda t: t.contiguous().view(torch.int16 if t.dtype == torch.float16 else torch.int32)
    assert torch.equal(bits(out), bits(wide)) and torch.equal(bits(lse), bits(wide_l))
    assert torch.equal(bits(out), bits(only)) and out.any()
    gold_out, gold_lse = B.route_ref(oracle, st)
    B.check_bar(wide.float().cpu().numpy(), gold_out, f"{name} vs fp64")
    B.check_lse(wide_l.cpu().numpy(), gold_lse, f"{name} vs fp64", lse_ref.LSE_TOL)


def test_captured_packed_route(env, oracle):
    """out=, workspace=, lse=: the packed route captured once; its replay is bitwise the eager uint16 route."""
    torch, ops = env
    name = "T600-window-chunk-two-levels"
    d, n_q = CASES[name][0], CASES[name][6]
    st, args, pargs, kw = _both(torch, ops, name)
    ws = torch.empty(ops.chunk_blocks_workspace_bytes(BS, NH, NH_K, n_q, d, CAP, BT), dtype=torch.uint8, device="cuda")
    out = torch.empty(BS, NH, n_q, d, dtype=torch.float16, device="cuda")
    lse = torch.empty(BS, NH, n_q, dtype=torch.float32, device="cuda")
    run = lambda: ops.pq_chunk_attn_blocks(*pargs, block_tokens=BT, out=out, lse=lse, workspace=ws, packed=True, **kw)
    run()      # eager once: module load, kernel attributes
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        run()
    out.fill_(float("nan"))
    lse.fill_(float("nan"))
    ws.fill_(0xFF)
    g.replay()
    torch.cuda.synchronize()
    wide, wide_l = ops.pq_chunk_attn_blocks(*args, block_tokens=BT, return_lse=True, **kw)
    torch.cuda.synchronize()
    assert torch.equal(out.view(torch.int16), wide.contiguous().view(torch.int16)) and torch.equal(lse.view(torch.int32), wide_l.view(torch.int32))
    gold_out, gold_lse = B.route_ref(oracle, st)
    B.check_bar(out.float().cpu().numpy(), gold_out, "captured vs fp64")
    B.check_lse(lse.cpu().numpy(), gold_lse, "captured vs fp64")
