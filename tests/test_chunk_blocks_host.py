"""CPU tests of the block route of chunk attention: the two new entry points (million_prefill_attn_lse,
million_pq_gather_rows) and ops.chunk_blocks_workspace_bytes refuse before any launch; the plan (ops.chunk_blocks_plan) cuts
the past into blocks that partition it, with the window in exactly one part and no merge of more than 8 parts; the route's own
roundings - fp16 partial outputs, fp32 merges, the intermediate merges of a plan with two levels - stay inside the attention
bar on the shapes tests/test_chunk_blocks_gpu.py runs and on peaked inputs, so the bar there is one exact kernels meet; and,
with `ops` stubbed, route=None / "chunk" log what the caches have always logged while "blocks" logs the new op and then the
same store calls."""
import ctypes
import subprocess
import tempfile
from pathlib import Path

import numpy as np
import pytest
import torch

from tests import chunk_blocks_model as B
from tests import flash_inputs as F
from tests import lse_ref
from tests.test_chunk_attn_gpu import _state
from tests.test_chunk_blocks_gpu import BS, CAP, CASES, NH, NH_K

ROOT = Path(__file__).resolve().parents[1]
SHAPE, ALIGN, ARG = -1, -2, -3


@pytest.fixture(scope="module")
def lib():
    from million_amd import build, _lib
    build.build()
    return _lib.load()


# ---------------------------------------------------------------- 1. refusals before any launch -----------------------------
def _pdesc(**kw):
    from million_amd import _lib
    d = _lib.PrefillDesc()
    d.struct_size = ctypes.sizeof(_lib.PrefillDesc)
    d.bs, d.nh, d.nh_k, d.d, d.n_q, d.n_kv, d.q_pos0, d.causal = 1, 8, 2, 128, 16, 64, 48, 1
    for name in ("q", "k", "v", "o"):
        setattr(d, f"{name}_stride_b", 8 * 64 * 128)
        setattr(d, f"{name}_stride_h", 64 * 128)
        setattr(d, f"{name}_stride_n", 128)
    for k, v in kw.items():
        setattr(d, k, v)
    return d


def test_prefill_lse_refuses_before_any_launch(lib):
    call = lambda d, q=0x1000, k=0x2000, v=0x3000, out=0x4000, lse=0x5000: lib.million_prefill_attn_lse(ctypes.byref(d), q, k, v, out, lse, None)
    err = lambda: lib.million_last_error()
    assert call(_pdesc(struct_size=12)) == ARG and b"struct_size" in err()
    assert lib.million_prefill_attn_lse(None, 0x1000, 0x2000, 0x3000, 0x4000, 0x5000, None) == ARG and b"struct_size" in err()
    assert call(_pdesc(), lse=None) == ARG and b"null lse" in err()
    assert call(_pdesc(), q=None) == ARG and b"null pointer" in err()
    assert call(_pdesc(), out=None) == ARG and b"null pointer" in err()
    assert call(_pdesc(d=96)) == SHAPE and b"d=96" in err()
    assert call(_pdesc(nh=7)) == SHAPE and b"nh=7" in err()
    assert call(_pdesc(n_kv=0)) == ARG and b"no keys" in err()
    assert call(_pdesc(), k=0x2008) == ALIGN and b"16-byte aligned" in err()
    assert call(_pdesc(), lse=0x5002) == ALIGN and b"lse must be 4-byte aligned" in err()
    assert call(_pdesc(k_stride_n=132)) == ALIGN and b"multiples of 8" in err()
    assert call(_pdesc(n_q=0)) == 0      # nothing to do


def _gdesc(**kw):
    from million_amd import _lib
    d = _lib.GatherRowsDesc()
    d.struct_size = ctypes.sizeof(_lib.GatherRowsDesc)
    d.bs, d.nh_k, d.d, d.M, d.C, d.code_bytes = 2, 2, 128, 64, 256, 1
    d.t0, d.t1, d.r, d.resid_start, d.resid_cap = 37, 171, 37, 50, 64
    d.resid_stride_b, d.resid_stride_h = 2 * 64 * 128, 64 * 128
    d.k_layout = d.v_layout = _lib.MILLION_KV_PAGED
    d.page_size, d.n_pages_cap = 64, 5
    d.rows_cap, d.o_stride_b, d.o_stride_h = 400, 2 * 400 * 128, 400 * 128
    for k, v in kw.items():
        setattr(d, k, v)
    return d


def test_gather_rows_desc_matches_header(lib):
    from million_amd import _lib
    src = ('#include "million_hip.h"\n#include <stdio.h>\n#include <stddef.h>\n'
           'int main(){printf("%zu %zu %zu %zu\\n", sizeof(million_gather_rows_desc), offsetof(million_gather_rows_desc, resid_stride_b),'
           ' offsetof(million_gather_rows_desc, k_stride_b), offsetof(million_gather_rows_desc, o_stride_h));return 0;}\n')
    with tempfile.TemporaryDirectory() as td:
        (Path(td) / "a.c").write_text(src)
        subprocess.check_call(["gcc", "-std=c11", "-I", str(ROOT / "include"), "-o", f"{td}/a", f"{td}/a.c"])
        size, off_res, off_k, off_o = map(int, subprocess.check_output([f"{td}/a"]).split())
    D = _lib.GatherRowsDesc
    assert (size, off_res, off_k, off_o) == (ctypes.sizeof(D), D.resid_stride_b.offset, D.k_stride_b.offset, D.o_stride_h.offset)


def test_gather_rows_refuses_before_any_launch(lib):
    ptrs = dict(k_codes=0x1000, v_codes=0x2000, k_ids=0x3000, v_ids=0x3000, k_cents=0x4000, v_cents=0x5000, k_res=0x6000, v_res=0x7000,
                k_out=0x8000, v_out=0x9000)

    def call(d, **over):
        p = dict(ptrs, **over)
        return lib.million_pq_gather_rows(ctypes.byref(d), *[p[n] for n in ("k_codes", "v_codes", "k_ids", "v_ids", "k_cents", "v_cents",
                                                                             "k_res", "v_res", "k_out", "v_out")], None)
    err = lambda: lib.million_last_error()
    assert call(_gdesc(struct_size=8)) == ARG and b"struct_size" in err()
    assert call(_gdesc(d=96, M=48)) == SHAPE and b"d=96" in err()
    assert call(_gdesc(M=3)) == SHAPE and b"d/M" in err()
    assert call(_gdesc(M=4)) == SHAPE and b"d/M" in err()                                    # d / M = 32
    assert call(_gdesc(C=1024)) == SHAPE and b"C=1024 with uint8 codes" in err()             # a C the code type cannot hold
    assert call(_gdesc(C=256, code_bytes=2)) == SHAPE and b"C=256 with uint16 codes" in err()
    assert call(_gdesc(C=8192, code_bytes=2)) == SHAPE and b"C=8192 with uint16 codes" in err()
    assert call(_gdesc(code_bytes=4)) == SHAPE and b"code_bytes=4" in err()
    assert call(_gdesc(t0=200)) == ARG and b"t0=200 t1=171" in err()
    assert call(_gdesc(r=65)) == ARG and b"r=65" in err()
    assert call(_gdesc(resid_start=64)) == ARG and b"resid_start=64" in err()
    assert call(_gdesc(rows_cap=170)) == ARG and b"171 rows into rows_cap=170" in err()
    assert call(_gdesc(k_layout=2)) == ARG and b"k_layout=2" in err()
    assert call(_gdesc(page_size=48)) == SHAPE and b"page_size=48" in err()
    assert call(_gdesc(n_pages_cap=2)) == ARG and b"n_pages_cap*page_size < t1" in err()
    # a table past the 32-bit limits: entries, then tokens per row
    assert call(_gdesc(bs=16384, nh_k=2, n_pages_cap=1 << 16)) == ARG and b"page table of 2147483648 entries" in err()
    assert call(_gdesc(bs=1, nh_k=1, page_size=128, n_pages_cap=1 << 24)) == ARG and b"2147483648 tokens per row" in err()
    assert call(_gdesc(bs=65536, nh_k=1)) == SHAPE and b"bs * nh_k" in err()
    assert call(_gdesc(), k_out=None) == ARG and b"null pointer (out)" in err()
    assert call(_gdesc(), v_cents=None) == ARG and b"null pointer (codes" in err()
    assert call(_gdesc(), k_ids=None) == ARG and b"null pointer (codes" in err()
    assert call(_gdesc(), v_res=None) == ARG and b"null pointer (window)" in err()
    assert call(_gdesc(), k_out=0x8008) == ALIGN and b"16-byte aligned" in err()
    assert call(_gdesc(), v_cents=0x5004) == ALIGN and b"16-byte aligned" in err()
    assert call(_gdesc(o_stride_h=400 * 128 + 4)) == ALIGN and b"multiples of 8" in err()
    assert call(_gdesc(resid_stride_b=2 * 64 * 128 + 2)) == ALIGN and b"multiples of 8" in err()
    assert call(_gdesc(code_bytes=2, C=1024, k_layout=0, k_stride_b=1001), k_ids=None) == ALIGN and b"2-byte aligned" in err()
    # nothing to write: no launch, whatever the pointers
    assert call(_gdesc(t0=5, t1=5, r=0), k_out=None, v_out=None) == 0


def test_ops_refuse_before_any_launch():
    from million_amd import ops
    with pytest.raises(RuntimeError, match="d=96"):
        ops.chunk_blocks_workspace_bytes(1, 8, 2, 16, 96, 64)
    with pytest.raises(RuntimeError, match="nh=7"):
        ops.chunk_blocks_workspace_bytes(1, 7, 2, 16, 128, 64)
    with pytest.raises(RuntimeError, match="block_tokens=0"):
        ops.chunk_blocks_workspace_bytes(1, 8, 2, 16, 128, 64, 0)
    with pytest.raises(RuntimeError, match="31 bits"):
        ops.chunk_blocks_workspace_bytes(1, 8, 2, 16, 128, 64, 1 << 31)
    with pytest.raises(RuntimeError, match="31 bits"):
        ops.chunk_blocks_workspace_bytes(1 << 12, 1 << 10, 2, 1 << 10, 128, 64)
    with pytest.raises(RuntimeError, match="exceed 64"):
        ops.chunk_blocks_plan(65 * 16, 0, False, 16)
    q = torch.zeros(2, 8, 5, 128, dtype=torch.float16)
    with pytest.raises(RuntimeError, match="dev_lengths"):      # by name, before anything about the tensors
        ops.pq_chunk_attn_blocks(q, None, None, None, None, None, None, None, None, 0, M=64, C=256, n_tokens=0, dev_lengths=torch.zeros(2, 4, dtype=torch.int32))
    with pytest.raises(RuntimeError, match="dev_n_q"):
        ops.pq_chunk_attn_blocks(q, None, None, None, None, None, None, None, None, 0, M=64, C=256, n_tokens=0, dev_n_q=torch.zeros(2, dtype=torch.int32))
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        ops.prefill_attn(q, q[:, :2], q[:, :2], return_lse=True)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        ops.pq_gather_rows(torch.zeros(2, 2, 8, 64, dtype=torch.uint8), torch.zeros(2, 2, 8, 64, dtype=torch.uint8),
                           torch.zeros(64, 256, 2, dtype=torch.float16), torch.zeros(64, 256, 2, dtype=torch.float16),
                           torch.zeros(2, 2, 8, 128, dtype=torch.float16), torch.zeros(2, 2, 8, 128, dtype=torch.float16), t0=0, t1=8)


# ---------------------------------------------------------------- 2. the plan -----------------------------------------------
BT = 128


@pytest.mark.parametrize("chunk", [False, True], ids=["past-only", "chunk"])
@pytest.mark.parametrize("r", [0, 37])
@pytest.mark.parametrize("T", [0, 1, BT - 1, BT, BT + 1, 9 * BT + 5])
def test_plan_partitions_the_past(T, r, chunk):
    from million_amd import ops
    from million_amd._lib import MILLION_MERGE_MAX_PARTS as P
    plan = ops.chunk_blocks_plan(T, r, chunk, BT)
    parts, groups = plan["parts"], plan["groups"]
    blocks = [p for p in parts if p[0] == "block"]
    # the ranges partition [0, T) in order, none longer than a block, none empty but a window-only block
    edge = 0
    for _, t0, t1, r_here in blocks:
        assert t0 == edge and t0 <= t1 <= t0 + BT and (t1 > t0 or (T == 0 and r_here == r > 0))
        edge = t1
    assert edge == T
    # the window in exactly one part: behind the last block's rows
    assert sum(1 for b in blocks if b[3]) == (1 if r else 0) and sum(b[3] for b in blocks) == r
    if r:
        assert blocks[-1][3] == r
    assert [p for p in parts if p[0] == "chunk"] == ([("chunk",)] if chunk else []) and (not chunk or parts[-1] == ("chunk",))
    assert len(parts) == -(-T // BT) + (1 if (r and T == 0) else 0) + (1 if chunk else 0)
    # every part in exactly one group, in order; no merge of more than 8; at most 8 groups
    assert [i for g in groups for i in g] == list(range(len(parts)))
    assert all(1 <= len(g) <= P for g in groups) and len(groups) <= P
    assert len(groups) == (-(-len(parts) // P))
    # the workspace is a function of the shapes and block_tokens only, and holds one block plus the window and 16 pairs
    ws = ops.chunk_blocks_workspace_bytes(BS, NH, NH_K, 70, 128, CAP, BT)
    up = lambda x: -(-x // 256) * 256
    assert ws == 2 * up(BS * NH_K * (BT + CAP) * 128 * 2) + 16 * (up(BS * NH * 70 * 128 * 2) + up(BS * NH * 70 * 4))


def test_default_block_keeps_one_merge_up_to_128k():
    from million_amd import ops
    for T in (32768, 131072):
        for r in (0, 128):
            assert len(ops.chunk_blocks_plan(T, r, True)["parts"]) <= 8
    assert len(ops.chunk_blocks_plan(131072 + ops.CHUNK_BLOCK_TOKENS, 0, True)["groups"]) == 2
    assert ops.chunk_blocks_workspace_bytes(1, 32, 8, 2048, 128, 128) == ops.chunk_blocks_workspace_bytes(1, 32, 8, 2048, 128, 128, ops.CHUNK_BLOCK_TOKENS)


# ---------------------------------------------------------------- 3. the route's own roundings ------------------------------
def _emulated_against_unsplit(oracle, st, T, r, chunk, bt, what):
    from million_amd import ops
    plan = ops.chunk_blocks_plan(T, r, chunk, bt)
    out, lse = B.emulate_route(oracle, st, plan)
    gold_out, gold_lse = B.route_ref(oracle, st)
    B.check_bar(out.astype(np.float64), gold_out, f"emulated {what} ({len(plan['parts'])} parts, {len(plan['groups'])} groups)")
    B.check_lse(lse, gold_lse, f"emulated {what}", lse_ref.LSE_TOL)


@pytest.mark.parametrize("name", list(CASES))
def test_rounding_of_the_route_at_the_gpu_shapes(name, oracle):
    """fp16 parts, fp32 merges, intermediate merges rounded too: exact kernels leave the bar on every shape the GPU tests run."""
    T, bt, r, rstart, n_q, chunk = CASES[name]
    st = _state(np.random.RandomState(len(name)), BS, NH, NH_K, 128, 64, 256, n_q, T, r, CAP, rstart, chunk)
    _emulated_against_unsplit(oracle, st, T, r, chunk, bt, name)


@pytest.mark.parametrize("peak", F.PEAKS)
@pytest.mark.parametrize("bt", [128, 64], ids=["one-level", "two-levels"])
def test_rounding_of_the_route_on_peaked_inputs(bt, peak, oracle):
    """One dominating key, in a code block, in the wrapped window or in the chunk: the parts' weights differ by e^16 and the bar
    still holds after one or two levels of merges."""
    T, r, rstart, n_q = 700, 37, 50, 70
    st = F.chunk_inputs(None, BS, NH, NH_K, 128, 64, 256, n_q, T, r, CAP, rstart, True, peak=peak)
    _emulated_against_unsplit(oracle, st, T, r, True, bt, f"peak in {peak}, block_tokens {bt}")


@pytest.mark.parametrize("name", ["stair9", "descending", "sink_local", "gauss8"])
def test_rounding_of_the_route_on_spread_inputs(name, oracle):
    T, r, rstart, n_q = 700, 37, 50, 70
    st = F.chunk_inputs(name, BS, NH, NH_K, 128, 64, 256, n_q, T, r, CAP, rstart, True)
    _emulated_against_unsplit(oracle, st, T, r, True, 64, f"{name}, two levels")


# ---------------------------------------------------------------- 4. call logs with ops stubbed -----------------------------
def _stub_ops(monkeypatch, calls):
    from million_amd import ops
    rec = lambda name: (lambda q, *a, **k: (calls.append((name, a[8], k)), (torch.zeros_like(q), torch.zeros(q.shape[:3])) if k.get("return_lse") else torch.zeros_like(q))[1])
    for name in ("pq_chunk_attn", "pq_chunk_attn_wide", "pq_chunk_attn_blocks"):
        monkeypatch.setattr(ops, name, rec(name))
    monkeypatch.setattr(ops, "pq_encode_into", lambda X, cents, dst, **k: calls.append(("enc", {kk: vv for kk, vv in k.items() if kk in ("token_start", "n", "x_row_start", "x_row_mod")}, {})))
    monkeypatch.setattr(ops, "attn_sink_merge", lambda *a, **k: calls.append(("sink_merge", None, {})))


def _paged(sink_tokens=0):
    from million_amd.pq_cache import PagedPQCache
    cache = PagedPQCache(bs=3, nh=8, num_key_value_heads=2, M=64, layer_num=2, d=128, page_size=32, extended_residual_size=64,
                         max_tokens=1024, device="cpu", sink_tokens=sink_tokens)
    cache.key_cent = cache.value_cent = torch.zeros(64, 256, 2, dtype=torch.float16)
    cache._kprep = cache._vprep = torch.zeros(1, dtype=torch.float16)
    cache._T_a[:], cache._r_a[:], cache._rs_a[:], cache._seen_a[:] = 96, 40, 50, 136
    return cache


def _paged_log(monkeypatch, route, sink_tokens=0):
    calls = []
    _stub_ops(monkeypatch, calls)
    cache = _paged(sink_tokens)
    if sink_tokens:
        cache._sink_a[:] = sink_tokens
    x = lambda bs, n: torch.zeros(bs, 2, n, 128, dtype=torch.float16)
    q = lambda bs, n: torch.zeros(bs, 8, n, 128, dtype=torch.float16)
    kw = {} if route == "default" else {"route": route}
    cache.extend(q(3, 10), x(3, 10), x(3, 10), 0, **kw)
    cache.extend_request(1, q(1, 5), x(1, 5), x(1, 5), 1, **kw)
    cache.extend_request(2, q(1, 5), x(1, 5), x(1, 5), 1, return_lse=True, **kw)
    state = (cache._T_a.copy(), cache._r_a.copy(), cache._rs_a.copy(), cache._seen_a.copy(), [l.clone() for l in cache.lengths])
    return calls, state


@pytest.mark.parametrize("sink_tokens", [0, 4])
def test_paged_routes_log(monkeypatch, sink_tokens):
    default, st_d = _paged_log(monkeypatch, "default", sink_tokens)
    # what the caches have always logged: one chunk-attention call, then the window in ring order and the chunk, K and V each
    names = [c[0] for c in default]
    sm = ["sink_merge"] if sink_tokens else []
    assert names == ["pq_chunk_attn"] + sm + ["enc"] * 4 + ["pq_chunk_attn"] + sm + ["enc"] * 4 + ["pq_chunk_attn"] + sm + ["enc"] * 4
    attn = [c for c in default if c[0] == "pq_chunk_attn"]
    assert [(c[1], c[2]["n_tokens"], c[2]["resid_start"], c[2].get("return_lse", False)) for c in attn] == \
        [(40, 96, 50, bool(sink_tokens))] * 2 + [(40, 96, 50, True)]
    assert [c[1] for c in default if c[0] == "enc"][:4] == [dict(token_start=96, n=40, x_row_start=50, x_row_mod=64)] * 2 + \
        [dict(token_start=136, n=10, x_row_start=0, x_row_mod=0)] * 2
    for route in (None, "chunk"):
        log, st = _paged_log(monkeypatch, route, sink_tokens)
        assert [(c[0], c[1], sorted(c[2])) for c in log] == [(c[0], c[1], sorted(c[2])) for c in default], route
    blocks, st_b = _paged_log(monkeypatch, "blocks", sink_tokens)
    # the new op with the chunk op's arguments, then the same store calls
    swap = lambda n: "pq_chunk_attn" if n == "pq_chunk_attn_blocks" else n
    assert "pq_chunk_attn" not in [c[0] for c in blocks] and [c[0] for c in blocks].count("pq_chunk_attn_blocks") == 3
    assert [(swap(c[0]), c[1], sorted(c[2])) for c in blocks] == [(c[0], c[1], sorted(c[2])) for c in default]
    assert [c[1] for c in blocks if c[0] == "enc"] == [c[1] for c in default if c[0] == "enc"]
    for a, b in zip(st_d[:4], st_b[:4]):
        assert (a == b).all()
    assert all(torch.equal(a, b) for a, b in zip(st_d[4], st_b[4]))


def test_paged_route_is_checked_and_ragged_takes_none(monkeypatch):
    calls = []
    _stub_ops(monkeypatch, calls)
    cache = _paged()
    x, q = torch.zeros(3, 2, 4, 128, dtype=torch.float16), torch.zeros(3, 8, 4, 128, dtype=torch.float16)
    with pytest.raises(ValueError, match="route='torch'"):
        cache.extend(q, x, x, 0, route="torch")
    assert not calls and list(cache._T_a[0]) == [96] * 3
    with pytest.raises(TypeError):
        cache.extend_ragged(q, x, x, 0, [4, 4, 4], route="blocks")


def test_wide_paged_cache_still_refuses_extend(monkeypatch):
    from million_amd.pq_cache import PagedPQCache
    calls = []
    _stub_ops(monkeypatch, calls)
    cache = PagedPQCache(bs=1, nh=8, num_key_value_heads=2, M=64, layer_num=1, d=128, page_size=32, extended_residual_size=64,
                         max_tokens=256, device="cpu", nbits=10, dtype=torch.uint16)
    x, q = torch.zeros(1, 2, 4, 128, dtype=torch.float16), torch.zeros(1, 8, 4, 128, dtype=torch.float16)
    for route in (None, "blocks"):
        with pytest.raises(NotImplementedError, match="nbits=10"):
            cache.extend(q, x, x, 0, route=route)
        with pytest.raises(NotImplementedError, match="nbits=10"):
            cache.extend_request(0, q, x, x, 0, route=route)
    assert not calls


@pytest.mark.parametrize("nbits", [8, 10])
def test_dynamic_routes_log(monkeypatch, nbits):
    from million_amd.pq_cache import DynamicPQCache

    def log(route):
        calls = []
        _stub_ops(monkeypatch, calls)
        cache = DynamicPQCache(bs=1, nh=4, num_key_value_heads=2, M=32, layer_num=1, d=64, nbits=nbits, max_tokens=512, device="cpu")
        cache.key_cent = cache.value_cent = torch.zeros(32, 2 ** nbits, 2, dtype=torch.float16)
        cache._kprep = cache._vprep = torch.zeros(1, dtype=torch.float16) if nbits == 8 else None
        cache._T[0], cache.residualed_tokens[0], cache.seen_tokens[0] = 128, 17, 145
        x = torch.zeros(1, 2, 9, 64, dtype=torch.float16)
        cache.extend(torch.zeros(1, 4, 9, 64, dtype=torch.float16), x, x, 0, **({} if route == "default" else {"route": route}))
        assert (cache._T[0], cache.residualed_tokens[0], cache.seen_tokens[0]) == (154, 0, 154)
        return calls

    op = "pq_chunk_attn" if nbits == 8 else "pq_chunk_attn_wide"
    default = log("default")
    assert [c[0] for c in default] == [op] + ["enc"] * 4 and default[0][1] == 17 and default[0][2] == dict(M=32, C=2 ** nbits, n_tokens=128)
    assert [c[1] for c in default[1:]] == [dict(token_start=128, n=17)] * 2 + [dict(token_start=145, n=9)] * 2
    assert log(None) == default and log("chunk") == default
    blocks = log("blocks")
    assert blocks[0] == ("pq_chunk_attn_blocks",) + default[0][1:] and blocks[1:] == default[1:]
