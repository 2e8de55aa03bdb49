"""CPU tests of the chunk-attention entry points (million_pq_chunk_attn): descriptor layout, argument validation before any
launch, the workspace formula and split heuristic, and the host bookkeeping of PagedPQCache.extend / DynamicPQCache.extend."""
import ctypes
import subprocess
import tempfile
from pathlib import Path

import pytest
import torch

ROOT = Path(__file__).resolve().parents[1]
ARG, SHAPE, WORKSPACE = -3, -1, -4


@pytest.fixture(scope="module")
def lib():
    from million_amd import build, _lib
    build.build()
    return _lib.load()


def _desc(**kw):
    from million_amd import _lib
    d = _lib.ChunkAttnDesc()
    d.struct_size = ctypes.sizeof(_lib.ChunkAttnDesc)
    d.bs, d.nh, d.nh_k, d.d, d.M, d.C = 1, 32, 8, 128, 64, 256
    d.n_q, d.n_c, d.n_tokens, d.r, d.resid_start, d.resid_cap = 16, 16, 1000, 0, 0, 128
    for k, v in kw.items():
        setattr(d, k, v)
    return d


def _call(lib, d, ptrs=None, ws_bytes=0):
    p = [None] * 13 if ptrs is None else ptrs
    return lib.million_pq_chunk_attn(ctypes.byref(d), *p, ws_bytes, None)


def test_desc_size_matches_header(lib):
    from million_amd import _lib
    src = ('#include "million_hip.h"\n#include <stdio.h>\n#include <stddef.h>\n'
           'int main(){printf("%zu %zu %zu\\n", sizeof(million_chunk_attn_desc), offsetof(million_chunk_attn_desc, k_layout),'
           ' offsetof(million_chunk_attn_desc, o_stride_n));return 0;}\n')
    with tempfile.TemporaryDirectory() as td:
        (Path(td) / "a.c").write_text(src)
        subprocess.check_call(["gcc", "-std=c11", "-I", str(ROOT / "include"), "-o", f"{td}/a", f"{td}/a.c"])
        size, off_layout, off_last = map(int, subprocess.check_output([f"{td}/a"]).split())
    assert size == ctypes.sizeof(_lib.ChunkAttnDesc)
    assert off_layout == _lib.ChunkAttnDesc.k_layout.offset
    assert off_last == _lib.ChunkAttnDesc.o_stride_n.offset


def test_argument_validation_without_gpu(lib):
    d = _desc(struct_size=7)
    assert _call(lib, d) == ARG and b"struct_size" in lib.million_last_error()
    for bad in (dict(d=96), dict(M=8), dict(d=64, M=128), dict(C=257), dict(C=0), dict(nh=33)):
        assert _call(lib, _desc(**bad)) == SHAPE, bad
    assert _call(lib, _desc(n_c=3)) == SHAPE and b"n_c" in lib.million_last_error()
    assert _call(lib, _desc(r=129)) == ARG and b"r=129" in lib.million_last_error()
    assert _call(lib, _desc(r=5, resid_start=128)) == ARG
    assert _call(lib, _desc(k_layout=1, page_size=48, n_pages_cap=100)) == SHAPE
    assert _call(lib, _desc(k_layout=1, page_size=64, n_pages_cap=2)) == SHAPE          # 128 tokens of pages < 1000
    assert _call(lib, _desc(k_layout=2)) == ARG
    assert _call(lib, _desc()) == ARG and b"null" in lib.million_last_error()           # null pointers
    # every pointer given but the workspace: the split call needs one
    fake = [16 * (i + 1) for i in range(13)]
    assert _call(lib, _desc(), fake, 0) == WORKSPACE
    # n_q = 0: nothing to do
    assert _call(lib, _desc(n_q=0, n_c=0)) == 0


def _splits_model(bs, nh_k, n_q, G, T):
    n_qb = -(-n_q * G // 256)
    blocks = bs * nh_k * n_qb
    return max(1, min(-(-256 // blocks), -(-T // 64), 64)), n_qb


@pytest.mark.parametrize("bs,nh,nh_k,n_q,T,d", [
    (1, 32, 8, 1, 32768, 128), (1, 32, 8, 16, 32768, 128), (4, 32, 8, 64, 32768, 128), (1, 32, 8, 16, 131072, 128),
    (1, 32, 8, 2048, 8192, 128), (1, 8, 8, 3, 63, 64), (1, 8, 1, 65, 1000, 64), (2, 4, 4, 257, 4097, 128),
    (1, 32, 8, 512, 32768, 128), (1, 8, 2, 16, 0, 128), (8, 64, 8, 1, 1, 128), (1, 1, 1, 1, 10 ** 6, 64)])
def test_workspace_and_split_heuristic(lib, bs, nh, nh_k, n_q, T, d):
    G = nh // nh_k
    desc = _desc(bs=bs, nh=nh, nh_k=nh_k, d=d, M=64, n_q=n_q, n_c=n_q, n_tokens=T)
    got = lib.million_chunk_attn_workspace_bytes(ctypes.byref(desc))
    S, n_qb = _splits_model(bs, nh_k, n_q, G, T)
    assert got == (bs * nh_k * S * n_q * G * (d + 2) * 4 if S > 1 else 0)
    # every split owns >= 1 code tile; the grid fills the 256 CUs where the context allows
    assert S == 1 or S <= -(-T // 64)
    blocks = bs * nh_k * n_qb
    if -(-T // 64) >= -(-256 // blocks) and -(-256 // blocks) <= 64:
        assert S * blocks >= 256
    assert S <= 64


def test_workspace_bytes_bad_desc_is_zero(lib):
    assert lib.million_chunk_attn_workspace_bytes(ctypes.byref(_desc(struct_size=3))) == 0
    assert lib.million_chunk_attn_workspace_bytes(ctypes.byref(_desc(nh=33))) == 0


def _cpu_paged_cache(monkeypatch, calls):
    from million_amd import ops
    from million_amd.pq_cache import PagedPQCache
    monkeypatch.setattr(ops, "pq_chunk_attn", lambda q, *a, **k: (calls.append(("attn", a[8], k)), torch.zeros_like(q))[1])
    monkeypatch.setattr(ops, "pq_encode_into", lambda X, cents, dst, **k: calls.append(("enc", k)))
    cache = PagedPQCache(bs=3, nh=8, num_key_value_heads=2, M=64, layer_num=2, d=128, page_size=32,
                         extended_residual_size=64, max_tokens=1024, device="cpu")
    cache.key_cent = cache.value_cent = torch.zeros(64, 256, 2, dtype=torch.float16)
    cache._kprep = cache._vprep = torch.zeros(1, dtype=torch.float16)
    return cache


def test_paged_extend_bookkeeping_without_launch(monkeypatch):
    calls = []
    cache = _cpu_paged_cache(monkeypatch, calls)
    x = lambda bs, n: torch.zeros(bs, 2, n, 128, dtype=torch.float16)
    q = lambda bs, n: torch.zeros(bs, 8, n, 128, dtype=torch.float16)
    # a state: T = 96 quantised, a wrapped window of 40 rows from ring row 50
    cache._T_a[:] = 96
    cache._r_a[:] = 40
    cache._rs_a[:] = 50
    cache._seen_a[:] = 136
    cache._pre_a[0] = 1
    cache.extend(q(3, 10), x(3, 10), x(3, 10), 0)
    attn = [c for c in calls if c[0] == "attn"]
    enc = [c[1] for c in calls if c[0] == "enc"]
    assert len(attn) == 1 and attn[0][1] == 40 and attn[0][2]["n_tokens"] == 96 and attn[0][2]["resid_start"] == 50
    # window rows in ring order, then the chunk; K and V each
    assert [(e["token_start"], e["n"], e["x_row_start"], e["x_row_mod"]) for e in enc] == \
        [(96, 40, 50, 64)] * 2 + [(136, 10, 0, 0)] * 2
    assert list(cache._T_a[0]) == [146] * 3 and list(cache._r_a[0]) == [0] * 3 and list(cache._rs_a[0]) == [0] * 3
    assert list(cache._seen_a[0]) == [146] * 3 and not cache._pre_a[0].any()
    assert cache.lengths[0].tolist() == [[146, 0, 0, 0]] * 3
    assert list(cache._T_a[1]) == [96] * 3 and list(cache._r_a[1]) == [40] * 3          # the other layer is untouched
    # one slot: the other slots' host and device lengths stay
    calls.clear()
    cache._sync_lengths(1)
    before = cache.lengths[1].clone()
    cache.extend_request(1, q(1, 5), x(1, 5), x(1, 5), 1)
    assert list(cache._T_a[1]) == [96, 141, 96] and list(cache._r_a[1]) == [40, 0, 40]
    assert cache.lengths[1][1].tolist() == [141, 0, 0, 0]
    assert torch.equal(cache.lengths[1][0], before[0]) and torch.equal(cache.lengths[1][2], before[2])
    with pytest.raises(RuntimeError):
        cache.extend(q(3, 4), x(3, 4), x(3, 4), 1)          # requests at different lengths
    # capacity
    with pytest.raises(RuntimeError):
        cache.extend(q(3, 2000), x(3, 2000), x(3, 2000), 0)


def test_paged_extend_on_empty_cache_is_prefill(monkeypatch):
    calls = []
    cache = _cpu_paged_cache(monkeypatch, calls)
    from million_amd.pq_cache import PagedPQCache
    seen = []
    monkeypatch.setattr(PagedPQCache, "_prefill_attention", lambda self, q, k, v: (seen.append(q.shape), q)[1])
    x = torch.zeros(3, 2, 7, 128, dtype=torch.float16)
    cache.extend(torch.zeros(3, 8, 7, 128, dtype=torch.float16), x, x, 0)
    assert seen and not [c for c in calls if c[0] == "attn"]
    assert list(cache._T_a[0]) == [7] * 3


def test_dynamic_extend_bookkeeping_without_launch(monkeypatch):
    from million_amd import ops
    from million_amd.pq_cache import DynamicPQCache
    calls = []
    monkeypatch.setattr(ops, "pq_chunk_attn", lambda q, *a, **k: (calls.append(("attn", a[8], k)), torch.zeros_like(q))[1])
    monkeypatch.setattr(ops, "pq_encode_into", lambda X, cents, dst, **k: calls.append(("enc", X.shape[2], k)))
    cache = DynamicPQCache(bs=1, nh=4, num_key_value_heads=2, M=32, layer_num=1, d=64, max_tokens=512, device="cpu")
    cache.key_cent = cache.value_cent = torch.zeros(32, 256, 2, dtype=torch.float16)
    cache._kprep = cache._vprep = torch.zeros(1, dtype=torch.float16)
    cache._T[0], cache.residualed_tokens[0], cache.seen_tokens[0] = 128, 17, 145
    x = torch.zeros(1, 2, 9, 64, dtype=torch.float16)
    cache.extend(torch.zeros(1, 4, 9, 64, dtype=torch.float16), x, x, 0)
    assert calls[0][0] == "attn" and calls[0][1] == 17 and calls[0][2]["n_tokens"] == 128
    enc = [(c[2]["token_start"], c[2]["n"]) for c in calls if c[0] == "enc"]
    assert enc == [(128, 17), (128, 17), (145, 9), (145, 9)]
    assert (cache._T[0], cache.residualed_tokens[0], cache.seen_tokens[0]) == (154, 0, 154)
