"""CPU tests of ragged chunk attention: the two device-length fields of million_chunk_attn_desc (layout, validation before
any launch, the workspace as a function of the bound) and the host bookkeeping of PagedPQCache.extend_ragged."""
import ctypes
import subprocess
import tempfile
from pathlib import Path

import pytest
import torch

from tests.test_chunk_attn_host import _call, _cpu_paged_cache, _desc

ROOT = Path(__file__).resolve().parents[1]
ARG, SHAPE = -3, -1
FAKE = 4096      # a non-null "device pointer": validation never dereferences it


@pytest.fixture(scope="module")
def lib():
    from million_amd import build, _lib
    build.build()
    return _lib.load()


def test_ragged_fields_match_header(lib):
    from million_amd import _lib
    src = ('#include "million_hip.h"\n#include <stdio.h>\n#include <stddef.h>\n'
           'int main(){printf("%zu %zu %zu\\n", sizeof(million_chunk_attn_desc), offsetof(million_chunk_attn_desc, dev_lengths),'
           ' offsetof(million_chunk_attn_desc, dev_n_q));return 0;}\n')
    with tempfile.TemporaryDirectory() as td:
        (Path(td) / "a.c").write_text(src)
        subprocess.check_call(["gcc", "-std=c11", "-I", str(ROOT / "include"), "-o", f"{td}/a", f"{td}/a.c"])
        size, off_len, off_nq = map(int, subprocess.check_output([f"{td}/a"]).split())
    assert size == ctypes.sizeof(_lib.ChunkAttnDesc)
    assert off_len == _lib.ChunkAttnDesc.dev_lengths.offset
    assert off_nq == _lib.ChunkAttnDesc.dev_n_q.offset
    # trailing fields: everything before them lies where it lay
    assert off_len == _lib.ChunkAttnDesc.o_stride_n.offset + 8 and off_nq == off_len + 8 and size == off_nq + 8


@pytest.mark.parametrize("kw", [dict(), dict(bs=4, n_q=64, n_c=64, n_tokens=32768), dict(n_q=1, n_c=0, n_tokens=40),
                                dict(bs=2, nh=8, nh_k=2, n_q=5, n_c=5, n_tokens=1000, d=64, M=16)])
def test_workspace_is_a_function_of_the_bound(lib, kw):
    plain = lib.million_chunk_attn_workspace_bytes(ctypes.byref(_desc(**kw)))
    for extra in (dict(dev_lengths=FAKE), dict(dev_n_q=FAKE), dict(dev_lengths=FAKE, dev_n_q=FAKE, r=77, resid_start=-9)):
        assert lib.million_chunk_attn_workspace_bytes(ctypes.byref(_desc(**kw, **extra))) == plain


def test_ragged_validation_without_gpu(lib):
    ptrs = [16 * (i + 1) for i in range(13)]
    no_win = list(ptrs)
    no_win[9] = no_win[10] = None          # k_resid, v_resid
    # host r = 0 needs no window; device lengths may name up to resid_cap rows: the window is required
    assert _call(lib, _desc(dev_lengths=FAKE), no_win, 0) == ARG and b"window" in lib.million_last_error()
    # r and resid_start of the descriptor are not read with device lengths: values that fail alone pass here
    assert _call(lib, _desc(r=129)) == ARG
    assert _call(lib, _desc(dev_lengths=FAKE, r=129, resid_start=-4), no_win, 0) == ARG and b"window" in lib.million_last_error()
    # codes, codebooks and ids go with the bound
    no_codes = list(ptrs)
    no_codes[3] = None
    assert _call(lib, _desc(dev_lengths=FAKE), no_codes, 0) == ARG and b"codes" in lib.million_last_error()
    # the page capacity is checked against the bound
    assert _call(lib, _desc(dev_lengths=FAKE, dev_n_q=FAKE, k_layout=1, page_size=64, n_pages_cap=2), ptrs, 0) == SHAPE
    # n_q = 0: nothing to do, whatever the pointers
    assert _call(lib, _desc(n_q=0, n_c=0, dev_lengths=FAKE, dev_n_q=FAKE)) == 0


def _ragged_cache(monkeypatch, calls):
    cache = _cpu_paged_cache(monkeypatch, calls)
    for b, (T, r, rs) in enumerate([(96, 40, 50), (32, 0, 0), (0, 0, 0)]):
        cache._T_a[0, b], cache._r_a[0, b], cache._rs_a[0, b], cache._seen_a[0, b] = T, r, rs, T + r
    cache._sync_lengths(0)
    cache._pre_a[0] = 1
    return cache


def test_extend_ragged_bookkeeping_without_launch(monkeypatch):
    calls = []
    cache = _ragged_cache(monkeypatch, calls)
    before = cache.lengths[0].clone()
    ids_before = cache.page_ids[0].clone()
    x = torch.zeros(3, 2, 10, 128, dtype=torch.float16)
    out = cache.extend_ragged(torch.zeros(3, 8, 10, 128, dtype=torch.float16), x, x, 0, [10, 0, 7])
    assert out.shape == (3, 8, 10, 128)
    attn = [c for c in calls if c[0] == "attn"]
    enc = [c[1] for c in calls if c[0] == "enc"]
    # one launch for the batch: the cache's device rows as they were, a bound that covers every slot, n_new on the device
    assert len(attn) == 1 and calls[0][0] == "attn"
    kw = attn[0][2]
    assert kw["dev_lengths"].data_ptr() == cache.lengths[0].data_ptr() and kw["n_tokens"] >= 96
    assert kw["dev_n_q"].dtype == torch.int32 and kw["dev_n_q"].tolist() == [10, 0, 7]
    assert kw["page_size"] == 32 and kw["k_page_ids"].shape[0] == 3
    # slot 0: the window in ring order, then its 10 rows; slot 2: its 7 rows at token 0; nothing for slot 1 (K and V each)
    assert [(e["token_start"], e["n"], e["x_row_start"], e["x_row_mod"], e["page_ids"].data_ptr()) for e in enc] == \
        [(96, 40, 50, 64, cache.page_ids[0][0:1].data_ptr())] * 2 + [(136, 10, 0, 0, cache.page_ids[0][0:1].data_ptr())] * 2 + \
        [(0, 7, 0, 0, cache.page_ids[0][2:3].data_ptr())] * 2
    assert list(cache._T_a[0]) == [146, 32, 7] and list(cache._r_a[0]) == [0, 0, 0] and list(cache._rs_a[0]) == [0, 0, 0]
    assert list(cache._seen_a[0]) == [146, 32, 7]
    assert list(cache._pre_a[0]) == [0, 1, 0]                      # encode-ahead joined per slot
    assert cache.lengths[0].tolist() == [[146, 0, 0, 0], before[1].tolist(), [7, 0, 0, 0]]
    assert torch.equal(cache.page_ids[0], ids_before)
    assert list(cache._T_a[1]) == [0, 0, 0]                        # the other layer is untouched


def test_extend_ragged_rejects_before_any_call(monkeypatch):
    calls = []
    cache = _ragged_cache(monkeypatch, calls)
    x = lambda n: torch.zeros(3, 2, n, 128, dtype=torch.float16)
    q = lambda n: torch.zeros(3, 8, n, 128, dtype=torch.float16)
    state = (cache._T_a.copy(), cache._r_a.copy(), cache._pre_a.copy(), cache.lengths[0].clone())
    with pytest.raises(RuntimeError):
        cache.extend_ragged(q(10), x(10), x(10), 0, [10, 7])                  # one n_new per slot
    with pytest.raises(RuntimeError):
        cache.extend_ragged(q(10), x(10), x(10), 0, [10, 0, 11])              # more rows than the tensors hold
    with pytest.raises(RuntimeError):
        cache.extend_ragged(q(10), x(10), x(10), 0, [10, -1, 0])
    with pytest.raises(RuntimeError):
        cache.extend_ragged(q(1000), x(1000), x(1000), 0, [900, 0, 5])        # capacity, per slot: 96 + 40 + 900 > 1024
    assert not calls
    assert (cache._T_a == state[0]).all() and (cache._r_a == state[1]).all() and (cache._pre_a == state[2]).all()
    assert torch.equal(cache.lengths[0], state[3])
