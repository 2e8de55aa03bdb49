"""CPU tests of ragged prompt attention: the dev_spans field of million_prefill_desc (layout), the argument checks of
ops.prefill_attn, the register / scratch figures of every prefill_attn instance, the host bookkeeping of
PagedPQCache.prefill_ragged, and the headroom of the GPU tests' inputs: the fp32 restatements of the two tile loops
(flash_inputs.model_plain, model_pipelined) sit at or below half the bar on every request of every batch
tests/test_prefill_ragged_gpu.py runs, so the bar there is one a correct kernel meets."""
import ctypes
import re
import subprocess
import sys
import tempfile
from pathlib import Path

import numpy as np
import pytest
import torch

from tests import flash_inputs as F
from tests import prefill_ragged_cases as R
from tests.test_chunk_attn_host import _cpu_paged_cache

ROOT = Path(__file__).resolve().parents[1]


@pytest.fixture(scope="module")
def lib():
    from million_amd import build, _lib
    build.build()
    return _lib.load()


def test_dev_spans_matches_header(lib):
    from million_amd import _lib
    src = ('#include "million_hip.h"\n#include <stdio.h>\n#include <stddef.h>\n'
           'int main(){printf("%zu %zu\\n", sizeof(million_prefill_desc), offsetof(million_prefill_desc, dev_spans));return 0;}\n')
    with tempfile.TemporaryDirectory() as td:
        (Path(td) / "a.c").write_text(src)
        subprocess.check_call(["gcc", "-std=c11", "-I", str(ROOT / "include"), "-o", f"{td}/a", f"{td}/a.c"])
        size, off = map(int, subprocess.check_output([f"{td}/a"]).split())
    assert size == ctypes.sizeof(_lib.PrefillDesc)
    assert off == _lib.PrefillDesc.dev_spans.offset
    # a trailing field: everything before it lies where it lay
    assert off == _lib.PrefillDesc.o_stride_n.offset + 8 and size == off + 8


def test_prefill_attn_checks_dev_spans():
    """The rows are checked before anything else, so each fault is named - without a GPU too."""
    from million_amd import ops
    q = torch.zeros(3, 8, 10, 128, dtype=torch.float16)
    kv = torch.zeros(3, 2, 10, 128, dtype=torch.float16)
    with pytest.raises(RuntimeError, match="int32"):
        ops.prefill_attn(q, kv, kv, dev_spans=torch.zeros(3, 4, dtype=torch.int64))
    with pytest.raises(RuntimeError, match="int32"):
        ops.prefill_attn(q, kv, kv, dev_spans=[[10, 10, 0, 0]] * 3)
    for bad in (torch.zeros(3, 3, dtype=torch.int32), torch.zeros(2, 4, dtype=torch.int32), torch.zeros(12, dtype=torch.int32),
                torch.zeros(3, 8, dtype=torch.int32)[:, ::2]):
        with pytest.raises(RuntimeError, match=r"shape \(bs, 4\)"):
            ops.prefill_attn(q, kv, kv, dev_spans=bad)
    with pytest.raises(RuntimeError, match="device of q"):
        ops.prefill_attn(q, kv, kv, dev_spans=torch.zeros(3, 4, dtype=torch.int32))      # a CPU tensor


def test_every_prefill_instance_has_no_scratch_no_spills_no_static_lds(lib):
    """The project's kernel-metadata check (tools/kernel_meta.py): three lockstep and three ragged instances; a ragged instance
    takes no more registers than a workgroup pair per CU allows (launch bounds: 2 x 512 threads -> 256) and no LDS of its own."""
    out = subprocess.run([sys.executable, str(ROOT / "tools" / "kernel_meta.py"), str(ROOT / "million_amd" / "libmillion_hip.so"), "prefill_attn"],
                         capture_output=True, text=True, check=True).stdout
    rows = [l for l in out.splitlines() if "prefill_attn" in l]
    names = sorted(l.split()[0] for l in rows)
    assert len(rows) == 6 and sum("Lb1" in x for x in names) == 3 and sum("Lb0" in x for x in names) == 3, out
    assert sum("pipe_kernel" in x for x in names) == 2 and sum("ILi128E" in x for x in names) == 2 and sum("ILi64E" in x for x in names) == 2, out
    for l in rows:
        assert l.rstrip().endswith("vgpr_spill 0 sgpr_spill 0 scratch 0 B"), l
        m = re.search(r"vgpr (\d+) .*lds (\d+) B", l)
        assert m and int(m.group(1)) <= 256 and int(m.group(2)) == 0, l


def test_prefill_ragged_bookkeeping_without_launch(monkeypatch):
    from million_amd import ops
    calls = []
    cache = _cpu_paged_cache(monkeypatch, calls)
    monkeypatch.setattr(ops, "prefill_attn", lambda q, k, v, **kw: (calls.append(("prefill", kw)), torch.zeros_like(q))[1])
    cache._T_a[0, 1], cache._r_a[0, 1], cache._rs_a[0, 1], cache._seen_a[0, 1] = 96, 40, 50, 136      # slot 1 is mid-sequence
    cache._sync_lengths(0)
    before = cache.lengths[0].clone()
    x = lambda bs, n: torch.zeros(bs, 2, n, 128, dtype=torch.float16)
    q = lambda bs, n: torch.zeros(bs, 8, n, 128, dtype=torch.float16)
    state = lambda: (cache._T_a.copy(), cache._r_a.copy(), cache._seen_a.copy(), cache.lengths[0].clone())
    s0 = state()
    with pytest.raises(RuntimeError, match="extend_ragged"):
        cache.prefill_ragged(q(3, 10), x(3, 10), x(3, 10), 0, [10, 1, 7])              # slot 1 holds tokens
    with pytest.raises(RuntimeError):
        cache.prefill_ragged(q(3, 10), x(3, 10), x(3, 10), 0, [10, 7])                 # one n_new per slot
    with pytest.raises(RuntimeError):
        cache.prefill_ragged(q(2, 10), x(2, 10), x(2, 10), 0, [10, 0])                 # tensors of the cache's batch
    with pytest.raises(RuntimeError):
        cache.prefill_ragged(q(3, 10), x(3, 10), x(3, 10), 0, [11, 0, 7])
    with pytest.raises(RuntimeError):
        cache.prefill_ragged(q(3, 10), x(3, 10), x(3, 10), 0, [10, 0, -1])
    with pytest.raises(RuntimeError, match="max_tokens"):
        cache.prefill_ragged(q(3, 1030), x(3, 1030), x(3, 1030), 0, [5, 0, 1030])      # capacity of every slot before any launch
    assert not calls and all((a == b).all() for a, b in zip(s0, state()))
    out = cache.prefill_ragged(q(3, 10), x(3, 10), x(3, 10), 0, [10, 0, 7])
    assert out.shape == (3, 8, 10, 128)
    # one launch for the batch, first; rows {n, n, 0, 0}; then each live slot's encodes (K and V) at token 0 of its own pages
    assert [c[0] for c in calls] == ["prefill", "enc", "enc", "enc", "enc"]
    kw = calls[0][1]
    assert kw["causal"] is True and kw["dev_spans"].dtype == torch.int32
    assert kw["dev_spans"].tolist() == [[10, 10, 0, 0], [0, 0, 0, 0], [7, 7, 0, 0]]
    enc = [c[1] for c in calls[1:]]
    assert [(e["token_start"], e["n"], e["page_ids"].data_ptr()) for e in enc] == \
        [(0, 10, cache.page_ids[0][0:1].data_ptr())] * 2 + [(0, 7, cache.page_ids[0][2:3].data_ptr())] * 2
    assert list(cache._T_a[0]) == [10, 96, 7] and list(cache._r_a[0]) == [0, 40, 0] and list(cache._seen_a[0]) == [10, 136, 7]
    assert cache.lengths[0].tolist() == [[10, 0, 0, 0], before[1].tolist(), [7, 0, 0, 0]]
    assert list(cache._T_a[1]) == [0, 0, 0]                                            # the other layer is untouched


# ---------------------------------------------------------------- headroom of the GPU tests' inputs ------------------------
def _headroom_cases():
    for batch in R.BATCHES:
        for name in (R.FAMILIES if batch != "poison" else [R.BASE]):
            for G, bound in R.GROUPS:
                yield pytest.param(name, batch, G, bound, id=f"{name}-{batch}-G{G}-bound{bound}")


@pytest.mark.parametrize("name,batch,G,bound", list(_headroom_cases()))
def test_inputs_leave_half_the_bar(name, batch, G, bound):
    """Per request, the first and the last query head (the heads of a family are draws of one distribution): both loops at
    d = 128, the plain loop at d = 64, every row against fp64."""
    causal, reqs = R.requests(batch, bound)
    nh = G * R.NH_K
    worst = 0.0
    for d, models in ((128, (F.model_plain, F.model_pipelined)), (64, (F.model_plain,))):
        q, k, v = R.inputs(name, len(reqs), G, bound, d)
        gold = R.gold(name, batch, G, bound, d)
        for b, req in enumerate(reqs):
            if not R.live(req):
                continue
            n_q, n_kv, q_pos0 = req
            vis = F.visible(n_q, n_kv, q_pos0, causal)
            for h in sorted({0, nh - 1}):
                hk = h // G
                for fn in models:
                    args = (F.prefill_tiles(n_kv),) if fn is F.model_plain else ()
                    got = fn(q[b, h, :n_q], k[b, hk, :n_kv], v[b, hk, :n_kv], vis, *args)
                    e = float(F.row_err(got, gold[b][0, h]).max())
                    worst = max(worst, e)
                    assert e <= 0.5 * F.REL_TOL, f"{fn.__name__} d{d} {name} {batch} G{G} request {b} {req} head {h}: worst row {e:.2e}"
    print(f"HEADROOM {name} {batch} G{G} bound{bound}: worst row {worst:.2e}")
