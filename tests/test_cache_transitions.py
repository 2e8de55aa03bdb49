"""The host bookkeeping of PagedPQCache (million_amd/pq_cache.py; DESIGN.md 5, "mirror transitions"):

  * the recorded life of tests/cache_trace_scenario.py - every `ops` call, mirror array, device length row, page table and
    allocator counter after every public call - is what tests/cache_trace.json says (written before the transitions got
    one owner each: the refactor's definition of "nothing changed");
  * a replayed step, note_replayed_step(kind), leaves the mirror where the live step of that kind leaves it - on the CPU for
    the kinds that need no stream, on the GPU for a whole run with encode-ahead."""
import json

import numpy as np
import pytest
import torch

from tests import cache_trace_scenario as S


def test_recorded_life_of_a_cache_is_unchanged():
    want = json.loads(S.TRACE.read_text())
    got = S.trace()
    assert sorted(got) == sorted(want)
    for run in want:
        assert got[run] == want[run], f"{run}: {S.first_difference(got[run], want[run])}"
    assert S.TRACE.stat().st_size < 100 * 1024


def _state(c):
    return [a.tolist() for a in c.host_state()]


# (kind, device lengths, begin_step in the live step, r, T, resid_start, encoded-ahead flags): (layers, requests) each
_L2 = lambda *rows: [list(rows[0]), list(rows[-1])]
LIVE_CASES = {
    "plain": ("plain", False, True, _L2([10] * 3), _L2([96] * 3), _L2([32] * 3), _L2([0] * 3)),
    "plain-ragged": ("plain", True, True, _L2([10, 0, 63], [11, 0, 63]), _L2([96, 0, 32]), _L2([32, 0, 5]), _L2([0] * 3)),
    "flush-host-lengths": ("flush", False, False, _L2([64] * 3), _L2([96] * 3), _L2([32] * 3), _L2([0] * 3)),
    "flush-flags-lost": ("flush", False, False, _L2([64] * 3), _L2([96] * 3), _L2([0] * 3), _L2([1] * 3, [1, 0, 1])),
    "flush-ragged": ("flush", True, False, _L2([64, 10, 64], [64, 64, 3]), _L2([96, 0, 32], [96, 64, 32]),
                     _L2([32, 0, 60], [0, 32, 1]), _L2([1, 1, 0], [0, 1, 1])),
    "commit-host-lengths": ("commit", False, True, _L2([64] * 3), _L2([96] * 3), _L2([32] * 3), _L2([1] * 3)),
    "commit-device-lengths": ("commit", True, True, _L2([64] * 3), _L2([96] * 3), _L2([32] * 3), _L2([1] * 3)),
}


@pytest.mark.parametrize("preallocate", [True, False], ids=["preallocated", "on-demand"])
@pytest.mark.parametrize("case", list(LIVE_CASES))
def test_replayed_step_leaves_the_mirror_where_the_live_step_does(case, preallocate):
    kind, use_dl, begin, r, T, rs, pre = LIVE_CASES[case]
    with S.Life(preallocate) as life:
        live, twin = life.cache(), life.cache()
        seen = (np.asarray(T) + np.asarray(r)).tolist()
        for c in (live, twin):
            c.set_host_state((seen, r, T, rs, pre))
            assert c.next_step_kind() == kind
        if begin:
            assert live.begin_step(use_dev_lengths=use_dl) == kind
        for l in range(live.layer_num):
            live.decoding_with_pages(S._q(3, 1), S._x(3, 1), S._x(3, 1), l, use_dev_lengths=use_dl)
        twin.note_replayed_step(kind)
        assert _state(twin) == _state(live)
        assert _state(live)[0] == (np.asarray(seen) + 1).tolist()      # and the live step was a step


@pytest.mark.gpu
@pytest.mark.parametrize("use_dl", [False, True], ids=["host-lengths", "device-lengths"])
def test_live_steps_with_encode_ahead_equal_replayed_steps_gpu(use_dl):
    """80 eager steps with begin_step on the GPU (window 64 over pages of 32: the smallest geometry whose encode-ahead step
    is not its commit), a CPU twin that only hears note_replayed_step(kind): the same mirror after every step, and with
    device lengths the device rows are the mirror's."""
    assert torch.cuda.is_available(), "GPU tests need an MI355X"
    from million_amd import ops
    from million_amd.pq_cache import PagedPQCache
    geom = dict(bs=2, nh=8, num_key_value_heads=2, M=64, layer_num=2, d=128, page_size=32, extended_residual_size=64, max_tokens=256)
    g = torch.Generator(device="cpu").manual_seed(3)
    rnd = lambda *s: torch.randn(*s, generator=g).half().cuda()
    cache, twin = PagedPQCache(**geom), PagedPQCache(**geom, device="cpu")
    cache.set_cent(rnd(64, 256, 2), rnd(64, 256, 2))
    for l in range(2):
        cache.prefill(rnd(2, 8, 32, 128), rnd(2, 2, 32, 128), rnd(2, 2, 32, 128), l)
    q, k, v = rnd(2, 8, 1, 128), rnd(2, 2, 1, 128), rnd(2, 2, 1, 128)
    for _ in range(20):      # a window of 20 rows to start from: two encode-ahead steps and two commits fit into 80 steps
        for l in range(2):
            cache.decoding_with_pages(q, k, v, l, use_dev_lengths=use_dl)
    twin.set_host_state(cache.host_state())
    kinds = []
    for i in range(80):
        kind = cache.begin_step(use_dev_lengths=use_dl)
        assert kind == twin.next_step_kind()
        for l in range(2):
            cache.decoding_with_pages(q, k, v, l, use_dev_lengths=use_dl)
        twin.note_replayed_step(kind)
        kinds.append(kind)
        assert _state(twin) == _state(cache), f"step {i} ({kind})"
        if use_dl:
            rows = np.stack([cache._T_a, cache._r_a, cache._rs_a, np.zeros_like(cache._T_a)], axis=2)
            assert cache._lengths_all.cpu().numpy().tolist() == rows.tolist(), f"step {i} ({kind})"
    assert all(kinds.count(x) >= 2 for x in ("plain", "pre", "commit")) and set(kinds) == {"plain", "pre", "commit"}
    assert ops.tail_faults() == 0
