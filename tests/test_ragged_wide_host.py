"""Host logic of the ragged life of a wide PagedPQCache (million_amd.paged_turns: flush, decode, prefill_ragged, extend_ragged;
DESIGN.md 4.19) on CPU caches with the launches stubbed, in the style of tests/test_attn_wide_host.py: the mirror and the launch log
of paged_turns.decode across a trace whose windows fill at different steps, against oracle.PagedPolicy per request; the same trace
through the cache's own method still raises; the ragged calls refuse before anything moves and leave the mirror per-slot calls
leave; the cache's own four methods keep their refusals."""
import numpy as np
import pytest

from tests import ragged_wide_common as R

KW = dict(bs=R.BS, nh=R.NH, num_key_value_heads=R.NHK, M=64, layer_num=R.LAYERS, d=128, page_size=R.PS, extended_residual_size=R.CAP,
          max_tokens=R.MAX_TOKENS, device="cpu")
PROMPTS = [70, 45, 33]


def _host_cache(monkeypatch, log, nbits=10, packed=False):
    import torch
    from million_amd import ops
    from million_amd.pq_cache import PagedPQCache
    rec = lambda name, ret=None: (lambda *a, **k: (log.append((name, k)), ret(*a, **k) if ret else None)[1])
    zeros_q = lambda q, *a, **k: torch.zeros_like(q)
    chunk = lambda q, *a, **k: (torch.zeros_like(q), torch.zeros(q.shape[:3])) if k.get("return_lse") else torch.zeros_like(q)
    for name, short, ret in (("pq_encode_into", "encode", None), ("pq_encode_into_packed", "encode_packed", None),
                             ("prefill_attn", "prefill_attn", lambda q, k, v, **kw: torch.zeros_like(q)),
                             ("pq_chunk_attn", "chunk", chunk), ("pq_chunk_attn_wide", "chunk_wide", chunk), ("pq_chunk_attn_packed", "chunk_packed", chunk),
                             ("pq_decode_attn", "decode", zeros_q), ("pq_decode_attn_wide", "decode_wide", zeros_q),
                             ("pq_decode_attn_packed", "decode_packed", zeros_q), ("pq_flush", "flush", None), ("pq_flush_wide", "flush_wide", None),
                             ("lengths_advance", "advance", None), ("pq_store_ragged", "store_ragged", None),
                             ("pq_store_ragged_wide", "store_ragged_wide", None)):
        monkeypatch.setattr(ops, name, rec(short, ret))
    cache = PagedPQCache(**KW, nbits=nbits, dtype=torch.uint8 if nbits == 8 else torch.uint16, packed=packed)
    cache.key_cent = cache.value_cent = torch.zeros(64, 2 ** nbits, 2, dtype=torch.float16)
    cache._kprep = cache._vprep = None
    return cache


def _rows(n, bs=1):
    import torch
    return torch.zeros(bs, R.NH, n, 128, dtype=torch.float16), torch.zeros(bs, R.NHK, n, 128, dtype=torch.float16)


def _mirror(cache, device_rows=True):
    return [a.copy() for a in cache.host_state()] + [cache._pages_a.copy()] + ([l.clone() for l in cache.lengths] if device_rows else [])


def _same(a, b):
    import torch
    return all(torch.equal(x, y) if isinstance(x, torch.Tensor) else np.array_equal(x, y) for x, y in zip(a, b))


def _prompts(cache):
    for b, n in enumerate(PROMPTS):
        q, k = _rows(n)
        for l in range(R.LAYERS):
            cache.prefill_request(b, q, k, k, l)


@pytest.mark.parametrize("packed", [False, True])
def test_decode_trace_follows_the_policy_per_request(monkeypatch, oracle, packed):
    from million_amd import paged_turns
    log = []
    cache = _host_cache(monkeypatch, log, packed=packed)
    _prompts(cache)
    pols = [oracle.PagedPolicy(page_size=R.PS, residual=R.CAP, prefill=n) for n in PROMPTS]
    q1, k1 = _rows(1, R.BS)
    dec = "decode_packed" if packed else "decode_wide"
    flush_steps = {b: [] for b in range(R.BS)}
    for step in range(150):
        if step == 20:      # slot 1 is recycled: its window fills 20 steps behind the others from now on
            cache.release(1)
            q, k = _rows(20)
            for l in range(R.LAYERS):
                cache.prefill_request(1, q, k, k, l)
            pols[1] = oracle.PagedPolicy(page_size=R.PS, residual=R.CAP, prefill=20)
        full = cache._r_a[0] >= R.CAP
        kind = cache.begin_step(use_dev_lengths=True)
        assert kind == cache.next_step_kind() == ("flush" if full.any() else "plain")
        T0 = cache._T_a.copy()
        del log[:]
        for l in range(R.LAYERS):
            paged_turns.decode(cache, q1, k1, k1, l, use_dev_lengths=True)
        names = [e[0] for e in log]
        assert names == (["flush_wide", dec] if full.any() else [dec]) * R.LAYERS, step
        if full.any():
            kw = log[0][1]
            assert (kw["n"], kw["page_size"], kw["min_r"], kw["packed"]) == (R.PS, R.PS, R.CAP, packed) and kw["dev_lengths"] is cache.lengths[0]
            assert np.array_equal(cache._T_a - T0, np.broadcast_to(full * R.PS, T0.shape))      # exactly the full requests moved
        for b, pol in enumerate(pols):
            flushes = pol.flushes
            T, r = pol.step()
            assert cache._T_a[:, b].tolist() == [T] * R.LAYERS and cache._r_a[:, b].tolist() == [r] * R.LAYERS, (step, b)
            if pol.flushes > flushes:
                flush_steps[b].append(step)
        kw = log[-1][1]
        assert kw["dev_lengths"] is cache.lengths[R.LAYERS - 1] and kw["n_tokens"] == cache.max_tokens
    assert flush_steps[0] == flush_steps[2] == [64, 96, 128] and flush_steps[1] == [84, 116, 148]      # different steps, one launch each


def test_the_cache_s_own_step_still_serves_lockstep_only(monkeypatch):
    """The trace the feature is for, through PagedPQCache.decoding_with_pages: it raises at the first full window, as before."""
    log = []
    cache = _host_cache(monkeypatch, log)
    _prompts(cache)
    q1, k1 = _rows(1, R.BS)
    for step in range(R.CAP):
        for l in range(R.LAYERS):
            cache.decoding_with_pages(q1, k1, k1, l, use_dev_lengths=True)
    before, n_log = _mirror(cache), len(log)
    for l in range(R.LAYERS):
        with pytest.raises(RuntimeError, match="lockstep"):
            cache.decoding_with_pages(q1, k1, k1, l, use_dev_lengths=True)
        with pytest.raises(RuntimeError, match="lockstep"):
            cache.flush_to_pages(l, use_dev_lengths=True)
    assert _same(before, _mirror(cache)) and len(log) == n_log


def test_flush_rule_is_the_8_bit_one(monkeypatch):
    """paged_turns.flush: lockstep with host lengths flushes at r >= page_size, with device lengths only full windows; requests
    at different lengths need device lengths; an 8-bit cache goes to its own method."""
    from million_amd import paged_turns
    log = []
    cache = _host_cache(monkeypatch, log)
    q, k = _rows(40, R.BS)
    for l in range(R.LAYERS):
        cache.prefill(q, k, k, l)
    cache._r_a[:] = R.PS + 3
    del log[:]
    paged_turns.flush(cache, 0, use_dev_lengths=True)
    assert not log and cache._T_a[0].tolist() == [40] * R.BS
    paged_turns.flush(cache, 0)
    assert [e[0] for e in log] == ["flush_wide"] and log[0][1]["dev_lengths"] is None and log[0][1]["min_r"] == 0
    assert (log[0][1]["token_start"], log[0][1]["x_row_start"]) == (40, 0)
    assert cache._T_a[0].tolist() == [40 + R.PS] * R.BS and cache._r_a[0].tolist() == [3] * R.BS and cache._rs_a[0].tolist() == [R.PS] * R.BS
    assert cache._dev_rows_stale
    cache._r_a[1] = [R.CAP, 5, R.CAP]
    del log[:]
    with pytest.raises(RuntimeError, match="use_dev_lengths=True"):
        paged_turns.flush(cache, 1)
    assert not log
    paged_turns.flush(cache, 1, use_dev_lengths=True)
    assert [e[0] for e in log] == ["flush_wide"] and cache._T_a[1].tolist() == [40 + R.PS, 40, 40 + R.PS] and cache._r_a[1].tolist() == [R.CAP - R.PS, 5, R.CAP - R.PS]
    cache._r_a[1] = [3, 5, 7]
    del log[:]
    paged_turns.flush(cache, 1, use_dev_lengths=True)
    assert not log
    plain = _host_cache(monkeypatch, log, nbits=8)
    for l in range(R.LAYERS):
        plain.prefill(q, k, k, l)
    plain._r_a[:] = R.CAP
    del log[:]
    paged_turns.flush(plain, 0, use_dev_lengths=True)
    q1, k1 = _rows(1, R.BS)
    paged_turns.decode(plain, q1, k1, k1, 1, use_dev_lengths=True)
    assert [e[0] for e in log] == ["flush", "flush", "decode"]


@pytest.mark.parametrize("device_store", [False, True])
@pytest.mark.parametrize("packed", [False, True])
def test_ragged_calls_leave_what_per_slot_calls_leave(monkeypatch, device_store, packed):
    from million_amd import paged_turns
    log = []
    cache, twin = _host_cache(monkeypatch, log, packed=packed), _host_cache(monkeypatch, log, packed=packed)
    q, k = _rows(70, R.BS)
    # refusals first: nothing moves, nothing is launched
    before = _mirror(cache)
    for args, msg in ((([70, 45], ), "one n_new per slot"), (([71, 0, 0], ), "outside"), (([-1, 0, 0], ), "outside")):
        for fn in (paged_turns.prefill_ragged, paged_turns.extend_ragged):
            with pytest.raises(RuntimeError, match="paged_turns." + fn.__name__ + ".*" + msg):
                fn(cache, q, k, k, 0, *args, device_store=device_store)
    assert _same(before, _mirror(cache)) and not log
    for l in range(R.LAYERS):
        out = paged_turns.prefill_ragged(cache, q, k, k, l, PROMPTS, device_store=device_store)
        assert out.shape == q.shape
        for b, n in enumerate(PROMPTS):
            twin.prefill_request(b, q[b:b + 1, :, :n], k[b:b + 1, :, :n], k[b:b + 1, :, :n], l)
    assert _same(_mirror(cache, not device_store), _mirror(twin, not device_store))
    names = [e[0] for e in log]
    assert ("store_ragged_wide" in names) == device_store and "store_ragged" not in names and "chunk" not in names
    if device_store:
        kw = [e[1] for e in log if e[0] == "store_ragged_wide"][0]
        assert kw == dict(M=64, C=1024, page_size=R.PS, packed=packed)
    before = _mirror(cache)
    with pytest.raises(RuntimeError, match="paged_turns.prefill_ragged: slot 0 holds tokens"):
        paged_turns.prefill_ragged(cache, q, k, k, 0, [5, 0, 0], device_store=device_store)
    q1, k1 = _rows(1, R.BS)
    for c in (cache, twin):
        for step in range(10):
            for l in range(R.LAYERS):
                paged_turns.decode(c, q1, k1, k1, l, use_dev_lengths=True)
    # capacity: slot 2 would pass max_tokens - refused before anything is joined or launched
    before, n_log = _mirror(cache), len(log)
    qb, kb = _rows(R.MAX_TOKENS, R.BS)
    with pytest.raises(RuntimeError, match="exceed max_tokens"):
        paged_turns.extend_ragged(cache, qb, kb, kb, 0, [5, 0, R.MAX_TOKENS - 40], device_store=device_store)
    assert _same(before, _mirror(cache)) and len(log) == n_log
    q9, k9 = _rows(9, R.BS)
    n_new = [5, 0, 9]
    del log[:]
    for l in range(R.LAYERS):
        out = paged_turns.extend_ragged(cache, q9, k9, k9, l, n_new, device_store=device_store)
        assert out.shape == q9.shape
        for b, n in enumerate(n_new):
            if n:
                paged_turns.extend_request(twin, b, q9[b:b + 1, :, :n], k9[b:b + 1, :, :n], k9[b:b + 1, :, :n], l)
    assert _same(_mirror(cache, not device_store), _mirror(twin, not device_store))
    assert cache._T_a[0].tolist() == [85, 45, 52] and cache._r_a[0].tolist() == [0, 10, 0]
    ragged = [e for e in log if e[0] == ("chunk_packed" if packed else "chunk_wide") and e[1].get("dev_n_q") is not None]
    assert len(ragged) == R.LAYERS and ragged[0][1]["dev_lengths"] is cache.lengths[0] and ragged[0][1]["n_tokens"] == 70


def test_the_cache_s_own_methods_still_refuse(monkeypatch):
    log = []
    cache = _host_cache(monkeypatch, log)
    _prompts(cache)
    q, k = _rows(5, R.BS)
    before, n_log = _mirror(cache), len(log)
    with pytest.raises(NotImplementedError, match="prefill_ragged of a cache with nbits=10"):
        cache.prefill_ragged(q, k, k, 0, [0, 0, 0])
    with pytest.raises(NotImplementedError, match="extend_ragged of a cache with nbits=10"):
        cache.extend_ragged(q, k, k, 0, [5, 0, 2])
    cache._r_a[:, 0] = R.CAP
    state = _mirror(cache)
    q1, k1 = _rows(1, R.BS)
    with pytest.raises(RuntimeError, match="lockstep"):
        cache.decoding_with_pages(q1, k1, k1, 0, use_dev_lengths=True)
    with pytest.raises(RuntimeError, match="lockstep"):
        cache.flush_to_pages(0, use_dev_lengths=True)
    assert _same(state, _mirror(cache)) and len(log) == n_log
    cache._r_a[:, 0] = 0
    assert _same(before, _mirror(cache))
