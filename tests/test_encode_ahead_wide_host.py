"""CPU side of encode-ahead on wide paged caches (include/million_hip.h: million_pq_flush_wide_layers; million_amd.paged_turns:
next_step_kind, begin_step, note_replayed_step): the symbol is prototyped, declared and exported; the entry refuses
bad shapes, arguments, nulls and alignments before any HIP call, in million_pq_flush_wide's order; ops.pq_flush_wide reaches the
one-layer entry exactly as before with 4-D windows and advance=True and the layered entry otherwise, and refuses mismatched layers
before the library; the step-kind state machine of paged_turns on CPU caches with the launches stubbed, in the style of
tests/test_ragged_wide_host.py - while the cache's own methods on the same wide cache keep saying 'plain' / 'flush' and launch
nothing."""
import ctypes

import numpy as np
import pytest

from tests import ragged_wide_common as R
from tests.test_flush_wide_host import A, ERR_ALIGN, ERR_ARG, ERR_SHAPE, _fdesc, _ops_args
from tests.test_ragged_wide_host import KW, _host_cache, _rows

NAME = "million_pq_flush_wide_layers"


@pytest.fixture(scope="module")
def lib():
    from million_amd import build, _lib
    build.build()
    return _lib.load()


def test_symbol(lib):
    from million_amd import _lib as L
    vp, i32, i64 = ctypes.c_void_p, ctypes.c_int32, ctypes.c_int64
    assert L.SYMBOLS[NAME] == (i32, [ctypes.POINTER(L.EncodeDesc)] + [vp] * 8 + [i32, i32, i32, i64, i64, i64, i32, i32, i32, vp])
    header = (L.HERE.parent / "include" / "million_hip.h").read_text()
    assert NAME + "(" in header and hasattr(lib, NAME)
    from million_amd import ops
    assert [f.flush_layers for f in ops.CODE_FORMATS] == ["million_pq_flush_layers"] + [NAME] * 2


def _call(lib, desc, cap=64, min_r=0, n_layers=3, strides=None, advance=0, packed=0, pif=0, **kw):
    a = dict(k_rows=A, v_rows=A + 0x10000, k_cents=A + 0x20000, v_cents=A + 0x30000, k_pool=A + 0x40000, v_pool=A + 0x50000,
             ids=A + 0x60000, dev=desc.dev_lengths)
    a.update(kw)
    x_ls, ids_ls, len_ls = strides or (desc.bs * desc.x_stride_b, desc.bs * desc.nh_k * desc.n_pages_cap, desc.bs * 4)
    return getattr(lib, NAME)(ctypes.byref(desc), a["k_rows"], a["v_rows"], a["k_cents"], a["v_cents"], a["k_pool"], a["v_pool"],
                              a["ids"], a["dev"], cap, min_r, n_layers, x_ls, ids_ls, len_ls, advance, packed, pif, None)


def _nulls(lib, desc, cap=64, n_layers=3, advance=0, packed=0):
    return getattr(lib, NAME)(ctypes.byref(desc), *([None] * 8), cap, 0, n_layers, 0, 0, 0, advance, packed, 0, None)


def test_flush_wide_layers_refuses_without_a_gpu(lib):
    from million_amd import _lib as L
    err = lib.million_last_error
    d = _fdesc(L)
    d.struct_size -= 8
    assert _call(lib, d) == ERR_ARG and b"flush_wide_layers" in err() and b"struct_size" in err()
    assert getattr(lib, NAME)(None, *([None] * 8), 64, 0, 3, 0, 0, 0, 0, 0, 0, None) == ERR_ARG
    # geometry, n > page_size, and the grid limit with layers: before any null pointer
    shapes = [dict(C=256), dict(C=300), dict(C=8192), dict(d=128, M=16), dict(d=96, M=48), dict(d=128, M=128), dict(ps=48), dict(ps=256),
              dict(n=33), dict(ps=64, n=65), dict(n=-1), dict(bs=0), dict(nhk=0), dict(bs=20000), dict(npc=0), dict(npc=2 ** 27)]
    for kw in shapes:
        for advance in (0, 1):
            d = _fdesc(L, **kw)
            assert _nulls(lib, d, advance=advance) == ERR_SHAPE, kw
            assert _call(lib, d, advance=advance) == ERR_SHAPE and b"flush_wide_layers" in err(), kw
            assert _call(lib, d, advance=advance, packed=1) == ERR_SHAPE, kw
    d = _fdesc(L, bs=100, nhk=8)      # 800 heads: one layer fits the grid, 41 layers do not (41 * 800 * 2 > 65535)
    assert _nulls(lib, d, n_layers=40) == ERR_ARG and b"null" in err()
    assert _nulls(lib, d, n_layers=41) == ERR_SHAPE and b"exceeds the grid" in err()
    assert _nulls(lib, _fdesc(L), n_layers=-1) == ERR_SHAPE and b"n_layers" in err()
    # nothing to flush, whatever the pointers
    assert _nulls(lib, _fdesc(L, n=0)) == 0 and _nulls(lib, _fdesc(L), n_layers=0) == 0 and _nulls(lib, _fdesc(L, n=0), advance=1) == 0
    for kw in (dict(), dict(C=512), dict(C=4096, M=32), dict(d=64, M=32, C=2048), dict(ps=64, cap=128, n=64)):
        for packed in (0, 1):
            for advance in (0, 1):
                assert _nulls(lib, _fdesc(L, **kw), cap=kw.get("cap", 64), advance=advance, packed=packed) == ERR_ARG and b"flush_wide_layers: null" in err(), kw
    d = _fdesc(L)
    for part in ("k_rows", "v_rows", "k_cents", "v_cents", "k_pool", "v_pool", "ids"):
        assert _call(lib, d, **{part: None}) == ERR_ARG and b"null" in err(), part
    for part in ("k_rows", "v_rows", "k_cents", "v_cents", "k_pool", "v_pool"):
        assert _call(lib, d, **{part: A + 0xc0008}) == ERR_ALIGN and b"flush_wide_layers" in err() and b"16-byte" in err(), part
    assert _call(lib, d, ids=A + 0x60002) == ERR_ALIGN and b"4-byte" in err()
    assert _call(lib, _fdesc(L, x_stride_n=132)) == ERR_ALIGN and b"strides" in err()
    assert _call(lib, d, strides=(3 * 2 * 64 * 128 + 4, 96, 12)) == ERR_ALIGN and b"strides" in err()      # the layer stride of the windows
    # the arguments around the descriptor
    assert _call(lib, _fdesc(L, dst_layout=L.MILLION_CODES_ROWMAJOR)) == ERR_ARG and b"KPAGES" in err()
    assert _call(lib, d, cap=0) == ERR_ARG and _call(lib, d, cap=128) == ERR_ARG and b"x_row_mod" in err()
    assert _call(lib, d, dev=A + 0x70000) == ERR_ARG and b"dev_lengths must equal" in err()
    dv = _fdesc(L, dev=A + 0x70000)
    assert _call(lib, dv, min_r=65) == ERR_ARG and _call(lib, dv, min_r=-1) == ERR_ARG and b"min_r" in err()
    assert _call(lib, d, pif=-1) == ERR_ARG and b"pairs_in_flight" in err()
    assert _call(lib, _fdesc(L, dev=A + 0x70002), min_r=32) == ERR_ALIGN
    assert _call(lib, _fdesc(L, dst_token_start=-1)) == ERR_ARG and b"dst_token_start" in err()
    assert _call(lib, _fdesc(L, dst_token_start=512 - 31)) == ERR_ARG and b"too short" in err()
    assert _call(lib, _fdesc(L, x_row_start=64)) == ERR_ARG and b"x_row_start" in err()
    assert _call(lib, _fdesc(L, dev=A + 0x70000, dst_token_start=-1, x_row_start=99), k_rows=None) == ERR_ARG and b"null" in err()      # not read with device lengths


# ---------------------------------------------------------------- ops ------------------------------------------------------
class _Lib:
    """Stands in for the loaded library: records (entry, arguments) and answers MILLION_OK."""

    def __init__(self, log):
        self.log = log

    def __getattr__(self, name):
        return lambda *a: (self.log.append((name, a)), 0)[1]


@pytest.mark.parametrize("packed", [False, True])
def test_ops_picks_the_entry(monkeypatch, packed):
    import torch
    from million_amd import ops
    log = []
    monkeypatch.setattr(ops, "_need_cuda", lambda *a: None)
    monkeypatch.setattr(ops, "_stream", lambda: 77)
    monkeypatch.setattr(ops.L, "load", lambda: _Lib(log))
    a = _ops_args(torch, packed)
    win, ids, lengths = a["win"], a["ids"], a["lengths"]
    ptrs = lambda w, i: (w.data_ptr(), w.data_ptr(), a["cents"].data_ptr(), a["cents"].data_ptr(), a["kp"].data_ptr(), a["vp"].data_ptr(), i.data_ptr())
    flush = lambda w, i, **kw: ops.pq_flush_wide(w, w, a["cents"], a["cents"], a["kp"], a["vp"], i, n=32, page_size=32, packed=packed, **kw)

    # 4-D, advance=True: million_pq_flush_wide with the arguments it always had
    flush(win, ids, dev_lengths=lengths, min_r=64)
    flush(win, ids, token_start=45, x_row_start=40, min_r=64)
    (n1, a1), (n2, a2) = log
    assert n1 == n2 == "million_pq_flush_wide" and len(a1) == 13
    assert a1[1:] == ptrs(win, ids) + (lengths.data_ptr(), 64, 64, int(packed), 77)
    assert a2[1:] == ptrs(win, ids) + (0, 64, 0, int(packed), 77)      # host lengths: min_r is not handed on
    d1, d2 = a1[0]._obj, a2[0]._obj
    assert (d1.bs, d1.nh_k, d1.n, d1.page_size, d1.n_pages_cap, d1.x_row_mod, d1.dev_lengths) == (3, 2, 32, 32, 16, 64, lengths.data_ptr())
    assert (d2.dst_token_start, d2.x_row_start, d2.dev_lengths) == (45, 40, None)

    # 4-D, advance=False: the layered entry, one layer, no strides
    del log[:]
    flush(win, ids, dev_lengths=lengths, min_r=32, advance=False, pairs_in_flight=2)
    (n1, a1), = log
    assert n1 == NAME and a1[1:] == ptrs(win, ids) + (lengths.data_ptr(), 64, 32, 1, 0, 0, 0, 0, int(packed), 2, 77)

    # 5-D: the layered entry with the strides of the layers; layers 1 .. 2 of a cache's 4
    W5 = torch.zeros(4, 3, 2, 64, 128, dtype=torch.float16)
    I5, L5 = torch.zeros(4, 3, 2, 16, dtype=torch.int32), torch.zeros(4, 3, 4, dtype=torch.int32)
    for advance in (True, False):
        del log[:]
        flush(W5[1:3], I5[1:3], dev_lengths=L5[1:3], min_r=32, advance=advance)
        flush(W5[1:3], I5[1:3], token_start=45, x_row_start=40, advance=advance)
        (n1, a1), (n2, a2) = log
        assert n1 == n2 == NAME
        assert a1[1:] == ptrs(W5[1], I5[1]) + (L5[1].data_ptr(), 64, 32, 2, 3 * 2 * 64 * 128, 3 * 2 * 16, 12, int(advance), int(packed), 0, 77)
        assert a2[1:] == ptrs(W5[1], I5[1]) + (0, 64, 0, 2, 3 * 2 * 64 * 128, 3 * 2 * 16, 0, int(advance), int(packed), 0, 77)
        assert a1[0]._obj.dev_lengths == L5[1].data_ptr() and (a1[0]._obj.bs, a1[0]._obj.x_stride_b) == (3, 2 * 64 * 128)

    # refused before the library
    del log[:]
    bad = [(dict(w=W5, i=I5[:3]), "layers"), (dict(w=W5, i=ids), "layered page_ids"), (dict(w=W5, i=I5, dev_lengths=L5[:2]), "layers"),
           (dict(w=W5, i=I5, dev_lengths=lengths), "layers"), (dict(w=W5, i=I5[:, :, :, :8]), "contiguous"),
           (dict(w=W5, i=I5, dev_lengths=L5[:, :, :2]), "contiguous|dev_lengths"), (dict(w=win, i=ids, pairs_in_flight=2), "pairs_in_flight"),
           (dict(w=win, i=ids, advance=False, pairs_in_flight=0), "pairs_in_flight"), (dict(w=W5, i=I5, n=33, advance=False), "n=33")]
    for kw, msg in bad:
        kw = dict(kw)
        w, i, n = kw.pop("w"), kw.pop("i"), kw.pop("n", 32)
        with pytest.raises(RuntimeError, match="pq_flush_wide.*(" + msg + ")"):
            ops.pq_flush_wide(w, w, a["cents"], a["cents"], a["kp"], a["vp"], i, n=n, page_size=32, packed=packed, **kw)
    v5 = torch.zeros(4, 3, 2, 64, 256, dtype=torch.float16)[..., :128]      # another layer stride than K's
    with pytest.raises(RuntimeError, match="pq_flush_wide.*layer stride"):
        ops.pq_flush_wide(W5, v5, a["cents"], a["cents"], a["kp"], a["vp"], I5, n=32, page_size=32, packed=packed)
    assert not log


def test_flush_pages_hands_advance_and_layers_through(monkeypatch):
    from million_amd import ops
    log = []
    for name in ("pq_flush", "pq_flush_wide"):
        monkeypatch.setattr(ops, name, lambda *a, _n=name, **k: log.append((_n, a, k)))
    kw = dict(n=32, page_size=32, token_start=45, x_row_start=40, dev_lengths="len5", min_r=32, advance=False)
    for fmt, name, extra in ((ops.FMT_U8, "pq_flush", {}), (ops.FMT_U16, "pq_flush_wide", dict(packed=False)), (ops.FMT_PACKED, "pq_flush_wide", dict(packed=True))):
        del log[:]
        fmt.flush_pages("kw5", "vw5", ("kc", "vc"), "kpool", "vpool", "ids5", **kw)
        assert log == [(name, ("kw5", "vw5", "kc", "vc", "kpool", "vpool", "ids5"), dict(kw, **extra))], fmt.name


# ---------------------------------------------------------------- the step kinds --------------------------------------------
class _Stream:
    def wait_stream(self, other):
        pass

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        return False


def _wide_cache(monkeypatch, log, packed=False, steps=None, **kw):
    """A CPU cache with nbits 10, every launch recorded (tests/test_ragged_wide_host.py) and the side stream a dummy."""
    import torch
    monkeypatch.setattr(torch.cuda, "current_stream", lambda *a, **k: _Stream())
    monkeypatch.setattr(torch.cuda, "Stream", lambda *a, **k: _Stream())
    monkeypatch.setattr(torch.cuda, "stream", lambda s: s)
    monkeypatch.setattr(torch.cuda, "is_current_stream_capturing", lambda: False)
    cache = _host_cache(monkeypatch, log, packed=packed)
    cache.encode_ahead_steps = steps
    return cache


def _prefill(cache, n=45):
    q, k = _rows(n, R.BS)
    for l in range(R.LAYERS):
        cache.prefill(q, k, k, l)


def _step(cache, paged_turns, use_dl=True):
    q1, k1 = _rows(1, R.BS)
    kind = paged_turns.begin_step(cache, use_dev_lengths=use_dl)
    for l in range(R.LAYERS):
        paged_turns.decode(cache, q1, k1, k1, l, use_dev_lengths=use_dl)
    return kind


@pytest.mark.parametrize("packed", [False, True])
@pytest.mark.parametrize("use_dl", [False, True])
@pytest.mark.parametrize("steps", [1, 2])
def test_three_flush_periods_in_lockstep(monkeypatch, packed, use_dl, steps):
    """plain ... pre ... commit, never 'flush'; 'pre0', 'pre1' when the layers are spread; one encode launch per 'pre' step with
    advance=False, one lengths_advance per 'commit' with device lengths, no flush launch in any decode call; the mirror is the
    in-line route's after every step; the cache's own next_step_kind / begin_step say 'plain' / 'flush' and launch nothing."""
    from million_amd import paged_turns
    log, ref_flushes = [], 0
    cache = _wide_cache(monkeypatch, log, packed, steps)
    _prefill(cache)
    ref = _host_cache(monkeypatch, log, packed=packed)      # in line: paged_turns.decode without begin_step (one recorder, one log)
    _prefill(ref)
    q1, k1 = _rows(1, R.BS)
    dec = "decode_packed" if packed else "decode_wide"
    at = cache.encode_ahead_at()
    assert at == R.CAP - R.PS + 4
    kinds = []
    for step in range(R.CAP + 2 * R.PS + 2):
        r = int(cache._r_a[0, 0])
        own = cache.next_step_kind()
        assert own == ("flush" if r >= R.CAP else "plain")
        n_log = len(log)
        assert cache.begin_step(use_dev_lengths=use_dl) == own and len(log) == n_log, "the cache's own begin_step launches nothing"
        assert cache.flush_ahead(use_dev_lengths=use_dl) is None and len(log) == n_log
        want = paged_turns.next_step_kind(cache)
        del log[:]
        kind = _step(cache, paged_turns, use_dl)
        assert kind == want
        kinds.append(kind)
        names = [e[0] for e in log]
        for l in range(R.LAYERS):
            paged_turns.decode(ref, q1, k1, k1, l, use_dev_lengths=use_dl)
        ref_flushes += [e[0] for e in log[len(names):]].count("flush_wide")
        if kind.startswith("pre"):
            g = int(kind[3:] or 0)
            assert names == ["flush_wide"] + [dec] * R.LAYERS, (step, names)
            kw = log[0][1]
            lo, hi = (0, R.LAYERS) if steps == 1 else (g, g + 1)
            assert (kw["n"], kw["page_size"], kw["advance"], kw["packed"], kw["min_r"]) == (R.PS, R.PS, False, packed, R.PS if use_dl else 0)
            assert (kw["token_start"], kw["x_row_start"]) == (int(cache._T_a[0, 0]), int(cache._rs_a[0, 0]))
            if use_dl:
                assert kw["dev_lengths"].data_ptr() == cache._lengths_all[lo].data_ptr() and kw["dev_lengths"].shape == (hi - lo, R.BS, 4)
            else:
                assert kw["dev_lengths"] is None
        elif kind == "commit":
            assert names == (["advance"] if use_dl else []) + [dec] * R.LAYERS, (step, names)
        else:
            assert kind == "plain" and names == [dec] * R.LAYERS, (step, kind, names)
        for x, y in zip(cache.host_state()[:4], ref.host_state()[:4]):
            assert np.array_equal(x, y), step
    assert "flush" not in kinds and kinds.count("commit") == 3
    pre = [i for i, k in enumerate(kinds) if k.startswith("pre")]
    assert [kinds[i] for i in pre] == (["pre"] if steps == 1 else ["pre0", "pre1"]) * 3
    assert pre[0] == at and kinds.index("commit") == R.CAP      # the first window: filled from empty
    assert ref_flushes == 3 * R.LAYERS      # the twin flushed in line, layer by layer


def test_default_spread_of_a_wide_cache(monkeypatch):
    """The default spread: a wide cache hides EA_WIDE_UNITS units of d x C per request (up to 4 requests) in a step, an 8-bit one 32
    pairs; the knob wins; never more steps than layers or than page_size - 16."""
    from million_amd.pq_cache import PagedPQCache
    assert (PagedPQCache.EA_PAIRS, PagedPQCache.EA_WIDE_UNITS) == (32, 1 << 21)
    cache = _wide_cache(monkeypatch, [])      # d 128, C 1024, 3 requests: 48 pairs per step, 6 pairs in all
    assert cache._ea_pairs() == 48 and cache._ea_groups() == [(0, R.LAYERS)]
    for bs, C, layers, pairs, groups in ((1, 4096, 32, 4, 8), (8, 4096, 32, 16, 16), (1, 1024, 32, 16, 2), (8, 1024, 32, 64, 4), (8, 512, 32, 128, 2),
                                         (1, 512, 32, 32, 1), (64, 4096, 32, 16, 32)):
        cache.bs, cache.C, cache.layer_num, cache.page_size = bs, C, layers, 64
        assert cache._ea_pairs() == pairs and len(cache._ea_groups()) == groups, (bs, C)
        assert cache._ea_groups()[0] == (0, layers // groups) and cache._ea_groups()[-1][1] == layers
    cache.bs, cache.C, cache.layer_num, cache.page_size = R.BS, 1024, R.LAYERS, R.PS
    cache.encode_ahead_steps = 2
    assert cache._ea_groups() == [(0, 1), (1, 2)]
    cache.encode_ahead_steps = 99
    assert cache._ea_groups() == [(0, 1), (1, 2)]
    u8 = _host_cache(monkeypatch, [], nbits=8)
    assert u8._ea_pairs() == 32 and u8._ea_groups() == [(0, R.LAYERS)]


def test_falls_back_when_requests_differ(monkeypatch):
    """Requests at different lengths: 'plain' / 'flush' only, and decode flushes in line; a slot released after a 'pre' step and
    prefilled again: its flag is gone, the batch is ragged, the kinds fall back."""
    from million_amd import paged_turns
    log = []
    cache = _wide_cache(monkeypatch, log, steps=1)
    _prefill(cache)
    kinds = [_step(cache, paged_turns) for _ in range(cache.encode_ahead_at() + 1)]
    assert kinds[-1] == "pre" and cache._pre_a.all()
    cache.release(1)
    q, k = _rows(20)
    for l in range(R.LAYERS):
        cache.prefill_request(1, q, k, k, l)
    assert not cache._pre_a[:, 1].any() and cache._pre_a[:, 0].all()
    seen = []
    for step in range(R.CAP):
        full = (cache._r_a[0] >= R.CAP)
        want = "flush" if full.any() else "plain"
        assert paged_turns.next_step_kind(cache) == want
        del log[:]
        assert _step(cache, paged_turns) == want
        seen.append(want)
        assert [e[0] for e in log].count("flush_wide") == (R.LAYERS if full.any() else 0)
        if full.any():
            assert log[0][1].get("advance", True) is True and log[0][1]["min_r"] == R.CAP
    assert seen.count("flush") == 2      # slots 0 and 2 together, slot 1 at a step of its own
    with pytest.raises(RuntimeError, match="different lengths"):
        _step(cache, paged_turns, use_dl=False)


def test_skipped_begin_step_flushes_in_line(monkeypatch):
    from million_amd import paged_turns
    log = []
    cache = _wide_cache(monkeypatch, log, steps=1)
    _prefill(cache)
    q1, k1 = _rows(1, R.BS)
    for step in range(R.CAP):      # no begin_step: nothing is encoded ahead
        for l in range(R.LAYERS):
            paged_turns.decode(cache, q1, k1, k1, l, use_dev_lengths=True)
    assert not cache._pre_a.any() and paged_turns.next_step_kind(cache) == "flush"
    del log[:]
    assert _step(cache, paged_turns) == "flush"
    assert [e[0] for e in log] == ["flush_wide", "decode_wide"] * R.LAYERS


@pytest.mark.parametrize("steps", [1, 2])
def test_note_replayed_step_leaves_the_live_mirror(monkeypatch, steps):
    """A replayed step moves the mirror as the live step does: twins, one stepped live, one only noted - default kind and given."""
    from million_amd import paged_turns
    live, noted = _wide_cache(monkeypatch, [], steps=steps), _wide_cache(monkeypatch, [], steps=steps)
    _prefill(live)
    _prefill(noted)
    for step in range(R.CAP + R.PS + 4):
        kind = paged_turns.next_step_kind(noted)
        assert kind == _step(live, paged_turns)
        paged_turns.note_replayed_step(noted, *(() if step % 2 else (kind,)))
        for x, y in zip(live.host_state(), noted.host_state()):
            assert np.array_equal(x, y), (step, kind)
    names = [k for k, _ in noted.capture_states()]
    assert names == ["plain"] + (["pre"] if steps == 1 else ["pre0", "pre1"]) + ["commit", "flush"]
    for kind, state in noted.capture_states():      # every captured state is the kind it is captured for
        noted.set_host_state(state)
        assert paged_turns.next_step_kind(noted) == kind


def test_an_8_bit_cache_is_handed_to_its_own_methods(monkeypatch):
    from million_amd import paged_turns
    calls = []
    cache = _host_cache(monkeypatch, [], nbits=8)
    monkeypatch.setattr(cache, "next_step_kind", lambda: calls.append("kind") or "plain")
    monkeypatch.setattr(cache, "begin_step", lambda use_dev_lengths=False: calls.append(("begin", use_dev_lengths)) or "plain")
    monkeypatch.setattr(cache, "note_replayed_step", lambda kind=None: calls.append(("note", kind)))
    assert paged_turns.next_step_kind(cache) == "plain" and paged_turns.begin_step(cache, use_dev_lengths=True) == "plain"
    paged_turns.note_replayed_step(cache)
    paged_turns.note_replayed_step(cache, "commit")
    assert calls == ["kind", ("begin", True), ("note", None), ("note", "commit")]
    assert KW["device"] == "cpu"
