"""CPU side of draft verification on wide caches: the C entries million_window_commit_wide / _rows_wide are
declared, prototyped and refuse what they must before any launch or look at a pointer; and the host logic of paged_turns.verify /
commit - on CPU caches with the launches stubbed - takes the format's launches, refuses a "heads" verify of more rows than the wide
decode kernel has columns before anything moves, picks the default route by the measured rule (pinned at its boundaries), moves the
mirror as the same number of paged_turns.decode steps, refuses what the 8-bit commit refuses before anything moves, hands an 8-bit
cache to its own methods and leaves the cache's own methods refusing."""
import ctypes

import numpy as np
import pytest

from tests import ragged_wide_common as R
from tests.test_attn_wide_host import A, ERR_ALIGN, ERR_ARG, ERR_SHAPE
from tests.test_verify_host import _wc_desc


@pytest.fixture(scope="module")
def lib():
    from million_amd import build, _lib
    build.build()
    return _lib.load()


COMMIT_ENTRIES = ("million_window_commit_wide", "million_window_commit_rows_wide")


# ---------------------------------------------------------------- symbols, header, the format table -------------------------
def test_symbols_and_header(lib):
    from million_amd import _lib as L
    from million_amd import ops
    vp, i32 = ctypes.c_void_p, ctypes.c_int32
    assert L.SYMBOLS["million_window_commit_wide"] == (i32, [ctypes.POINTER(L.WindowCommitDesc)] + [vp] * 11 + [i32, vp])
    assert L.SYMBOLS["million_window_commit_rows_wide"] == (i32, [ctypes.POINTER(L.WindowCommitDesc)] + [vp] * 12 + [i32, vp])
    header = (L.HERE.parent / "include" / "million_hip.h").read_text()
    for name in COMMIT_ENTRIES:
        assert name + "(" in header and hasattr(lib, name), name
    # every format names its commit entries - the ops call them by these names - and has the job a cache asks; a verification's decode
    # pass is the format's decode entry (decode_attn, decode_pages without an append)
    for f in ops.CODE_FORMATS:
        for field in ("commit", "commit_rows", "decode_attn"):
            assert getattr(f, field) in L.SYMBOLS, (f.name, field)
        assert callable(f.commit_pages) and callable(f.decode_pages)
    assert (ops.FMT_U8.commit, ops.FMT_U8.commit_rows) == ("million_window_commit", "million_window_commit_rows")
    assert ops.FMT_U16.commit == ops.FMT_PACKED.commit == COMMIT_ENTRIES[0] and ops.FMT_U16.commit_rows == ops.FMT_PACKED.commit_rows == COMMIT_ENTRIES[1]
    assert callable(ops.window_commit_wide)


def test_the_commit_job_hands_each_op_its_own_keywords(monkeypatch):
    from million_amd import ops
    log = []
    for name in ("window_commit", "window_commit_wide"):
        monkeypatch.setattr(ops, name, lambda *a, _n=name, **k: log.append((_n, a, k)))
    cents, prep = ("kc", "vc"), ("kp", "vp")
    for f in ops.CODE_FORMATS:
        f.commit_pages("kn", "vn", "kres", "vres", cents, prep, "kpool", "vpool", "ids", "len", "dev_n", M=64, C=1024, n_bound=4)
        assert log[-1] == ("window_commit" if f.prepared else "window_commit_wide",
                           ("kn", "vn", "kres", "vres", *(prep if f.prepared else cents), "kpool", "vpool", "ids", "len", "dev_n"),
                           dict(n_bound=4, **(dict(M=64, C=1024) if f.prepared else {"packed": f is ops.FMT_PACKED})))


# ---------------------------------------------------------------- the commit entries refuse before any launch ---------------
_WC_ARGS = ("k_new", "v_new", "k_resid", "v_resid", "k_cents", "v_cents", "k_pool", "v_pool", "page_ids", "dev_lengths", "dev_n")


def _wc_call(lib, name, desc, packed=0, **over):
    args = {nm: A + 0x10000 * i for i, nm in enumerate(_WC_ARGS)}
    args["dev_rows"] = A + 0x10000 * len(_WC_ARGS)
    args.update(over)
    rows = [args["dev_rows"]] if name.endswith("rows_wide") else []
    return getattr(lib, name)(ctypes.byref(desc), *[args[nm] for nm in _WC_ARGS], *rows, packed, None)


@pytest.mark.parametrize("name", COMMIT_ENTRIES)
def test_commit_entry_refuses_without_a_gpu(lib, name):
    from million_amd import _lib as L
    err = lib.million_last_error
    wide = lambda **kw: _wc_desc(L, **{"C": 1024, **kw})
    nulls = [None] * (12 if name.endswith("rows_wide") else 11)
    d = wide()
    d.struct_size += 8
    assert _wc_call(lib, name, d) == ERR_ARG and b"struct_size" in err()
    # C = 256 (8-bit codes), C no power of two, d / M = 8, d = 96, packed pages with M no multiple of 4; n_bound; page_size; resid_cap
    for kw, word in ((dict(C=256), b"C=256"), (dict(C=768), b"C=768"), (dict(M=16), b"M=16"), (dict(d=96, M=48), b"d=96"), (dict(n_bound=0, ps=64), b"n_bound"),
                     (dict(n_bound=17, ps=64), b"n_bound"), (dict(n_bound=33, ps=32), b"page_size=32"), (dict(ps=48), b"page_size"),
                     (dict(ps=64, cap=32), b"resid_cap")):
        d = wide(**kw)
        assert getattr(lib, name)(ctypes.byref(d), *nulls, 0, None) == ERR_SHAPE and word in err(), kw      # with every pointer null
        assert _wc_call(lib, name, d) == ERR_SHAPE and name[len("million_"):].encode() in err(), kw
    for kw in (dict(), dict(C=512), dict(C=4096, M=32), dict(d=64, M=32, C=2048), dict(d=64, M=16, C=512), dict(ps=64), dict(ps=128, cap=128)):
        for packed in (0, 1):
            assert getattr(lib, name)(ctypes.byref(wide(**kw)), *nulls, packed, None) == ERR_ARG and b"null" in err(), kw
    for part in _WC_ARGS + (("dev_rows",) if name.endswith("rows_wide") else ()):
        assert _wc_call(lib, name, wide(), **{part: None}) == ERR_ARG and b"null" in err(), part
    assert _wc_call(lib, name, wide(), k_cents=None) == ERR_ARG and b"plain" in err()      # the codebooks as they are: no prepared image
    assert _wc_call(lib, name, wide(), k_new=A + 8) == ERR_ALIGN and b"aligned" in err()
    assert _wc_call(lib, name, wide(), k_cents=A + 0x40008) == ERR_ALIGN
    assert _wc_call(lib, name, wide(), dev_n=A + 2) == ERR_ALIGN
    if name.endswith("rows_wide"):
        assert _wc_call(lib, name, wide(), dev_rows=A + 2) == ERR_ALIGN and b"dev_rows" in err()
    d = wide()
    d.new_stride_n = 132
    assert _wc_call(lib, name, d) == ERR_ALIGN and b"stride" in err()
    d = wide()
    d.lengths_layer_stride = 4
    assert _wc_call(lib, name, d) == ERR_ARG and b"layer strides" in err()
    # the 8-bit entries keep refusing wide codebooks
    assert lib.million_window_commit(ctypes.byref(wide()), *([A] * 11), None) == ERR_SHAPE


# ---------------------------------------------------------------- paged_turns.verify / commit on the host -------------------
KW = dict(nh=R.NH, num_key_value_heads=R.NHK, M=64, layer_num=R.LAYERS, d=128, page_size=R.PS, extended_residual_size=R.CAP, max_tokens=256,
          device="cpu")


def _host_cache(monkeypatch, log, *, bs=3, nbits=10, packed=False, preallocate=True):
    """A PagedPQCache on the CPU with every launch stubbed and logged by name: what is left is the host logic."""
    import torch
    from million_amd import ops
    from million_amd.pq_cache import PagedPQCache
    rec = lambda name, ret=None: (lambda *a, **k: (log.append((name, a, k)), ret(*a, **k) if ret else None)[1])
    heads = lambda q, *a, **k: (torch.zeros_like(q), torch.zeros(q.shape[0], q.shape[1], 1))
    chunk = lambda q, *a, **k: (torch.zeros_like(q), torch.zeros(q.shape[:3])) if k.get("return_lse") else torch.zeros_like(q)
    zeros_q = lambda q, *a, **k: (torch.zeros_like(q), torch.zeros(q.shape[0], q.shape[1], 1)) if k.get("return_lse") else torch.zeros_like(q)
    for name, ret in (("pq_encode_into", None), ("pq_encode_into_packed", None), ("prefill_attn", lambda q, k, v, **kw: torch.zeros_like(q)),
                      ("pq_decode_attn", heads), ("pq_chunk_attn", chunk), ("pq_chunk_attn_wide", chunk),
                      ("pq_chunk_attn_packed", chunk), ("pq_decode_attn_wide", zeros_q), ("pq_decode_attn_packed", zeros_q), ("pq_flush", None),
                      ("pq_flush_wide", None), ("lengths_advance", None), ("window_commit", None), ("window_commit_wide", None),
                      ("attn_block_merge", lambda q, k, v, out_a, lse_a, dev_n, **kw: (out_a, lse_a) if kw.get("return_lse") else out_a),
                      ("decode_workspace_bytes", lambda *a, **k: 16),
                      ("decode_wide_workspace_bytes", lambda *a, **k: 16)):
        monkeypatch.setattr(ops, name, rec(name, ret))
    cache = PagedPQCache(**KW, bs=bs, nbits=nbits, dtype=torch.uint8 if nbits == 8 else torch.uint16, packed=packed, preallocate=preallocate)
    cache.key_cent = cache.value_cent = torch.zeros(64, 2 ** nbits, 2, dtype=torch.float16)
    cache._kprep = cache._vprep = None
    return cache


def _rows(bs, n):
    import torch
    return torch.zeros(bs, R.NH, n, 128, dtype=torch.float16), torch.zeros(bs, R.NHK, n, 128, dtype=torch.float16)


def _verify_all(cache, n=4, layers=None, **kw):
    from million_amd import paged_turns
    q, k = _rows(cache.bs, n)
    return [paged_turns.verify(cache, q, k, k, l, **kw) for l in (range(cache.layer_num) if layers is None else layers)]


def _mirror(cache):
    return [a.copy() for a in cache.host_state()] + [cache._pages_a.copy()]


def _place(cache, b, T, r, st):
    """Slot b of every layer at {T, r, start}, its pages assigned, without a launch."""
    cache._T_a[:, b], cache._r_a[:, b], cache._rs_a[:, b], cache._seen_a[:, b] = T, r, st, T + r
    if not cache.preallocate:
        for l in range(cache.layer_num):
            cache._assign_pages(l, -(-T // cache.page_size), b)


# (T, r, start) per slot and n_accept: no flush anywhere; exactly one flush (slot 0: r + a = cap + 1, slot 2: a full window); a slot
# that accepts nothing beside one that flushes
CASES = {"no-flush": ([(32, 10, 0), (0, 0, 0), (64, 60, 40)], [4, 2, 4]),
         "one-flush": ([(32, 61, 5), (0, 3, 0), (64, 64, 63)], [4, 1, 3]),
         "zero-slots": ([(32, 63, 5), (0, 0, 0), (64, 64, 63)], [0, 0, 2])}


@pytest.mark.parametrize("packed", [False, True])
@pytest.mark.parametrize("preallocate", [True, False])
@pytest.mark.parametrize("case", list(CASES))
def test_commit_moves_the_mirror_as_decode_steps(monkeypatch, case, preallocate, packed):
    from million_amd import paged_turns
    state, n_accept = CASES[case]
    log = []
    twins = [_host_cache(monkeypatch, log, bs=1, packed=packed, preallocate=preallocate) for _ in state]      # (the stubs are one set: one log)
    cache = _host_cache(monkeypatch, log, packed=packed, preallocate=preallocate)
    for b, row in enumerate(state):
        _place(cache, b, *row)
        _place(twins[b], 0, *row)
    out = _verify_all(cache, n_draft=[4, 2, 4], route="heads")
    assert all(o.shape == (3, R.NH, 4, 128) for o in out)
    names = [e[0] for e in log]
    dec = "pq_decode_attn_packed" if packed else "pq_decode_attn_wide"      # the format's decode launch over 16 rows per kv head, no append
    assert names == ["decode_wide_workspace_bytes"] + [dec, "attn_block_merge"] * R.LAYERS
    assert "k_new" not in log[1][2] and log[1][2]["return_lse"] and log[1][2]["workspace"].numel() == 16 and log[1][1][0].shape == (3, R.NH * 4, 1, 128)
    before = _mirror(cache)
    del log[:]
    paged_turns.commit(cache, n_accept)
    assert [e[0] for e in log] == ["window_commit_wide"] and log[0][2]["packed"] == packed and log[0][2]["n_bound"] == 4 and "dev_rows" not in log[0][2]
    assert log[0][1][10].tolist() == n_accept
    q1, k1 = _rows(1, 1)
    for b, tw in enumerate(twins):
        for _ in range(n_accept[b]):
            for l in range(R.LAYERS):
                paged_turns.decode(tw, q1, k1, k1, l, use_dev_lengths=True)
        for mine, theirs in zip(_mirror(cache), _mirror(tw)):
            assert np.array_equal(mine[:, b], theirs[:, 0]), (case, b, mine[:, b], theirs[:, 0])
    flushed = [b for b, ((T, r, st), a) in enumerate(zip(state, n_accept)) if a and r + a > R.CAP]
    assert flushed == {"no-flush": [], "one-flush": [0, 2], "zero-slots": [2]}[case]
    for b in range(3):
        assert (cache._T_a[:, b] == state[b][0] + (R.PS if b in flushed else 0)).all()
        if not n_accept[b]:
            assert all(np.array_equal(x[:, b], y[:, b]) for x, y in zip(before, _mirror(cache)))
    # life goes on: a decode step, a flush and an extend take the mirror from here
    q3, k3 = _rows(3, 1)
    for l in range(R.LAYERS):
        paged_turns.decode(cache, q3, k3, k3, l, use_dev_lengths=True)
    with pytest.raises(RuntimeError, match="verify"):
        paged_turns.commit(cache, [0, 0, 0])      # the verification was consumed


def test_routes_and_trees_take_the_format_s_ops(monkeypatch):
    from million_amd import paged_turns
    log = []
    cache = _host_cache(monkeypatch, log, packed=True)
    _place(cache, 0, 32, 10, 0)
    # the wide rule (profiles/verify_wide.txt), at each of its boundaries: 16 / 17 rows per kv head, 16383 / 16384 tokens of the longest
    # request, 8 / 9 rows and 1 / 2 requests below that
    assert [cache._verify_route(n) for n in (1, 2, 4, 5, 16)] == ["chunk"] * 5      # 3 requests, 32 tokens
    cache._T_a[1, 1] = 16383
    assert [cache._verify_route(n) for n in (1, 2, 4)] == ["chunk"] * 3
    cache._T_a[1, 1] = 16384      # one slot of one layer is enough: the longest request
    assert [cache._verify_route(n) for n in (1, 2, 4, 5, 16)] == ["heads", "heads", "heads", "chunk", "chunk"]
    cache._T_a[1, 1] = 32
    one = _host_cache(monkeypatch, log, bs=1)
    assert [one._verify_route(n) for n in (1, 2, 3, 4, 16)] == ["heads", "heads", "chunk", "chunk", "chunk"]      # 4, 8 | 12, 16, 64 rows
    one._T_a[:] = 16384
    assert [one._verify_route(n) for n in (3, 4, 5)] == ["heads", "heads", "chunk"]      # 12, 16 | 20 rows
    two = _host_cache(monkeypatch, log, bs=2)
    assert [two._verify_route(n) for n in (1, 2)] == ["chunk", "chunk"]
    assert (type(cache).VERIFY_WIDE_HEADS_ROWS, type(cache).VERIFY_WIDE_HEADS_TOKENS, type(cache).VERIFY_WIDE_SHORT_ROWS) == (16, 16384, 8)
    plain = _host_cache(monkeypatch, log, nbits=8)
    assert [plain._verify_route(n) for n in (4, 16, 17)] == ["heads", "heads", "chunk"]      # the 8-bit rule is what it was
    cache = _host_cache(monkeypatch, log, packed=True)      # (the stubs log into the last cache's list: this one again)
    _place(cache, 0, 32, 10, 0)
    _verify_all(cache, n=5)
    assert [e[0] for e in log] == ["pq_chunk_attn_packed"] * R.LAYERS and log[0][1][1] is not None      # the rows as chunk
    del log[:]
    # "heads" is one launch of a kernel with 16 score columns: 20 rows per kv head are refused before anything is joined or recorded
    _verify_all(cache, n=4, route="heads", layers=[0])
    rec, n_log = cache._verify_rec, len(log)
    with pytest.raises(RuntimeError, match=r"paged_turns.verify: route='heads' serves at most 16 rows per kv head .* got n \* nh / nh_k = 20; use route='chunk'"):
        _verify_all(cache, n=5, route="heads")
    assert cache._verify_rec is rec and rec["layers"] == {0} and len(log) == n_log
    del log[:]
    tree = [-1, 0, 1, -1, 3]
    _verify_all(cache, n=5, route="chunk", tree=tree)
    assert [e[0] for e in log] == ["pq_chunk_attn_packed", "attn_block_merge"] * R.LAYERS
    assert log[0][1][1] is None and log[1][2]["dev_mask"] is not None      # the past only, then the masked block
    del log[:]
    with pytest.raises(RuntimeError, match="path="):
        paged_turns.commit(cache, [2, 0, 0])      # chain commit after a tree
    with pytest.raises(RuntimeError, match="no chain from a root"):
        paged_turns.commit(cache, path=[[1, 2], [], []])
    assert not log
    paged_turns.commit(cache, path=[[3, 4], [0], []])
    assert [e[0] for e in log] == ["window_commit_wide"] and log[0][2]["dev_rows"].tolist() == [[3, 4, 0, 0, 0], [0, 0, 0, 0, 0], [0, 0, 0, 0, 0]]
    assert cache._r_a[0].tolist() == [12, 1, 0]
    with pytest.raises(RuntimeError, match=r"paged_turns.verify: route 'rows'"):
        _verify_all(cache, route="rows")
    with pytest.raises(RuntimeError, match=r"paged_turns.verify: 17 draft rows"):
        _verify_all(cache, n=17)


def test_commit_refusals_move_nothing(monkeypatch):
    """Every refusal of the 8-bit commit, on a wide cache: before the mirror, the pages or the launch log move."""
    from million_amd import paged_turns
    log = []
    cache = _host_cache(monkeypatch, log, preallocate=False)
    for b in range(3):
        _place(cache, b, 0, 62, 0)
    snap = lambda: _mirror(cache) + [set(cache.page_manager.free_pages)]
    same = lambda x, y: all(np.array_equal(a, b) if isinstance(a, np.ndarray) else a == b for a, b in zip(x, y))
    before = snap()

    def refused(match, n_accept=None, **kw):
        n_log = len(log)
        with pytest.raises(RuntimeError, match=match):
            paged_turns.commit(cache, n_accept, **kw)
        assert same(before, snap()) and len(log) == n_log

    refused("verify", [1, 1, 1])                       # no verify at all
    refused("n_accept or path")
    _verify_all(cache, layers=[0])
    refused("every layer", [1, 1, 1])                  # no full verify
    _verify_all(cache, n_draft=[4, 0, 2])
    refused("n_accept", [4, 1, 2])                     # n_accept > n_draft
    refused("n_accept", [4, 0])
    refused("n_accept", [-1, 0, 0])
    refused("whose paths are range", path=[[1], [], []])      # a path after a chain
    cache._r_a[1, 0] += 1                              # layer 1 of slot 0 a row ahead: mid-step
    before = snap()
    refused("mid-step", [1, 0, 0])
    cache._r_a[1, 0] -= 1
    taken = [cache.page_manager.allocate_page() for _ in range(len(cache.page_manager.free_pages) - 3)]      # a flush of one slot needs 4
    before = snap()
    refused("free pages", [4, 0, 0])                   # too few pages
    for pid in taken:
        cache.page_manager.free_page(pid)
    _place(cache, 1, 256, 62, 0)                       # the page table of slot 1 is full
    _verify_all(cache)
    before = snap()
    refused("max_tokens", [0, 3, 0])
    del log[:]
    paged_turns.commit(cache, [4, 0, 2])
    assert [e[0] for e in log] == ["window_commit_wide"] and cache._T_a[:, 0].tolist() == [32, 32] and cache._r_a[:, 0].tolist() == [34, 34]


def test_an_8_bit_cache_is_delegated_and_the_cache_s_own_methods_still_refuse(monkeypatch):
    from million_amd import paged_turns
    log = []
    plain = _host_cache(monkeypatch, log, nbits=8)
    _place(plain, 0, 32, 10, 0)
    calls = []
    monkeypatch.setattr(type(plain), "verify", lambda self, *a, **k: calls.append(("verify", a[3], k)) or "out")
    monkeypatch.setattr(type(plain), "commit", lambda self, *a, **k: calls.append(("commit", a, k)))
    q, k = _rows(3, 4)
    assert paged_turns.verify(plain, q, k, k, 1, n_draft=[4, 1, 0], route="chunk") == "out"
    paged_turns.commit(plain, [1, 1, 0])
    paged_turns.commit(plain, path=[[0], [], []])
    assert calls == [("verify", 1, dict(n_draft=[4, 1, 0], use_dev_lengths=True, route="chunk", return_lse=False, tree=None)),
                     ("commit", ([1, 1, 0],), dict(path=None)), ("commit", (None,), dict(path=[[0], [], []]))]
    monkeypatch.undo()
    log = []
    for packed in (False, True):
        wide = _host_cache(monkeypatch, log, packed=packed)
        before = _mirror(wide)
        with pytest.raises(NotImplementedError, match="verify of a cache with nbits=10"):
            wide.verify(q, k, k, 0)
        with pytest.raises(NotImplementedError, match="commit of a cache with nbits=10"):
            wide.commit([1, 1, 1])
        assert not log and all(np.array_equal(x, y) for x, y in zip(before, _mirror(wide)))
