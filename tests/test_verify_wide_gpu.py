"""Draft verification on wide caches on the GPU: million_amd.paged_turns.verify against an fp64 softmax over
what the cache holds on the device (tests/chunk_wide_model.py, tests/verify_tree_model.py); paged_turns.commit against batch-1 twin
caches that take the accepted rows through paged_turns.decode one by one; one captured "heads" verify replayed after a commit
moved the lengths.

Bars (the project's; tests/test_attn_wide_gpu.py, tests/test_verify_gpu.py).  Rows against fp64: rel-L2 < 1e-3, lse within
lse_ref.LSE_TOL.  Two routes against each other: 2e-3.  Everything a commit leaves - device lengths, host mirror, live codes (packed:
through both planes), live window rows - and the decode step after it: bitwise.

The "heads" route is one launch of the wide decode kernel, which has 16 score columns: at G = 4 it exists for n <= 4 and the test
asserts that n = 5 and n = 16 are refused by name, with the cache unmoved; the chunk route serves every n.

tests/cache_life_driver.py / tests/cache_verify_life.py model uint8 codes of 256 centroids (cache_life_model.Model, C) and call the
cache's own verify / commit: they take no wide backend without being edited, so there is no lifecycle file for wide caches."""
import numpy as np
import pytest

from tests import chunk_wide_model as CM
from tests import lse_ref as LR
from tests import ragged_wide_common as R
from tests import verify_tree_model as TM

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def env():
    import torch
    from million_amd import build, ops
    build.build()
    assert torch.cuda.is_available()
    yield torch, ops
    assert ops.tail_faults() == 0


# ---------------------------------------------------------------- caches ------------------------------------------------------
BS, NH, NHK, NL, CPS, CCAP = R.BS, R.NH, R.NHK, R.LAYERS, R.PS, R.CAP      # 3 slots, G = 4, 2 layers, page_size 32, window 64
CODES = [(128, 64, 10), (128, 32, 12)]      # (d, M, nbits): (M 64, C 1024), (M 32, C 4096)


def _books(d, M, nbits):
    rs = np.random.RandomState(2000 + nbits)
    return [rs.standard_normal((M, 2 ** nbits, d // M)).astype(np.float16) for _ in range(2)]


def _cache(torch, d, M, nbits, packed, bs=BS):
    from million_amd.pq_cache import PagedPQCache
    c = PagedPQCache(bs=bs, nh=NH, num_key_value_heads=NHK, M=M, layer_num=NL, d=d, page_size=CPS, extended_residual_size=CCAP,
                     max_tokens=R.MAX_TOKENS, nbits=nbits, dtype=torch.uint16, packed=packed, device="cuda")
    ck, cv = _books(d, M, nbits)
    c.set_cent(R.to_dev(torch, ck), R.to_dev(torch, cv))
    return c


def _rows(torch, rs, bs, n, d):
    f = lambda h: torch.from_numpy(rs.standard_normal((bs, h, n, d)).astype(np.float16)).cuda()
    return f(NH), f(NHK), f(NHK)


def _set_window(torch, cache, b, k_rows, v_rows, start):
    """Slot b of every layer: the window holds k_rows / v_rows (layers, nh_k, r, d) from ring slot `start`; mirror and device rows."""
    r = k_rows.shape[2]
    ring = torch.from_numpy((start + np.arange(r)) % CCAP).cuda()
    for t, x in ((cache._kres_all, k_rows), (cache._vres_all, v_rows)):
        if r:
            t[:, b].index_copy_(2, ring, torch.from_numpy(x).cuda())
    cache._seen_a[:, b] += r - cache._r_a[:, b]
    cache._r_a[:, b], cache._rs_a[:, b] = r, start if r else 0
    for l in range(NL):
        cache._sync_lengths(l, b)


def _poison_dead_rows(torch, cache):
    dead = np.ones((NL, cache.bs, CCAP), bool)
    for l in range(NL):
        for b in range(cache.bs):
            dead[l, b, (int(cache._rs_a[l, b]) + np.arange(int(cache._r_a[l, b]))) % CCAP] = False
    mask = torch.from_numpy(dead).cuda()[:, :, None, :].expand(-1, -1, NHK, -1)
    cache._kres_all[mask] = float("nan")
    cache._vres_all[mask] = float("nan")


def _snap(torch, cache):
    return dict(k_pool=R.to_np(torch, cache.key_page_pool), v_pool=R.to_np(torch, cache.value_page_pool), ids=cache._page_ids_all.cpu().numpy(),
                lengths=cache._lengths_all.cpu().numpy(), k_res=cache._kres_all.cpu().numpy().view(np.uint16),
                v_res=cache._vres_all.cpu().numpy().view(np.uint16), host=[a.copy() for a in cache.host_state()], pages=cache._pages_a.copy())


def _same(a, b):
    flat = lambda s: [s[k] for k in ("k_pool", "v_pool", "ids", "lengths", "k_res", "v_res", "pages")] + s["host"]
    return all(np.array_equal(x, y) for x, y in zip(flat(a), flat(b)))


def _row_err(out, gold):
    out, gold = np.asarray(out, np.float64), np.asarray(gold, np.float64)
    return np.linalg.norm(out - gold, axis=-1) / np.maximum(np.linalg.norm(gold, axis=-1), 1e-300)


def _held(snap, cache, l, b):
    """What slot b of layer l holds, read from a snapshot of the device: its codes (1, nh_k, T, M), its windows and {T, r, start}."""
    T, r, st = (int(x) for x in snap["lengths"][l, b, :3])
    kc, vc = R.codes_of([snap["k_pool"], snap["v_pool"]], snap["ids"][l, b], 0, T, cache.M, cache.C, cache.packed)
    return kc[None], vc[None], snap["k_res"][l, b:b + 1].view(np.float16), snap["v_res"][l, b:b + 1].view(np.float16), T, r, st


# ---------------------------------------------------------------- 1. paged_turns.verify ---------------------------------------
@pytest.fixture(scope="module")
def filled(env):
    """One cache per (codes, packed), built once: slots at 70 / 45 / 0 coded tokens and windows of 64 (full) / 3 / 40 rows from
    ring slot 50, NaN in every dead ring row; verify never moves it (asserted by every test that borrows it)."""
    torch, ops = env
    made = {}

    def get(d, M, nbits, packed):
        key = (d, M, nbits, packed)
        if key not in made:
            rs = np.random.RandomState(nbits + packed)
            cache = _cache(torch, d, M, nbits, packed)
            for b, T in enumerate((70, 45, 0)):
                if T:
                    for l in range(NL):
                        cache.prefill_request(b, *_rows(torch, rs, 1, T, d), l)
            for b, r in enumerate((CCAP, 3, 40)):
                f = lambda: rs.standard_normal((NL, NHK, r, d)).astype(np.float16)
                _set_window(torch, cache, b, f(), f(), 50)
            _poison_dead_rows(torch, cache)
            torch.cuda.synchronize()
            made[key] = cache
        return made[key]
    return get


def _verify_ref(cache, snap, l, q, k, v, n_valid, masks=None):
    """fp64 (out, lse) of a verification over what every slot of layer l holds: the chain through chunk_wide_model.chunk_attn with the
    rows as chunk; a tree through the same model over the past only, then verify_tree_model.tree_block_merge."""
    ck, cv = cache.key_cent.cpu().numpy(), cache.value_cent.cpu().numpy()
    qn, kn, vn = q.cpu().numpy(), k.cpu().numpy(), v.cpu().numpy()
    outs, lses = [], []
    for b in range(cache.bs):
        kc, vc, kw, vw, T, r, st = _held(snap, cache, l, b)
        chunk = {} if masks is not None else dict(k_chunk=kn[b:b + 1], v_chunk=vn[b:b + 1])
        o, s = CM.chunk_attn(np.nan_to_num(qn[b:b + 1]), kc, vc, ck, cv, kw, vw, r, T=T, start=st, n_q=n_valid[b],
                             **{k_: np.nan_to_num(v_) for k_, v_ in chunk.items()})
        if masks is not None:
            o, s = TM.tree_block_merge(np.nan_to_num(qn[b:b + 1]), np.nan_to_num(kn[b:b + 1]), np.nan_to_num(vn[b:b + 1]), o, s, masks[b:b + 1], [n_valid[b]])
        outs.append(o)
        lses.append(s)
    return np.concatenate(outs), np.concatenate(lses)


def _check_verify(got, ref, n_valid, what, tol=1e-3):
    (go, gl), (ro, rl) = got, ref
    go, gl = go.float().cpu().numpy(), gl.cpu().numpy()
    worst = 0.0
    for b, nv in enumerate(n_valid):
        assert not go[b, :, nv:].any() and np.all(np.isneginf(gl[b, :, nv:])), f"{what}: slot {b}: rows past n_draft={nv}"
        if nv:
            assert np.isfinite(go[b, :, :nv]).all(), f"{what}: slot {b}: non-finite output"
            e = _row_err(go[b, :, :nv], ro[b, :, :nv])
            worst = max(worst, float(e.max()))
            assert e.max() < tol, f"{what}: slot {b}: worst row rel-L2 {e.max():.3e}"
            assert np.abs(gl[b, :, :nv] - rl[b, :, :nv]).max() <= LR.LSE_TOL, f"{what}: slot {b}: lse off by {np.abs(gl[b, :, :nv] - rl[b, :, :nv]).max():.3e}"
    return worst


@pytest.mark.parametrize("n", [1, 4, 5, 16])
@pytest.mark.parametrize("d,M,nbits,packed", [CODES[0] + (False,), CODES[1] + (True,)])
def test_verify_against_the_device_state(env, filled, d, M, nbits, packed, n):
    """G = 4 and n_draft = [n, 1, 0]: 4 n rows per kv head - the "heads" route up to n = 4 (16 rows, the columns of the wide decode
    kernel) beside the chunk route, the chunk route alone above, where "heads" is refused; NaN in every q / K / V row past n_draft."""
    torch, ops = env
    from million_amd import paged_turns
    cache = filled(d, M, nbits, packed)
    rs = np.random.RandomState(n)
    n_draft = [n, 1, 0]
    q, k, v = _rows(torch, rs, BS, n, d)
    for b, nv in enumerate(n_draft):
        q[b, :, nv:], k[b, :, nv:], v[b, :, nv:] = float("nan"), float("nan"), float("nan")
    before = _snap(torch, cache)
    with pytest.raises(NotImplementedError, match="nbits"):
        cache.verify(q, k, v, 0, n_draft=n_draft)
    for l in range(NL):
        chunk = paged_turns.verify(cache, q, k, v, l, n_draft=n_draft, route="chunk", return_lse=True)
        if n * (NH // NHK) <= 16:
            heads = paged_turns.verify(cache, q, k, v, l, n_draft=n_draft, route="heads", return_lse=True)
        else:
            with pytest.raises(RuntimeError, match="route='heads' serves at most 16 rows per kv head"):
                paged_turns.verify(cache, q, k, v, l, n_draft=n_draft, route="heads", return_lse=True)
            heads = None
        auto = paged_turns.verify(cache, q, k, v, l, n_draft=n_draft)
        torch.cuda.synchronize()
        assert _same(before, _snap(torch, cache)), f"layer {l}: verify moved lengths, pages or window bytes"
        ref = _verify_ref(cache, before, l, q, k, v, n_draft)
        what = f"M{M} nbits{nbits} packed{packed} n{n} layer{l}"
        w = _check_verify(chunk, ref, n_draft, what + " chunk")
        if heads is not None:
            w = max(w, _check_verify(heads, ref, n_draft, what + " heads"))
            e = _row_err(heads[0].float().cpu().numpy(), chunk[0].float().cpu().numpy())
            assert e.max() < 2e-3, f"{what}: routes differ by {e.max():.3e}"
        assert cache._verify_route(n) == "chunk"      # three requests of at most 70 tokens (profiles/verify_wide.txt)
        e = _row_err(auto.float().cpu().numpy(), chunk[0].float().cpu().numpy())
        assert e.max() < 2e-3, f"{what}: route=None differs from the chunk route by {e.max():.3e}"
        for b, nv in enumerate(n_draft):      # the staged rows: bitwise the live K / V rows
            assert torch.equal(cache._kstage[l, b, :, :nv].view(torch.int16), k[b, :, :nv].view(torch.int16))
            assert torch.equal(cache._vstage[l, b, :, :nv].view(torch.int16), v[b, :, :nv].view(torch.int16))
        print(f"{what}: worst row rel-L2 {w:.3e}")
    cache._verify_rec = None


@pytest.mark.parametrize("route", ["heads", "chunk"])
def test_verify_a_tree(env, filled, route):
    """Two roots, depth 3: node i sees its ancestors and itself; n_draft = [n, 3, 0] live nodes are a prefix of the tree.  "heads":
    the tree of 4 nodes (16 rows per kv head); "chunk": a fifth node under the second root."""
    torch, ops = env
    from million_amd import paged_turns
    d, M, nbits = CODES[0]
    cache = filled(d, M, nbits, True)
    parents = [-1, 0, 1, -1] if route == "heads" else [-1, 0, 1, -1, 3]
    n = len(parents)
    n_draft = [n, 3, 0]
    assert max(TM.depth(parents, i) for i in range(n)) == 3 and parents.count(-1) == 2
    masks = np.stack([TM.ancestor_masks(parents)] * BS)
    q, k, v = _rows(torch, np.random.RandomState(77), BS, n, d)
    before = _snap(torch, cache)
    got = paged_turns.verify(cache, q, k, v, 1, n_draft=n_draft, route=route, return_lse=True, tree=parents)
    chain = paged_turns.verify(cache, q, k, v, 1, n_draft=n_draft, route=route, return_lse=True)
    torch.cuda.synchronize()
    assert _same(before, _snap(torch, cache))
    w = _check_verify(got, _verify_ref(cache, before, 1, q, k, v, n_draft, masks), n_draft, f"tree {route}")
    assert not torch.equal(got[0][0, :, 3], chain[0][0, :, 3])      # node 3 is a root: it does not see nodes 0 .. 2
    print(f"tree {route}: worst row rel-L2 {w:.3e}")
    cache._verify_rec = None


# ---------------------------------------------------------------- 2. commit = single decode steps, bit for bit ----------------
def _compare_with_twins(torch, A, twins, what):
    torch.cuda.synchronize()
    sa = _snap(torch, A)
    for b, tw in enumerate(twins):
        st = _snap(torch, tw)
        for l in range(NL):
            assert np.array_equal(sa["lengths"][l, b, :3], st["lengths"][l, 0, :3]), \
                f"{what}: device lengths of layer {l} slot {b}: {sa['lengths'][l, b].tolist()}, twin {st['lengths'][l, 0].tolist()}"
            mine, theirs = [int(a[l, b]) for a in sa["host"]], [int(a[l, 0]) for a in st["host"]]
            assert mine == theirs and int(sa["pages"][l, b]) == int(st["pages"][l, 0]), f"{what}: host mirror of layer {l} slot {b}: {mine}, twin {theirs}"
            ka, va, kwa, vwa, T, r, rs_ = _held(sa, A, l, b)
            kt, vt, kwt, vwt, *_ = _held(st, tw, l, 0)
            assert (T, r, rs_) == (int(A._T_a[l, b]), int(A._r_a[l, b]), int(A._rs_a[l, b])), f"{what}: mirror and device rows of layer {l} slot {b} disagree"
            assert np.array_equal(ka, kt) and np.array_equal(va, vt), f"{what}: codes of layer {l} slot {b} differ from the twin's"
            ring = (rs_ + np.arange(r)) % CCAP
            for x, y, side in ((kwa, kwt, "K"), (vwa, vwt, "V")):
                assert np.array_equal(x[0][:, ring].view(np.uint16), y[0][:, ring].view(np.uint16)), f"{what}: {side} window rows of layer {l} slot {b} differ from the twin's"


@pytest.mark.parametrize("d,M,nbits,packed", [c + (p,) for c in CODES for p in (False, True)])
def test_commit_equals_single_decode_steps(env, d, M, nbits, packed):
    """Round 1, a chain of 4: windows of 60 / 61 / 64 rows take 4 / 4 / 2 rows - r + a = cap (no flush), r + a = cap + 1 (a flush
    of window rows alone), r = cap (a full window).  Round 2, a tree of 5 (two roots, depth 3) and path=: the windows are at
    64 / 33 / 34 and take [0, 1, 2] (a full window again) / [3, 4] / nothing.  Then one decode step on both sides."""
    torch, ops = env
    from million_amd import paged_turns
    rs = np.random.RandomState(nbits + 10 * packed)
    A, twins = _cache(torch, d, M, nbits, packed), [_cache(torch, d, M, nbits, packed, bs=1) for _ in range(BS)]
    for b, T in ((0, 45), (2, 64)):      # slot 1 has no coded tokens
        rows = [_rows(torch, rs, 1, T, d) for _ in range(NL)]
        for l in range(NL):
            A.prefill_request(b, *rows[l], l)
            twins[b].prefill_request(0, *rows[l], l)
    for b, (r, st) in enumerate(((60, 0), (61, 9), (64, 63))):
        kw, vw = (rs.standard_normal((NL, NHK, r, d)).astype(np.float16) for _ in range(2))
        _set_window(torch, A, b, kw, vw, st)
        _set_window(torch, twins[b], 0, kw, vw, st)
    _compare_with_twins(torch, A, twins, "start")

    def a_round(n, n_accept, what, tree=None, path=None):
        _poison_dead_rows(torch, A)
        qkv = [_rows(torch, rs, BS, n, d) for _ in range(NL)]
        for l in range(NL):
            out = paged_turns.verify(A, *qkv[l], l, tree=tree)
            assert torch.isfinite(out).all(), f"{what}: layer {l}: non-finite verify output"
        _poison_dead_rows(torch, A)
        with pytest.raises(NotImplementedError, match="nbits"):
            A.commit(n_accept)
        if path is None:
            paged_turns.commit(A, n_accept)
        else:
            paged_turns.commit(A, path=path)
        for b, tw in enumerate(twins):
            for i in (range(n_accept[b]) if path is None else path[b]):
                for l in range(NL):
                    q, k, v = qkv[l]
                    paged_turns.decode(tw, q[b:b + 1, :, i:i + 1].contiguous(), k[b:b + 1, :, i:i + 1].contiguous(),
                                       v[b:b + 1, :, i:i + 1].contiguous(), l, use_dev_lengths=True)
        _compare_with_twins(torch, A, twins, what)

    a_round(4, [4, 4, 2], "chain")
    assert A._T_a[0].tolist() == [45, 32, 96] and A._r_a[0].tolist() == [64, 33, 34] and A._rs_a[0].tolist() == [0, 41, 31]
    a_round(5, [3, 2, 0], "tree path", tree=[-1, 0, 1, -1, 3], path=[[0, 1, 2], [3, 4], []])
    assert A._T_a[0].tolist() == [77, 32, 96] and A._r_a[0].tolist() == [35, 35, 34]
    # one ordinary decode step on both sides: the same state, the same split cut (it depends on the bound alone), the same bits
    for l in range(NL):
        q, k, v = _rows(torch, rs, BS, 1, d)
        out = paged_turns.decode(A, q, k, v, l, use_dev_lengths=True)
        for b, tw in enumerate(twins):
            o1 = paged_turns.decode(tw, q[b:b + 1].contiguous(), k[b:b + 1].contiguous(), v[b:b + 1].contiguous(), l, use_dev_lengths=True)
            assert torch.isfinite(out[b]).all() and torch.equal(out[b].view(torch.int16), o1[0].view(torch.int16)), f"decode step after the commits: layer {l} slot {b}"
    _compare_with_twins(torch, A, twins, "after a decode step")


# ---------------------------------------------------------------- 3. one captured verify ---------------------------------------
def test_a_captured_heads_verify_follows_the_lengths(env):
    """The "heads" verify of one layer, captured once; a commit then moves every slot's lengths (slot 2 flushes a page), and the
    replay is bitwise the eager call on the moved cache."""
    torch, ops = env
    from million_amd import paged_turns
    d, M, nbits = CODES[0]
    rs = np.random.RandomState(5)
    cache = _cache(torch, d, M, nbits, True)
    for b, T in enumerate((70, 45, 33)):
        for l in range(NL):
            cache.prefill_request(b, *_rows(torch, rs, 1, T, d), l)
    for b, r in enumerate((10, 0, 62)):
        f = lambda: rs.standard_normal((NL, NHK, r, d)).astype(np.float16)
        _set_window(torch, cache, b, f(), f(), 7)
    n = 4      # 16 rows per kv head: every column of the launch
    static = _rows(torch, rs, BS, n, d)
    warm = paged_turns.verify(cache, *static, 0, route="heads", return_lse=True)      # workspace, staging rows and dev_n exist from here on
    rec = cache._verify_rec      # (kept: the captured launches read its dev_n)
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        cap_out, cap_lse = paged_turns.verify(cache, *static, 0, route="heads", return_lse=True)
    g.replay()
    torch.cuda.synchronize()
    assert torch.equal(cap_out.view(torch.int16), warm[0].view(torch.int16)) and torch.equal(cap_lse, warm[1])
    paged_turns.verify(cache, *static, 1, route="heads")
    paged_turns.commit(cache, [3, 1, 4])
    assert cache._T_a[0].tolist() == [70, 45, 65] and cache._r_a[0].tolist() == [13, 1, 34]
    for dst, src in zip(static, _rows(torch, rs, BS, n, d)):      # other rows in the same buffers
        dst.copy_(src)
    g.replay()
    eager = paged_turns.verify(cache, *static, 0, route="heads", return_lse=True)
    torch.cuda.synchronize()
    assert torch.equal(cap_out.view(torch.int16), eager[0].view(torch.int16)) and torch.equal(cap_lse, eager[1])
    assert not torch.equal(cap_out.view(torch.int16), warm[0].view(torch.int16)) and rec["dev_n"].tolist() == [n] * BS
