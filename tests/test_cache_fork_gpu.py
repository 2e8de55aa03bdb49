"""GPU tests of the request fork (million_cache_fork behind ops.cache_fork and PagedPQCache.fork):

  1. the C call against the numpy model of its contract (tests/cache_fork_model.py), byte for byte on the pools, tables,
     windows and lengths of EVERY slot - so what must stay untouched is checked with what must change;
  2. a forked slot decodes the same bits as a slot that was filled the slow way, the source is not disturbed;
  3. a shared page outlives its first owner;
  4. the intended use: one prompt, several questions (extend_request), and the fork of a prefix;
  5. refusals change nothing.

The oracle bar is the suite's (rel-L2 and mean-abs < 1e-3, tests/test_gpu_parity.py); everything else is bitwise."""
import numpy as np
import pytest

from tests import cache_fork_model as FM
from tests import synth

pytestmark = pytest.mark.gpu

REL_TOL = MEAN_ABS_TOL = 1e-3      # the oracle bar of tests/test_gpu_parity.py


@pytest.fixture(scope="module")
def env():
    import torch
    assert torch.cuda.is_available(), "GPU tests need an MI355X"
    from million_amd import ops, _lib
    _lib.load()
    yield torch, ops
    assert ops.tail_faults() == 0      # no split merge of the decode steps of this file gave up


# ---------------------------------------------------------------- 1. the byte model ----------------------------------------
LAYERS, BS, RCAP, START, R = 3, 4, 128, 100, 60
NAN16 = np.int16(0x7E00)


def _host_tables(seed, *, nhk, d, M, ps, T, extra=40, src=0):
    """Tables of distinct ids, pools with a per-page pattern, windows that hold NaN outside the ring span, garbage rows."""
    rs = np.random.RandomState(seed)
    cap_pages = -(-209 // ps) + 1
    n_tab = LAYERS * BS * nhk * cap_pages
    n_pool = n_tab + extra
    perm = rs.permutation(n_pool)
    ids = perm[:n_tab].reshape(LAYERS, BS, nhk, cap_pages).astype(np.int32)
    spare = perm[n_tab:].astype(np.int32)                              # ids no table names: the tail pages of SHARE
    page = np.arange(n_pool)[:, None, None]
    kp = (page * 7 + np.arange(ps)[None, :, None] * 3 + np.arange(M)[None, None, :]).astype(np.uint8)
    vp = (page * 11 + np.arange(M)[None, :, None] * 5 + np.arange(ps)[None, None, :]).astype(np.uint8)
    span = (START + np.arange(R)) % RCAP
    kr = np.full((LAYERS, BS, nhk, RCAP, d), NAN16, np.int16)
    vr = np.full((LAYERS, BS, nhk, RCAP, d), NAN16, np.int16)
    kr[:, :, :, span] = rs.standard_normal((LAYERS, BS, nhk, R, d)).astype(np.float16).view(np.int16)
    vr[:, :, :, span] = rs.standard_normal((LAYERS, BS, nhk, R, d)).astype(np.float16).view(np.int16)
    ln = rs.randint(1, 200, (LAYERS, BS, 4)).astype(np.int32)
    ln[:, src] = (T, R, START, 0x7EADBEEF)
    return [ids, kp, vp, kr, vr, ln], spare


NAMES = ("page_ids", "k_pool", "v_pool", "k_resid", "v_resid", "lengths")


def _run_both(torch, ops, host, dst, tail, *, src=0, mode, n_pages_bound, prefix=-1, what=""):
    want = [a.copy() for a in host]
    dst = np.asarray(dst, np.int32)
    copied = FM.fork(*want, dst, tail, src=src, mode=mode, n_pages_bound=n_pages_bound, prefix_tokens=prefix)
    dev = [torch.from_numpy(a.copy()).cuda() for a in host]
    dev[3], dev[4] = dev[3].view(torch.float16), dev[4].view(torch.float16)
    ops.cache_fork(*dev, torch.from_numpy(dst).cuda(), None if tail is None else torch.from_numpy(tail).cuda(), src=src,
                   share=mode == FM.SHARE, n_pages_bound=n_pages_bound, prefix_tokens=prefix)
    torch.cuda.synchronize()
    dev[3], dev[4] = dev[3].view(torch.int16), dev[4].view(torch.int16)
    for name, w, g in zip(NAMES, want, dev):
        g = g.cpu().numpy()
        if not np.array_equal(w, g):
            bad = np.argwhere(w != g)
            raise AssertionError(f"{what}: {name} differs from the model at {len(bad)} places, first {bad[0].tolist()}: "
                                 f"model {w[tuple(bad[0])]}, device {g[tuple(bad[0])]}")
    return copied


@pytest.mark.parametrize("mode", [FM.SHARE, FM.COPY], ids=["share", "copy"])
@pytest.mark.parametrize("ps", [32, 64, 128])
def test_fork_call_equals_the_model_byte_for_byte(env, ps, mode):
    torch, ops = env
    n_cases = n_copied = 0
    for nhk in (1, 2):
        for d, M in ((128, 64), (64, 16)):
            for T in (0, 17, 64, 209):
                host, spare = _host_tables(1000 + T + nhk, nhk=nhk, d=d, M=M, ps=ps, T=T)
                cap_pages = host[0].shape[3]
                for dst in ([2], [3, 1, 2]):
                    tail = spare[:len(dst) * LAYERS * nhk].reshape(len(dst), LAYERS, nhk).copy() if mode == FM.SHARE else None
                    for prefix in (-1, 0, 40, 64):
                        what = f"nh_k={nhk} d={d} M={M} page={ps} T={T} dst={dst} prefix={prefix}"
                        copied = _run_both(torch, ops, host, dst, tail, mode=mode, n_pages_bound=cap_pages, prefix=prefix, what=what)
                        Te = T if prefix < 0 else min(T, prefix)
                        pages = (-(-Te // ps) if mode == FM.COPY else (1 if Te % ps else 0)) * LAYERS * nhk * len(dst)
                        assert len(copied) == pages, what
                        n_cases, n_copied = n_cases + 1, n_copied + len(copied)
    assert n_cases == 2 * 2 * 4 * 2 * 4 and n_copied > 0


@pytest.mark.parametrize("mode", [FM.SHARE, FM.COPY], ids=["share", "copy"])
def test_fork_call_on_untrusted_values(env, mode):
    """A device T above the bound, lengths out of range, table entries and tail ids outside the pool, destinations that take
    no part: the model's answer, byte for byte, and the call ends clean."""
    torch, ops = env
    nhk, d, M, ps = 2, 128, 64, 64
    share = mode == FM.SHARE
    tails = lambda spare, n: spare[:n * LAYERS * nhk].reshape(n, LAYERS, nhk).copy() if share else None
    # T = 209 on the device, a bound of two pages: T reads as 128
    host, spare = _host_tables(7, nhk=nhk, d=d, M=M, ps=ps, T=209)
    copied = _run_both(torch, ops, host, [1, 3], tails(spare, 2), mode=mode, n_pages_bound=2, what="T above the bound")
    assert len(copied) == (0 if share else 2 * LAYERS * nhk * 2)
    # rows of garbage: T far above / below, r and start out of range (one layer each)
    host, spare = _host_tables(8, nhk=nhk, d=d, M=M, ps=ps, T=209)
    host[5][0, 0] = (2 ** 31 - 1, 2 ** 31 - 1, RCAP, 5)
    host[5][1, 0] = (-7, -1, -1, 5)
    host[5][2, 0] = (130, 128, 127, 5)
    _run_both(torch, ops, host, [2], tails(spare, 1), mode=mode, n_pages_bound=host[0].shape[3], what="garbage rows")
    # ids outside the pool: a source entry, a destination entry (COPY) / a tail id (SHARE); nothing is copied for those pages
    host, spare = _host_tables(9, nhk=nhk, d=d, M=M, ps=ps, T=209)
    n_pool = host[1].shape[0]
    host[0][0, 0, 0, 3] = n_pool                                       # the source's tail page of (layer 0, head 0)
    host[0][1, 0, 1, 1] = -1
    host[0][2, 2, 0, 0] = 1 << 30                                      # a destination entry
    tail = tails(spare, 2)
    if share:
        tail[0, 1, 0], tail[1, 2, 1] = n_pool + 5, -3
    copied = _run_both(torch, ops, host, [2, 1], tail, mode=mode, n_pages_bound=host[0].shape[3], what="ids outside the pool")
    assert len(copied) == (2 * LAYERS * nhk - 4 if share else 2 * LAYERS * nhk * 4 - 5)
    # the source itself, slots outside [0, bs) and a repeated slot take no part; any source slot
    host, spare = _host_tables(10, nhk=nhk, d=d, M=M, ps=ps, T=100, src=2)
    copied = _run_both(torch, ops, host, [2, BS, 3, 3, -1, 0], tails(spare, 6), src=2, mode=mode, n_pages_bound=host[0].shape[3],
                       what="destinations that take no part")
    assert {c[1] for c in copied} == {3, 0}


# ---------------------------------------------------------------- the cache under test --------------------------------------
GEOM = dict(bs=3, nh=8, num_key_value_heads=2, M=64, layer_num=2, d=128, page_size=64, extended_residual_size=128, max_tokens=1024)
N_PROMPT, N_STEPS = 209, 140
C = 256


class _World:
    """One prompt, decode rows for two kinds of request (A: the source's own, B: what the twin and the fork are fed), questions."""

    def __init__(self):
        nhk, nh, d, M = GEOM["num_key_value_heads"], GEOM["nh"], GEOM["d"], GEOM["M"]
        n = N_PROMPT + N_STEPS + 16
        self.hist = {}
        for who, seed in (("A", 4100), ("B", 4200), ("other", 4300)):      # (layers, 1, nh_k, n, d) K and V histories
            k = [synth.encode_case(seed + l, 1, nhk, n, d, M, C) for l in range(2)]
            v = [synth.encode_case(seed + 10 + l, 1, nhk, n, d, M, C) for l in range(2)]
            self.hist[who] = (np.stack([c["X"] for c in k]), np.stack([c["X"] for c in v]))
        for side in (0, 1):                                                # the same prompt under both continuations
            self.hist["B"][side][:, :, :, :N_PROMPT] = self.hist["A"][side][:, :, :, :N_PROMPT]
        self.ck = synth.encode_case(4400, 1, nhk, 1, d, M, C)["cents"]
        self.cv = synth.encode_case(4401, 1, nhk, 1, d, M, C)["cents"]
        rs = np.random.RandomState(4500)
        self.q = {who: rs.standard_normal((N_STEPS + 16, 2, 1, nh, 1, d)).astype(np.float16) for who in ("A", "B", "other")}
        self.qp = rs.standard_normal((1, nh, N_PROMPT, d)).astype(np.float16)


@pytest.fixture(scope="module")
def world():
    return _World()


def _new_cache(torch, world, preallocate, **kw):
    from million_amd.pq_cache import PagedPQCache
    cache = PagedPQCache(**dict(GEOM, **kw), preallocate=preallocate, device="cuda")
    cache.set_cent(torch.from_numpy(world.ck).cuda(), torch.from_numpy(world.cv).cuda())
    return cache


def _dev(torch, a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def _prefill(torch, cache, world, b, who, n=N_PROMPT):
    for l in range(2):
        K, V = world.hist[who]
        cache.prefill_request(b, _dev(torch, world.qp[:, :, :n]), _dev(torch, K[l][:, :, :n]), _dev(torch, V[l][:, :, :n]), l)


def _decode(torch, cache, world, feeds, steps, pos0=0):
    """feeds[b] = (history name, position of the request's first decode row).  Returns [step][layer] outputs (bs, nh, 1, d)."""
    outs = []
    for i in range(pos0, pos0 + steps):
        row = []
        for l in range(2):
            q = np.concatenate([world.q[w][i, l] for w, _ in feeds])
            kn = np.concatenate([world.hist[w][0][l][:, :, p + i:p + i + 1] for w, p in feeds])
            vn = np.concatenate([world.hist[w][1][l][:, :, p + i:p + i + 1] for w, p in feeds])
            row.append(cache.decoding_with_pages(_dev(torch, q), _dev(torch, kn), _dev(torch, vn), l, use_dev_lengths=True).clone())
        outs.append(row)
    return outs


def _bits(torch, outs, b):
    return torch.stack([o[b] for row in outs for o in row]).cpu().numpy().view(np.int16)


def _oracle_check(oracle, world, who, n_prompt, steps, out, l, what):
    pol = oracle.PagedPolicy(page_size=GEOM["page_size"], residual=GEOM["extended_residual_size"], prefill=n_prompt)
    for _ in range(steps):
        T, r = pol.step()
    K, V = world.hist[who][0][l], world.hist[who][1][l]
    kc, vc = oracle.pq_encode(K[:, :, :T], world.ck), oracle.pq_encode(V[:, :, :T], world.cv)
    kres = np.zeros((1, 2, 128, 128), np.float16)
    vres = np.zeros((1, 2, 128, 128), np.float16)
    kres[:, :, :r], vres[:, :, :r] = K[:, :, T:T + r], V[:, :, T:T + r]
    gold = oracle.decode_attn(world.q[who][steps - 1, l], kc, vc, world.ck, world.cv, kres, vres, r)
    out = out.astype(np.float64)
    rel = np.linalg.norm(out - gold) / np.linalg.norm(gold)
    mae = np.abs(out - gold).mean()
    print(f"{what}: T={T} r={r} rel-L2 {rel:.3e} mean-abs {mae:.3e}")
    assert np.isfinite(out).all() and rel < REL_TOL and mae < MEAN_ABS_TOL, f"{what}: rel={rel:.3e} mean_abs={mae:.3e}"


# ---------------------------------------------------------------- 2. same bits as a slot filled the slow way ----------------
@pytest.mark.parametrize("preallocate", [False, True], ids=["on-demand", "preallocated"])
def test_forked_slot_decodes_the_bits_of_a_prefilled_slot(env, oracle, world, preallocate):
    torch, ops = env
    feeds = [("A", N_PROMPT), ("B", N_PROMPT), ("B", N_PROMPT)]
    runs = {}
    for fork in (True, False):
        cache = _new_cache(torch, world, preallocate)
        _prefill(torch, cache, world, 0, "A")
        _prefill(torch, cache, world, 1, "B")
        if fork:
            cache.fork(0, 2)
            assert cache._lengths_all.cpu().tolist() == [[[N_PROMPT, 0, 0, 0]] * 3] * 2
        runs[fork] = _decode(torch, cache, world, feeds, N_STEPS)
        if fork:
            assert cache._T_a.tolist() == [[N_PROMPT + 64] * 3] * 2 and cache._r_a.tolist() == [[N_STEPS - 64] * 3] * 2      # a flush was crossed
            assert cache._lengths_all.cpu().numpy()[:, :, :3].tolist() == [[[N_PROMPT + 64, N_STEPS - 64, 64]] * 3] * 2
    twin, forked = _bits(torch, runs[True], 1), _bits(torch, runs[True], 2)
    steps = np.flatnonzero((twin != forked).any(axis=(1, 2, 3))) // 2
    assert steps.size == 0, f"the forked slot differs from the prefilled one from step {steps[0]} on"
    assert np.array_equal(_bits(torch, runs[True], 0), _bits(torch, runs[False], 0)), "the fork disturbed its source"
    assert np.array_equal(twin, _bits(torch, runs[False], 1))
    for l in range(2):
        _oracle_check(oracle, world, "B", N_PROMPT, N_STEPS, runs[True][-1][l][2:3].float().cpu().numpy(), l, f"forked slot, layer {l}")
    assert ops.tail_faults() == 0


# ---------------------------------------------------------------- 3. a shared page outlives its first owner ----------------
def test_shared_pages_outlive_the_source(env, oracle, world):
    torch, ops = env
    cache = _new_cache(torch, world, False)
    pm = cache.page_manager
    _prefill(torch, cache, world, 0, "A")
    _prefill(torch, cache, world, 1, "B")
    assert pm.get_stats()["allocated_pages"] == 2 * 2 * 4 * 2          # 209 tokens: 3 full pages and a tail per (layer, kv head)
    cache.fork(0, 2)
    assert pm.get_stats()["allocated_pages"] == 2 * 2 * (4 + 4 + 1)
    assert cache.sharing_stats() == {"shared_pages": 12, "extra_references": 12}
    src_tails = [cache._host_pids[l][0][h][3] for l in range(2) for h in range(2)]
    shared = [cache._host_pids[l][0][h][j] for l in range(2) for h in range(2) for j in range(3)]
    cache.release(0)
    assert pm.get_stats()["allocated_pages"] == 2 * 2 * (4 + 4) and cache.sharing_stats() == {"shared_pages": 0, "extra_references": 0}
    assert all(pm.ref_count(p) == 1 for p in shared) and all(pm.ref_count(p) == 0 for p in src_tails)
    _prefill(torch, cache, world, 0, "other", n=100)                   # a different prompt: two pages per (layer, kv head)
    mine = {p for l in range(2) for h in range(2) for p in cache._host_pids[l][0][h]}
    assert set(src_tails) <= mine and not mine & set(shared) and pm.get_stats()["allocated_pages"] == 2 * 2 * (4 + 4 + 2)
    free = torch.tensor(sorted(pm.free_pages), dtype=torch.long, device="cuda")
    cache.key_page_pool[free] = 0xFF
    cache.value_page_pool[free] = 0xFF
    outs = _decode(torch, cache, world, [("other", 100), ("B", N_PROMPT), ("B", N_PROMPT)], N_STEPS)
    assert np.array_equal(_bits(torch, outs, 1), _bits(torch, outs, 2))
    for l in range(2):
        _oracle_check(oracle, world, "B", N_PROMPT, N_STEPS, outs[-1][l][2:3].float().cpu().numpy(), l, f"fork after release(source), layer {l}")
        _oracle_check(oracle, world, "other", 100, N_STEPS, outs[-1][l][0:1].float().cpu().numpy(), l, f"new request in the source's slot, layer {l}")
    for b in range(3):
        cache.release(b)
    assert pm.get_stats()["allocated_pages"] == 0 and cache.sharing_stats() == {"shared_pages": 0, "extra_references": 0}
    assert ops.tail_faults() == 0


# ---------------------------------------------------------------- 4. one prompt, several questions --------------------------
def _ask(torch, cache, world, b, who, pos, n=5):
    """extend_request of n rows of a history, every layer; then the slot's lengths rows and pages as host values."""
    outs = []
    for l in range(2):
        K, V = world.hist[who]
        q = world.q[who][pos % 64:pos % 64 + n, l, 0, :, 0].transpose(1, 0, 2)[None]      # (1, nh, n, d)
        outs.append(cache.extend_request(b, _dev(torch, q), _dev(torch, K[l][:, :, pos:pos + n]), _dev(torch, V[l][:, :, pos:pos + n]), l))
    return torch.stack(outs).cpu().numpy().view(np.int16)


def _codes(torch, cache, b, T):
    """The K and V codes of slot b's first T tokens, every layer, gathered through its page table."""
    ps = cache.page_size
    n = -(-T // ps)
    ids = cache._page_ids_all[:, b, :, :n].long()
    k = cache.key_page_pool[ids].reshape(2, 2, n * ps, cache.M)[:, :, :T]
    v = cache.value_page_pool[ids].permute(0, 1, 2, 4, 3).reshape(2, 2, n * ps, cache.M)[:, :, :T]
    return k.cpu().numpy(), v.cpu().numpy()


@pytest.mark.parametrize("preallocate", [False, True], ids=["on-demand", "preallocated"])
def test_fork_then_a_question_per_request(env, world, preallocate):
    """Ten decode steps put rows into the source's window; slots 1 and 2, which decoded along from empty, are released and
    become forks; three different questions.  The other cache prefills every slot on its own."""
    torch, ops = env
    slow, fast = _new_cache(torch, world, preallocate), _new_cache(torch, world, preallocate)
    for b in range(3):
        _prefill(torch, slow, world, b, "A")
    _prefill(torch, fast, world, 0, "A")
    feeds = [("A", N_PROMPT)] * 3
    o_slow, o_fast = _decode(torch, slow, world, feeds, 10), _decode(torch, fast, world, feeds, 10)
    assert np.array_equal(_bits(torch, o_slow, 0), _bits(torch, o_fast, 0))
    fast.release(1)
    fast.release(2)
    fast.fork(0, [1, 2])
    assert fast._lengths_all.cpu().tolist() == slow._lengths_all.cpu().tolist() == [[[N_PROMPT, 10, 0, 0]] * 3] * 2
    for b, (who, pos) in enumerate((("A", N_PROMPT + 10), ("B", N_PROMPT + 40), ("other", 7))):
        assert np.array_equal(_ask(torch, slow, world, b, who, pos), _ask(torch, fast, world, b, who, pos)), f"slot {b}"
    assert fast._lengths_all.cpu().tolist() == slow._lengths_all.cpu().tolist() == [[[N_PROMPT + 15, 0, 0, 0]] * 3] * 2
    for b in range(3):
        for a, c in zip(_codes(torch, slow, b, N_PROMPT + 15), _codes(torch, fast, b, N_PROMPT + 15)):
            assert np.array_equal(a, c), f"codes of slot {b}"
    # and the requests go on decoding, each its own rows
    feeds = [("A", N_PROMPT), ("B", N_PROMPT), ("other", N_PROMPT)]
    o_slow, o_fast = _decode(torch, slow, world, feeds, 3, pos0=20), _decode(torch, fast, world, feeds, 3, pos0=20)
    for b in range(3):
        assert np.array_equal(_bits(torch, o_slow, b), _bits(torch, o_fast, b)), f"slot {b} after its question"
    if not preallocate:
        assert fast.page_manager.get_stats()["allocated_pages"] == 2 * 2 * (4 + 1 + 1)      # 224 tokens: the 4th page is private to each
        assert fast.sharing_stats() == {"shared_pages": 12, "extra_references": 24}
    assert ops.tail_faults() == 0


@pytest.mark.parametrize("preallocate", [False, True], ids=["on-demand", "preallocated"])
def test_fork_of_a_prefix(env, world, preallocate):
    torch, ops = env
    slow, fast = _new_cache(torch, world, preallocate), _new_cache(torch, world, preallocate)
    _prefill(torch, slow, world, 1, "A", n=150)
    _prefill(torch, fast, world, 0, "A")
    _decode(torch, fast, world, [("A", N_PROMPT)] * 3, 4)              # a window the prefix must not take along
    fast.release(1)
    fast.fork(0, 1, n_tokens=150)
    assert fast._lengths_all[:, 1].cpu().tolist() == slow._lengths_all[:, 1].cpu().tolist() == [[150, 0, 0, 0]] * 2
    assert fast._lengths_all[:, 0].cpu().tolist() == [[N_PROMPT, 4, 0, 0]] * 2
    assert np.array_equal(_ask(torch, slow, world, 1, "B", N_PROMPT + 3), _ask(torch, fast, world, 1, "B", N_PROMPT + 3))
    for a, c in zip(_codes(torch, slow, 1, 155), _codes(torch, fast, 1, 155)):
        assert np.array_equal(a, c)
    assert fast._T_a[:, 1].tolist() == [155, 155] and fast._seen_a[:, 1].tolist() == [155, 155]
    assert ops.tail_faults() == 0


# ---------------------------------------------------------------- 5. refusals ----------------------------------------------
@pytest.mark.parametrize("preallocate", [False, True], ids=["on-demand", "preallocated"])
def test_refused_forks_change_nothing(env, world, preallocate):
    torch, ops = env
    cache = _new_cache(torch, world, preallocate)
    _prefill(torch, cache, world, 0, "A")
    _prefill(torch, cache, world, 1, "B", n=40)
    snap = lambda: ([t.clone() for t in (cache.key_page_pool, cache.value_page_pool, cache._page_ids_all, cache._lengths_all,
                                         cache._kres_all, cache._vres_all)],
                    [a.copy() for a in cache.host_state()] + [cache._pages_a.copy()],
                    (cache.page_manager.get_stats(), cache.sharing_stats(), sorted(cache.page_manager.free_pages)))
    before = snap()
    for args, kw in (((0, 1), {}), ((0, [2, 1]), {}), ((0, 0), {}), ((0, [2, 0]), {}), ((0, 2), dict(n_tokens=N_PROMPT + 1)),
                     ((0, 2), dict(n_tokens=-1)), ((0, 3), {}), ((0, [2, 2]), {})):
        with pytest.raises(RuntimeError):
            cache.fork(*args, **kw)
    torch.cuda.synchronize()
    after = snap()
    assert all(torch.equal(a, b) for a, b in zip(before[0], after[0]))
    assert all(np.array_equal(a, b) for a, b in zip(before[1], after[1])) and before[2] == after[2]
    cache.fork(0, 2, n_tokens=N_PROMPT)                                # and the call that is allowed still works
    assert cache._lengths_all[:, 2].cpu().tolist() == [[N_PROMPT, 0, 0, 0]] * 2
