"""GPU tests of draft verification over a tree: ops.attn_block_merge(dev_mask=) against the fp64 formula
(tests/verify_tree_model.py) and, bit for bit, against the chain's launch on every node's gathered ancestor chain; masks and row
indices nobody checked; a replayed graph whose mask changes between replays; PagedPQCache.verify(tree=) against an fp64 softmax
over what the cache holds on the device, restricted to every node's ancestors; PagedPQCache.commit(path=) against batch-1 twin
caches that take the path's rows through decoding_with_pages one by one.

Bars (those of test_verify_gpu.py).  Outputs against fp64: per-row rel-L2 < 1e-3, lse within lse_ref.LSE_TOL.  Two routes, or the
tree's launch and the chain's, of one attention against each other: 2e-3.  The masked launch against the chain's launch on the
gathered chain, and everything a commit leaves: bitwise."""
import numpy as np
import pytest

from tests import cache_life_model as CL
from tests import lse_ref as R
from tests import test_verify_gpu as VG
from tests import verify_tree_model as TM

pytestmark = pytest.mark.gpu

REL_TOL = 1e-3


@pytest.fixture(scope="module")
def env():
    import torch
    assert torch.cuda.is_available(), "GPU tests need an MI355X"
    from million_amd import ops, _lib
    _lib.load()
    yield torch, ops
    assert ops.tail_faults() == 0


def _dev(torch, a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def _bits(t):
    a = t.cpu().numpy()
    return a.view(np.uint16) if a.dtype == np.float16 else a.view(np.uint32)


def _block(rs, bs, nh, nhk, n, d):
    f16 = lambda *s: rs.standard_normal(s).astype(np.float16)
    q, k, v, out_a = f16(bs, nh, n, d), f16(bs, nhk, n, d), f16(bs, nhk, n, d), f16(bs, nh, n, d)
    lse_a = (rs.standard_normal((bs, nh, n)) * 2 + 3).astype(np.float32)
    return q, k, v, out_a, lse_a


def _trees_for(bs, n, seed0=0):
    """bs trees of n nodes from different families (verify_tree_model.random_tree), the first one off a chain where n allows."""
    return [TM.random_tree(seed0 + 3 + b, n) for b in range(bs)]


# ---------------------------------------------------------------- 1. the masked merge against the formula -------------------
@pytest.mark.parametrize("bs,nh,nhk,n,d,valid", [(2, 8, 2, 5, 128, [5, 1]), (2, 8, 2, 5, 128, [0, 4]), (1, 4, 4, 16, 64, [16]),
                                                 (3, 8, 8, 1, 128, [0, 1, 1])])
def test_tree_merge_against_the_formula(bs, nh, nhk, n, d, valid, env):
    torch, ops = env
    rs = np.random.RandomState(bs * 1000 + n)
    q, k, v, out_a, lse_a = _block(rs, bs, nh, nhk, n, d)
    lse_a[0, 0] = -np.inf                  # a head without a past: the block's own attention
    out_a[0, 0] = np.nan                   # (whose out is not used)
    if n > 1:
        lse_a[0, 1, 1] = np.nan            # a NaN row between finite neighbours
    for b, nb in enumerate(valid):         # NaN in every q / k / v row at or past n_b
        q[b, :, nb:], k[b, :, nb:], v[b, :, nb:] = np.nan, np.nan, np.nan
    trees = _trees_for(bs, n)
    masks = np.stack([TM.ancestor_masks(t) for t in trees])
    want_o, want_l = TM.tree_block_merge(q, k, v, out_a, lse_a, masks, valid)
    dev_n = _dev(torch, np.asarray(valid, np.int32))
    q_t = _dev(torch, q.transpose(0, 2, 1, 3)).transpose(1, 2)      # token-major under the (bs, nh, n, d) shape
    k_st, v_st = torch.zeros(bs, nhk, 16, d, dtype=torch.float16).cuda(), torch.zeros(bs, nhk, 16, d, dtype=torch.float16).cuda()
    oa = _dev(torch, out_a)
    got_o, got_l = ops.attn_block_merge(q_t, _dev(torch, k), _dev(torch, v), oa, _dev(torch, lse_a), dev_n, out=oa, return_lse=True,
                                        k_stage=k_st, v_stage=v_st, dev_mask=_dev(torch, masks))
    assert got_o.data_ptr() == oa.data_ptr()      # out aliased to out_a
    plain = ops.attn_block_merge(_dev(torch, q), _dev(torch, k), _dev(torch, v), _dev(torch, out_a), _dev(torch, lse_a), dev_n,
                                 dev_mask=_dev(torch, masks))
    torch.cuda.synchronize()
    go, gl = got_o.cpu().numpy(), got_l.cpu().numpy()
    assert np.array_equal(go.view(np.uint16), plain.cpu().numpy().view(np.uint16))
    assert np.array_equal(_bits(k_st[:, :, :n]), k.view(np.uint16)) and np.array_equal(_bits(v_st[:, :, :n]), v.view(np.uint16))
    assert not k_st[:, :, n:].any() and not v_st[:, :, n:].any()
    worst = worst_l = 0.0
    for b, nb in enumerate(valid):
        assert not go[b, :, nb:].view(np.uint16).any() and np.all(np.isneginf(gl[b, :, nb:])), f"request {b}: rows past n_b={nb}"
        for h in range(nh):
            for i in range(nb):
                if np.isnan(lse_a[b, h, i]):
                    assert np.isnan(go[b, h, i]).all() and np.isnan(gl[b, h, i])
                    continue
                assert np.isfinite(go[b, h, i]).all() and np.isfinite(gl[b, h, i]), (b, h, i)
                worst = max(worst, float(VG._row_err(go[b, h, i], want_o[b, h, i])))
                worst_l = max(worst_l, abs(float(gl[b, h, i]) - want_l[b, h, i]))
    print(f"tree merge {(bs, nh, nhk, n, d)} valid {valid} trees {trees}: worst row rel-L2 {worst:.3e}, worst lse error {worst_l:.3e}")
    assert worst < REL_TOL and worst_l <= R.LSE_TOL


def test_tree_merge_refuses_a_bad_mask_tensor(env):
    torch, ops = env
    rs = np.random.RandomState(1)
    q, k, v, out_a, lse_a = (_dev(torch, a) for a in _block(rs, 2, 4, 2, 3, 64))
    for bad in (torch.zeros(2, 3, dtype=torch.int64).cuda(), torch.zeros(2, 4, dtype=torch.int32).cuda(),
                torch.zeros(3, 2, dtype=torch.int32).cuda().t(), torch.zeros(2, 3, dtype=torch.int32)):
        with pytest.raises(RuntimeError):
            ops.attn_block_merge(q, k, v, out_a, lse_a, dev_mask=bad)


# ---------------------------------------------------------------- 2. gathered chains, bitwise -------------------------------
@pytest.mark.parametrize("nh,nhk,d", [(8, 2, 128), (4, 4, 64)])
def test_tree_rows_equal_the_chain_launch_on_gathered_chains(nh, nhk, d, env):
    """A masked key has weight exactly 0 and the kept terms are added in the same ascending order: row i of the masked launch
    is, bit for bit, the last row of the chain's launch on q[chain], k[chain], v[chain], out_a[chain], lse_a[chain]."""
    torch, ops = env
    n_rows = 0
    for seed, n, ps in TM.tree_set():
        if n == 1 and seed > 1:
            continue
        rs = np.random.RandomState(100 * n + seed)
        q, k, v, out_a, lse_a = _block(rs, 2, nh, nhk, n, d)
        valid = [n, max(1, n - 2)]
        t = [_dev(torch, a) for a in (q, k, v, out_a, lse_a)]
        masks = _dev(torch, np.stack([TM.ancestor_masks(ps)] * 2))
        got_o, got_l = ops.attn_block_merge(*t, _dev(torch, np.asarray(valid, np.int32)), return_lse=True, dev_mask=masks)
        go, gl = _bits(got_o), _bits(got_l)
        for i in range(n):
            c = TM.chain_of(ps, i)
            live = [b for b in range(2) if i < valid[b]]
            wo, wl = ops.attn_block_merge(*[x[:, :, c].contiguous() for x in t], return_lse=True)
            wo, wl = _bits(wo), _bits(wl)
            for b in live:
                assert np.array_equal(go[b, :, i], wo[b, :, -1]) and np.array_equal(gl[b, :, i], wl[b, :, -1]), \
                    f"tree {ps} node {i} request {b}: the masked row differs from the chain launch on {c}"
                n_rows += 1
        if ps == [i - 1 for i in range(n)]:      # a chain tree: the chain's call on all rows
            wo, wl = ops.attn_block_merge(*t, _dev(torch, np.asarray(valid, np.int32)), return_lse=True)
            assert np.array_equal(go, _bits(wo)) and np.array_equal(gl, _bits(wl)), f"chain tree of {n}"
    assert n_rows > 300


# ---------------------------------------------------------------- 3. masks nobody checked -------------------------------------
def test_tree_merge_on_untrusted_masks(env):
    torch, ops = env
    bs, nh, nhk, n, d = 3, 8, 2, 16, 128
    rs = np.random.RandomState(33)
    q, k, v, out_a, lse_a = _block(rs, bs, nh, nhk, n, d)
    valid = [16, 5, 0]
    trees = [TM.random_tree(3, n), TM.random_tree(2, n), TM.random_tree(6, n)]
    clean = np.stack([TM.ancestor_masks(t) for t in trees])
    dirty = clean.copy()
    for b in range(bs):
        for i in range(n):
            dirty[b, i] |= np.int32(-1 << (i + 1))                     # every bit above i, bits 16 .. 31 among them
            if b == 1 and i % 2:
                dirty[b, i] &= np.int32(~(1 << i))                     # and the row's own bit cleared
            if i >= valid[b]:
                dirty[b, i] = np.int32(rs.randint(-2 ** 31, 2 ** 31))  # rows at or past n_b: anything
    assert not np.array_equal(dirty, clean)
    res = []
    for masks in (clean, dirty):
        t = [_dev(torch, a) for a in (q, k, v, out_a, lse_a)]
        k_st, v_st = (torch.full((bs, nhk, 16, d), 7.0, dtype=torch.float16).cuda() for _ in range(2))
        o, l = ops.attn_block_merge(*t, _dev(torch, np.asarray(valid, np.int32)), return_lse=True, k_stage=k_st, v_stage=v_st,
                                    dev_mask=_dev(torch, masks))
        res.append([_bits(x) for x in (o, l, k_st, v_st)])
    for name, a, b in zip(("out", "lse", "k_stage", "v_stage"), *res):
        assert np.array_equal(a, b), f"{name} moved with mask bits the kernel must not read"
    want_o, _ = TM.tree_block_merge(q, k, v, out_a, lse_a, clean, valid)
    assert VG._row_err(res[0][0].view(np.float16)[0], want_o[0]).max() < REL_TOL


# ---------------------------------------------------------------- 4. a replayed graph ----------------------------------------
def test_tree_merge_graph_replay_follows_the_mask(env):
    torch, ops = env
    bs, nh, nhk, n, d = 2, 8, 2, 8, 128
    rs = np.random.RandomState(44)
    t = [_dev(torch, a) for a in _block(rs, bs, nh, nhk, n, d)]
    dev_n = _dev(torch, np.asarray([8, 6], np.int32))
    mask_sets = [np.stack([TM.ancestor_masks(TM.binary_tree(n)), TM.ancestor_masks(TM.random_tree(2, n))]),
                 np.stack([TM.ancestor_masks(TM.random_tree(1, n)), TM.ancestor_masks(TM.random_tree(3, n))])]
    masks = _dev(torch, mask_sets[0])
    out, lse = torch.zeros(bs, nh, n, d, dtype=torch.float16).cuda(), torch.zeros(bs, nh, n).cuda()
    call = lambda m, o, l: ops.attn_block_merge(*t, dev_n, out=o, lse_out=l, dev_mask=m)
    call(masks, out, lse)      # eager once: module load outside the capture
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        call(masks, out, lse)
    seen = []
    for ms in mask_sets:
        masks.copy_(torch.from_numpy(ms))
        out.fill_(float("nan"))
        lse.fill_(float("nan"))
        g.replay()
        torch.cuda.synchronize()
        eo, el = call(_dev(torch, ms), torch.zeros_like(out), torch.zeros_like(lse))
        torch.cuda.synchronize()
        assert np.array_equal(_bits(out), _bits(eo)) and np.array_equal(_bits(lse), _bits(el)), "a replay differs from the eager call"
        seen.append(_bits(out).copy())
    assert not np.array_equal(seen[0], seen[1])


# ---------------------------------------------------------------- 5. cache.verify(tree=) -------------------------------------
GEOMS = {"d128-M64-G4-n8": dict(nh=8, nhk=2, d=128, M=64, n=8),
         "d128-M64-G1-n3": dict(nh=2, nhk=2, d=128, M=64, n=3),
         "d64-M32-G4-n5": dict(nh=8, nhk=2, d=64, M=32, n=5)}
PS, CAP = 64, 128


def _tree_ref(oracle, cache, snap, l, q, k, v, trees, n_valid):
    """fp64 (out, lse) of verify(tree=) over what every slot of layer l holds on the device: every row's attention over the
    codes and the window rows (lse_ref.chunk_ref without a chunk), merged with the block rows its mask names."""
    qn, kn, vn = q.cpu().numpy(), k.cpu().numpy(), v.cpu().numpy()
    cap = cache.extended_residual_size
    outs, lses = [], []
    for b in range(cache.bs):
        T, r, st_ = (int(x) for x in snap["lengths"][l, b, :3])
        kc, vc = CL.gather_codes(snap, l, b, T, cache.page_size) if T else (np.zeros((cache.num_key_value_heads, 0, cache.M), np.uint8),) * 2
        ring = (st_ + np.arange(r)) % cap
        st = dict(q=np.nan_to_num(qn[b:b + 1]), k_res=snap["k_res"][l, b:b + 1], k_codes=kc[None], v_codes=vc[None],
                  k_cents=cache.key_cent.cpu().numpy(), v_cents=cache.value_cent.cpu().numpy(),
                  k_win=snap["k_res"][l, b:b + 1].view(np.float16)[:, :, ring], v_win=snap["v_res"][l, b:b + 1].view(np.float16)[:, :, ring],
                  k_ch=None, v_ch=None)
        o, s = R.chunk_ref(oracle, st, [n_valid[b]])
        outs.append(o)
        lses.append(s)
    masks = np.stack([TM.ancestor_masks(t) for t in trees])
    return TM.tree_block_merge(qn, kn, vn, np.concatenate(outs), np.concatenate(lses), masks, n_valid)


@pytest.mark.parametrize("T", [0, 63, 200])
@pytest.mark.parametrize("name", list(GEOMS))
def test_verify_tree_against_the_device_state(name, T, env, oracle):
    """Three slots, paging on demand with 0xFF in every free page, NaN in every dead ring row and in every q / K / V row past
    n_draft.  Per window length: one tree shared by every slot with every node live - both routes, the staging buffers, and
    every node against the chain's verify() of its gathered chain - then a tree per slot with n_draft = [n, 0, 2]."""
    torch, ops = env
    g = GEOMS[name]
    nh, nhk, d, n, bs = g["nh"], g["nhk"], g["d"], g["n"], 3
    rs = np.random.RandomState(T + n)
    cache = VG._cache(torch, bs=bs, nh=nh, nhk=nhk, d=d, M=g["M"], ps=PS, cap=CAP, preallocate=False, max_tokens=1024)
    if T:
        for b in range(bs):
            cache.prefill_request(b, *VG._rows(torch, rs, 1, nh, nhk, T, d), 0)
    shared = TM.binary_tree(n) if n == 8 else TM.random_tree(2, n)
    per_slot = [shared, TM.random_tree(1, n), TM.random_tree(3, n)]
    worst = 0.0
    for r in (0, 17, CAP):
        VG._set_window(torch, cache, rs, r, start=0 if r == 0 else 5)
        VG._poison_free_pages(torch, cache)
        for tree, trees, n_draft in ((shared, [shared] * bs, [n] * bs), (per_slot, per_slot, [n, 0, 2])):
            q, k, v = VG._rows(torch, rs, bs, nh, nhk, n, d)
            for b, nv in enumerate(n_draft):
                q[b, :, nv:], k[b, :, nv:], v[b, :, nv:] = float("nan"), float("nan"), float("nan")
            torch.cuda.synchronize()
            before = CL.snapshot(cache)
            heads = cache.verify(q, k, v, 0, n_draft=n_draft, route="heads", return_lse=True, tree=tree)
            rec = cache._verify_rec
            chunk = cache.verify(q, k, v, 0, n_draft=n_draft, route="chunk", return_lse=True, tree=tree)
            auto = cache.verify(q, k, v, 0, n_draft=n_draft, tree=tree)
            assert cache._verify_rec is rec and rec["tree"] == tuple(tuple(t) for t in trees)
            torch.cuda.synchronize()
            assert VG._same(before, CL.snapshot(cache)), f"T={T} r={r}: verify(tree=) moved lengths, pages or window bytes"
            assert np.array_equal(_bits(cache._kstage[0, :, :, :n]), _bits(k)) and np.array_equal(_bits(cache._vstage[0, :, :, :n]), _bits(v)), \
                "the staging buffers hold all n rows, bit for bit"
            ref = _tree_ref(oracle, cache, before, 0, q, k, v, trees, n_draft)
            what = f"{name} T={T} r={r} n_draft={n_draft}"
            worst = max(worst, VG._check_verify(heads, ref, n_draft, what + " heads"), VG._check_verify(chunk, ref, n_draft, what + " chunk"))
            ho, co = heads[0].float().cpu().numpy(), chunk[0].float().cpu().numpy()
            for b, nv in enumerate(n_draft):
                if nv:
                    e = VG._row_err(ho[b, :, :nv], co[b, :, :nv])
                    assert e.max() < 2e-3, f"{what}: routes differ by {e.max():.3e}"
                    e = VG._row_err(auto[b, :, :nv].float().cpu().numpy(), ho[b, :, :nv])
                    assert e.max() < 2e-3, f"{what}: route=None differs by {e.max():.3e}"
            if tree is shared:      # every node against the chain's verify of its gathered chain
                for i in range(n):
                    c = TM.chain_of(shared, i)
                    lin = cache.verify(q[:, :, c], k[:, :, c], v[:, :, c], 0, route="heads")
                    e = VG._row_err(lin[:, :, -1].float().cpu().numpy(), ho[:, :, i])
                    assert e.max() < 2e-3, f"{what}: node {i} differs from the chain's verify of {c} by {e.max():.3e}"
                assert "tree" not in cache._verify_rec
    print(f"{name} T={T}: worst row rel-L2 {worst:.3e} (bar {REL_TOL:.0e})")


# ---------------------------------------------------------------- 6. commit(path=) = single steps, bit for bit ---------------
NH, NHK, D, M_, LAYERS, BS, N = 8, 2, 128, 64, 2, 3, 6


def _pick_path(rs, parents, n_live):
    """The empty path now and then, else the chain of a random live node (the deeper of two draws)."""
    if n_live == 0 or rs.randint(0, 6) == 0:
        return []
    return max((TM.chain_of(parents, int(x)) for x in rs.randint(0, n_live, 2)), key=len)


@pytest.mark.parametrize("cap,preallocate", [(64, True), (32, True), (64, False)], ids=["cap64", "cap32", "cap64-on-demand"])
def test_commit_path_equals_single_steps(cap, preallocate, env):
    """Rounds of verify(n = 6, a random tree per slot) + commit(path=) on a cache of 3 slots against 3 batch-1 twins that take
    the path's rows through decoding_with_pages; free pages are 0xFF and dead ring rows NaN before every verify and commit.
    cap = 32 is the page size: a flush there takes the whole window and the path's last rows land on ring slots of flushed rows."""
    torch, ops = env
    ps = 32
    rs = np.random.RandomState(7 * cap + preallocate)
    mk = lambda bs: VG._cache(torch, bs=bs, nh=NH, nhk=NHK, d=D, M=M_, ps=ps, cap=cap, layers=LAYERS, max_tokens=512, preallocate=preallocate)
    A, twins = mk(BS), [mk(1) for _ in range(BS)]
    for b, T in ((0, 45), (2, 64)):      # slot 1 starts empty
        hs = np.random.RandomState(T)
        rows = [VG._rows(torch, hs, 1, NH, NHK, T, D) for _ in range(LAYERS)]
        for l in range(LAYERS):
            A.prefill_request(b, *rows[l], l)
            twins[b].prefill_request(0, *rows[l], l)
    VG._compare_with_twins(torch, A, twins, "start")
    rows_in, rounds, wrapped, reordered = [0] * BS, 0, 0, 0
    while min(rows_in) < 100:
        trees = [TM.random_tree(int(rs.randint(1000)), N) for _ in range(BS)]
        n_draft = [N, int(rs.randint(0, N + 1)), N]
        path = [[] for _ in range(BS)] if rounds == 1 else [_pick_path(rs, trees[b], n_draft[b]) for b in range(BS)]
        VG._poison_free_pages(torch, A)
        VG._poison_dead_rows(torch, A)
        qkv = [VG._rows(torch, rs, BS, NH, NHK, N, D) for _ in range(LAYERS)]
        for l in range(LAYERS):
            out = A.verify(*qkv[l], l, n_draft=n_draft, tree=trees)
            assert all(torch.isfinite(out[b, :, :n_draft[b]]).all() for b in range(BS)), f"round {rounds} layer {l}: non-finite verify output"
        VG._poison_free_pages(torch, A)
        VG._poison_dead_rows(torch, A)
        for b, p in enumerate(path):
            r0 = int(A._r_a[0, b])
            wrapped += bool(p) and r0 + len(p) > cap and r0 > 0
            reordered += p != list(range(len(p)))
        A.commit(path=path)
        for b, tw in enumerate(twins):
            for i in path[b]:
                for l in range(LAYERS):
                    q, k, v = qkv[l]
                    tw.decoding_with_pages(q[b:b + 1, :, i:i + 1].contiguous(), k[b:b + 1, :, i:i + 1].contiguous(),
                                           v[b:b + 1, :, i:i + 1].contiguous(), l, use_dev_lengths=True)
        VG._compare_with_twins(torch, A, twins, f"round {rounds} (path {path})")
        rows_in = [x + len(p) for x, p in zip(rows_in, path)]
        rounds += 1
    assert all(int(A._T_a[0, b]) >= 2 * ps for b in range(BS)), "a slot crossed fewer than two flushes"
    assert wrapped >= 3 and reordered >= 10, (wrapped, reordered)      # flushes with rows of the path on both sides; paths off range(a)
    if not preallocate:
        used = lambda c: c.page_manager.get_stats()["allocated_pages"]
        assert used(A) == sum(used(tw) for tw in twins), f"{used(A)} pages in use, the twins hold {[used(tw) for tw in twins]}"
    print(f"cap {cap} preallocate {preallocate}: {rounds} rounds, rows per slot {rows_in}, T {A._T_a[0].tolist()}, {wrapped} flushes, {reordered} paths off range(a)")


def test_commit_path_refusals_move_nothing(env):
    torch, ops = env
    rs = np.random.RandomState(13)
    cache = VG._cache(torch, bs=2, nh=NH, nhk=NHK, d=D, M=M_, ps=32, cap=64, layers=LAYERS, max_tokens=256)
    for l in range(LAYERS):
        cache.prefill(*VG._rows(torch, rs, 2, NH, NHK, 40, D), l)
    qkv = [VG._rows(torch, rs, 2, NH, NHK, 5, D) for _ in range(LAYERS)]
    tree = [-1, 0, 0, 1, -1]
    for l in range(LAYERS):
        cache.verify(*qkv[l], l, n_draft=[5, 3], tree=tree)
    torch.cuda.synchronize()
    before = CL.snapshot(cache)
    for match, a, kw in (("path", ([1, 1],), {}), ("path", (), dict(path=[[1], []])), ("path", (), dict(path=[[0, 3], []])),
                         ("path", (), dict(path=[[0], [0, 1, 3]])), ("path", ([1, 0],), dict(path=[[0, 1], []]))):
        with pytest.raises(RuntimeError, match=match):
            cache.commit(*a, **kw)
        torch.cuda.synchronize()
        assert VG._same(before, CL.snapshot(cache)), f"a refused commit ({a}, {kw}) moved something"
    with pytest.raises(RuntimeError, match="tree"):
        cache.verify(*qkv[0], 0, tree=[-1, 0, 0, 1, 4])
    r0, st0, cap = int(cache._r_a[0, 0]), int(cache._rs_a[0, 0]), cache.extended_residual_size
    assert r0 + 3 <= cap
    cache.commit(path=[[0, 1, 3], [0, 2]])
    torch.cuda.synchronize()
    assert cache._r_a.tolist() == [[r0 + 3, r0 + 2]] * LAYERS
    ring = cache._kres_all.cpu().numpy()
    slots = lambda a: [(st0 + r0 + j) % cap for j in range(a)]
    for l in range(LAYERS):
        k = qkv[l][1].cpu().numpy()
        assert np.array_equal(ring[l, 0][:, slots(3)], k[0][:, [0, 1, 3]]) and np.array_equal(ring[l, 1][:, slots(2)], k[1][:, [0, 2]])


# ---------------------------------------------------------------- 7. row indices nobody checked -------------------------------
UNTRUSTED_IDX = [[3, -5, 100, 1],                       # 4 rows: 3, 0 (clamped), 3 (clamped), 1
                 [2, 0, -1, 0x7FFFFFFF],                # 2 rows; the entries at or past a_b are never used
                 [-1, 0x7FFFFFFF, -1, 0x7FFFFFFF],      # no rows
                 [1, 7, 0, 0x7FFFFFFF]]                 # 3 rows: 1, 3 (clamped), 0


@pytest.mark.parametrize("d,M,C", [(64, 16, 128), (128, 64, 256)])
def test_window_commit_on_untrusted_row_indices(d, M, C, env, oracle):
    """ops.window_commit(dev_rows=) on the lengths rows and row counts of test_window_commit_on_untrusted_rows (outside their
    ranges, two layers with different values) and on indices outside [0, 4): verify_tree_model.commit_rows - single decode
    steps over the gathered, clamped rows.  Pools, windows, lengths, dev_n, dev_rows: every byte."""
    from tests import store_ragged_model as SM
    torch, ops = env
    layers, bs, nhk, ps, cap, npc, nb = 2, 4, 2, 32, 64, 8, 4
    rs = np.random.RandomState(d + M + 1)
    f16 = lambda *s: rs.standard_normal(s).astype(np.float16)
    k_new, v_new = f16(layers, bs, nhk, nb, d), f16(layers, bs, nhk, nb, d)
    k_win, v_win = f16(layers, bs, nhk, cap, d), f16(layers, bs, nhk, cap, d)
    k_cents, v_cents = f16(M, C, d // M), f16(M, C, d // M)
    n_real = layers * bs * nhk * npc
    n_pool = n_real + 5
    ids = rs.permutation(n_pool)[:n_real].reshape(layers, bs, nhk, npc).astype(np.int32)
    lengths = np.array([[row + (VG.WORD3,) for row in layer] for layer in VG.UNTRUSTED_ROWS], np.int32)
    idx = np.asarray(UNTRUSTED_IDX, np.int32)
    k_pool, v_pool = np.full((n_pool, ps, M), 0xA5, np.uint8), np.full((n_pool, M, ps), 0xA5, np.uint8)

    want_len, want_kw, want_vw, want_kp, want_vp = lengths.copy(), k_win.copy(), v_win.copy(), k_pool.copy(), v_pool.copy()
    for l in range(layers):
        for b in range(bs):
            T, r, st, a = SM.clamp(VG.UNTRUSTED_ROWS[l][b] + (VG.UNTRUSTED_N[b],), cap_tok=npc * ps, resid_cap=cap, n_bound=nb)
            T2, r2, st2, coded, ring = TM.commit_rows(T, r, st, a, ps, cap, UNTRUSTED_IDX[b], nb)
            if a == 0 or T2 > npc * ps:
                continue
            want_len[l, b, :3] = (T2, r2, st2)
            for win, new, cents, side in ((k_win, k_new, k_cents, "k"), (v_win, v_new, v_cents, "v")):
                want_w = want_kw if side == "k" else want_vw
                for slot, e in enumerate(ring):
                    if e is not None and e[0] == "n":
                        want_w[l, b, :, slot] = new[l, b, :, e[1]]
                if coded:
                    toks = sorted(coded)
                    src = np.stack([win[l, b, :, (st + coded[t][1]) % cap] if coded[t][0] == "w" else new[l, b, :, coded[t][1]] for t in toks], axis=1)
                    codes = oracle.pq_encode(src[None], cents)[0]
                    for j, t in enumerate(toks):
                        for h in range(nhk):
                            if side == "k":
                                want_kp[ids[l, b, h, t // ps], t % ps, :] = codes[h, j]
                            else:
                                want_vp[ids[l, b, h, t // ps], :, t % ps] = codes[h, j]
    # what the table says, before the kernel is asked: the lengths move as for million_window_commit; which rows went where
    assert want_len[0, :, :3].tolist() == [[32, 36, 32], [250, 64, 5], [10, -3, -1], [40, 13, 0]]
    assert want_len[1, :, :3].tolist() == [[10 ** 9, 62, 63], [63, 33, 28], [-7, 9999, 12], [0, 3, 0]]
    assert np.array_equal(want_kw[0, 0, :, :4], k_new[0, 0][:, [3, 0, 3, 1]]) and np.array_equal(want_vw[0, 3, :, 10:13], v_new[0, 3][:, [1, 3, 0]])
    assert np.array_equal(want_kw[1, 3, :, :3], k_new[1, 3][:, [1, 3, 0]])

    dev = lambda a: _dev(torch, a)
    kc, vc = dev(k_cents), dev(v_cents)
    t = dict(k_new=dev(k_new), v_new=dev(v_new), k_win=dev(k_win), v_win=dev(v_win), k_pool=dev(k_pool), v_pool=dev(v_pool),
             ids=dev(ids), lengths=dev(lengths), dev_n=dev(np.asarray(VG.UNTRUSTED_N, np.int32)), dev_rows=dev(idx))
    for bad in (t["dev_rows"].long(), t["dev_rows"][:, :3], t["dev_rows"].t().contiguous().t(), t["dev_rows"].cpu()):
        with pytest.raises(RuntimeError):
            ops.window_commit(t["k_new"], t["v_new"], t["k_win"], t["v_win"], ops.prepare_cents(kc, cache=False), ops.prepare_cents(vc, cache=False),
                              t["k_pool"], t["v_pool"], t["ids"], t["lengths"], t["dev_n"], M=M, C=C, n_bound=nb, dev_rows=bad)
    ops.window_commit(t["k_new"], t["v_new"], t["k_win"], t["v_win"], ops.prepare_cents(kc, cache=False), ops.prepare_cents(vc, cache=False),
                      t["k_pool"], t["v_pool"], t["ids"], t["lengths"], t["dev_n"], M=M, C=C, n_bound=nb, dev_rows=t["dev_rows"])
    torch.cuda.synchronize()
    got = {k: v.cpu().numpy() for k, v in t.items()}
    assert got["dev_n"].tolist() == VG.UNTRUSTED_N and np.array_equal(got["dev_rows"], idx), "dev_n and dev_rows are read, never written"
    assert (got["lengths"][:, :, 3] == VG.WORD3).all(), "word 3 of a lengths row was written"
    assert np.array_equal(got["lengths"], want_len), f"lengths {got['lengths'][:, :, :3].tolist()}, expected {want_len[:, :, :3].tolist()}"
    for name, want in (("k_win", want_kw), ("v_win", want_vw)):
        assert np.array_equal(got[name].view(np.uint16), want.view(np.uint16)), f"{name}: window rows differ at (layer, slot, head, row) {np.unique(np.argwhere(got[name] != want)[:, :4], axis=0)[:8].tolist()}"
    for name, want in (("k_pool", want_kp), ("v_pool", want_vp)):
        assert np.array_equal(got[name], want), f"{name}: pages {np.unique(np.argwhere(got[name] != want)[:, 0])[:8].tolist()} differ"
    assert np.array_equal(got["k_new"], k_new) and np.array_equal(got["v_new"], v_new) and np.array_equal(got["ids"], ids)
