"""GPU tests of draft verification: ops.attn_block_merge against the fp64 formula (tests/verify_model.py), PagedPQCache.verify
against an fp64 softmax over what the cache holds on the device (lse_ref.chunk_ref), PagedPQCache.commit against batch-1 twin
caches that take the accepted rows through decoding_with_pages one by one, poisoned free pages and dead ring rows, refusals.

Bars.  Outputs against fp64: per-row (per-head) rel-L2 < 1e-3, lse within lse_ref.LSE_TOL.  Two routes, or two batch sizes, of one
attention against each other: 2e-3 (each within 1e-3 of the fp64 value; the bar of test_attn_lse_gpu.py).  Everything a commit
leaves - device lengths, host mirror, live code bytes, live window rows - bitwise."""
import numpy as np
import pytest

from tests import cache_life_model as CL
from tests import lse_ref as R
from tests import verify_model as VM

pytestmark = pytest.mark.gpu

REL_TOL = 1e-3


@pytest.fixture(scope="module")
def env():
    import torch
    assert torch.cuda.is_available(), "GPU tests need an MI355X"
    from million_amd import ops, _lib
    _lib.load()
    yield torch, ops
    assert ops.tail_faults() == 0      # no split merge of the decode launches of this file gave up


def _row_err(out, gold):
    """||out - gold|| / ||gold|| over d for every row."""
    out, gold = np.asarray(out, np.float64), np.asarray(gold, np.float64)
    return np.linalg.norm(out - gold, axis=-1) / np.maximum(np.linalg.norm(gold, axis=-1), 1e-300)


def _same(before, after):
    return all(np.array_equal(before[k], after[k]) if isinstance(before[k], np.ndarray) else before[k] == after[k] for k in before)


# ---------------------------------------------------------------- 1. ops.attn_block_merge -------------------------------------
@pytest.mark.parametrize("bs,nh,nhk,n,d,valid", [(2, 8, 2, 5, 128, [5, 1]), (1, 4, 4, 16, 64, [16]), (1, 4, 4, 16, 64, [0]),
                                                 (3, 8, 8, 1, 128, [0, 1, 1])])
def test_block_merge_against_the_formula(bs, nh, nhk, n, d, valid, env):
    torch, ops = env
    rs = np.random.RandomState(bs * 1000 + n)
    f16 = lambda *s: rs.standard_normal(s).astype(np.float16)
    q, k, v, out_a = f16(bs, nh, n, d), f16(bs, nhk, n, d), f16(bs, nhk, n, d), f16(bs, nh, n, d)
    lse_a = (rs.standard_normal((bs, nh, n)) * 2 + 3).astype(np.float32)
    lse_a[0, 0] = -np.inf                  # a head without a past: the block's own attention
    out_a[0, 0] = np.nan                   # (whose out is not used)
    if n > 1:
        lse_a[0, 1, 1] = np.nan            # a NaN row between finite neighbours
    for b, nb in enumerate(valid):         # NaN in every q / k / v row at or past n_b
        q[b, :, nb:], k[b, :, nb:], v[b, :, nb:] = np.nan, np.nan, np.nan
    want_o, want_l = VM.block_merge(q, k, v, out_a, lse_a, valid)
    dev = lambda a: torch.from_numpy(np.ascontiguousarray(a)).cuda()
    dev_n = dev(np.asarray(valid, np.int32))
    # q token-major under the (bs, nh, n, d) shape: a strided view
    q_t = dev(q.transpose(0, 2, 1, 3)).transpose(1, 2)
    assert not q_t.is_contiguous() or n == 1 or nh == 1
    k_st, v_st = torch.zeros(bs, nhk, 16, d, dtype=torch.float16).cuda(), torch.zeros(bs, nhk, 16, d, dtype=torch.float16).cuda()
    oa = dev(out_a)
    got_o, got_l = ops.attn_block_merge(q_t, dev(k), dev(v), oa, dev(lse_a), dev_n, out=oa, return_lse=True, k_stage=k_st, v_stage=v_st)
    assert got_o.data_ptr() == oa.data_ptr()      # out aliased to out_a
    # and into a fresh out, without lse and staging: the same bits
    plain = ops.attn_block_merge(dev(q), dev(k), dev(v), dev(out_a), dev(lse_a), dev_n)
    torch.cuda.synchronize()
    go, gl = got_o.cpu().numpy(), got_l.cpu().numpy()
    assert np.array_equal(go.view(np.uint16), plain.cpu().numpy().view(np.uint16))
    assert np.array_equal(k_st[:, :, :n].cpu().numpy().view(np.uint16), k.view(np.uint16))      # staging rows: bitwise k, v
    assert np.array_equal(v_st[:, :, :n].cpu().numpy().view(np.uint16), v.view(np.uint16))
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
                worst = max(worst, float(_row_err(go[b, h, i], want_o[b, h, i])))
                worst_l = max(worst_l, abs(float(gl[b, h, i]) - want_l[b, h, i]))
    print(f"block merge {(bs, nh, nhk, n, d)} valid {valid}: worst row rel-L2 {worst:.3e}, worst lse error {worst_l:.3e}")
    assert worst < REL_TOL and worst_l <= R.LSE_TOL


def test_block_merge_without_dev_n_serves_every_row(env):
    torch, ops = env
    rs = np.random.RandomState(7)
    bs, nh, nhk, n, d = 2, 4, 2, 3, 64
    f16 = lambda *s: rs.standard_normal(s).astype(np.float16)
    q, k, v, out_a = f16(bs, nh, n, d), f16(bs, nhk, n, d), f16(bs, nhk, n, d), f16(bs, nh, n, d)
    lse_a = rs.standard_normal((bs, nh, n)).astype(np.float32)
    dev = lambda a: torch.from_numpy(a).cuda()
    got_o, got_l = ops.attn_block_merge(dev(q), dev(k), dev(v), dev(out_a), dev(lse_a), return_lse=True)
    want_o, want_l = VM.block_merge(q, k, v, out_a, lse_a)
    assert _row_err(got_o.cpu().numpy(), want_o).max() < REL_TOL and np.abs(got_l.cpu().numpy() - want_l).max() <= R.LSE_TOL


# ---------------------------------------------------------------- caches ---------------------------------------------------------
def _cache(torch, *, bs, nh, nhk, d, M, ps, cap, layers=1, max_tokens=2048, preallocate=True):
    from million_amd.pq_cache import PagedPQCache
    from tests import synth
    cache = PagedPQCache(bs=bs, nh=nh, num_key_value_heads=nhk, M=M, layer_num=layers, d=d, page_size=ps,
                         extended_residual_size=cap, max_tokens=max_tokens, preallocate=preallocate)
    cent = lambda seed: torch.from_numpy(synth.encode_case(seed, 1, nhk, 1, d, M, 256)["cents"])
    cache.set_cent(cent(5100), cent(5101))
    return cache


def _rows(torch, rs, bs, nh, nhk, n, d):
    f = lambda h: torch.from_numpy(rs.standard_normal((bs, h, n, d)).astype(np.float16)).cuda()
    return f(nh), f(nhk), f(nhk)


def _set_window(torch, cache, rs, r, start):
    """Every slot's window of every layer: r random rows from ring slot `start`, NaN in every dead row; mirror and device rows."""
    cap, nk, d = cache.extended_residual_size, cache.num_key_value_heads, cache.d
    r = np.broadcast_to(np.asarray(r), (cache.bs,))
    for t in (cache._kres_all, cache._vres_all):
        t.fill_(float("nan"))
        for b in range(cache.bs):
            if r[b]:
                ring = torch.from_numpy((start + np.arange(int(r[b]))) % cap).cuda()
                t[:, b].index_copy_(2, ring, torch.from_numpy(rs.standard_normal((cache.layer_num, nk, int(r[b]), d)).astype(np.float16)).cuda())
    cache._r_a[:] = r[None, :]
    cache._rs_a[:] = start
    for l in range(cache.layer_num):
        cache._sync_lengths(l)


def _poison_free_pages(torch, cache):
    if not cache.preallocate and cache.page_manager.free_pages:
        free = torch.tensor(sorted(cache.page_manager.free_pages), dtype=torch.long).cuda()
        cache.key_page_pool[free] = 0xFF
        cache.value_page_pool[free] = 0xFF


def _poison_dead_rows(torch, cache):
    cap = cache.extended_residual_size
    dead = np.ones((cache.layer_num, cache.bs, cap), bool)
    for l in range(cache.layer_num):
        for b in range(cache.bs):
            dead[l, b, (int(cache._rs_a[l, b]) + np.arange(int(cache._r_a[l, b]))) % cap] = False
    mask = torch.from_numpy(dead).cuda()[:, :, None, :].expand(-1, -1, cache.num_key_value_heads, -1)
    cache._kres_all[mask] = float("nan")
    cache._vres_all[mask] = float("nan")


def _verify_ref(oracle, cache, snap, l, q, k, v, n_valid):
    """fp64 (out, lse) of verify over what every slot of layer l holds on the device: lse_ref.chunk_ref per slot."""
    qn, kn, vn = q.cpu().numpy(), k.cpu().numpy(), v.cpu().numpy()
    cap = cache.extended_residual_size
    outs, lses = [], []
    for b in range(cache.bs):
        T, r, st_ = (int(x) for x in snap["lengths"][l, b, :3])
        kc, vc = CL.gather_codes(snap, l, b, T, cache.page_size) if T else (np.zeros((cache.num_key_value_heads, 0, cache.M), np.uint8),) * 2
        ring = (st_ + np.arange(r)) % cap
        st = dict(q=qn[b:b + 1], k_res=snap["k_res"][l, b:b + 1], k_codes=kc[None], v_codes=vc[None],
                  k_cents=cache.key_cent.cpu().numpy(), v_cents=cache.value_cent.cpu().numpy(),
                  k_win=snap["k_res"][l, b:b + 1].view(np.float16)[:, :, ring], v_win=snap["v_res"][l, b:b + 1].view(np.float16)[:, :, ring],
                  k_ch=kn[b:b + 1], v_ch=vn[b:b + 1])
        o, s = R.chunk_ref(oracle, st, [n_valid[b]])
        outs.append(o)
        lses.append(s)
    return np.concatenate(outs), np.concatenate(lses)


def _check_verify(got, ref, n_valid, what, tol=REL_TOL):
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
            assert np.abs(gl[b, :, :nv] - rl[b, :, :nv]).max() <= R.LSE_TOL, f"{what}: slot {b}: lse off by {np.abs(gl[b, :, :nv] - rl[b, :, :nv]).max():.3e}"
    return worst


# ---------------------------------------------------------------- 2. verify ----------------------------------------------------
GEOMS = {"d128-M64-G4-n4": dict(nh=8, nhk=2, d=128, M=64, n=4),       # 16 rows per kv head: one pass, streaming kernel
         "d128-M64-G1-n3": dict(nh=2, nhk=2, d=128, M=64, n=3),       # 3 rows: lean kernel
         "d64-M32-G4-n5": dict(nh=8, nhk=2, d=64, M=32, n=5)}         # 20 rows: more than one pass
PS, CAP = 64, 128


@pytest.mark.parametrize("T", [0, 63, 1000])
@pytest.mark.parametrize("name", list(GEOMS))
def test_verify_against_the_device_state(name, T, env, oracle):
    torch, ops = env
    g = GEOMS[name]
    nh, nhk, d, n, bs = g["nh"], g["nhk"], g["d"], g["n"], 2
    rs = np.random.RandomState(T + n)
    cache = _cache(torch, bs=bs, nh=nh, nhk=nhk, d=d, M=g["M"], ps=PS, cap=CAP)
    if T:
        cache.prefill(*_rows(torch, rs, bs, nh, nhk, T, d), 0)
    worst = 0.0
    for r in (0, 17, CAP):
        _set_window(torch, cache, rs, r, start=0 if r == 0 else 5)
        q, k, v = _rows(torch, rs, bs, nh, nhk, n, d)
        torch.cuda.synchronize()
        before = CL.snapshot(cache)
        heads = cache.verify(q, k, v, 0, route="heads", return_lse=True)
        chunk = cache.verify(q, k, v, 0, route="chunk", return_lse=True)
        host = cache.verify(q, k, v, 0, route="heads", use_dev_lengths=False)      # lockstep: host lengths
        auto = cache.verify(q, k, v, 0)
        torch.cuda.synchronize()
        assert _same(before, CL.snapshot(cache)), f"T={T} r={r}: verify moved lengths, pages or window bytes"
        ref = _verify_ref(oracle, cache, before, 0, q, k, v, [n] * bs)
        what = f"{name} T={T} r={r}"
        worst = max(worst, _check_verify(heads, ref, [n] * bs, what + " heads"), _check_verify(chunk, ref, [n] * bs, what + " chunk"))
        e = _row_err(heads[0].float().cpu().numpy(), chunk[0].float().cpu().numpy())
        assert e.max() < 2e-3, f"{what}: routes differ by {e.max():.3e}"
        for other, tag in ((host, "host lengths"), (auto, "route=None")):      # (another launch plan of the same attention)
            e = _row_err(other.float().cpu().numpy(), heads[0].float().cpu().numpy())
            assert e.max() < 2e-3, f"{what}: {tag} differs from device lengths by {e.max():.3e}"
        assert cache._verify_route(n) == "heads" and cache._verify_route(16) == ("heads" if 16 * (nh // nhk) <= 64 else "chunk")
        assert np.array_equal(cache._kstage[0, :, :, :n].cpu().numpy(), k.cpu().numpy()) and np.array_equal(cache._vstage[0, :, :, :n].cpu().numpy(), v.cpu().numpy())
    print(f"{name} T={T}: worst row rel-L2 {worst:.3e} (bar {REL_TOL:.0e})")


@pytest.mark.parametrize("name", list(GEOMS))
def test_verify_ragged_batch(name, env, oracle):
    """Three slots at different lengths, device lengths, n_draft = [n, 0, 2]; paging on demand with 0xFF in every free page and
    NaN in every dead ring row and in every q / K / V row past n_draft."""
    torch, ops = env
    g = GEOMS[name]
    nh, nhk, d, n, bs = g["nh"], g["nhk"], g["d"], g["n"], 3
    rs = np.random.RandomState(n)
    cache = _cache(torch, bs=bs, nh=nh, nhk=nhk, d=d, M=g["M"], ps=PS, cap=CAP, preallocate=False, max_tokens=1024)
    for b, T in enumerate((200, 77, 0)):
        if T:
            cache.prefill_request(b, *_rows(torch, rs, 1, nh, nhk, T, d), 0)
    _set_window(torch, cache, rs, [CAP, 3, 40], start=100)
    _poison_free_pages(torch, cache)
    n_draft = [n, 0, 2]
    q, k, v = _rows(torch, rs, bs, nh, nhk, n, d)
    for b, nv in enumerate(n_draft):
        q[b, :, nv:], k[b, :, nv:], v[b, :, nv:] = float("nan"), float("nan"), float("nan")
    torch.cuda.synchronize()
    before = CL.snapshot(cache)
    heads = cache.verify(q, k, v, 0, n_draft=n_draft, route="heads", return_lse=True)
    chunk = cache.verify(q, k, v, 0, n_draft=n_draft, route="chunk", return_lse=True)
    torch.cuda.synchronize()
    assert _same(before, CL.snapshot(cache)), "verify moved lengths, pages or window bytes"
    ref = _verify_ref(oracle, cache, before, 0, q, k, v, n_draft)
    w = max(_check_verify(heads, ref, n_draft, name + " ragged heads"), _check_verify(chunk, ref, n_draft, name + " ragged chunk"))
    print(f"{name} ragged: worst row rel-L2 {w:.3e}")


# ---------------------------------------------------------------- 3. commit = single steps, bit for bit -----------------------
NH, NHK, D, M_, LAYERS, BS, N = 8, 2, 128, 64, 2, 3, 4


def _compare_with_twins(torch, A, twins, what):
    torch.cuda.synchronize()
    sa = CL.snapshot(A)
    cap, ps = A.extended_residual_size, A.page_size
    for b, tw in enumerate(twins):
        st = CL.snapshot(tw)
        for l in range(A.layer_num):
            assert np.array_equal(sa["lengths"][l, b, :3], st["lengths"][l, 0, :3]), \
                f"{what}: device lengths of layer {l} slot {b}: {sa['lengths'][l, b].tolist()}, twin {st['lengths'][l, 0].tolist()}"
            mine = [int(a[l, b]) for a in (A._T_a, A._r_a, A._rs_a, A._seen_a)]
            theirs = [int(a[l, 0]) for a in (tw._T_a, tw._r_a, tw._rs_a, tw._seen_a)]
            assert mine == theirs and mine[:3] == sa["lengths"][l, b, :3].tolist(), f"{what}: host mirror of layer {l} slot {b}: {mine}, twin {theirs}"
            T, r, rs_ = mine[:3]
            if T:
                for side, x, y in zip("KV", CL.gather_codes(sa, l, b, T, ps), CL.gather_codes(st, l, 0, T, ps)):
                    assert np.array_equal(x, y), f"{what}: {side} codes of layer {l} slot {b} differ from the twin's at tokens {np.unique(np.argwhere(x != y)[:, 1])[:8].tolist()}"
            ring = (rs_ + np.arange(r)) % cap
            for side in ("k_res", "v_res"):
                assert np.array_equal(sa[side][l, b][:, ring], st[side][l, 0][:, ring]), f"{what}: {side} window rows of layer {l} slot {b} differ from the twin's"
    return sa


@pytest.mark.parametrize("cap,preallocate,fork", [(64, True, False), (32, True, False), (64, False, False), (64, False, True)],
                         ids=["cap64", "cap32", "cap64-on-demand", "cap64-on-demand-fork"])
def test_commit_equals_single_steps(cap, preallocate, fork, env):
    """Rounds of verify(n = 4) + commit(n_accept) on a cache of 3 slots against 3 batch-1 twins that take the accepted rows through
    decoding_with_pages; free pages are 0xFF and dead ring rows NaN before every verify and every commit."""
    torch, ops = env
    ps = 32
    rs = np.random.RandomState(cap + 2 * preallocate + fork)
    mk = lambda bs: _cache(torch, bs=bs, nh=NH, nhk=NHK, d=D, M=M_, ps=ps, cap=cap, layers=LAYERS, max_tokens=512, preallocate=preallocate)
    A, twins = mk(BS), [mk(1) for _ in range(BS)]

    def history(cache, b):      # a prompt of 70 tokens (two pages and a tail) and 5 decode steps, the same rows wherever it runs
        hs = np.random.RandomState(99)
        for l in range(LAYERS):
            cache.prefill_request(b, *_rows(torch, hs, 1, NH, NHK, 70, D), l)
        if cache.bs == 1:
            for _ in range(5):
                for l in range(LAYERS):
                    cache.decoding_with_pages(*_rows(torch, hs, 1, NH, NHK, 1, D), l, use_dev_lengths=True)
    shared = {}
    if fork:
        # slot 0 is built in a batch-1 cache of its own and restored into A (a decode step of A would move every slot), then forked
        donor = mk(1)
        history(donor, 0)
        A.swap_in(0, donor.swap_out(0))
        A.fork(0, [1, 2])
        for tw in twins:
            history(tw, 0)
        torch.cuda.synchronize()
        pm = A.page_manager
        pids = sorted(p for p in pm.allocated_pages if pm.ref_count(p) > 1)
        assert pids, "the fork shares no page"
        shared = {p: (A.key_page_pool[p].cpu().numpy().copy(), A.value_page_pool[p].cpu().numpy().copy()) for p in pids}
    else:
        for b, T in ((0, 45), (2, 64)):      # slot 1 starts empty
            hs = np.random.RandomState(T)
            rows = [_rows(torch, hs, 1, NH, NHK, T, D) for _ in range(LAYERS)]
            for l in range(LAYERS):
                A.prefill_request(b, *rows[l], l)
                twins[b].prefill_request(0, *rows[l], l)
    _compare_with_twins(torch, A, twins, "start")
    rows_in = [0] * BS
    rounds = 0
    while min(rows_in) < 100:
        n_accept = [0] * BS if rounds == 1 else [int(x) for x in rs.randint(0, N + 1, BS)]
        _poison_free_pages(torch, A)
        _poison_dead_rows(torch, A)
        qkv = [_rows(torch, rs, BS, NH, NHK, N, D) for _ in range(LAYERS)]
        for l in range(LAYERS):
            out = A.verify(*qkv[l], l)
            assert torch.isfinite(out).all(), f"round {rounds} layer {l}: non-finite verify output"
        _poison_free_pages(torch, A)
        _poison_dead_rows(torch, A)
        A.commit(n_accept)
        for b, tw in enumerate(twins):
            for i in range(n_accept[b]):
                for l in range(LAYERS):
                    q, k, v = qkv[l]
                    tw.decoding_with_pages(q[b:b + 1, :, i:i + 1].contiguous(), k[b:b + 1, :, i:i + 1].contiguous(),
                                           v[b:b + 1, :, i:i + 1].contiguous(), l, use_dev_lengths=True)
        _compare_with_twins(torch, A, twins, f"round {rounds} (n_accept {n_accept})")
        rows_in = [x + a for x, a in zip(rows_in, n_accept)]
        rounds += 1
    assert all(int(A._T_a[0, b]) >= 2 * ps for b in range(BS)), "a slot crossed fewer than two flushes"
    # one ordinary decode step on both: the same state, so the same attention (the batch sizes differ, hence the two-kernel bar)
    for l in range(LAYERS):
        q, k, v = _rows(torch, rs, BS, NH, NHK, 1, D)
        out = A.decoding_with_pages(q, k, v, l, use_dev_lengths=True)
        for b, tw in enumerate(twins):
            o1 = tw.decoding_with_pages(q[b:b + 1].contiguous(), k[b:b + 1].contiguous(), v[b:b + 1].contiguous(), l, use_dev_lengths=True)
            e = _row_err(out[b:b + 1].float().cpu().numpy(), o1.float().cpu().numpy())
            assert torch.isfinite(out[b]).all() and e.max() < 2e-3, f"decode step after the rounds: layer {l} slot {b}: {e.max():.3e}"
    _compare_with_twins(torch, A, twins, "after a decode step")
    if not preallocate and not fork:
        used = lambda c: c.page_manager.get_stats()["allocated_pages"]
        assert used(A) == sum(used(tw) for tw in twins), f"{used(A)} pages in use, the twins hold {[used(tw) for tw in twins]}"
    for p, (kb, vb) in shared.items():      # a page with several owners is never written
        assert np.array_equal(A.key_page_pool[p].cpu().numpy(), kb) and np.array_equal(A.value_page_pool[p].cpu().numpy(), vb), f"shared page {p} was written"
    print(f"cap {cap} preallocate {preallocate} fork {fork}: {rounds} rounds, rows per slot {rows_in}, T {A._T_a[0].tolist()}")


# ---------------------------------------------------------------- 4. million_window_commit on rows nobody checked ---------------
# {T, r, start} per slot and dev_n: layer 0 and layer 1 hold different values for the same slots, so a wrong layer stride shows.
UNTRUSTED_ROWS = [[(-5, 1000, 64), (250, 64, 5), (10, -3, -1), (40, 10, 70)],
                  [(10 ** 9, 62, 63), (31, 63, 60), (-7, 9999, 12), (0, 0, -5)]]
UNTRUSTED_N = [1000, 2, -4, 3]
WORD3 = 0x7EADBEEF


@pytest.mark.parametrize("d,M,C", [(64, 16, 128), (128, 64, 256)])
def test_window_commit_on_untrusted_rows(d, M, C, env, oracle):
    """ops.window_commit on lengths rows and row counts outside their ranges: T into [0, 256], r into [0, 64], a start outside
    [0, 64) reads as 0, dev_n into [0, 4] (tests/store_ragged_model.clamp); then verify_model.commit_closed.  Layer 0: slot 0
    (0, 64, 0) with 4 rows flushes tokens 0..31 and becomes (32, 36, 32); slot 1 would flush past the 256-token table and slot 2
    has no rows: both untouched, the row included; slot 3 (40, 10, 0) takes 3 rows into ring slots 10..12.  Layer 1: slot 0's T far
    past the table (untouched), slot 1 flushes tokens 31..62 across a page boundary.  Pools, windows, lengths, dev_n: every byte."""
    from tests import store_ragged_model as SM
    torch, ops = env
    layers, bs, nhk, ps, cap, npc, nb = 2, 4, 2, 32, 64, 8, 4
    rs = np.random.RandomState(d + M)
    f16 = lambda *s: rs.standard_normal(s).astype(np.float16)
    k_new, v_new = f16(layers, bs, nhk, nb, d), f16(layers, bs, nhk, nb, d)
    k_win, v_win = f16(layers, bs, nhk, cap, d), f16(layers, bs, nhk, cap, d)
    k_cents, v_cents = f16(M, C, d // M), f16(M, C, d // M)
    n_real = layers * bs * nhk * npc
    n_pool = n_real + 5                                                     # spare pages no table entry names
    ids = rs.permutation(n_pool)[:n_real].reshape(layers, bs, nhk, npc).astype(np.int32)
    lengths = np.array([[row + (WORD3,) for row in layer] for layer in UNTRUSTED_ROWS], np.int32)
    k_pool, v_pool = np.full((n_pool, ps, M), 0xA5, np.uint8), np.full((n_pool, M, ps), 0xA5, np.uint8)

    want_len, want_kw, want_vw, want_kp, want_vp = lengths.copy(), k_win.copy(), v_win.copy(), k_pool.copy(), v_pool.copy()
    for l in range(layers):
        for b in range(bs):
            T, r, st, a = SM.clamp(UNTRUSTED_ROWS[l][b] + (UNTRUSTED_N[b],), cap_tok=npc * ps, resid_cap=cap, n_bound=nb)
            T2, r2, st2, coded, ring = VM.commit_closed(T, r, st, a, ps, cap)
            if a == 0 or T2 > npc * ps:
                continue                                                    # no part / a flush past the table: nothing moves
            want_len[l, b, :3] = (T2, r2, st2)
            for win, new, cents, side in ((k_win, k_new, k_cents, "k"), (v_win, v_new, v_cents, "v")):
                want_w = want_kw if side == "k" else want_vw
                for slot, e in enumerate(ring):
                    if e is not None and e[0] == "n":
                        want_w[l, b, :, slot] = new[l, b, :, e[1]]
                if coded:
                    toks = sorted(coded)
                    src = np.stack([win[l, b, :, (st + coded[t][1]) % cap] if coded[t][0] == "w" else new[l, b, :, coded[t][1]] for t in toks], axis=1)
                    codes = oracle.pq_encode(src[None], cents)[0]           # (nh_k, tokens, M)
                    for j, t in enumerate(toks):
                        for h in range(nhk):
                            if side == "k":
                                want_kp[ids[l, b, h, t // ps], t % ps, :] = codes[h, j]
                            else:
                                want_vp[ids[l, b, h, t // ps], :, t % ps] = codes[h, j]
    # what the table above says, before the kernel is asked
    assert want_len[0, :, :3].tolist() == [[32, 36, 32], [250, 64, 5], [10, -3, -1], [40, 13, 0]]
    assert want_len[1, :, :3].tolist() == [[10 ** 9, 62, 63], [63, 33, 28], [-7, 9999, 12], [0, 3, 0]]
    assert np.array_equal(want_kw[0, 0, :, :4], k_new[0, 0]) and np.array_equal(want_vw[0, 3, :, 10:13], v_new[0, 3, :, :3])

    dev = lambda a: torch.from_numpy(np.ascontiguousarray(a)).cuda()
    kc, vc = dev(k_cents), dev(v_cents)
    t = dict(k_new=dev(k_new), v_new=dev(v_new), k_win=dev(k_win), v_win=dev(v_win), k_pool=dev(k_pool), v_pool=dev(v_pool),
             ids=dev(ids), lengths=dev(lengths), dev_n=dev(np.asarray(UNTRUSTED_N, np.int32)))
    ops.window_commit(t["k_new"], t["v_new"], t["k_win"], t["v_win"], ops.prepare_cents(kc, cache=False), ops.prepare_cents(vc, cache=False),
                      t["k_pool"], t["v_pool"], t["ids"], t["lengths"], t["dev_n"], M=M, C=C, n_bound=nb)
    torch.cuda.synchronize()
    got = {k: v.cpu().numpy() for k, v in t.items()}
    assert got["dev_n"].tolist() == UNTRUSTED_N, "dev_n is read, never written"
    assert (got["lengths"][:, :, 3] == WORD3).all(), "word 3 of a lengths row was written"
    assert np.array_equal(got["lengths"], want_len), f"lengths {got['lengths'][:, :, :3].tolist()}, expected {want_len[:, :, :3].tolist()}"
    for name, want in (("k_win", want_kw), ("v_win", want_vw)):
        assert np.array_equal(got[name].view(np.uint16), want.view(np.uint16)), f"{name}: window rows differ at (layer, slot, head, row) {np.unique(np.argwhere(got[name] != want)[:, :4], axis=0)[:8].tolist()}"
    for name, want in (("k_pool", want_kp), ("v_pool", want_vp)):
        assert np.array_equal(got[name], want), f"{name}: pages {np.unique(np.argwhere(got[name] != want)[:, 0])[:8].tolist()} differ"
    assert np.array_equal(got["k_new"], k_new) and np.array_equal(got["v_new"], v_new) and np.array_equal(got["ids"], ids)


# ---------------------------------------------------------------- 5. refusals ---------------------------------------------------
def test_commit_refusals_move_nothing(env):
    torch, ops = env
    rs = np.random.RandomState(11)
    cache = _cache(torch, bs=2, nh=NH, nhk=NHK, d=D, M=M_, ps=32, cap=32, layers=LAYERS, max_tokens=64)
    for l in range(LAYERS):
        cache.prefill(*_rows(torch, rs, 2, NH, NHK, 64, D), l)      # the page table is full
    for _ in range(30):
        for l in range(LAYERS):
            cache.decoding_with_pages(*_rows(torch, rs, 2, NH, NHK, 1, D), l, use_dev_lengths=True)
    qkv = [_rows(torch, rs, 2, NH, NHK, N, D) for _ in range(LAYERS)]
    torch.cuda.synchronize()
    before = CL.snapshot(cache)

    def refused(match, n_accept=(1, 1)):
        with pytest.raises(RuntimeError, match=match):
            cache.commit(list(n_accept))
        torch.cuda.synchronize()
        assert _same(before, CL.snapshot(cache)), f"a refused commit ({match}) moved something"

    refused("verify")                                   # no verify at all
    cache.verify(*qkv[0], 0)
    refused("verify")                                   # one layer of two
    cache.verify(*qkv[1], 1, n_draft=[4, 2])            # another n_draft: a new verification, of one layer
    refused("verify")
    for l in range(LAYERS):
        cache.verify(*qkv[l], l, n_draft=[4, 2])
    refused("n_accept", (1, 3))                         # n_accept[b] > n_draft[b]
    refused("n_accept", (1,))
    refused("max_tokens", (3, 2))                       # r = 30, a = 3: a flush past the page table
    with pytest.raises(RuntimeError, match="verify"):
        cache.verify(*_rows(torch, rs, 2, NH, NHK, 17, D), 0)      # more than 16 rows
    cache.commit([2, 2])                                # fills the window: no flush, legal
    torch.cuda.synchronize()
    assert cache._r_a.tolist() == [[32, 32]] * LAYERS and cache._T_a.tolist() == [[64, 64]] * LAYERS
    assert np.array_equal(CL.snapshot(cache)["lengths"][:, :, :3], np.tile(np.array([64, 32, 0]), (LAYERS, 2, 1)))
    with pytest.raises(RuntimeError, match="verify"):
        cache.commit([0, 0])                            # the verification was consumed


def test_commit_mid_step_is_refused(env):
    torch, ops = env
    rs = np.random.RandomState(12)
    cache = _cache(torch, bs=1, nh=NH, nhk=NHK, d=D, M=M_, ps=32, cap=64, layers=LAYERS, max_tokens=256)
    qkv = [_rows(torch, rs, 1, NH, NHK, N, D) for _ in range(LAYERS)]
    for l in range(LAYERS):
        cache.verify(*qkv[l], l)
    cache.decoding_with_pages(*_rows(torch, rs, 1, NH, NHK, 1, D), 0, use_dev_lengths=True)      # layer 0 of a decode step
    torch.cuda.synchronize()
    before = CL.snapshot(cache)
    with pytest.raises(RuntimeError, match="mid-step"):
        cache.commit([2])
    torch.cuda.synchronize()
    assert _same(before, CL.snapshot(cache)), "a refused commit moved something"
    cache.decoding_with_pages(*_rows(torch, rs, 1, NH, NHK, 1, D), 1, use_dev_lengths=True)
    with pytest.raises(RuntimeError, match="since the cache last moved"):
        cache.commit([2])                               # between steps again, but the cache moved after verify
    for l in range(LAYERS):
        cache.verify(*qkv[l], l)
    cache.commit([4])
    assert cache._r_a[:, 0].tolist() == [5, 5] and cache._seen_a[:, 0].tolist() == [5, 5]
