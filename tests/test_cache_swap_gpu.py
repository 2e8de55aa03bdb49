"""GPU tests of the request swap (million_cache_swap behind ops.cache_swap, PagedPQCache.swap_out / swap_in, formats.save_request):

  1. the C call against the numpy model of blob format 1 (tests/cache_swap_model.py), byte for byte on the blob (with guard
     bytes) and on the pools, tables, windows and lengths of EVERY slot - so what must stay untouched is checked with what must
     change; calls on a range of layers; untrusted table values and ids;
  2. a restored slot decodes the bits of a slot that was never swapped, across flushes, on demand and preallocated;
  3. swapping a sibling out leaves the shared pages with the others; a restored slot owns private pages;
  4. through a file into a new cache; other codebooks are refused.

A slot's decode output is a function of its own codes, window and lengths alone (use_dev_lengths=True: the launch shape does
not depend on any request), so outputs of the same request at the same position compare bitwise whatever the other slots hold.
The oracle bar is the suite's (rel-L2 and mean-abs < 1e-3, tests/test_gpu_parity.py); everything else is bitwise."""
import numpy as np
import pytest

from tests import cache_life_model as LM
from tests import cache_swap_model as SM
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
LAYERS, BS, NHK, D, CAP_PAGES, GUARD = 2, 6, 2, 128, 5, 256
NAN16 = np.int16(0x7E00)
NAMES = ("page_ids", "k_pool", "v_pool", "k_resid", "v_resid", "lengths")


def _requests(ps, cap):
    """One entry per slot: every T, r and start the format has an edge at (r = cap with start > 0 wraps)."""
    return np.asarray([[0, 0, cap, cap - 1], [1, 1, 1, 5], [2, ps - 1, 0, 0], [3, ps, cap, 5], [4, ps + 17, 1, cap - 1],
                       [5, 3 * ps + ps - 1, cap, 0]], np.int32)


def _host_tables(seed, table, *, ps, M, cap, extra=9):
    """Scattered, non-monotone ids; random pools with 0xFF in every tail page past T; NaN in the ring rows outside each slot's
    live window; lengths rows of garbage (the table is authoritative)."""
    rs = np.random.RandomState(seed)
    n_tab = LAYERS * BS * NHK * CAP_PAGES
    n_pool = n_tab + extra
    ids = rs.permutation(n_pool)[:n_tab].reshape(LAYERS, BS, NHK, CAP_PAGES).astype(np.int32)
    kp = rs.randint(0, 256, (n_pool, ps, M)).astype(np.uint8)
    vp = rs.randint(0, 256, (n_pool, M, ps)).astype(np.uint8)
    kr = np.full((LAYERS, BS, NHK, cap, D), NAN16, np.int16)
    vr = np.full((LAYERS, BS, NHK, cap, D), NAN16, np.int16)
    for slot, T, r, st in table.tolist():
        if not 0 <= slot < BS:
            continue
        T, r, st = min(max(T, 0), CAP_PAGES * ps), min(max(r, 0), cap), st if 0 <= st < cap else 0
        if T % ps:
            tail = ids[:, slot, :, T // ps].flatten()
            kp[tail, T % ps:] = 0xFF
            vp[tail, :, T % ps:] = 0xFF
        span = (st + np.arange(r)) % cap
        kr[:, slot][:, :, span] = rs.standard_normal((LAYERS, NHK, r, D)).astype(np.float16).view(np.int16)
        vr[:, slot][:, :, span] = rs.standard_normal((LAYERS, NHK, r, D)).astype(np.float16).view(np.int16)
    ln = rs.randint(1, 200, (LAYERS, BS, 4)).astype(np.int32)
    return [ids, kp, vp, kr, vr, ln]


def _layout(table, *, ps, M, cap, bound=CAP_PAGES, layers=LAYERS):
    """Offsets of the entries' blobs one behind the other, sized by the clamped values; the total."""
    sizes = []
    for e in table:
        _, T, r, _ = SM.clamp_entry(e, page_size=ps, n_pages_bound=bound, resid_cap=cap)
        sizes.append(layers * NHK * SM.row_bytes(T, r, ps, M, D))
    offs = np.concatenate([[0], np.cumsum(sizes)]).astype(np.int64)
    return offs[:-1].copy(), int(offs[-1])


def _differs(what, name, want, got):
    if not np.array_equal(want, got):
        bad = np.argwhere(want != got)
        raise AssertionError(f"{what}: {name} differs from the model at {len(bad)} places, first {bad[0].tolist()}: "
                             f"model {want[tuple(bad[0])]}, device {got[tuple(bad[0])]}")


def _run_both(torch, ops, direction, host, table, offs, blob, *, what, **kw):
    """The call and the model on copies of the same arrays; `blob` (numpy, guards included) is the blob's state before the
    call.  Every array is compared; returns the model's (arrays, blob with guards)."""
    want, want_blob = [a.copy() for a in host], blob.copy()
    dev = [torch.from_numpy(a.copy()).cuda() for a in host]
    dev[3], dev[4] = dev[3].view(torch.float16), dev[4].view(torch.float16)
    dev_blob = torch.from_numpy(blob.copy()).cuda()
    inner = slice(GUARD, blob.size - GUARD)
    if direction == SM.PACK:
        SM.pack(*want[:5], table, offs, want_blob[inner], **kw)
    else:
        SM.unpack(*want, table, offs, want_blob[inner], **kw)
    ops.cache_swap(direction, *dev, torch.from_numpy(table).cuda(), torch.from_numpy(offs).cuda(), dev_blob[inner], **kw)
    torch.cuda.synchronize()
    dev[3], dev[4] = dev[3].view(torch.int16), dev[4].view(torch.int16)
    got_blob = dev_blob.cpu().numpy()
    assert (got_blob[:GUARD] == 0x3C).all() and (got_blob[-GUARD:] == 0x3C).all(), f"{what}: guard bytes around the blob were written"
    _differs(what, "blob", want_blob, got_blob)
    for name, w, g in zip(NAMES, want, dev):
        _differs(what, name, w, g.cpu().numpy())
    return want, want_blob


def _guarded(n, fill=0xA5):
    blob = np.full(n + 2 * GUARD, fill, np.uint8)
    blob[:GUARD] = blob[n + GUARD:] = 0x3C
    return blob


@pytest.mark.parametrize("ps,M", [(32, 64), (32, 32), (64, 64), (64, 32), (128, 64), (128, 32), (64, 16)])
def test_swap_call_equals_the_model_byte_for_byte(env, ps, M):
    torch, ops = env
    cap = max(ps, 64)
    table = _requests(ps, cap)
    src = _host_tables(100 + ps + M, table, ps=ps, M=M, cap=cap)
    offs, total = _layout(table, ps=ps, M=M, cap=cap)
    what = f"page={ps} M={M}"
    # PACK: the blob is the model's, the guards are intact, every cache array is bit-identical
    after, blob = _run_both(torch, ops, SM.PACK, src, table, offs, _guarded(total), what=what + " pack")
    assert all(np.array_equal(a, b) for a, b in zip(after, src))
    for (slot, T, r, st), off in zip(table.tolist(), offs.tolist()):      # the model itself: nothing past T reached the blob
        n_live, rb = -(-T // ps), SM.row_bytes(T, r, ps, M, D)
        if T % ps:
            row = blob[GUARD + off:GUARD + off + rb]
            pb = ps * M
            assert not row[(n_live - 1) * pb + (T % ps) * M:n_live * pb].any()
            assert not row[(2 * n_live - 1) * pb:2 * n_live * pb].reshape(M, ps)[:, T % ps:].any()
    # UNPACK into fresh ids: other tables, other slots (entry i to slot 5 - i), windows of NaN, pools of other bytes
    t2 = table.copy()
    t2[:, 0] = 5 - t2[:, 0]
    dst = _host_tables(200 + ps + M, np.zeros((0, 4), np.int32), ps=ps, M=M, cap=cap)
    after, _ = _run_both(torch, ops, SM.UNPACK, dst, t2, offs, blob, what=what + " unpack")
    assert np.array_equal(after[0], dst[0])
    named = np.zeros(dst[1].shape[0], bool)
    for (s_src, T, r, st), s_dst in zip(table.tolist(), t2[:, 0].tolist()):
        for a, b in zip(SM.live_data(*src[:5], s_src, T, r, st), SM.live_data(*after[:5], s_dst, T, r, st)):
            assert np.array_equal(a, b), f"{what}: slot {s_src} -> {s_dst}"
        named[dst[0][:, s_dst, :, :-(-T // ps)].flatten()] = True
        dead = np.setdiff1d(np.arange(cap), (st + np.arange(r)) % cap)
        assert (after[3][:, s_dst][:, :, dead] == NAN16).all() and (after[4][:, s_dst][:, :, dead] == NAN16).all()
        assert after[5][:, s_dst].tolist() == [[T, r, st, 0]] * LAYERS
    assert np.array_equal(after[1][~named], dst[1][~named]) and np.array_equal(after[2][~named], dst[2][~named])


def test_swap_call_on_a_range_of_layers(env):
    """layer0 = 1, n = 1: the call touches the byte range of its layer in every entry's blob, and the rows of its layer."""
    torch, ops = env
    ps, M, cap = 64, 64, 128
    table = _requests(ps, cap)
    src = _host_tables(31, table, ps=ps, M=M, cap=cap)
    offs, total = _layout(table, ps=ps, M=M, cap=cap)
    _, whole = _run_both(torch, ops, SM.PACK, src, table, offs, _guarded(total), what="all layers")
    per_layer = np.asarray([NHK * SM.row_bytes(T, r, ps, M, D) for _, T, r, _ in table.tolist()], np.int64)
    _, part = _run_both(torch, ops, SM.PACK, src, table, offs + per_layer, _guarded(total), what="pack of layer 1", layer0=1, n_layers=1)
    mine = np.zeros(total, bool)
    for off, n in zip(offs.tolist(), per_layer.tolist()):
        mine[off + n:off + 2 * n] = True
    inner = slice(GUARD, -GUARD)
    assert np.array_equal(part[inner][mine], whole[inner][mine]) and (part[inner][~mine] == 0xA5).all()
    dst = _host_tables(32, np.zeros((0, 4), np.int32), ps=ps, M=M, cap=cap)
    after, _ = _run_both(torch, ops, SM.UNPACK, dst, table, offs + per_layer, whole, what="unpack of layer 1", layer0=1, n_layers=1)
    assert all(np.array_equal(a[0], b[0]) for a, b in zip(after[3:], dst[3:]))         # layer 0: windows and lengths as they were
    pages0 = dst[0][0].flatten()
    assert np.array_equal(after[1][pages0], dst[1][pages0]) and np.array_equal(after[2][pages0], dst[2][pages0])
    assert after[5][1, :, :].tolist() == [[T, r, st, 0] for _, T, r, st in table.tolist()]
    for slot, T, r, st in table.tolist():
        for a, b in zip(SM.live_data(*src[:5], slot, T, r, st), SM.live_data(*after[:5], slot, T, r, st)):
            assert np.array_equal(a[1], b[1])


def test_swap_call_on_untrusted_values(env):
    """Slots outside the batch, T past the bound, r past the window, a start outside the ring, ids of -1 and n_pool, offsets
    that are misaligned or leave the blob: the model's clamped result, byte for byte, no write anywhere else, and the call
    ends clean."""
    torch, ops = env
    ps, M, cap, bound = 64, 32, 64, 3
    table = np.asarray([[BS, 70, 3, 1], [1, 2 ** 31 - 1, 2 ** 31 - 1, cap], [-1, 70, 3, 1], [2, -7, -1, -1], [3, 100, 200, -5],
                        [4, 3 * ps + 1, 5, 2 ** 30], [0, 70, 3, 1], [5, 70, 3, 1], [1, 10, 1, 0]], np.int32)
    src = _host_tables(41, table, ps=ps, M=M, cap=cap)
    n_pool = src[1].shape[0]
    src[0][0, 1, 0, 1], src[0][1, 1, 1, 2], src[0][1, 3, 0, 0], src[0][0, 4, 1, 2] = -1, n_pool, 1 << 30, -(1 << 31)
    offs, total = _layout(table, ps=ps, M=M, cap=cap, bound=bound)
    offs[6] += 8                       # misaligned: slot 0 takes no part
    offs[7] = total - 16               # its rows leave the blob: slot 5 takes no part
    kw = dict(n_pages_bound=bound)
    took = SM.entries(table, offs, bs=BS, nhk=NHK, page_size=ps, M=M, d=D, resid_cap=cap, n_pages_bound=bound, n_layers=LAYERS,
                      blob_bytes=total)
    assert [t[:4] for t in took] == [(1, bound * ps, cap, 0), (2, 0, 0, 0), (3, 100, cap, 0), (4, bound * ps, 5, 0), (1, 10, 1, 0)]
    _, blob = _run_both(torch, ops, SM.PACK, src, table, offs, _guarded(total), what="untrusted pack", **kw)
    o = GUARD + int(offs[1])
    assert not blob[o + ps * M:o + 2 * ps * M].any() and blob[o:o + ps * M].any()      # layer 0 head 0 page 1: id -1 packs as zeros
    dst = _host_tables(42, np.zeros((0, 4), np.int32), ps=ps, M=M, cap=cap)
    dst[0][0, 1, 0, 0], dst[0][1, 4, 1, 1] = n_pool, -1
    # (without the last entry: two entries that name one slot overlap on UNPACK, which the contract leaves open)
    after, _ = _run_both(torch, ops, SM.UNPACK, dst, table[:-1], offs[:-1], blob, what="untrusted unpack", **kw)
    assert after[5][:, 1].tolist() == [[bound * ps, cap, 0, 0]] * LAYERS
    for s in (0, 5):
        assert all(np.array_equal(a[:, s], b[:, s]) for a, b in zip(after[3:], dst[3:]))


# ---------------------------------------------------------------- the cache under test --------------------------------------
GEOMS = {"on-demand": LM.GEOMS["share-64-ahead"], "preallocated": LM.GEOMS["copy-128"]}      # both M = 64: one world
N_STEPS_MAX = 2 * 128 + 64
C = 256


def _n_prompt(geom):
    return 3 * geom["page_size"] + 17      # a few pages plus a partial page


class _World:
    """Histories for three kinds of request (A: the one that is swapped, B, other), their queries, the codebooks."""

    def __init__(self):
        nhk, nh, d, M = LM.BASE["num_key_value_heads"], LM.BASE["nh"], LM.BASE["d"], 64
        n = 3 * 128 + 17 + N_STEPS_MAX
        self.hist = {}
        for who, seed in (("A", 5100), ("B", 5200), ("other", 5300)):      # (layers, 1, nh_k, n, d) K and V histories
            k = [synth.encode_case(seed + l, 1, nhk, n, d, M, C) for l in range(2)]
            v = [synth.encode_case(seed + 10 + l, 1, nhk, n, d, M, C) for l in range(2)]
            self.hist[who] = (np.stack([c["X"] for c in k]), np.stack([c["X"] for c in v]))
        self.ck, self.cv = LM.codebooks(LM.GEOMS["share-64-ahead"])
        rs = np.random.RandomState(5500)
        self.q = {who: rs.standard_normal((N_STEPS_MAX, 2, 1, nh, 1, d)).astype(np.float16) for who in self.hist}
        self.qp = rs.standard_normal((1, nh, 3 * 128 + 17, d)).astype(np.float16)


@pytest.fixture(scope="module")
def world():
    return _World()


def _new_cache(torch, world, geom, ck=None, cv=None):
    from million_amd.pq_cache import PagedPQCache
    cache = PagedPQCache(**LM.cache_kwargs(geom), device="cuda")
    cache.set_cent(torch.from_numpy(world.ck if ck is None else ck).cuda(), torch.from_numpy(world.cv if cv is None else cv).cuda())
    return cache


def _dev(torch, a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def _prefill(torch, cache, world, b, who, n):
    for l in range(2):
        K, V = world.hist[who]
        cache.prefill_request(b, _dev(torch, world.qp[:, :, :n]), _dev(torch, K[l][:, :, :n]), _dev(torch, V[l][:, :, :n]), l)


def _decode(torch, cache, world, feeds, steps):
    """feeds[b] = (history name, rows the request's prompt had, decode steps it has taken): step i feeds slot b decode row
    (taken + i) of its history.  Returns bits[b][taken + i] = (layers, nh, d) int16 of the slot's output at that position."""
    bits = [dict() for _ in feeds]
    for i in range(steps):
        row = []
        for l in range(2):
            q = np.concatenate([world.q[w][t + i, l] for w, _, t in feeds])
            kn = np.concatenate([world.hist[w][0][l][:, :, n + t + i:n + t + i + 1] for w, n, t in feeds])
            vn = np.concatenate([world.hist[w][1][l][:, :, n + t + i:n + t + i + 1] for w, n, t in feeds])
            row.append(cache.decoding_with_pages(_dev(torch, q), _dev(torch, kn), _dev(torch, vn), l, use_dev_lengths=True).clone())
        out = torch.stack(row, dim=1).cpu().numpy()[:, :, :, 0].view(np.int16)      # (bs, layers, nh, d)
        for b, (_, _, t) in enumerate(feeds):
            bits[b][t + i] = out[b]
    return bits


def _same_bits(a, b, positions, what):
    for p in positions:
        assert np.array_equal(a[p], b[p]), f"{what}: the outputs differ from decode position {p} on"


def _oracle_check(oracle, world, geom, who, n_prompt, steps, out_bits, what):
    pol = oracle.PagedPolicy(page_size=geom["page_size"], residual=geom["extended_residual_size"], prefill=n_prompt)
    for _ in range(steps):
        T, r = pol.step()
    cap = geom["extended_residual_size"]
    for l in range(2):
        K, V = world.hist[who][0][l], world.hist[who][1][l]
        kc, vc = oracle.pq_encode(K[:, :, :T], world.ck), oracle.pq_encode(V[:, :, :T], world.cv)
        kres, vres = np.zeros((1, 2, cap, 128), np.float16), np.zeros((1, 2, cap, 128), np.float16)
        kres[:, :, :r], vres[:, :, :r] = K[:, :, T:T + r], V[:, :, T:T + r]
        gold = oracle.decode_attn(world.q[who][steps - 1, l], kc, vc, world.ck, world.cv, kres, vres, r)
        out = out_bits[l].view(np.float16).astype(np.float64).reshape(gold.shape)
        rel = np.linalg.norm(out - gold) / np.linalg.norm(gold)
        mae = np.abs(out - gold).mean()
        print(f"{what}, layer {l}: T={T} r={r} rel-L2 {rel:.3e} mean-abs {mae:.3e}")
        assert np.isfinite(out).all() and rel < REL_TOL and mae < MEAN_ABS_TOL, f"{what}: rel={rel:.3e} mean_abs={mae:.3e}"


def _poison_free_pages(torch, cache):
    free = torch.tensor(sorted(cache.page_manager.free_pages), dtype=torch.long, device="cuda")
    cache.key_page_pool[free] = 0xFF
    cache.value_page_pool[free] = 0xFF


# ---------------------------------------------------------------- 2. bit-exact resumption ----------------------------------
@pytest.mark.parametrize("kind", ["on-demand", "preallocated"])
def test_restored_slot_decodes_the_bits_of_a_slot_never_swapped(env, oracle, world, kind):
    torch, ops = env
    geom = GEOMS[kind]
    ps, cap, n = geom["page_size"], geom["extended_residual_size"], _n_prompt(geom)
    s1, k, s2 = cap + 5, 4, ps + 10                                    # one flush, the other request's steps, another flush
    cache = _new_cache(torch, world, geom)
    _prefill(torch, cache, world, 0, "A", n)
    _prefill(torch, cache, world, 1, "A", n)
    never = _decode(torch, cache, world, [("A", n, 0), ("A", n, 0), ("other", 0, 0), ("other", 0, 0)], s1)[0]
    assert cache._T_a[:, :2].tolist() == [[n + ps] * 2] * 2 and cache._r_a[:, :2].tolist() == [[s1 - ps] * 2] * 2      # a flush was crossed
    snap = cache.swap_out(1)
    assert snap.blob.is_pinned() and snap.meta["T"] == n + ps and snap.meta["r"] == s1 - ps and snap.meta["start"] == ps % cap
    assert snap.blob.numel() == 2 * 2 * SM.row_bytes(n + ps, s1 - ps, ps, 64, 128)
    assert cache._lengths_all[:, 1].cpu().tolist() == [[0, 0, 0, 0]] * 2
    # the slot and (on demand) the pages serve another request in between; the window rows of slot 1 are overwritten
    _prefill(torch, cache, world, 1, "B", 100)
    never.update(_decode(torch, cache, world, [("A", n, s1), ("B", 100, 0), ("other", 0, s1), ("other", 0, s1)], k)[0])
    cache.release(1)
    cache.release(2)
    if not geom["preallocate"]:
        _poison_free_pages(torch, cache)
    cache._kres_all[:, 2] = float("nan")
    cache._vres_all[:, 2] = float("nan")
    cache.swap_in(2, snap)
    assert cache._lengths_all[:, 2].cpu().tolist() == [[n + ps, s1 - ps, ps % cap, 0]] * 2
    got = _decode(torch, cache, world, [("A", n, s1 + k), ("B", 0, 0), ("A", n, s1), ("other", 0, s1 + k)], s2)
    never.update(got[0])
    assert cache._T_a[:, 2].tolist() == [n + 2 * ps] * 2, "the restored slot did not cross its next flush"
    _same_bits(never, got[2], range(s1, s1 + s2), f"{kind}: restored slot 2 against slot 0")
    _oracle_check(oracle, world, geom, "A", n, s1 + k + s2, never[s1 + k + s2 - 1], f"{kind}: slot 0 after {s1 + k + s2} steps")
    _oracle_check(oracle, world, geom, "A", n, s1 + s2, got[2][s1 + s2 - 1], f"{kind}: restored slot after {s1 + s2} steps")


# ---------------------------------------------------------------- 3. shared pages ------------------------------------------
def test_swap_of_a_sibling_leaves_shared_pages_with_the_others(env, world):
    torch, ops = env
    geom = GEOMS["on-demand"]
    ps, cap, n = geom["page_size"], geom["extended_residual_size"], _n_prompt(geom)
    steps = cap + 3
    runs = {}
    for swap in (False, True):
        cache = _new_cache(torch, world, geom)
        pm = cache.page_manager
        _prefill(torch, cache, world, 0, "A", n)
        cache.fork(0, [1, 2])
        assert pm.get_stats()["allocated_pages"] == 2 * 2 * (4 + 1 + 1)
        assert cache.sharing_stats() == {"shared_pages": 12, "extra_references": 24}
        if swap:
            snap = cache.swap_out(1)
            assert pm.get_stats()["allocated_pages"] == 2 * 2 * (4 + 1) and cache.sharing_stats() == {"shared_pages": 12, "extra_references": 12}
            _poison_free_pages(torch, cache)
            cache.swap_in(3, snap)
            assert pm.get_stats()["allocated_pages"] == 2 * 2 * (4 + 1 + 4) and cache.sharing_stats() == {"shared_pages": 12, "extra_references": 12}
            mine = [p for l in range(2) for h in range(2) for p in cache._host_pids[l][3][h]]
            theirs = {p for l in range(2) for b in (0, 2) for h in range(2) for p in cache._host_pids[l][b][h]}
            assert len(set(mine)) == 2 * 2 * 4 and not set(mine) & theirs and all(pm.ref_count(p) == 1 for p in mine)
            assert cache._page_ids_all[:, 3, :, :4].cpu().flatten().tolist() == mine
        who = 3 if swap else 1
        feeds = [("A", n, 0)] + [("B", n, 0) if b in (2, who) else ("other", 0, 0) for b in (1, 2, 3)]
        runs[swap] = _decode(torch, cache, world, feeds, steps)
        assert cache._T_a[:, 2].tolist() == [n + ps] * 2                # a flush with shared pages behind it
        for b in range(4):
            cache.release(b)
        assert pm.get_stats()["allocated_pages"] == 0 and cache.sharing_stats() == {"shared_pages": 0, "extra_references": 0}
    for b in (0, 2):
        _same_bits(runs[False][b], runs[True][b], range(steps), f"slot {b} with and without its sibling swapped out")
    _same_bits(runs[True][2], runs[True][3], range(steps), "the restored sibling against the one that stayed")


# ---------------------------------------------------------------- 4. through a file into a new cache ------------------------
@pytest.mark.parametrize("kind", ["on-demand", "preallocated"])
def test_through_a_file_into_a_new_cache(env, world, tmp_path, kind):
    torch, ops = env
    from million_amd import formats
    geom = GEOMS[kind]
    n = _n_prompt(geom)
    a = _new_cache(torch, world, geom)
    _prefill(torch, a, world, 0, "A", n)
    idle = [("other", 0, 0)] * 3
    _decode(torch, a, world, [("A", n, 0)] + idle, 10)
    snap = a.snapshot_request(0)
    assert a._lengths_all[:, 0].cpu().tolist() == [[n, 10, 0, 0]] * 2      # the slot goes on
    back = formats.load_request(formats.save_request(tmp_path / "request.pt", snap))
    assert torch.equal(back.blob, snap.blob) and back.meta == snap.meta and not back.blob.is_pinned()
    b = _new_cache(torch, world, geom)
    b.swap_in(1, back)
    assert b._lengths_all.cpu().tolist() == [[[0] * 4, [n, 10, 0, 0], [0] * 4, [0] * 4]] * 2
    want = _decode(torch, a, world, [("A", n, 10)] + idle, 5)[0]
    got = _decode(torch, b, world, [("other", 0, 0), ("A", n, 10)] + idle[:2], 5)[1]
    _same_bits(want, got, range(10, 15), f"{kind}: a new cache restored from the file")
    c = _new_cache(torch, world, geom, ck=world.cv, cv=world.ck)       # the same geometry, other codebooks
    before = [t.clone() for t in (c.key_page_pool, c.value_page_pool, c._page_ids_all, c._lengths_all, c._kres_all, c._vres_all)]
    with pytest.raises(RuntimeError, match="codebooks"):
        c.swap_in(1, back)
    torch.cuda.synchronize()
    assert all(torch.equal(x, y) for x, y in zip(before, (c.key_page_pool, c.value_page_pool, c._page_ids_all, c._lengths_all, c._kres_all, c._vres_all)))
    assert c.page_manager.get_stats()["allocated_pages"] == b.page_manager.get_stats()["allocated_pages"] - (0 if geom["preallocate"] else 2 * 2 * 4)
    c.swap_in(1, back, check_codebooks=False)
    assert c._lengths_all[:, 1].cpu().tolist() == [[n, 10, 0, 0]] * 2 and c._T_a[:, 1].tolist() == [n, n]
    again = c.snapshot_request(1)
    assert torch.equal(again.blob, snap.blob)                          # the format is canonical: the same request, the same bytes


# ---------------------------------------------------------------- the grid-stride loop --------------------------------------
N_FILLER = 53000      # entries that take no part: 2 layers x 2 kv heads x 5 tasks per row x 53000 > the kernel's grid cap of 2^20


def test_swap_call_with_more_tasks_than_workgroups(env):
    """The task count follows the bounds, so a long table of entries that take no part makes the list longer than the grid: the
    six requests, spread over the table, are served by workgroups on a later turn of their loop."""
    torch, ops = env
    ps, M, cap = 64, 32, 64
    real = _requests(ps, cap)
    table = np.tile(np.asarray([[-1, 70, 3, 1], [BS, 1, 1, 0]], np.int32), (N_FILLER // 2, 1))
    where = np.linspace(0, N_FILLER - 1, len(real)).astype(int)
    table[where] = real
    offs = np.zeros(N_FILLER, np.int64)
    offs[where], total = _layout(real, ps=ps, M=M, cap=cap)
    src = _host_tables(51, real, ps=ps, M=M, cap=cap)
    _, blob = _run_both(torch, ops, SM.PACK, src, table, offs, _guarded(total), what="long table, pack")
    _, want = _run_both(torch, ops, SM.PACK, src, real, offs[where], _guarded(total), what="the six requests alone")
    assert np.array_equal(blob, want)
    dst = _host_tables(52, np.zeros((0, 4), np.int32), ps=ps, M=M, cap=cap)
    after, _ = _run_both(torch, ops, SM.UNPACK, dst, table, offs, blob, what="long table, unpack")
    for slot, T, r, st in real.tolist():
        for a, b in zip(SM.live_data(*src[:5], slot, T, r, st), SM.live_data(*after[:5], slot, T, r, st)):
            assert np.array_equal(a, b)
