"""GPU tests of the request fork over wide code pages (million_cache_fork_wide behind ops.cache_fork_wide, million_amd.paged_turns.fork):

  1. the C call against tests/cache_fork_model.py's rules over pages of either kind (tests/cache_swap_wide_model.py: fork), byte
     for byte on the pools, tables, windows and lengths of EVERY slot: SHARE with a partial tail page, SHARE at a multiple of the
     page size, COPY; prefixes; a duplicate destination, dst == src and slots outside the batch; one captured call that follows
     the source's device row; untrusted rows, slots and ids;
  2. through paged_turns, packed and uint16, on demand and preallocated: a forked slot decodes the bits of a twin slot given the
     same prompt by prefill_request, across a flush; the source's pages and outputs do not change under the destinations'
     flushes; releasing the source leaves the shared pages with the others; a fork of a prefix."""
import numpy as np
import pytest

from tests import cache_fork_model as FM
from tests import cache_swap_wide_model as WM
from tests import fork_swap_wide_common as X

pytestmark = pytest.mark.gpu

LAYERS, BS, NHK, CAP, NPC = X.LAYERS, X.BS, X.NHK, X.CAP, X.NPC
PS, N_PROMPT, FIRST, STEPS = X.PS, X.N_PROMPT, X.FIRST, X.STEPS
World, new_cache, prefill, decode, same_bits = X.World, X.new_cache, X.prefill, X.decode, X.same_bits
INT_MAX = 2 ** 31 - 1
CASES = [f + (32,) for f in X.FORMATS] + [X.FORMATS[3] + (64,), X.FORMATS[3] + (128,)]


@pytest.fixture(scope="module")
def env():
    import torch
    assert torch.cuda.is_available(), "GPU tests need an MI355X"
    from million_amd import ops, _lib
    _lib.load()
    yield torch, ops
    assert ops.tail_faults() == 0


_SCENES = {}


def _scene(oracle, d, M, nbits, ps, packed):
    """Cache arrays with extra free pages for the tail ids of every entry of DST; the pages of slots 1 and 2 and the free ones hold 0xA5."""
    key = (d, M, nbits, ps)
    if key not in _SCENES:
        _SCENES[key] = X.tables(nbits + ps + 1, d, M, 2 ** nbits, ps, oracle, extra=len(DST) * LAYERS * NHK + 5)
    host = [a.copy() for a in _SCENES[key]["packed" if packed else "u16"]]
    mine = host[0][:, 0].flatten()
    rest = np.setdiff1d(np.arange(host[1].shape[0]), mine)
    for a in host[1:3]:
        a[rest] = 0xA5 * (0x101 if a.dtype == np.uint16 else 1)
    host[3][:, 1:] = host[4][:, 1:] = 0x7E00
    return host


def _free_ids(host, n):
    used = set(host[0].flatten().tolist())
    return np.asarray([i for i in range(host[1].shape[0]) if i not in used][:n], np.int32)


def _launch(torch, ops, dev, dst, tail, *, ps, M, C, packed, src, mode, bound, prefix):
    ops.cache_fork_wide(*dev, dst, tail, src=src, share=mode == FM.SHARE, n_pages_bound=bound, prefix_tokens=prefix, C=C, packed=packed,
                        page_size=ps, M=M)


def _run_both(torch, ops, host, dst, tail, *, ps, M, C, src=0, mode, bound=NPC, prefix=-1, what=""):
    want = [a.copy() for a in host]
    packed = WM.is_packed(host[1])
    dev = [X.to_dev(torch, a) for a in host]
    dev[3], dev[4] = dev[3].view(torch.float16), dev[4].view(torch.float16)
    copied = WM.fork(*want, dst, tail, page_size=ps, src=src, mode=mode, n_pages_bound=bound, prefix_tokens=prefix)
    _launch(torch, ops, dev, torch.from_numpy(np.asarray(dst, np.int32)).cuda(), None if tail is None else torch.from_numpy(tail).cuda(),
            ps=ps, M=M, C=C, packed=packed, src=src, mode=mode, bound=bound, prefix=prefix)
    torch.cuda.synchronize()
    dev[3], dev[4] = dev[3].view(torch.int16), dev[4].view(torch.int16)
    for name, w, g in zip(X.NAMES, want, dev):
        g = X.to_np(torch, g)
        if not np.array_equal(w, g):
            bad = np.argwhere(w != g)
            raise AssertionError(f"{what}: {name} differs from the model at {len(bad)} places, first {bad[0].tolist()}")
    return want, copied


DST = np.asarray([1, 0, 1, 2, BS, -1], np.int32)      # a duplicate, the source itself, slots outside the batch: they take no part


@pytest.mark.parametrize("packed", [False, True], ids=["uint16", "packed"])
@pytest.mark.parametrize("d,M,nbits,ps", CASES)
def test_fork_wide_call_equals_the_model_byte_for_byte(env, oracle, d, M, nbits, ps, packed):
    torch, ops = env
    C = 2 ** nbits
    for mode, T, prefix, n_copied in ((FM.SHARE, 2 * ps + 5, -1, 1), (FM.SHARE, 2 * ps, -1, 0), (FM.COPY, 2 * ps + 5, -1, 3),
                                      (FM.SHARE, 2 * ps + 5, 0, 0), (FM.SHARE, 2 * ps + 5, 33, 1), (FM.COPY, 2 * ps + 5, 33, -(-33 // ps))):
        host = _scene(oracle, d, M, nbits, ps, packed)
        host[5][:, 0] = (T, 40, 50, 9)
        tail = _free_ids(host, len(DST) * LAYERS * NHK).reshape(len(DST), LAYERS, NHK) if mode == FM.SHARE else None
        what = f"d={d} M={M} C={C} page={ps} mode={mode} T={T} prefix={prefix}"
        after, copied = _run_both(torch, ops, host, DST, tail, ps=ps, M=M, C=C, mode=mode, prefix=prefix, what=what)
        assert len(copied) == 2 * LAYERS * NHK * n_copied, what      # destinations 1 and 2
        Tw = T if prefix < 0 else min(T, prefix)
        assert after[5][:, 1].tolist() == after[5][:, 2].tolist() == [[Tw, 40, 50, 0] if prefix < 0 else [Tw, 0, 0, 0]] * LAYERS
        assert np.array_equal(after[5][:, 0], host[5][:, 0])
        for b in (1, 2):
            want = WM.live_codes(*host[:3], 0, Tw, page_size=ps, M=M, C=C)
            got = WM.live_codes(*after[:3], b, Tw, page_size=ps, M=M, C=C)
            assert all(np.array_equal(x, y) for x, y in zip(want, got)), what


@pytest.mark.parametrize("packed", [False, True], ids=["uint16", "packed"])
def test_a_captured_fork_follows_the_source_s_row(env, oracle, packed):
    torch, ops = env
    d, M, nbits, ps = X.FORMATS[3] + (32,)
    C = 2 ** nbits
    host = _scene(oracle, d, M, nbits, ps, packed)
    host[5][:, 0] = (ps + 3, 7, 60, 0)
    dst = np.asarray([2, 1], np.int32)
    tail = _free_ids(host, 2 * LAYERS * NHK).reshape(2, LAYERS, NHK)
    dev = [X.to_dev(torch, a) for a in host]
    dev[3], dev[4] = dev[3].view(torch.float16), dev[4].view(torch.float16)
    d_dst, d_tail = torch.from_numpy(dst).cuda(), torch.from_numpy(tail).cuda()
    kw = dict(ps=ps, M=M, C=C, packed=packed, src=0, mode=FM.SHARE, bound=NPC, prefix=-1)
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        _launch(torch, ops, dev, d_dst, d_tail, **kw)      # warm up outside the capture
    torch.cuda.current_stream().wait_stream(side)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        _launch(torch, ops, dev, d_dst, d_tail, **kw)
    for row in ((ps + 3, 7, 60, 0), (3 * ps + 1, CAP, 0, 5), (2 * ps, 0, 3, 0)):
        want = [a.copy() for a in host]
        want[5][:, 0] = row
        for i, a in enumerate(want):      # the device arrays as the host has them, the source's row changed
            dev[i].view(torch.uint8).copy_(torch.from_numpy(a.view(np.uint8)).cuda())
        WM.fork(*want, dst, tail, page_size=ps, src=0, mode=FM.SHARE, n_pages_bound=NPC)
        graph.replay()
        torch.cuda.synchronize()
        for i, (name, w) in enumerate(zip(X.NAMES, want)):
            g = X.to_np(torch, dev[i].view(torch.int16) if i in (3, 4) else dev[i])
            assert np.array_equal(w, g), (row, name)


@pytest.mark.parametrize("mode", [FM.SHARE, FM.COPY], ids=["share", "copy"])
@pytest.mark.parametrize("packed", [False, True], ids=["uint16", "packed"])
def test_fork_wide_call_on_untrusted_values(env, oracle, packed, mode):
    """Source rows, destination slots, table entries and tail ids that are negative, INT_MAX or past the pool: clamped or dropped
    by contract (the kernel: load_len_row's clamps, forkw_dst's slot test, the unsigned id tests in front of s_src / s_dst).  The
    result is the model's; every other byte is unchanged."""
    torch, ops = env
    d, M, nbits, ps = X.FORMATS[3] + (32,)
    C = 2 ** nbits
    n_pool = _scene(oracle, d, M, nbits, ps, packed)[1].shape[0]
    dst = np.asarray([INT_MAX, 2, -INT_MAX - 1, 1, BS], np.int32)
    for row in ((INT_MAX, INT_MAX, INT_MAX, 1), (-1, -1, -1, 0), (2 * ps + 1, CAP + 1, CAP, 0)):
        host = _scene(oracle, d, M, nbits, ps, packed)
        host[5][0, 0] = row
        host[5][1, 0] = (ps + 1, 3, 2, 0)
        host[0][0, 0, 0, 0] = -1              # source ids outside the pool: the copy is dropped
        host[0][1, 0, 1, 1] = n_pool
        host[0][0, 2, 1, 0] = INT_MAX         # destination entries (COPY)
        host[0][1, 1, 0, 0] = -INT_MAX - 1
        tail = None
        if mode == FM.SHARE:
            tail = _free_ids(host, len(dst) * LAYERS * NHK).reshape(len(dst), LAYERS, NHK)
            tail[1, 0, 0], tail[1, 1, 1], tail[3, 0, 1] = -1, INT_MAX, n_pool
        _run_both(torch, ops, host, dst, tail, ps=ps, M=M, C=C, mode=mode, what=f"untrusted {row} mode={mode}")


# ---------------------------------------------------------------- 2. the cache, through paged_turns ------------------------
def _pools(torch, cache):
    return [X.to_np(torch, cache.key_page_pool), X.to_np(torch, cache.value_page_pool)]


def _pages_of(cache, b, n):
    return np.asarray([cache._host_pids[l][b][h][:n] for l in range(LAYERS) for h in range(NHK)]).flatten()


@pytest.mark.parametrize("preallocate", [False, True], ids=["on-demand", "preallocated"])
@pytest.mark.parametrize("packed", [False, True], ids=["uint16", "packed"])
def test_a_forked_slot_decodes_the_bits_of_a_prefilled_twin(env, packed, preallocate):
    torch, ops = env
    from million_amd import paged_turns
    w = World(128, 64, 10)
    twin, cache, solo = (new_cache(torch, w, packed, preallocate) for _ in range(3))      # solo: the source's life without a fork
    for b in range(BS):
        prefill(torch, twin, w, b)
    decode(torch, twin, w, [N_PROMPT] * BS, FIRST)
    for c in (cache, solo):
        prefill(torch, c, w, 0)
        decode(torch, c, w, [N_PROMPT, None, None], FIRST)
    with pytest.raises(NotImplementedError, match="nbits"):
        cache.fork(0, [1, 2])
    paged_turns.fork(cache, 0, [1, 2])      # 69 coded tokens - two shared pages and a tail page - and a window of FIRST rows
    n_full = N_PROMPT // PS
    if not preallocate:
        assert cache.sharing_stats() == {"shared_pages": LAYERS * NHK * n_full, "extra_references": 2 * LAYERS * NHK * n_full}
    src_pages = _pages_of(cache, 0, n_full)
    before = [p[src_pages].copy() for p in _pools(torch, cache)]
    # the source goes on with its own rows, slot 1 with the same ones, slot 2 with others; every window fills and is flushed
    p0 = N_PROMPT + FIRST
    pos = [p0, p0, p0 + 7]
    want, got = decode(torch, twin, w, pos, STEPS), decode(torch, cache, w, pos, STEPS)
    alone = decode(torch, solo, w, [p0, None, None], STEPS)
    assert [int(cache._T_a[0, b]) for b in range(BS)] == [N_PROMPT + PS] * BS, "the steps crossed a flush in every slot"
    for b in range(BS):
        assert same_bits(want[b], got[b]), f"slot {b} against the prefilled twin"
    assert same_bits(got[0], alone[0]), "the source's outputs are those of a cache that never forked"
    assert same_bits(got[0], got[1]) and not same_bits(got[1], got[2])
    assert all(np.array_equal(a, q[src_pages]) for a, q in zip(before, _pools(torch, cache))), "the shared pages did not change"
    # ... and a fresh fork of the source's first tokens decodes the bits of a slot prefilled with them
    cache.release(1)
    twin.release(1)
    paged_turns.fork(cache, 0, 1, n_tokens=N_PROMPT)
    prefill(torch, twin, w, 1)
    cache.release(0)      # the shared pages stay with the others
    assert all(np.array_equal(a, q[src_pages]) for a, q in zip(before, _pools(torch, cache)))
    want = decode(torch, twin, w, [None, N_PROMPT, None], 5)
    got = decode(torch, cache, w, [None, N_PROMPT, None], 5)
    assert same_bits(want[1], got[1])
    if not preallocate:
        cache.release(1)
        cache.release(2)
        assert cache.page_manager.get_stats()["allocated_pages"] == 0


@pytest.mark.parametrize("preallocate", [False, True], ids=["on-demand", "preallocated"])
@pytest.mark.parametrize("packed", [False, True], ids=["uint16", "packed"])
def test_fork_of_a_prefix_and_on_with_the_other_turns(env, packed, preallocate):
    torch, ops = env
    from million_amd import paged_turns
    w = World(128, 32, 12)
    twin, cache = new_cache(torch, w, packed, preallocate), new_cache(torch, w, packed, preallocate)
    solo = new_cache(torch, w, packed, preallocate)      # the source's life without any fork
    for c in (cache, solo):
        prefill(torch, c, w, 0)
    assert same_bits(decode(torch, cache, w, [N_PROMPT, None, None], 3)[0], decode(torch, solo, w, [N_PROMPT, None, None], 3)[0])
    paged_turns.fork(cache, 0, 2, n_tokens=33)      # a partial tail page: copied into a private page; no window
    prefill(torch, twin, w, 2, n=33)
    assert cache._lengths_all[:, 2].tolist() == [[33, 0, 0, 0]] * LAYERS and int(cache._seen_a[0, 2]) == 33
    # a later turn of the fork through paged_turns.extend_request, then decode steps: the twin's bits
    outs = []
    for c in (cache, twin):
        per = []
        for l in range(LAYERS):
            q, k, v = (X.to_dev(torch, A[l][:, :, 33:40]) for A in (w.Q, w.K, w.V))
            per.append(paged_turns.extend_request(c, 2, q, k, v, l).view(torch.int16).cpu().numpy())
        outs.append(per)
    assert same_bits(outs[0], outs[1])
    want = decode(torch, twin, w, [None, None, 40], 5)
    got = decode(torch, cache, w, [N_PROMPT + 3, None, 40], 5)
    assert same_bits(want[2], got[2])
    # the source went on with its own rows beside the fork, unchanged by the fork's stores
    assert same_bits(got[0], decode(torch, solo, w, [N_PROMPT + 3, None, None], 5)[0])
