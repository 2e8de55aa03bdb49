"""GPU tests of the request swap over wide code pages (million_cache_swap_wide behind ops.cache_swap_wide; blob format 2):

  1. the C call against the numpy model (tests/cache_swap_wide_model.py), byte for byte on the blob (with guard bytes, staging
     poisoned with 0xA5) and on the pools, tables, windows and lengths of EVERY slot - what must stay untouched is checked with
     what must change; the blob of a packed pool is the blob of a uint16 pool with the same codes; a range of layers; a task list
     longer than the grid; untrusted table values and ids;
  2. through million_amd.paged_turns, packed and uint16, on demand and preallocated: a slot swapped out and back into another slot
     decodes the bits of a twin that was never swapped, also through a file into a new cache; a snapshot of a uint16 cache goes
     into a packed cache and back; snapshot_request leaves the slot decoding unchanged.

Requests: T in {0, 1, 31, 32, 33, 69} (T mod 4 and T mod 16 at 0, 1 and their last value), r in {0, 1, cap}, one ring start that
makes the live rows wrap.  A slot's decode output is a function of its own codes, window and lengths alone (use_dev_lengths=True),
so outputs of the same request at the same position compare bitwise whatever the other slots hold."""
import numpy as np
import pytest

from tests import cache_swap_wide_model as WM
from tests import fork_swap_wide_common as X
from tests import packed_model as P

pytestmark = pytest.mark.gpu

LAYERS, BS, NHK, NH, CAP, NPC, GUARD = X.LAYERS, X.BS, X.NHK, X.NH, X.CAP, X.NPC, 256
INT_MAX = 2 ** 31 - 1
# every format at pages of 32; one of them at 64 and 128 too
CASES = [f + (32,) for f in X.FORMATS] + [X.FORMATS[3] + (64,), X.FORMATS[3] + (128,)]
REQUESTS = np.asarray([[0, 0, CAP, CAP - 1], [1, 1, 1, 5], [2, 31, 0, 0], [0, 32, CAP, 5], [1, 33, 1, CAP - 1], [2, 69, CAP, 0]], np.int32)


@pytest.fixture(scope="module")
def env():
    import torch
    assert torch.cuda.is_available(), "GPU tests need an MI355X"
    from million_amd import ops, _lib
    _lib.load()
    yield torch, ops
    assert ops.tail_faults() == 0


_SCENES = {}


def _scene(oracle, d, M, nbits, ps):
    key = (d, M, nbits, ps)
    if key not in _SCENES:
        _SCENES[key] = X.tables(nbits + ps, d, M, 2 ** nbits, ps, oracle)
    return {k: [a.copy() for a in v] for k, v in _SCENES[key].items()}


def _differs(what, name, want, got):
    if not np.array_equal(want, got):
        bad = np.argwhere(want != got)
        raise AssertionError(f"{what}: {name} differs from the model at {len(bad)} places, first {bad[0].tolist()}: "
                             f"model {want[tuple(bad[0])]}, device {got[tuple(bad[0])]}")


def _guarded(n, fill=0xA5):
    blob = np.full(n + 2 * GUARD, fill, np.uint8)
    blob[:GUARD] = blob[n + GUARD:] = 0x3C
    return blob


def _run_both(torch, ops, direction, host, table, offs, blob, *, ps, M, C, what, **kw):
    """The call and the model on copies of the same arrays; `blob` (numpy, guards included) is the blob's state before the call.
    Every array is compared; returns the model's (arrays, blob with guards)."""
    want, want_blob = [a.copy() for a in host], blob.copy()
    packed = WM.is_packed(host[1])
    dev = [X.to_dev(torch, a) for a in host]
    dev[3], dev[4] = dev[3].view(torch.float16), dev[4].view(torch.float16)
    dev_blob = torch.from_numpy(blob.copy()).cuda()
    inner = slice(GUARD, blob.size - GUARD)
    if direction == WM.PACK:
        WM.pack(*want[:5], table, offs, want_blob[inner], page_size=ps, M=M, C=C, **kw)
    else:
        WM.unpack(*want, table, offs, want_blob[inner], page_size=ps, M=M, C=C, **kw)
    ops.cache_swap_wide(direction, *dev, torch.from_numpy(table).cuda(), torch.from_numpy(offs).cuda(), dev_blob[inner], C=C, packed=packed,
                        page_size=ps, M=M, **kw)
    torch.cuda.synchronize()
    dev[3], dev[4] = dev[3].view(torch.int16), dev[4].view(torch.int16)
    got_blob = dev_blob.cpu().numpy()
    assert (got_blob[:GUARD] == 0x3C).all() and (got_blob[-GUARD:] == 0x3C).all(), f"{what}: guard bytes around the blob were written"
    _differs(what, "blob", want_blob, got_blob)
    for name, w, g in zip(X.NAMES, want, dev):
        _differs(what, name, w, X.to_np(torch, g))
    return want, want_blob


def _poisoned(host, seed):
    """The arrays of `host` with other scattered ids and 0xA5 in every pool byte, NaN in every window row."""
    rs = np.random.RandomState(seed)
    dst = [a.copy() for a in host]
    dst[0] = rs.permutation(dst[1].shape[0])[:dst[0].size].reshape(dst[0].shape).astype(np.int32)
    for a in dst[1:3]:
        a[...] = 0xA5 * (0x101 if a.dtype == np.uint16 else 1)
    dst[3][...] = dst[4][...] = 0x7E00
    return dst


@pytest.mark.parametrize("d,M,nbits,ps", CASES)
def test_swap_wide_call_equals_the_model_byte_for_byte(env, oracle, d, M, nbits, ps):
    torch, ops = env
    C = 2 ** nbits
    scene = _scene(oracle, d, M, nbits, ps)
    kw = dict(ps=ps, M=M, C=C)
    offs, total = X.layout(REQUESTS, ps, M, d, C)
    pad = 64      # staging outside the entries' ranges keeps its poison
    blobs = {}
    for name, host in scene.items():
        what = f"d={d} M={M} C={C} page={ps} {name}"
        after, blobs[name] = _run_both(torch, ops, WM.PACK, host, REQUESTS, offs + pad, _guarded(total + 2 * pad), what=what + " pack", **kw)
        assert all(np.array_equal(a, b) for a, b in zip(after, host))
        inner = blobs[name][GUARD:-GUARD]
        assert (inner[:pad] == 0xA5).all() and (inner[-pad:] == 0xA5).all()
    assert np.array_equal(blobs["u16"], blobs["packed"]), "blob(packed pool) == blob(uint16 pool)"
    # UNPACK, three slots a call (the slots of a call must differ), into poisoned arrays of either kind
    for name, host in scene.items():
        for part in (slice(0, 3), slice(3, 6)):
            dst = _poisoned(host, 7)
            after, _ = _run_both(torch, ops, WM.UNPACK, dst, REQUESTS[part], offs[part] + pad, blobs["u16"],
                                 what=f"d={d} M={M} C={C} page={ps} {name} unpack {part}", **kw)
            for slot, T, r, st in REQUESTS[part].tolist():
                want = WM.live_codes(*scene["packed"][:3], slot, T, page_size=ps, M=M, C=C)
                got = WM.live_codes(*after[:3], slot, T, page_size=ps, M=M, C=C)
                assert all(np.array_equal(a, b) for a, b in zip(want, got)), (name, slot)


@pytest.mark.parametrize("packed", [False, True], ids=["uint16", "packed"])
def test_swap_wide_call_on_a_range_of_layers(env, oracle, packed):
    torch, ops = env
    d, M, nbits, ps = X.FORMATS[3] + (32,)
    C = 2 ** nbits
    host = _scene(oracle, d, M, nbits, ps)["packed" if packed else "u16"]
    table = REQUESTS[3:]
    offs, total = X.layout(table, ps, M, d, C, layers=1)
    kw = dict(ps=ps, M=M, C=C, layer0=1, n_layers=1)
    _, blob = _run_both(torch, ops, WM.PACK, host, table, offs, _guarded(total), what="layer 1 pack", **kw)
    dst = _poisoned(host, 11)
    after, _ = _run_both(torch, ops, WM.UNPACK, dst, table, offs, blob, what="layer 1 unpack", **kw)
    assert np.array_equal(after[5][0], dst[5][0]) and after[5][1, 2].tolist() == [69, CAP, 0, 0]


N_FILLER = 44000      # entries that take no part: 2 layers x 2 kv heads x 6 tasks per row x 44000 > the kernel's grid cap of 2^20


@pytest.mark.parametrize("packed", [False, True], ids=["uint16", "packed"])
def test_swap_wide_call_with_more_tasks_than_workgroups(env, oracle, packed):
    """The task count follows the bounds (d 128, M 64, pages of 32: 4 page tasks of one page, one window task, one lengths task
    per row), so a long table of entries that take no part makes the list longer than the grid: the requests, spread over the
    table, are served by workgroups on a later turn of their loop."""
    torch, ops = env
    d, M, nbits, ps = X.FORMATS[0] + (32,)
    C = 2 ** nbits
    host = _scene(oracle, d, M, nbits, ps)["packed" if packed else "u16"]
    real = REQUESTS[3:]
    table = np.tile(np.asarray([[-1, 70, 3, 1], [BS, 1, 1, 0]], np.int32), (N_FILLER // 2, 1))
    where = np.linspace(0, N_FILLER - 1, len(real)).astype(int)
    table[where] = real
    offs = np.zeros(N_FILLER, np.int64)
    offs[where], total = X.layout(real, ps, M, d, C)
    kw = dict(ps=ps, M=M, C=C)
    assert P.page_bytes(ps, M, C) * 2 > 4096 and LAYERS * NHK * (NPC + 2) * N_FILLER > 2 ** 20
    _, blob = _run_both(torch, ops, WM.PACK, host, table, offs, _guarded(total), what="long table, pack", **kw)
    _, want = _run_both(torch, ops, WM.PACK, host, real, offs[where], _guarded(total), what="the requests alone", **kw)
    assert np.array_equal(blob, want)
    _run_both(torch, ops, WM.UNPACK, _poisoned(host, 13), table, offs, blob, what="long table, unpack", **kw)


@pytest.mark.parametrize("packed", [False, True], ids=["uint16", "packed"])
def test_swap_wide_call_on_untrusted_values(env, oracle, packed):
    """Slots, lengths, starts, offsets and ids that are negative, INT_MAX or past the pool: clamped or dropped by contract (the
    kernel: swapw_entry's slot test, clamp_len_row and offset test; the unsigned id test in front of every pool address).  The
    result is the model's, guards and every other byte unchanged."""
    torch, ops = env
    d, M, nbits, ps = X.FORMATS[3] + (32,)
    C = 2 ** nbits
    host = _scene(oracle, d, M, nbits, ps)["packed" if packed else "u16"]
    n_pool = host[1].shape[0]
    host[0][0, 0, 0, 1] = -1
    host[0][1, 0, 1, 0] = n_pool
    host[0][0, 2, 1, 2] = INT_MAX
    host[0][1, 2, 0, 3] = -INT_MAX - 1
    table = np.asarray([[0, INT_MAX, INT_MAX, INT_MAX], [-1, 5, 1, 0], [INT_MAX, 5, 1, 0], [1, -5, -1, -3], [2, 100, 7, CAP],
                        [1, 33, 1, 0], [1, 33, 1, 0], [1, 33, 1, 0], [1, 33, 1, 0]], np.int32)
    offs, total = X.layout(table[:5], ps, M, d, C)
    offs = np.concatenate([offs, [-16, 8, total, INT_MAX * 4096]]).astype(np.int64)      # negative, unaligned, no room, far outside
    kw = dict(ps=ps, M=M, C=C)
    _, blob = _run_both(torch, ops, WM.PACK, host, table, offs, _guarded(total), what="untrusted pack", **kw)
    dst = _poisoned(host, 17)
    dst[0][...] = host[0]
    _run_both(torch, ops, WM.UNPACK, dst, table, offs, blob, what="untrusted unpack", **kw)


# ---------------------------------------------------------------- 2. the cache, through paged_turns ------------------------
PS, N_PROMPT, FIRST, STEPS = X.PS, X.N_PROMPT, X.FIRST, X.STEPS
World, new_cache, prefill, decode, same_bits = X.World, X.new_cache, X.prefill, X.decode, X.same_bits


@pytest.mark.parametrize("preallocate", [False, True], ids=["on-demand", "preallocated"])
@pytest.mark.parametrize("packed", [False, True], ids=["uint16", "packed"])
def test_a_swapped_slot_decodes_the_bits_of_a_twin(env, packed, preallocate, tmp_path):
    torch, ops = env
    from million_amd import formats, paged_turns
    w = World(128, 64, 10)
    twin, cache = new_cache(torch, w, packed, preallocate), new_cache(torch, w, packed, preallocate)
    for c in (twin, cache):
        prefill(torch, c, w, 0)
    first = decode(torch, twin, w, [N_PROMPT, None, None], FIRST)
    assert same_bits(first[0], decode(torch, cache, w, [N_PROMPT, None, None], FIRST)[0])
    with pytest.raises(NotImplementedError, match="nbits"):
        cache.swap_out(0)
    keep = paged_turns.snapshot_request(cache, 0)      # the slot keeps decoding, unchanged
    assert keep.meta["version"] == 2 and keep.blob.numel() == LAYERS * NHK * ops.cache_swap_row_bytes_wide(N_PROMPT, FIRST, PS, w.M, w.d, w.C)
    snap = paged_turns.swap_out(cache, 0)
    assert torch.equal(snap.blob, keep.blob) and not cache._T_a[:, 0].any() and not cache._lengths_all[:, 0].any().item()
    prefill(torch, cache, w, 0, n=20)                  # something else uses the slot and, on demand, its pages
    paged_turns.swap_in(cache, 2, snap)
    fresh = new_cache(torch, w, packed, preallocate)   # ... and through a file into a new cache
    paged_turns.swap_in(fresh, 1, formats.load_request(formats.save_request(tmp_path / "r.pt", snap)))
    want = decode(torch, twin, w, [N_PROMPT + FIRST, None, None], STEPS)[0]      # crosses the flush at r = 64
    assert int(twin._T_a[0, 0]) == N_PROMPT + PS
    assert same_bits(want, decode(torch, cache, w, [None, None, N_PROMPT + FIRST], STEPS)[2])
    assert same_bits(want, decode(torch, fresh, w, [None, N_PROMPT + FIRST, None], STEPS)[1])


@pytest.mark.parametrize("d,M,nbits", [X.FORMATS[0], X.FORMATS[1], X.FORMATS[3]])
def test_a_snapshot_migrates_between_uint16_and_packed_caches(env, d, M, nbits):
    torch, ops = env
    from million_amd import paged_turns
    w = World(d, M, nbits)
    u16, pk = new_cache(torch, w, False, False), new_cache(torch, w, True, True)
    prefill(torch, u16, w, 0)
    prefill(torch, pk, w, 0)
    a, b = decode(torch, u16, w, [N_PROMPT, None, None], FIRST)[0], decode(torch, pk, w, [N_PROMPT, None, None], FIRST)[0]
    assert same_bits(a, b), "the packed decode launch is bitwise the uint16 launch's"
    s16, spk = paged_turns.snapshot_request(u16, 0), paged_turns.snapshot_request(pk, 0)
    assert torch.equal(s16.blob, spk.blob) and s16.meta == spk.meta, "one blob, whichever pool format it was packed from"
    paged_turns.swap_in(pk, 1, s16)      # uint16 -> packed
    paged_turns.swap_in(u16, 2, spk)     # packed -> uint16
    p = N_PROMPT + FIRST
    want = decode(torch, u16, w, [p, None, p], STEPS)
    got = decode(torch, pk, w, [p, p, None], STEPS)
    assert int(u16._T_a[0, 0]) == N_PROMPT + PS, "the steps crossed a flush"
    assert same_bits(want[0], want[2]) and same_bits(want[0], got[0]) and same_bits(want[0], got[1])
    assert torch.equal(paged_turns.snapshot_request(u16, 2).blob, paged_turns.snapshot_request(pk, 1).blob)
