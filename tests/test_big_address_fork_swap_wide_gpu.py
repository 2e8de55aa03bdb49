"""Far addresses of fork and swap over wide code pages (million_cache_fork_wide, million_cache_swap_wide): one packed pool pair
and one uint16 pool pair run past 4 GiB, and the table names the pages whose byte offset id * page_bytes crosses 2^31 and 2^32 -
a packed page is no power of two, so pages straddle both boundaries.  Fork (COPY), PACK and UNPACK run twice, through the far
ids and on a compact twin, and everything they write must be bitwise equal; afterwards nothing but the named pages may differ
from the sentinel the far pools were filled with.  The skip rule is tests/test_big_address_gpu.py's."""
import numpy as np
import pytest

from tests import big_address as BA
from tests import cache_fork_model as FM
from tests import cache_swap_wide_model as WM
from tests import fork_swap_wide_common as X
from tests import packed_model as P

pytestmark = pytest.mark.gpu

NEED_FREE = 12 << 30
D, M, NBITS, PS = 128, 64, 10, 32
C = 2 ** NBITS
SPARE = 16      # pages past 2^32


@pytest.fixture(scope="module")
def env():
    import torch
    assert torch.cuda.is_available(), "GPU tests need an MI355X"
    from million_amd import ops, _lib
    _lib.load()
    return torch, ops


def _far_map(ids, n_compact, page_bytes, seed):
    """compact id -> far id: the compact ids in the table's page-major order (page 0 of every row first: live in every request)
    get the ids around both boundaries, the first and the last page; the others ids dealt from the whole pool."""
    n_far = BA.HI // page_bytes + SPARE
    b31, b32 = (BA.HI // 2) // page_bytes, BA.HI // page_bytes
    first = [b31 - 1, b31, b31 + 1, b32 - 1, b32, b32 + 1, 0, n_far - 1]
    assert b31 * page_bytes <= BA.HI // 2 < (b31 + 1) * page_bytes and b32 * page_bytes <= BA.HI < (b32 + 1) * page_bytes
    rs = np.random.RandomState(seed)
    rest = [int(i) for i in rs.permutation(n_far)[:n_compact + len(first)] if int(i) not in first][:n_compact - len(first)]
    order = list(dict.fromkeys(ids.transpose(3, 0, 1, 2).flatten().tolist()))
    order += [i for i in range(n_compact) if i not in set(order)]
    c2f = np.zeros(n_compact, np.int64)
    c2f[order] = first + rest
    assert len(set(c2f.tolist())) == n_compact
    return c2f, n_far


@pytest.mark.parametrize("packed", [True, False], ids=["packed", "uint16"])
def test_fork_and_swap_wide_far(env, oracle, packed):
    torch, ops = env
    free = torch.cuda.mem_get_info()[0]
    if free < NEED_FREE:
        pytest.skip(f"{free / 2 ** 30:.1f} GiB of device memory free, the far pools want {NEED_FREE >> 30} GiB")
    host = X.tables(77, D, M, C, PS, oracle)["packed" if packed else "u16"]
    page_bytes = P.page_bytes(PS, M, C) if packed else PS * M * 2
    n_compact = host[1].shape[0]
    c2f, n_far = _far_map(host[0], n_compact, page_bytes, 78)
    assert n_far * page_bytes > BA.HI
    flats = [torch.empty(n_far * page_bytes, dtype=torch.uint8, device="cuda") for _ in range(2)]
    views = [f.view(n_far, page_bytes) if packed else f.view(torch.uint16).view(n_far, *host[i + 1].shape[1:]) for i, f in enumerate(flats)]
    kw = dict(C=C, packed=packed, page_size=PS, M=M)
    far_ids = torch.from_numpy(c2f[host[0]].astype(np.int32)).cuda()
    all_far = torch.from_numpy(c2f).cuda()

    def far_arrays(arrs):
        """Device arrays over the far pools holding what `arrs` holds; everything else of the pools is the sentinel."""
        for f, v, a in zip(flats, views, arrs[1:3]):
            f.fill_(BA.SENTINEL)
            BA.scatter_pool(v, X.to_dev(torch, a), c2f)
        rest = [X.to_dev(torch, a) for a in arrs[3:]]
        return [far_ids.clone(), views[0], views[1], rest[0].view(torch.float16), rest[1].view(torch.float16), rest[2]]

    def twin_arrays(arrs):
        dev = [X.to_dev(torch, a) for a in arrs]
        dev[3], dev[4] = dev[3].view(torch.float16), dev[4].view(torch.float16)
        return dev

    def same(twin, far, what):
        torch.cuda.synchronize()
        for i in (1, 2):
            got = BA.gather_pool(far[i], all_far)
            assert np.array_equal(X.to_np(torch, got), X.to_np(torch, twin[i])), f"{what}: {X.NAMES[i]} differs from the compact twin's"
        assert torch.equal(far[0], far_ids), f"{what}: the table was written"
        for i in (3, 4, 5):
            assert torch.equal(far[i].view(torch.int16) if i < 5 else far[i], twin[i].view(torch.int16) if i < 5 else twin[i]), (what, X.NAMES[i])

    def only_named(twin, far, what):
        """The named pages are the twin's and nothing else of the far pools was written.  Destroys the far pages."""
        torch.cuda.synchronize()
        for i in (1, 2):
            BA.assert_only_these_pages(far[i], all_far, twin[i], flats[i - 1], f"{what}: {X.NAMES[i]}")

    # ---- fork, COPY: slot 0 -> slots 1 and 2, every live page
    host[5][:, 0] = (2 * PS + 5, 40, 50, 0)
    dst = torch.tensor([1, 2], dtype=torch.int32).cuda()
    want = [a.copy() for a in host]
    copied = WM.fork(*want, np.asarray([1, 2]), None, page_size=PS, src=0, mode=FM.COPY, n_pages_bound=X.NPC)
    assert len(copied) == 2 * X.LAYERS * X.NHK * 3
    moved = c2f[[c[4] for c in copied] + [c[5] for c in copied]] * page_bytes
    assert (moved < BA.HI // 2).any() and ((moved >= BA.HI // 2) & (moved < BA.HI)).any() and (moved + page_bytes > BA.HI).any()
    twin, far = twin_arrays(host), far_arrays(host)
    for dev in (twin, far):
        ops.cache_fork_wide(*dev, dst, None, src=0, share=False, n_pages_bound=X.NPC, **kw)
    same(twin, far, "fork")
    assert all(np.array_equal(w, X.to_np(torch, t.view(torch.int16) if t.dtype == torch.float16 else t)) for w, t in zip(want, twin)), "the twin is the model's"
    only_named(twin, far, "fork")

    # ---- PACK: three requests from far pages; the blob is the twin's, byte for byte
    table = np.asarray([[0, 2 * PS + 5, X.CAP, 5], [1, PS, 1, X.CAP - 1], [2, 4 * PS - 1, 0, 0]], np.int32)
    offs, total = X.layout(table, PS, M, D, C)
    d_table, d_offs = torch.from_numpy(table).cuda(), torch.from_numpy(offs).cuda()
    twin, far = twin_arrays(host), far_arrays(host)
    blobs = []
    for dev in (twin, far):
        blob = torch.full((total,), 0x3C, dtype=torch.uint8, device="cuda")
        ops.cache_swap_wide(WM.PACK, *dev, d_table, d_offs, blob, n_pages_bound=X.NPC, **kw)
        blobs.append(blob)
    same(twin, far, "pack (nothing but the blob is written)")
    want_blob = np.full(total, 0x3C, np.uint8)
    WM.pack(*host[:5], table, offs, want_blob, page_size=PS, M=M, C=C)
    assert np.array_equal(blobs[0].cpu().numpy(), want_blob) and torch.equal(blobs[0], blobs[1])

    # ---- UNPACK: the blob into far pages of a poisoned state
    dst_host = [a.copy() for a in host]
    for a in dst_host[1:3]:
        a[...] = 0x5A * (0x101 if a.dtype == np.uint16 else 1)
    dst_host[3][...] = dst_host[4][...] = 0x7E00
    twin, far = twin_arrays(dst_host), far_arrays(dst_host)
    for dev in (twin, far):
        ops.cache_swap_wide(WM.UNPACK, *dev, d_table, d_offs, blobs[0], n_pages_bound=X.NPC, **kw)
    same(twin, far, "unpack")
    want = [a.copy() for a in dst_host]
    WM.unpack(*want, table, offs, want_blob, page_size=PS, M=M, C=C)
    assert np.array_equal(want[1], X.to_np(torch, twin[1])) and np.array_equal(want[2], X.to_np(torch, twin[2]))
    only_named(twin, far, "unpack")
    del flats, views, far
    torch.cuda.empty_cache()
