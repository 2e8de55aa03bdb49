"""GPU test of the shared nearest-centroid scan (csrc/pq_scan.h): every kernel that runs it - and pq_flush_kernel, which carries
the same loop in its own body - encodes the SAME tie-heavy rows, and each is compared bit for bit with oracle.pq_encode, hence
with every other.  The tie rule (strict '<' over increasing c: the lowest index wins) only shows on exact ties, so the input
is built to be full of them - duplicated centroid rows, centroids and inputs on a small grid of halves (every distance is
exact in fp32, many are equal), inputs that equal a centroid - and the test first checks on the CPU that at least a quarter
of the oracle's (row, subspace) pairs have two or more centroids at the exact minimum.

d_m in {1, 2, 4, 8}; C = 256, and C = 3: an empty centroid quarter in the LDS kernels; n = 130 rows: two full 64-lane blocks
and a two-lane tail; nh_k = 2, bs = 1."""
import numpy as np
import pytest

from tests import kmeans_ref as R

pytestmark = pytest.mark.gpu

N, NHK = 130, 2
CASES = [(d, M, C) for d, M in ((64, 64), (128, 64), (128, 32), (128, 16)) for C in (256, 3)]
FILL = 0xA5
_SCENES = {}


def _dists(X, cents):
    """(rows, M, C) fp32 distances by the contract: e = x - c, sq = e * e, a sequential sum."""
    M, C, dm = cents.shape
    e = X.astype(np.float32).reshape(-1, M, 1, dm) - cents.astype(np.float32)[None]
    sq = e * e
    acc = sq[..., 0].copy()
    for k in range(1, dm):
        acc = acc + sq[..., k]
    return acc


def _codebook(rs, M, C, dm):
    """Grid points in {-2, -1.5, .., 2}^dm; a third of each subspace's rows are copies of other rows of it."""
    cents = (rs.randint(-4, 5, size=(M, C, dm)) * 0.5).astype(np.float16)
    for m in range(M):
        dst = rs.permutation(C)[:max(C // 3, 1)]
        src = (dst + rs.randint(1, C, size=len(dst))) % C
        cents[m, dst] = cents[m, src]      # one assignment: a source that is itself a destination gives its old row
    return cents


def scene(O, d, M, C):
    """Inputs and the oracle's codes, once per shape and never changed: X (1, NHK, N, d) fp16, the K and V codebooks, ref_k /
    ref_v (1, NHK, N, M)."""
    if (d, M, C) in _SCENES:
        return _SCENES[(d, M, C)]
    rs = np.random.RandomState(1000 * d + 10 * M + C)
    dm = d // M
    kc, vc = _codebook(rs, M, C, dm), _codebook(rs, M, C, dm)
    X = (rs.randint(-5, 6, size=(1, NHK, N, d)) * 0.5).astype(np.float16)
    Xs = X.reshape(1, NHK, N, M, dm)
    for h in range(NHK):      # every fifth row of head h: sub-vectors that ARE centroids (K codebook on head 0, V on head 1)
        rows = np.arange(h, N, 5)
        picks = rs.randint(0, C, size=(len(rows), M))
        Xs[0, h, rows] = (kc, vc)[h][np.arange(M)[None, :], picks]
    sc = dict(X=X, kc=kc, vc=vc, ref_k=O.pq_encode(X, kc), ref_v=O.pq_encode(X, vc))
    for cents, ref in ((kc, sc["ref_k"]), (vc, sc["ref_v"])):
        dist = _dists(X.reshape(-1, d), cents)
        assert np.array_equal(dist.argmin(-1), ref.reshape(-1, M)), "the oracle takes the lowest index at the minimum"
        tied = ((dist == dist.min(-1, keepdims=True)).sum(-1) >= 2).mean()
        print(f"d={d} M={M} C={C}: {tied:.3f} of the (row, subspace) pairs have >= 2 centroids at the exact minimum")
        assert tied >= 0.25, "a test without ties proves nothing about the tie rule"
    _SCENES[(d, M, C)] = sc
    return sc


@pytest.fixture(scope="module")
def env():
    import torch
    assert torch.cuda.is_available(), "GPU tests need an MI355X"
    from million_amd import ops, _lib
    _lib.load()
    return torch, ops, _lib


def _cu(torch, a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


@pytest.mark.parametrize("d,M,C", CASES)
def test_encode_small_call(d, M, C, env, oracle):
    """million_pq_encode into a row-major store at n = 130: the LDS kernel (prepared or raw codebook, it reads the raw one)."""
    torch, ops, L = env
    sc = scene(oracle, d, M, C)
    X, kc = _cu(torch, sc["X"]), _cu(torch, sc["kc"])
    for use_prepared in (True, False):
        dst = torch.full((1, NHK, N + 3, M), FILL, dtype=torch.uint8, device="cuda")
        ops.pq_encode_into(X, kc, dst, token_start=2, use_prepared=use_prepared)
        got = dst.cpu().numpy()
        assert np.array_equal(got[:, :, 2:2 + N], sc["ref_k"]), use_prepared
        assert (got[:, :, :2] == FILL).all() and (got[:, :, 2 + N:] == FILL).all()


@pytest.mark.parametrize("d,M,C", CASES)
def test_encode_bulk_call(d, M, C, env, oracle):
    """The same call at the smallest size the launcher gives to the scalar-cache kernel (1024 four-subspace waves): 16 (b, head)
    pairs x 16 / ceil(M / 16) token blocks, the last one with a two-lane tail; pair p holds the rows rotated by 7 p.  Prepared
    codebook (fp32 table) and raw (fp16 table)."""
    torch, ops, L = env
    sc = scene(oracle, d, M, C)
    bs, tblocks = 8, 16 // -(-M // 16)
    n = 64 * tblocks - 62
    # launch_dm (csrc/encode.hip) gives a uint8 call to pq_encode_kernel from `waves4 >= 1024` on; this is its formula.  If that
    # threshold moves, move this shape with it: below it the call runs the LDS kernel, which test_encode_small_call covers
    assert tblocks * -(-M // 16) * 4 * bs * NHK == 1024
    idx = (np.arange(n)[None, :] + 7 * np.arange(bs * NHK)[:, None]) % N                      # (pairs, n)
    src_h = np.arange(bs * NHK) % NHK                                                         # pair p shows rows of head p % 2
    Xb = sc["X"][0][src_h[:, None], idx].reshape(bs, NHK, n, d)
    want = sc["ref_k"][0][src_h[:, None], idx].reshape(bs, NHK, n, M)
    Xd, kc = _cu(torch, Xb), _cu(torch, sc["kc"])
    for use_prepared in (True, False):
        dst = torch.full((bs, NHK, n, M), FILL, dtype=torch.uint8, device="cuda")
        ops.pq_encode_into(Xd, kc, dst, use_prepared=use_prepared)
        assert np.array_equal(dst.cpu().numpy(), want), use_prepared


@pytest.mark.parametrize("d,M,C", CASES)
def test_flush(d, M, C, env, oracle):
    """million_pq_flush: rows 0..63 as the K window and rows 64..127 as the V window, both wrapped around a 128-row ring, into
    the second page of shuffled K and transposed V page tables."""
    torch, ops, L = env
    sc = scene(oracle, d, M, C)
    cap, ps, start = 128, 64, 100
    ring = (start + np.arange(64)) % cap
    kw, vw = np.zeros((1, NHK, cap, d), np.float16), np.zeros((1, NHK, cap, d), np.float16)
    kw[:, :, ring], vw[:, :, ring] = sc["X"][:, :, :64], sc["X"][:, :, 64:128]
    ids = np.array([[[5, 2], [0, 3]]], np.int32)
    k_pool = torch.full((6, ps, M), FILL, dtype=torch.uint8, device="cuda")
    v_pool = torch.full((6, M, ps), FILL, dtype=torch.uint8, device="cuda")
    ops.pq_flush(_cu(torch, kw), _cu(torch, vw), _cu(torch, sc["kc"]), _cu(torch, sc["vc"]), k_pool, v_pool, _cu(torch, ids),
                 n=64, page_size=ps, token_start=ps, x_row_start=start)
    kp, vp = k_pool.cpu().numpy(), v_pool.cpu().numpy()
    for h in range(NHK):
        assert np.array_equal(kp[ids[0, h, 1]], sc["ref_k"][0, h, :64]), h
        assert np.array_equal(vp[ids[0, h, 1]].T, sc["ref_v"][0, h, 64:128]), h
    rest = [p for p in range(6) if p not in ids[0, :, 1]]
    assert (kp[rest] == FILL).all() and (vp[rest] == FILL).all()


@pytest.mark.parametrize("d,M,C", CASES)
def test_store_ragged(d, M, C, env, oracle):
    """million_pq_store_ragged: one request whose window holds r = 5 rows from ring position 3, and n_b = 125 new rows, behind
    T = 40 tokens: the 130 rows become tokens 40..169 of its K pages and transposed V pages."""
    torch, ops, L = env
    sc = scene(oracle, d, M, C)
    cap, ps, npc, T, r, start = 64, 32, 8, 40, 5, 3
    win = np.zeros((1, NHK, cap, d), np.float16)
    win[:, :, start:start + r] = sc["X"][:, :, :r]
    new = _cu(torch, sc["X"][:, :, r:])
    ids = np.random.RandomState(5).permutation(NHK * npc).astype(np.int32).reshape(1, NHK, npc)
    k_pool = torch.full((NHK * npc, ps, M), FILL, dtype=torch.uint8, device="cuda")
    v_pool = torch.full((NHK * npc, M, ps), FILL, dtype=torch.uint8, device="cuda")
    lengths = torch.tensor([[T, r, start, 77]], dtype=torch.int32, device="cuda")
    wd = _cu(torch, win)
    ops.pq_store_ragged(new, new, wd, wd, ops.prepare_cents(_cu(torch, sc["kc"]), cache=False),
                        ops.prepare_cents(_cu(torch, sc["vc"]), cache=False), k_pool, v_pool, _cu(torch, ids), lengths,
                        torch.tensor([N - r], dtype=torch.int32, device="cuda"), M=M, C=C, page_size=ps)
    assert lengths.tolist() == [[T + N, 0, 0, 77]]
    got_k = oracle.pool_to_k_rowmajor(k_pool.cpu().numpy(), ids, T + N)
    got_v = oracle.pool_to_v_rowmajor(v_pool.cpu().numpy(), ids, T + N)
    assert np.array_equal(got_k[:, :, T:], sc["ref_k"]) and np.array_equal(got_v[:, :, T:], sc["ref_v"])
    assert (got_k[:, :, :T] == FILL).all() and (got_v[:, :, :T] == FILL).all()


@pytest.mark.parametrize("d,M,C", CASES)
def test_train_assign_step(d, M, C, env, oracle):
    """million_pq_train's assign step.  The training set is the K codebook written out as C rows, then the 130 rows of head 0;
    init_rows = 0 .. C-1, so the first table IS the codebook.  No entry point returns the assign step's codes: one iteration's
    counts and centroids (fp32 and fp16 input) are compared bit for bit with the numpy model run on codes that are, for the
    130 rows, the oracle's codes of the other tests."""
    from tests.test_train_gpu import assert_same, gpu_train
    torch, ops, L = env
    sc = scene(oracle, d, M, C)
    X16 = np.concatenate([sc["kc"].transpose(1, 0, 2).reshape(C, d), sc["X"][0, 0]])
    X32 = X16.astype(np.float32)
    cents0 = R.init_from_rows(X32, M, np.arange(C))
    assert np.array_equal(cents0, sc["kc"].astype(np.float32))
    assert np.array_equal(R.assign(X32, cents0)[0][C:], sc["ref_k"][0, 0])
    want = R.lloyd(X32, cents0, 1)
    assert_same(gpu_train(X32, M, C, 1, rows=np.arange(C)), want, f"fp32 rows {(d, M, C)}")
    assert_same(gpu_train(torch.from_numpy(X16).cuda(), M, C, 1, rows=np.arange(C)), want, f"fp16 rows {(d, M, C)}")
