"""GPU tests of PQ codebook training (million_pq_train / million_amd.train): centroids and counts bitwise equal to the numpy
restatement of the contract (tests/kmeans_ref.py), objectives within 1e-9 relative (fp64 sums of the same fp32 terms: only
the order differs), and the trained codebook through the rest of the pipeline."""
import numpy as np
import pytest

from tests import kmeans_ref as R

pytestmark = pytest.mark.gpu

# (n, d, M, C): d_m in {1, 2, 4, 8}; C in {16, 128, 256, 1024} (1024: uint16 codes); n below one chunk, not a multiple of the
# chunk, M not a multiple of the 4 subspaces a wave takes; the last one is Llama-shaped
CASES = [
    (1000, 8, 8, 16),
    (5000, 16, 8, 128),
    (4500, 24, 6, 256),
    (9000, 32, 4, 1024),
    (3000, 6, 3, 16),
    (8192, 128, 64, 256),
]


def mixture(rs, n, d, n_modes=24, spread=0.35):
    """A Gaussian mixture sample, fp32."""
    modes = rs.standard_normal((n_modes, d)).astype(np.float32) * 2.0
    return (modes[rs.randint(0, n_modes, size=n)] + spread * rs.standard_normal((n, d)).astype(np.float32)).astype(np.float32)


def gpu_train(X, M, C, niter, *, rows=None, cents0=None, **kw):
    import torch
    from million_amd import train
    Xd = X if isinstance(X, torch.Tensor) else torch.from_numpy(X).cuda()
    cents, counts, obj = train.kmeans_pq(
        Xd, M, C, niter,
        init_rows=None if rows is None else torch.from_numpy(np.asarray(rows, dtype=np.int32)).cuda(),
        cents_init=None if cents0 is None else torch.from_numpy(cents0).cuda(), **kw)
    torch.cuda.synchronize()
    return cents.cpu().numpy(), counts.cpu().numpy(), obj.cpu().numpy()


def assert_same(got, want, what):
    cents, counts, obj = got
    rc, rn, ro = want
    bad = int((cents.view(np.uint32) != rc.view(np.uint32)).sum())
    ro = np.asarray(ro)
    err = np.abs(obj - ro)
    print(f"{what}: {bad} of {cents.size} centroid words differ, counts equal {np.array_equal(counts, rn)}, "
          f"worst objective error {err.max():.3e} at objective {ro[err.argmax()]:.6g}")
    assert np.array_equal(counts, rn), what
    assert bad == 0, what
    assert (err <= 1e-9 * np.abs(ro)).all(), (what, err.max())      # 1e-9 relative; an objective of exactly 0 must be 0


@pytest.mark.parametrize("n,d,M,C", CASES)
def test_one_iteration_from_cents_init_is_bitwise(oracle, n, d, M, C):
    rs = np.random.RandomState(n + C)
    X = mixture(rs, n, d)
    cents0 = R.init_from_rows(X, M, rs.permutation(n)[:C])
    assert_same(gpu_train(X, M, C, 1, cents0=cents0), R.lloyd(X, cents0, 1), f"1 iteration {(n, d, M, C)}")


@pytest.mark.parametrize("n,d,M,C", CASES)
def test_25_iterations_from_init_rows_are_bitwise(oracle, n, d, M, C):
    rs = np.random.RandomState(7 * n + C)
    X = mixture(rs, n, d)
    rows = rs.permutation(n)[:C]
    assert_same(gpu_train(X, M, C, 25, rows=rows), R.lloyd(X, R.init_from_rows(X, M, rows), 25), f"25 iterations {(n, d, M, C)}")


@pytest.mark.parametrize("n,d,M,C", [(5000, 16, 8, 128), (4500, 32, 4, 256), (2000, 8, 8, 1024)])
def test_fp16_input_gives_the_bits_of_fp32_input(n, d, M, C):
    import torch
    rs = np.random.RandomState(5)
    X16 = mixture(rs, n, d).astype(np.float16)
    rows = rs.permutation(n)[:C]
    a = gpu_train(torch.from_numpy(X16).cuda(), M, C, 6, rows=rows)
    b = gpu_train(X16.astype(np.float32), M, C, 6, rows=rows)
    for x, y in zip(a, b):
        assert x.tobytes() == y.tobytes()


def test_repeatable_and_independent_of_workspace_contents():
    import ctypes
    import torch
    from million_amd import _lib, train
    n, d, M, C = 9000, 32, 16, 256
    rs = np.random.RandomState(11)
    X = mixture(rs, n, d)
    rows = rs.permutation(n)[:C]
    a = gpu_train(X, M, C, 8, rows=rows)
    b = gpu_train(X, M, C, 8, rows=rows)
    need = _lib.load().million_pq_train_workspace_bytes(ctypes.byref(train._desc(n, d, M, C, 8, True, d)))
    assert need == train.workspace_bytes(n, d, M, C)
    ws = torch.full((need,), 0xFF, dtype=torch.uint8, device="cuda")
    c = gpu_train(X, M, C, 8, rows=rows, workspace=ws)
    for x, y, z in zip(a, b, c):
        assert x.tobytes() == y.tobytes() == z.tobytes()


def test_captured_graph_replays_the_same_bits():
    import torch
    from million_amd import train
    n, d, M, C, niter = 6000, 64, 32, 128, 5
    rs = np.random.RandomState(13)
    X = torch.from_numpy(mixture(rs, n, d)).cuda()
    rows = torch.from_numpy(rs.permutation(n)[:C].astype(np.int32)).cuda()
    want = [t.clone() for t in train.kmeans_pq(X, M, C, niter, init_rows=rows)]
    torch.cuda.synchronize()
    ws = torch.empty(train.workspace_bytes(n, d, M, C), dtype=torch.uint8, device="cuda")
    out = torch.zeros(M, C, d // M, dtype=torch.float32, device="cuda")
    counts = torch.zeros(M, C, dtype=torch.int32, device="cuda")
    obj = torch.zeros(niter, dtype=torch.float64, device="cuda")
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        train.kmeans_pq(X, M, C, niter, init_rows=rows, workspace=ws, out=out, counts=counts, objective=obj)
    for _ in range(2):
        out.zero_(); counts.zero_(); obj.zero_()
        g.replay()
        torch.cuda.synchronize()
        for got, w in zip((out, counts, obj), want):
            assert got.cpu().numpy().tobytes() == w.cpu().numpy().tobytes()


def test_forced_splits_are_bitwise_and_leave_no_empty_cluster(oracle):
    """Fewer distinct rows than centroids: duplicate initial centroids tie, the lowest index takes every point, the others
    are empty and go through the split rule - on every iteration."""
    rs = np.random.RandomState(17)
    n, d, M, C = 700, 16, 4, 16
    distinct = rs.standard_normal((10, d)).astype(np.float32)
    X = distinct[np.arange(n) % 10]
    rows = np.arange(C)                                       # rows 10..15 repeat rows 0..5
    for niter in (1, 6):
        cents0 = R.init_from_rows(X, M, rows)
        want = R.lloyd(X, cents0, niter)
        codes, _ = R.assign(X, cents0)
        assert len(np.unique(codes[:, 0])) < C                # the first update does meet empty clusters
        got = gpu_train(X, M, C, niter, rows=rows)
        assert_same(got, want, f"forced splits, {niter} iterations")
        assert (got[1] > 0).all() and (got[1].sum(axis=1) == n).all()


def test_pipeline_train_save_load_encode_decode_attend(tmp_path, oracle):
    import torch
    from million_amd import formats, ops, train
    from million_amd.pq_cache import PagedPQCache
    O = oracle
    rs = np.random.RandomState(23)
    d, M, nbits, n = 128, 64, 8, 8192
    C = 2 ** nbits
    Xk, Xv = mixture(rs, n, d), mixture(rs, n, d)
    seed = 1234
    ck, stats = train.train_pq(Xk, M, nbits, niter=10, seed=seed, return_stats=True)      # numpy in, CPU tensor out (the reference's types)
    cv = train.train_pq(torch.from_numpy(Xv).cuda(), M, nbits, niter=10, seed=seed)       # device tensor in and out
    assert ck.dtype == torch.float32 and tuple(ck.shape) == (M, C, d // M) and not ck.is_cuda and cv.is_cuda
    assert len(stats["objective"]) == 10 and stats["objective"][-1] < stats["objective"][0]
    assert int(stats["counts"].sum()) == n * M
    formats.save_centroids(tmp_path, ck, cv, nbits)
    lk, lv = formats.load_centroids(tmp_path, M, nbits, d=d, device="cuda")
    assert torch.equal(lk.cpu(), ck.half()) and torch.equal(lv.cpu(), cv.cpu().half())

    # reconstruction error of the trained codebook < that of the codebook it started from (the same seeded rows)
    gen = torch.Generator(device="cpu")
    gen.manual_seed(seed)
    rows = torch.randperm(n, generator=gen)[:C].numpy()
    X16 = torch.from_numpy(Xk).cuda().half()[None, None]

    def recon_err(cents16):
        codes = ops.pq_encode(X16, cents16)
        rec = ops.pq_decode(codes, cents16)
        return float(((rec.float() - X16.float()) ** 2).sum())

    e_init = recon_err(torch.from_numpy(R.init_from_rows(Xk, M, rows)).cuda().half())
    e_trained = recon_err(lk)
    print(f"reconstruction error: initial rows {e_init:.6g}, trained {e_trained:.6g}")
    assert e_trained < e_init

    # one decode step of PagedPQCache on the trained tables, against the oracle (the bar of smoke(): rel-L2 < 1e-3)
    bs, nh, nhk, ps, n_prompt = 1, 8, 2, 64, 200
    K = mixture(rs, bs * nhk * (n_prompt + 1), d).reshape(bs, nhk, n_prompt + 1, d).astype(np.float16)
    V = mixture(rs, bs * nhk * (n_prompt + 1), d).reshape(bs, nhk, n_prompt + 1, d).astype(np.float16)
    Q = rs.standard_normal((bs, nh, 1, d)).astype(np.float16)
    dev = torch.device("cuda", torch.cuda.current_device())
    cache = PagedPQCache(bs=bs, nh=nh, num_key_value_heads=nhk, M=M, layer_num=1, d=d, page_size=ps,
                         extended_residual_size=128, max_tokens=1024, device=dev)
    cache.set_cent(lk, lv)
    Kd, Vd, Qd = torch.from_numpy(K).to(dev), torch.from_numpy(V).to(dev), torch.from_numpy(Q).to(dev)
    cache.prefill(Qd.expand(-1, -1, 1, -1).repeat(1, 1, n_prompt, 1), Kd[:, :, :n_prompt].contiguous(),
                  Vd[:, :, :n_prompt].contiguous(), 0)
    out = cache.decoding_with_pages(Qd, Kd[:, :, n_prompt:].contiguous(), Vd[:, :, n_prompt:].contiguous(), 0)
    T, r = O.PagedPolicy(page_size=ps, residual=128, prefill=n_prompt).step()
    assert (cache._T[0], cache.residualed_tokens[0]) == (T, r)
    ck16, cv16 = lk.cpu().numpy(), lv.cpu().numpy()
    kres = np.zeros((bs, nhk, 128, d), np.float16)
    vres = np.zeros((bs, nhk, 128, d), np.float16)
    kres[:, :, :r], vres[:, :, :r] = K[:, :, T:T + r], V[:, :, T:T + r]
    gold = O.decode_attn(Q, O.pq_encode(K[:, :, :T], ck16), O.pq_encode(V[:, :, :T], cv16), ck16, cv16, kres, vres, r)
    o = out.float().cpu().numpy().astype(np.float64)
    rel = np.linalg.norm(o - gold) / np.linalg.norm(gold)
    print(f"decode step on trained tables: rel-L2 {rel:.2e}")
    assert rel < 1e-3


def test_cli_writes_files_that_load_unchanged(tmp_path):
    """tools/train_codebooks.py: .fvecs samples in, the reference's two .pq.pt files out; they load as set_cent wants them."""
    import importlib.util
    import torch
    from million_amd import formats, train
    spec = importlib.util.spec_from_file_location("train_codebooks", formats.Path(__file__).resolve().parents[1] / "tools" / "train_codebooks.py")
    cli = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(cli)
    rs = np.random.RandomState(29)
    d, M, nbits = 32, 8, 6
    Xk, Xv = mixture(rs, 3000, d), mixture(rs, 2500, d)
    formats.write_fvecs(tmp_path / "k.fvecs", Xk, mode="wb")
    formats.write_fvecs(tmp_path / "v.fvecs", Xv, mode="wb")
    out = tmp_path / "cents"
    assert cli.main(["--keys", str(tmp_path / "k.fvecs"), "--values", str(tmp_path / "v.fvecs"), "--out", str(out),
                     "--M", str(M), "--nbits", str(nbits), "--niter", "4", "--seed", "99"]) == 0
    kp, vp = formats.centroid_paths(out, M, nbits)
    assert kp.exists() and vp.exists()
    raw = torch.load(kp, map_location="cpu", weights_only=True)
    assert raw.dtype == torch.float32 and tuple(raw.shape) == (M, 2 ** nbits, d // M)
    assert torch.equal(raw, train.train_pq(Xk, M, nbits, 4, seed=99))          # the file holds what train_pq returns
    lk, lv = formats.load_centroids(out, M, nbits, d=d, device="cuda")
    assert lk.dtype == torch.float16 and lk.is_cuda and tuple(lv.shape) == (M, 2 ** nbits, d // M)
