"""CPU tests of PQ codebook training: the numpy restatement of the contract (tests/kmeans_ref.py) behaves like Lloyd's
k-means, and the C ABI of million_pq_train validates its descriptor before any launch."""
import ctypes
import subprocess
import tempfile
from pathlib import Path

import numpy as np
import pytest

from tests import kmeans_ref as R

ROOT = Path(__file__).resolve().parents[1]


@pytest.fixture(scope="module")
def lib():
    from million_amd import build, _lib
    build.build()
    return _lib.load()


def planted(rs, n_per, M, C, dm, spread=0.01):
    """Well-separated clusters: in every subspace centre c sits at 10 * c in every dim; row i belongs to centre i % C."""
    n = n_per * C
    centres = np.broadcast_to((10.0 * np.arange(C, dtype=np.float32))[None, :, None], (M, C, dm)).copy()
    centres += rs.uniform(-1, 1, size=centres.shape).astype(np.float32)
    label = np.arange(n) % C
    X = centres[:, label, :].transpose(1, 0, 2).reshape(n, M * dm) + spread * rs.standard_normal((n, M * dm)).astype(np.float32)
    return X.astype(np.float32), centres, label


def test_restatement_recovers_planted_centres(oracle):
    rs = np.random.RandomState(0)
    M, C, dm = 3, 8, 2
    X, centres, label = planted(rs, 40, M, C, dm)
    cents0 = R.init_from_rows(X, M, np.arange(C))            # rows 0..C-1: one point of every planted cluster
    cents, counts, objs = R.lloyd(X, cents0, 5)
    assert cents.dtype == np.float32 and cents.shape == (M, C, dm)
    assert np.abs(cents - centres).max() < 0.02              # ~ spread / sqrt(40) per coordinate
    assert (counts == 40).all()
    codes, _ = R.assign(X, cents)
    assert (codes == label[:, None]).all()


def test_restatement_objective_never_increases(oracle):
    rs = np.random.RandomState(1)
    X = rs.standard_normal((3000, 16)).astype(np.float32)
    M, C = 4, 32
    cents0 = R.init_from_rows(X, M, rs.permutation(3000)[:C])
    _, counts, objs = R.lloyd(X, cents0, 12)
    assert len(objs) == 12
    # Lloyd's monotonicity holds in exact arithmetic; fp32 means may move the fp64 sum by rounding only
    for a, b in zip(objs, objs[1:]):
        assert b <= a * (1 + 1e-6), objs
    assert objs[-1] < 0.8 * objs[0]
    assert counts.sum(axis=1).tolist() == [3000] * M


def test_split_rule_on_a_hand_made_case():
    cents = np.array([[[1.0, 2.0, 3.0, 4.0], [9.0, 9.0, 9.0, 9.0], [5.0, 6.0, 7.0, 8.0], [0.5, 0.5, 0.5, 0.5]]], dtype=np.float32)
    counts = np.array([[7, 0, 7, 0]], dtype=np.int32)
    n = R.split(cents, counts)
    hi, lo = np.float32(1 + 1 / 1024), np.float32(1 - 1 / 1024)
    # c = 1: donors 0 and 2 tie at 7, the lowest index gives: 7 -> 4 + 3.  c = 3: cluster 2 (7) is now the largest: 7 -> 4 + 3.
    assert n == 2
    assert counts.tolist() == [[4, 3, 4, 3]]
    v0 = np.array([1.0, 2.0, 3.0, 4.0], dtype=np.float32)
    v2 = np.array([5.0, 6.0, 7.0, 8.0], dtype=np.float32)
    pat_new = np.array([hi, lo, hi, lo], dtype=np.float32)
    pat_old = np.array([lo, hi, lo, hi], dtype=np.float32)
    assert np.array_equal(cents[0, 1], v0 * pat_new) and np.array_equal(cents[0, 0], v0 * pat_old)
    assert np.array_equal(cents[0, 3], v2 * pat_new) and np.array_equal(cents[0, 2], v2 * pat_old)


def test_train_symbols_exported(lib):
    from million_amd import _lib
    for name in ("million_pq_train", "million_pq_train_workspace_bytes"):
        assert name in _lib.SYMBOLS and hasattr(lib, name)
    hdr = (ROOT / "include" / "million_hip.h").read_text()
    assert "million_train_desc" in hdr and "#define MILLION_HIP_VERSION 1" in hdr


def test_train_desc_size_matches_header(lib):
    from million_amd import _lib
    src = '#include "million_hip.h"\n#include <stdio.h>\n#include <stddef.h>\nint main(){printf("%zu %zu %zu\\n", sizeof(million_train_desc), offsetof(million_train_desc, x_stride_n), offsetof(million_train_desc, eps));return 0;}\n'
    with tempfile.TemporaryDirectory() as td:
        (Path(td) / "a.c").write_text(src)
        subprocess.check_call(["gcc", "-std=c11", "-I", str(ROOT / "include"), "-o", f"{td}/a", f"{td}/a.c"])
        size, off_stride, off_eps = map(int, subprocess.check_output([f"{td}/a"]).split())
    assert size == ctypes.sizeof(_lib.TrainDesc)
    assert off_stride == _lib.TrainDesc.x_stride_n.offset and off_eps == _lib.TrainDesc.eps.offset


def test_workspace_formula(lib):
    from million_amd import train
    for n, d, M, C in ((8192, 128, 64, 256), (65536, 128, 64, 256), (1000, 8, 8, 16), (4097, 24, 6, 1024), (300, 32, 4, 2),
                       (5000, 10, 10, 4096)):
        desc = train._desc(n, d, M, C, 3, True, d)
        got = lib.million_pq_train_workspace_bytes(ctypes.byref(desc))
        assert got == train.workspace_bytes(n, d, M, C) and got > 0, (n, d, M, C)
    # N = 65536, M = 64, C = 256, d_m = 2: 4 MiB of codes + 16 chunks x 64 x 256 x 3 words + 4096 partials of the objective
    assert train.workspace_bytes(65536, 128, 64, 256) == 64 * 65536 + 16 * 64 * 256 * 3 * 4 + 4096 * 8


def test_bad_descriptors_are_refused_without_a_launch(lib):
    from million_amd import train
    fake = 0x1000      # never dereferenced: every case below fails in the host checks

    def call(desc, init_rows=fake, cents_init=None, ws=fake):
        return lib.million_pq_train(ctypes.byref(desc), fake, init_rows, cents_init, fake, None, None, ws, 1 << 40, None)

    err = lambda: lib.million_last_error().decode()
    d = train._desc(100, 16, 4, 256, 3, True, 16)                  # N < C
    assert call(d) == -1 and "n=100" in err() and "C=256" in err()
    assert lib.million_pq_train_workspace_bytes(ctypes.byref(d)) == 0
    d = train._desc(1000, 18, 4, 16, 3, True, 18)                  # d % M != 0
    assert call(d) == -1 and "d=18" in err() and "M=4" in err()
    d = train._desc(1000, 64, 4, 16, 3, True, 64)                  # d_m = 16
    assert call(d) == -1 and "d/M=16" in err()
    for C in (1, 8192):
        d = train._desc(10000, 16, 4, C, 3, True, 16)
        assert call(d) == -1 and f"C={C}" in err()
    d = train._desc(1 << 24, 16, 4, 16, 3, True, 16)               # counts would no longer be exact in fp32
    assert call(d) == -1 and "2^24" in err()
    good = train._desc(1000, 16, 4, 16, 3, True, 16)
    assert call(good, init_rows=fake, cents_init=fake) == -3 and "exactly one" in err()
    assert call(good, init_rows=None, cents_init=None) == -3 and "exactly one" in err()
    d = train._desc(1000, 16, 4, 16, 0, True, 16)
    assert call(d) == -3 and "niter=0" in err()
    d = train._desc(1000, 16, 4, 16, 3, True, 16)
    d.struct_size = 5
    assert call(d) == -3 and "struct_size" in err()
    rc = lib.million_pq_train(ctypes.byref(good), fake, fake, None, fake, None, None, fake * 256, 16, None)
    assert rc == -4 and "workspace" in err()                       # too small
    rc = lib.million_pq_train(ctypes.byref(good), fake + 4, fake, None, fake, None, None, fake, 1 << 40, None)
    assert rc == -2                                                # x not aligned to a d_m = 4 fp32 sub-vector


def test_train_pq_refuses_cpu_tensors():
    import torch
    from million_amd import train
    with pytest.raises(RuntimeError):
        train.train_pq(torch.zeros(512, 16), 4, 4)
    with pytest.raises(RuntimeError):
        train.kmeans_pq(torch.zeros(512, 16), 4, 16, 1, init_rows=torch.zeros(16, dtype=torch.int32))


def test_new_kernels_have_no_scratch_and_no_spills(lib):
    """The project's kernel-metadata check (tools/kernel_meta.py) on the training kernels."""
    import sys
    out = subprocess.run([sys.executable, str(ROOT / "tools" / "kernel_meta.py"), str(ROOT / "million_amd" / "libmillion_hip.so"), "kmeans_"],
                         capture_output=True, text=True, check=True).stdout
    rows = [l for l in out.splitlines() if "kmeans_" in l]
    assert len(rows) == 16 + 16 + 2 + 1, out                      # assign, update: d_m x dtype x code width; gather; finish
    for l in rows:
        assert l.rstrip().endswith("vgpr_spill 0 sgpr_spill 0 scratch 0 B"), l
