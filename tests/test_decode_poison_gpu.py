"""GPU side of the poisoned-memory matrix (tests/decode_poison.py): million_pq_decode_attn / _append on memory where every byte
outside the live data is 0xFF (codes, unused pages, the pages page-table entries past the context name) or NaN (window rows
outside the ring's span, out).  Each call matches the fp64 oracle on clean memory and gives the same bits on poisoned memory.

test_lds_poison_child runs the C = 128 rows and the chunk kernel's poisoned cases against the diagnostic library, whose kernels
fill their whole LDS allocation with 0xFFFF (fp16 NaN) before their first LDS write: a read of LDS the kernel never wrote is
then a NaN every time, not whatever an earlier workgroup left there."""
import json
import os
import subprocess
import sys
from pathlib import Path

import pytest

from tests import decode_poison as P

pytestmark = pytest.mark.gpu

ROOT = Path(__file__).resolve().parents[1]


@pytest.fixture(scope="module")
def env():
    import torch
    assert torch.cuda.is_available(), "GPU tests need an MI355X"
    from million_amd import ops, _lib
    return torch, ops, _lib.load(), _lib


@pytest.mark.parametrize("case", P.CASES, ids=[c.name for c in P.CASES])
def test_decode_attn_poisoned_memory(case, env, oracle):
    torch, ops, lib, L = env
    P.check_case(case, torch, ops, lib, L, oracle)


def test_lds_poison_child():
    """The C = 128 rows of the matrix and the four test_chunk_attn_total cases, in a child process on
    libmillion_hip_dbgids.so (one library per process)."""
    dbg = ROOT / "million_amd" / "libmillion_hip_dbgids.so"
    if not dbg.exists():
        pytest.skip("million_amd/libmillion_hip_dbgids.so not built (make debug-ids)")
    env_ = dict(os.environ, MILLION_HIP_LIB=str(dbg))
    r = subprocess.run([sys.executable, str(ROOT / "tests" / "lds_poison_child.py")], env=env_, capture_output=True, text=True,
                       timeout=600)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-4000:]
    res = json.loads(r.stdout.strip().splitlines()[-1])
    assert res["lib"] == dbg.name
    assert res["bad_ids_before"] == 0 and res["bad_ids_after"] == 0
    failed = {c["name"]: c["error"] for c in res["cases"] if c["error"]}
    assert not failed, failed
    assert len(res["cases"]) == len([c for c in P.CASES if c.C == 128]) + 4
