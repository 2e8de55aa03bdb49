"""Child process of test_ragged_lds_poison_child: runs with MILLION_HIP_LIB pointing at the -DMILLION_DEBUG_CHECK_IDS build of
the library (million_amd/libmillion_hip_dbgids.so), whose chunk kernels - the ragged instances included - fill their whole LDS
allocation with 0xFFFF (fp16 NaN) before their first LDS write.  A ragged instance that gathers from LDS it never wrote (a
codebook it did not stage, a tile row its producer skipped) then reads NaN on every run.

Runs the cases of test_ragged_parity_and_totality on poisoned memory against the fp64 model and prints one JSON line: per case
the first failed assertion, or null."""
from __future__ import annotations

import json
import sys
import traceback
from pathlib import Path

ROOT = Path(__file__).resolve().parents[1]
sys.path.insert(0, str(ROOT))


def main():
    import torch
    from million_amd import _lib, ops
    from oracle import oracle as O
    from tests import test_chunk_ragged_gpu as R

    _lib.load()
    O.build()
    res = {"lib": str(_lib.LIB_PATH.name), "cases": []}
    for name, (d, M, C, G, n_q, bound, rows, chunk, ps, i64) in R.RAGGED.items():
        err = None
        try:
            sc = R.Scene(len(name), d, M, C, G, n_q, bound, rows, chunk, ps=ps, i64=i64)
            sc.check(O, sc.run_ragged(torch, ops, O, poison=True), what=name)
        except AssertionError as e:
            err = str(e)[:400]
        except Exception:
            err = traceback.format_exc(limit=2)[-400:]
        res["cases"].append({"name": name, "error": err})
    print(json.dumps(res))


if __name__ == "__main__":
    main()
