"""Child process of test_lds_poison_child: runs with MILLION_HIP_LIB pointing at the -DMILLION_DEBUG_CHECK_IDS build of the
library (million_amd/libmillion_hip_dbgids.so), whose decode-attention and chunk kernels fill their whole LDS allocation with
0xFFFF (fp16 NaN) before their first LDS write.  A kernel that gathers from LDS it never wrote then reads NaN on every run.

Runs the C = 128 rows of the poisoned-memory matrix (tests/decode_poison.py, every assertion of check_case) and the four cases
of test_chunk_attn_total, and prints one JSON line: per case the first failed assertion, or null."""
from __future__ import annotations

import json
import sys
import traceback
from pathlib import Path

import numpy as np

ROOT = Path(__file__).resolve().parents[1]
sys.path.insert(0, str(ROOT))

CHUNK_TOTAL = [(128, 64, 128, "paged"), (128, 32, 256, "rowmajor"), (64, 64, 128, "rowmajor"), (64, 16, 256, "paged")]


def main():
    import torch
    from million_amd import _lib, ops
    from oracle import oracle as O
    from tests import decode_poison as P
    from tests import test_chunk_attn_gpu as CA

    lib = _lib.load()
    res = {"lib": str(_lib.LIB_PATH.name), "bad_ids_before": int(lib.million_debug_bad_page_ids()), "cases": []}
    O.build()
    for c in [c for c in P.CASES if c.C == 128]:
        err = None
        try:
            P.check_case(c, torch, ops, lib, _lib, O)
        except AssertionError as e:
            err = str(e)[:400]
        except Exception:
            err = traceback.format_exc(limit=2)[-400:]
        res["cases"].append({"name": c.name, "error": err})
    for d, M, C, layout in CHUNK_TOTAL:      # test_chunk_attn_total
        err = None
        try:
            st = CA._state(np.random.RandomState(11), 2, 8, 2, d, M, C, 33, 1000, 40, 64, 50, True)
            out = CA._run(torch, ops, O, st, M, C, layout, 64, False, poison=True)
            gold = CA.model(O, st["q"], st["k_codes"], st["v_codes"], st["k_cents"], st["v_cents"], st["k_win"], st["v_win"],
                            st["k_ch"], st["v_ch"])
            CA._check(out, gold, "total")
        except AssertionError as e:
            err = str(e)[:400]
        except Exception:
            err = traceback.format_exc(limit=2)[-400:]
        res["cases"].append({"name": f"chunk-total-{d}-{M}-{C}-{layout}", "error": err})
    res["bad_ids_after"] = int(lib.million_debug_bad_page_ids())
    print(json.dumps(res))


if __name__ == "__main__":
    main()
