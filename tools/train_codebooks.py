#!/usr/bin/env python3
"""Train the key and value PQ codebooks from sampled vectors, on the GPU.

  python tools/train_codebooks.py --keys key_samples.fvecs --values value_samples.fvecs --out centroids/<model>/<dataset> \\
      --M 64 --nbits 8 [--niter 25] [--seed 1234] [--max-points-per-centroid 256]

Reads the two `.fvecs` sample files (the reference's sampler writes them, scripts/utils/fvecio.py:35-43), runs
`million_amd.train.train_pq` on each and writes `key_cent_{M}_{nbits}.pq.pt` / `val_cent_{M}_{nbits}.pq.pt` through
`formats.save_centroids` - the files `formats.load_centroids` and the reference's main_pq.py:257-260 read.  This is the
reference's training stage (main_pq.py:222-237 around pq_utils.py:586-609) without faiss."""
import argparse
import sys
import time
from pathlib import Path

sys.path.insert(0, str(Path(__file__).resolve().parents[1]))


def main(argv=None) -> int:
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--keys", required=True, help=".fvecs file of sampled key vectors")
    ap.add_argument("--values", required=True, help=".fvecs file of sampled value vectors")
    ap.add_argument("--out", required=True, help="directory the two .pq.pt files are written to")
    ap.add_argument("--M", type=int, required=True, help="subspaces")
    ap.add_argument("--nbits", type=int, default=8, help="bits per code: 2**nbits centroids per subspace")
    ap.add_argument("--niter", type=int, default=25)
    ap.add_argument("--seed", type=int, default=1234)
    ap.add_argument("--max-points-per-centroid", type=int, default=256)
    args = ap.parse_args(argv)

    import torch
    from million_amd import formats, train

    cents = {}
    for side, path in (("key", args.keys), ("value", args.values)):
        X = formats.read_fvecs(path)
        if X.size == 0:
            raise SystemExit(f"{path}: no vectors")
        t0 = time.perf_counter()
        c, stats = train.train_pq(X, args.M, args.nbits, args.niter, seed=args.seed,
                                  max_points_per_centroid=args.max_points_per_centroid, return_stats=True)
        torch.cuda.synchronize()
        obj = stats["objective"]
        print(f"{side}: {X.shape[0]} vectors of d={X.shape[1]} ({stats['n_train']} used), {args.niter} iterations in "
              f"{time.perf_counter() - t0:.2f} s, objective {obj[0]:.6g} -> {obj[-1]:.6g}, "
              f"smallest cluster {int(stats['counts'].min())} points")
        cents[side] = c
    kp, vp = formats.save_centroids(args.out, cents["key"], cents["value"], args.nbits)
    print(f"wrote {kp}\nwrote {vp}")
    return 0


if __name__ == "__main__":
    sys.exit(main())
