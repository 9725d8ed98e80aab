"""Pairwise-complete covariance (ggl_covariance_pairwise / _subsets) at p = 500, N = 2000 with 20 % missing: one matrix, and
B = 20 subsets of b = 447 columns (the StARS subsamples of that N), as recorded in profiles/pairwise_covariance.txt.

    python tools/bench_pairwise.py [--p 500] [--N 2000] [--B 20] [--b 447] [--missing 0.2] [--rounds 5] [--device-only]

Whole calls from host data to host matrix, every route once per round with the routes alternating, after one warm-up round:
median (min - max) of --rounds.

  pairwise   the device route: upload, row statistics, four-product Gram kernel, pair-count check, download of S and counts
  host       (a) utils.host_pairwise_covariance: numpy, the holes filled with zeros and four matmuls, on the host's threads
  complete   (b) utils.sample_covariance on the same array with the holes filled: the complete-data call, one product where the
             pairwise kernel runs four -- the floor it is measured against

(c) the kernels' own times: run this tool with --device-only under ``rocprofv3 --kernel-trace --stats`` and compare the
averages of k_gram_nt_pairwise and k_gram_nt in the kernel statistics.  One JSON line per workload."""
import argparse
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def rounds_ms(routes, rounds):
    """{name: [ms per round]}: one warm-up round, then every route once per round, in turn."""
    for fn in routes.values():
        fn()
    t = {name: [] for name in routes}
    for _ in range(rounds):
        for name, fn in routes.items():
            t0 = time.perf_counter()
            fn()
            t[name].append(1e3 * (time.perf_counter() - t0))
    return t


def summary(ms):
    return {"median_ms": float(np.median(ms)), "min_ms": float(np.min(ms)), "max_ms": float(np.max(ms))}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--p", type=int, default=500)
    ap.add_argument("--N", type=int, default=2000)
    ap.add_argument("--B", type=int, default=20)
    ap.add_argument("--b", type=int, default=447)
    ap.add_argument("--missing", type=float, default=0.2)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--device-only", action="store_true", help="skip the host route (for a profiler run)")
    args = ap.parse_args()
    from gglasso_amd import utils
    rng = np.random.default_rng(0)
    X = rng.standard_normal((args.p, args.N)) + rng.uniform(-10, 10, (args.p, 1))
    hole = rng.random(X.shape) < args.missing
    hole[:, :2] = False
    X[hole] = np.nan
    filled = np.where(hole, 0.0, X)
    idx = np.stack([np.sort(np.random.default_rng([1, r]).choice(args.N, args.b, replace=False)) for r in range(args.B)])
    idx[:, :2] = (0, 1)

    single = {"pairwise": lambda: utils.sample_covariance(X, missing='pairwise', return_counts=True),
              "complete": lambda: utils.sample_covariance(filled)}
    subsets = {"pairwise": lambda: utils.sample_covariance_subsets(X, idx, missing='pairwise', return_counts=True),
               "complete": lambda: utils.sample_covariance_subsets(filled, idx)}
    if not args.device_only:
        single["host"] = lambda: utils.host_pairwise_covariance(X, True)
        subsets["host"] = lambda: utils.host_pairwise_covariance(X, True, idx)
    for what, routes, K, n in (("single", single, 1, args.N), ("subsets", subsets, args.B, args.b)):
        out = {"workload": what, "K": K, "p": args.p, "N": n, "missing": args.missing, "rounds": args.rounds}
        for name, ms in rounds_ms(routes, args.rounds).items():
            out[name] = summary(ms)
        print(json.dumps(out), flush=True)


if __name__ == "__main__":
    main()
