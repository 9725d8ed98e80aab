"""Nearest-correlation projection of indefinite skeptic matrices: the device route (rank_step on the FP64 matrix cores +
k_nc_update) against the numpy twin with ``numpy.linalg.eigh`` in the loop, at the size of profiles/nearest_correlation.txt.

    python tools/bench_nearcorr.py [--shape p,N,B,b] [--calls 5] [--part single,subsets] [--kernel-only]

The inputs are skeptic matrices of rounded data (ties) with p > N, so they are indefinite.  Two workloads, one JSON line each
(whole-call times from the matrices on the host to the projections on the host; the two routes alternate, --calls rounds after
one warm-up round, reported as median, min and max):

* single    the matrix of all N observations.
* subsets   the B subsample matrices of StARS, b observations each, one (B,p,p) stack in lock-step.

Routes: ``device`` = ``utils.nearest_correlation``, ``host`` = ``utils.host_nearest_correlation`` (per matrix, one after the
other).  Reported beside the times: iterations per matrix on both routes, the L-step's eigendecomposition fallbacks over a
device call, max |device - host| and the smallest eigenvalue of the device result.

``--kernel-only`` makes --calls device calls of each workload and nothing else, for a run under ``rocprofv3 --kernel-trace
--stats``: the share of k_nc_update, and the product launches per rank_step (launches of the product kernels over
calls x iterations), are read off its table."""
import argparse
import json
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from tools.bench_stars import alternate_ms      # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--shape", default="500,300,20,240", help="p,N,B,b")
    ap.add_argument("--calls", type=int, default=5)
    ap.add_argument("--part", default="single,subsets")
    ap.add_argument("--kernel-only", action="store_true", help="only device calls (for a profiler run)")
    args = ap.parse_args()
    from gglasso_amd import model_selection as ms, utils
    p, N, B, b = (int(v) for v in args.shape.split(","))
    X = np.round(np.random.default_rng(0).standard_normal((p, N)), 1)
    idx = ms.stars_subsamples(N, B, b)
    work = {"single": utils.skeptic_correlation(X)[None], "subsets": utils.skeptic_correlation(X, idx)}
    for part in args.part.split(","):
        S = work[part]
        shape = {"part": part, "p": p, "N": N, "B": S.shape[0], "b": N if part == "single" else b, "calls": args.calls,
                 "lambda_min_in": float(min(np.linalg.eigvalsh(s).min() for s in S))}
        if args.kernel_only:
            for _ in range(args.calls):
                _, info = utils.nearest_correlation(S, return_info=True)
            print(json.dumps({**shape, "kernel_only": True, "iterations": info["iterations"].tolist(),
                              "fallbacks": info["fallbacks"]}), flush=True)
            continue
        got = {}

        def device():
            got["dev"] = utils.nearest_correlation(S, return_info=True)

        def host():
            got["host"] = utils.host_nearest_correlation(S, return_info=True)

        dev_ms, host_ms = alternate_ms([device, host], args.calls)
        (out, info), (ref, rinfo) = got["dev"], got["host"]
        print(json.dumps({**shape, "device_ms": dev_ms, "host_ms": host_ms,
                          "iterations_device": info["iterations"].tolist(), "iterations_host": rinfo["iterations"].tolist(),
                          "converged": bool(info["converged"].all()), "fallbacks": info["fallbacks"],
                          "shrink_max": float(info["shrink"].max()),
                          "max_abs_device_minus_host": float(np.abs(out - ref).max()),
                          "lambda_min_out": float(min(np.linalg.eigvalsh(o).min() for o in out))}), flush=True)


if __name__ == "__main__":
    main()
