"""ggl_covariance (centred) against numpy.cov(bias=True) on the host, at the sizes of profiles/covariance_gram.txt.

    python tools/bench_covariance.py [--shape K,p,N ...] [--calls 5] [--device-only]

Whole-call time of the device route (allocation, upload, row means, Gram kernel, download of S): median of --calls after one
warm-up call, and the same for numpy.cov.  One JSON line per shape.  The kernels' own times come from running this tool with
--device-only for ONE shape under ``rocprofv3 --kernel-trace --stats``: the averages of k_row_means and k_gram_nt in the
kernel statistics are the device time with upload and download excluded, and p (p+1) N / t(k_gram_nt) is the Gram kernel's
useful rate (the flop of the tile pairs I <= J, as the symmetric product kernel's 36.7 TF/s at p = 500 is counted)."""
import argparse
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

SHAPES = ["1,1000,2000", "32,500,1000", "1,4000,8000"]


def median_ms(fn, calls):
    fn()
    t = []
    for _ in range(calls):
        t0 = time.perf_counter()
        fn()
        t.append(1e3 * (time.perf_counter() - t0))
    return float(np.median(t))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--shape", action="append", help="K,p,N (repeatable); default the three recorded sizes")
    ap.add_argument("--calls", type=int, default=5)
    ap.add_argument("--device-only", action="store_true", help="skip numpy.cov (for a profiler run)")
    args = ap.parse_args()
    from gglasso_amd import _lib, utils
    for shape in args.shape or SHAPES:
        K, p, N = (int(v) for v in shape.split(","))
        rng = np.random.default_rng(0)
        Xs = [rng.standard_normal((p, N)) + rng.uniform(-10, 10, (p, 1)) for _ in range(K)]
        out = {"K": K, "p": p, "N": N, "calls": args.calls,
               "device_call_ms": median_ms(lambda: utils._covariance_call(Xs, _lib.COV_CENTER), args.calls)}
        out["whole_call_TFs"] = 2.0 * K * p * p * N / (out["device_call_ms"] * 1e9)
        if not args.device_only:
            out["numpy_cov_ms"] = median_ms(lambda: [np.cov(x, bias=True) for x in Xs], args.calls)
        print(json.dumps(out), flush=True)


if __name__ == "__main__":
    main()
