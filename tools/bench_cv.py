"""K-fold cross-validation of lambda1: the device route against the route without the held-out-score entry point, at the
size of profiles/cross_validation.txt.

    python tools/bench_cv.py [--shape p,N,F,L] [--calls 5] [--part score,search] [--kernel-only]

Two comparisons, one JSON line each (whole-call times; the routes of a comparison alternate, --calls rounds after one
warm-up round, reported as median, min and max):

* score   the scoring step of K = L * F snapshots: ``HipEngine.heldout_scores`` (4 K numbers come back) against the download
          of the Theta stack (``ggl_get_snapshots``) + the numpy inner product with the test covariances, the log dets from
          ``HipEngine.selection_stats`` on that side too.  ``bytes`` is what the kernel has to read from HBM, K p^2 doubles.
* search  the whole ``model_selection.cv_search`` against the same search with ``heldout_scores`` replaced by that
          download route.

The kernel's own time comes from running this tool with ``--kernel-only`` (snapshots planted once, then --calls calls of
heldout_scores, nothing else) under ``rocprofv3 --kernel-trace --stats``: the average of k_heldout_dot over bytes gives its
share of the HBM peak (8 TB/s)."""
import argparse
import json
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

from bench_stars import alternate_ms, make_problem      # noqa: E402

HBM_PEAK = 8.0e12      # bytes / s


def planted_engine(p, K, seed=1):
    """An engine whose K snapshots are sparse, symmetric and diagonally dominant (positive definite: finite log dets)."""
    from gglasso_amd.solver import HipEngine
    rng = np.random.default_rng(seed)
    T = np.triu(rng.standard_normal((K, p, p)) * (rng.random((K, p, p)) < 0.05), 1)
    T = T + T.transpose(0, 2, 1)
    T[:, np.arange(p), np.arange(p)] = np.abs(T).sum(axis=2) + 1.0
    eye = np.broadcast_to(np.eye(p), (K, p, p))
    eng = HipEngine(eye, eye, eye, 0 * eye)
    eng.set_state(np.ascontiguousarray(eye), T, np.zeros((K, p, p)))
    for k in range(K):
        eng.snapshot_k(k)
    return eng, T


def download_scores(eng, X, test, center=True, out=None):
    """``HipEngine.heldout_scores`` without the entry point: every Theta comes down, numpy forms the inner products."""
    from gglasso_amd import utils
    S_test = utils.sample_covariance_subsets(X, test, center=center)
    Th = eng.snapshots(names=('Theta',))['Theta']
    F = S_test.shape[0]
    st = eng.selection_stats()
    st[:, 0] = np.einsum('lfij,fij->lf', Th.reshape(-1, F, *Th.shape[1:]), S_test).reshape(-1)
    return st


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--shape", default="500,2000,5,10", help="p,N,F,L")
    ap.add_argument("--calls", type=int, default=5)
    ap.add_argument("--part", default="score,search")
    ap.add_argument("--kernel-only", action="store_true", help="only device calls of heldout_scores (for a profiler run)")
    args = ap.parse_args()
    import contextlib
    import io
    from gglasso_amd import model_selection as ms
    from gglasso_amd.solver import HipEngine
    p, N, F, L = (int(v) for v in args.shape.split(","))
    X = make_problem(p, N)
    train, test = ms.cv_folds(N, F)
    lam = np.geomspace(0.6, 0.15, L)
    K = L * F
    shape = {"p": p, "N": N, "F": F, "m": int(test.shape[1]), "L": L, "K": K, "calls": args.calls}
    parts = args.part.split(",")
    theta_bytes = 8.0 * K * p * p

    if args.kernel_only:
        eng, _ = planted_engine(p, K)
        try:
            for _ in range(args.calls):
                eng.heldout_scores(X, test)
        finally:
            eng.close()
        print(json.dumps({**shape, "kernel_only": True, "bytes": theta_bytes}), flush=True)
        return

    if "score" in parts:
        eng, T = planted_engine(p, K)
        try:
            dev, host = eng.heldout_scores(X, test), download_scores(eng, X, test)
            scale = np.abs(host[:, 0]).max()
            dev_ms, host_ms = alternate_ms([lambda: eng.heldout_scores(X, test), lambda: download_scores(eng, X, test)],
                                           args.calls)
        finally:
            eng.close()
        print(json.dumps({**shape, "part": "score", "bytes": theta_bytes, "same_stats_bits": bool(np.array_equal(dev[:, 1:], host[:, 1:])),
                          "max_rel_diff_inner": float(np.abs(dev[:, 0] - host[:, 0]).max() / scale),
                          "device_call_ms": dev_ms, "download_numpy_ms": host_ms}), flush=True)

    if "search" in parts:
        out = {}
        real = HipEngine.heldout_scores

        def device():
            with contextlib.redirect_stdout(io.StringIO()):
                out["dev"] = ms.cv_search(X, lam, folds=(train, test))

        def host():
            HipEngine.heldout_scores = download_scores
            try:
                with contextlib.redirect_stdout(io.StringIO()):
                    out["host"] = ms.cv_search(X, lam, folds=(train, test))
            finally:
                HipEngine.heldout_scores = real

        dev_ms, host_ms = alternate_ms([device, host], args.calls)
        (sol, st), (sol_h, st_h) = out["dev"], out["host"]
        print(json.dumps({**shape, "part": "search", "device_route_ms": dev_ms, "download_route_ms": host_ms,
                          "same_IX": st["IX"] == st_h["IX"],
                          "max_abs_diff_NLL": float(np.abs(st["NLL"] - st_h["NLL"]).max()),
                          "same_solution_bits": bool(np.array_equal(sol["Theta"], sol_h["Theta"])),
                          "IX": st["IX"], "lambda1": float(st["BEST"]["lambda1"]), "CV": [float(v) for v in st["CV"]],
                          "FAILED": st["FAILED"], "NOT_PD": st["NOT_PD"]}), flush=True)


if __name__ == "__main__":
    main()
