"""The refit of neighbourhood selection and its cross-validation at the size of profiles/neighborhood_selection.txt.

    python tools/bench_mbrefit.py [--shape p,N,F,L] [--calls 5] [--part search,twin] [--twin-units 200] [--kernel-only]

One JSON line per part (whole-call times; the routes of a comparison alternate, --calls rounds after one warm-up round,
reported as median, min and max):

* search  ``model_selection.cv_search(method='mb')`` against ``cv_search`` for the graphical lasso on the same data, folds and
          grid (``scale=True``).  The two score different statistics (held-out prediction error of node-wise regressions
          against the held-out Gaussian likelihood); the line also carries both choices.
* twin    the refit step alone, ``utils.neighborhood_refit`` on the (F,L,p,p) stack of graphs of the train matrices (host
          buffers in and out, the transfers included), against the numpy twin's per-node routine given the same graphs.  The
          twin runs ``--twin-units`` (fold, lambda, node) units spread over the stack; the line carries that time, the count
          and the plain proportion to all units; that the twin scales so is not measured.

``--kernel-only``: the train matrices once, then --calls calls of ``HipEngine.neighborhood_cv`` and nothing else, for a run
under ``rocprofv3 --kernel-trace --stats``; the line carries the units per degree bin and the mean degree."""
import argparse
import contextlib
import io
import json
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from bench_stars import alternate_ms, make_problem      # noqa: E402  (tools/ is the script's directory)


def degree_bins(deg, status):
    return {"units": int(deg.size), "degree_mean": float(deg.mean()), "degree_max": int(deg.max()),
            "units_degree_0": int((deg == 0).sum()), "units_wave_bin_1_32": int(((deg >= 1) & (deg <= 32)).sum()),
            "units_workgroup_bin_33_128": int(((deg > 32) & (deg <= 128)).sum()), "units_above_cap": int((deg > 128).sum()),
            "status_counts": [int((status == s).sum()) for s in (0, 1, 2, 3)]}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--shape", default="500,2000,5,10", help="p,N,F,L")
    ap.add_argument("--calls", type=int, default=5)
    ap.add_argument("--part", default="search,twin")
    ap.add_argument("--twin-units", type=int, default=200)
    ap.add_argument("--kernel-only", action="store_true")
    args = ap.parse_args()
    from gglasso_amd import model_selection as ms, solver, utils
    p, N, F, L = (int(v) for v in args.shape.split(","))
    X = make_problem(p, N)
    Xs = np.ascontiguousarray(X / np.sqrt(X.var(axis=1))[:, None])         # what cv_search(scale=True) splits: one scale for all folds
    train, test = ms.cv_folds(N, F, 0)
    lam = np.geomspace(0.6, 0.15, L)
    shape = {"p": p, "N": N, "F": F, "m": int(test.shape[1]), "L": L, "calls": args.calls}
    parts = args.part.split(",")

    if args.kernel_only:
        eye = np.broadcast_to(np.eye(p), (F, p, p))
        eng = solver.HipEngine(eye, eye, eye, np.broadcast_to(np.zeros((p, p)), (F, p, p)))
        try:
            eng.set_data_subsets(Xs, train, center=True)
            for _ in range(args.calls):
                out = eng.neighborhood_cv(Xs, test, lam, 'and')
        finally:
            eng.close()
        print(json.dumps({**shape, "kernel_only": True, **degree_bins(out['degree'], out['status'])}), flush=True)
        return

    got = {}

    def search(method):
        def run():
            with contextlib.redirect_stdout(io.StringIO()):
                got[method] = ms.cv_search(X, lam, folds=(train, test), scale=True, method=method)
        return run

    if "search" in parts:
        mb_ms, gl_ms = alternate_ms([search('mb'), search('glasso')], args.calls)
        (_, st_mb), (_, st_gl) = got['mb'], got['glasso']
        print(json.dumps({**shape, "part": "search", "mb_ms": mb_ms, "glasso_ms": gl_ms, "mb_CV": [float(v) for v in st_mb["CV"]],
                          "mb_IX": st_mb["IX"], "glasso_CV": [float(v) for v in st_gl["CV"]], "glasso_IX": st_gl["IX"]}), flush=True)

    if "twin" in parts:
        S_tr, S_te = utils.sample_covariance_subsets(Xs, train), utils.sample_covariance_subsets(Xs, test)
        W = utils.neighborhood_selection(S_tr, lam, 'and')                  # (F,L,p,p)
        res = {}

        def device():
            res['out'] = utils.neighborhood_refit(S_tr, W, 1e-8, S_te)

        n_units = F * L * p
        pick = np.linspace(0, n_units - 1, min(args.twin_units, n_units)).astype(np.int64)

        def twin():
            with np.errstate(all='ignore'):
                for u in pick:
                    f, l, j = u // (L * p), (u // p) % L, u % p
                    utils._host_refit_node(S_tr[f], S_te[f], W[f, l, j], j, 1e-8, utils.MB_REFIT_MAX_DEG)

        dev_ms, twin_ms = alternate_ms([device, twin], args.calls)
        print(json.dumps({**shape, "part": "twin", "device_refit_ms": dev_ms, "twin_units": int(pick.size), "twin_units_ms": twin_ms,
                          "twin_all_units_by_proportion_ms": twin_ms["median"] * n_units / pick.size,
                          **degree_bins(res['out']['DEGREE'], res['out']['STATUS']),
                          "note": "the twin ran twin_units units spread over the stack; the proportion to all units is arithmetic, "
                                  "its scaling is not measured"}), flush=True)


if __name__ == "__main__":
    main()
