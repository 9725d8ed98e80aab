"""Neighbourhood selection with penalty weights and the scaled lasso at the size of profiles/neighborhood_selection.txt.

    python tools/bench_neighborhood_weighted.py [--shape p,N,B,L] [--calls 5] [--part kernel,scaled,precision] [--kernel-only MODE]

One JSON line per part (whole-call times; the routes of a comparison alternate, --calls rounds after one warm-up round,
reported as median, min and max):

* kernel     ``HipEngine.neighborhood_stability`` on the B subsample matrices (``scale=True``) through the unweighted
             instantiation of ``k_mb_path`` against the same call through the weighted one with a table of ones in plain
             mode: the same arithmetic, so the gap is the cost of the weight reads, of the larger LDS footprint and of the
             table's upload.  Everything else is shared.
* scaled     the same call in scaled mode at the grid times ``1`` (on correlations sigma <= 1, so the thresholds are lower
             than the plain ones): time, sweeps and outer iterations per (subsample, lambda, node) unit, statuses.
* precision  ONE ``utils.scaled_lasso_precision`` call on all N observations against the whole ``stars_search(method='mb')``
             and ``cv_search(method='mb')`` along the grid.  Three different statistics: the figures say what each costs.

``--kernel-only plain|unit|scaled``: the subsample matrices once, then --calls calls of that route and nothing else, for a run
under ``rocprofv3 --kernel-trace --stats``."""
import argparse
import contextlib
import io
import json
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from bench_stars import alternate_ms, make_problem      # noqa: E402  (tools/ is the script's directory)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--shape", default="500,2000,20,10", help="p,N,B,L")
    ap.add_argument("--calls", type=int, default=5)
    ap.add_argument("--part", default="kernel,scaled,precision")
    ap.add_argument("--kernel-only", default=None, choices=("plain", "unit", "scaled"))
    args = ap.parse_args()
    from gglasso_amd import model_selection as ms, solver, utils
    p, N, B, L = (int(v) for v in args.shape.split(","))
    X = make_problem(p, N)
    idx = ms.stars_subsamples(N, B)
    lam = np.geomspace(0.6, 0.15, L)
    ones = np.ones((p, p))
    shape = {"p": p, "N": N, "B": B, "b": int(idx.shape[1]), "L": L, "calls": args.calls}
    parts = args.part.split(",")
    routes = {"plain": {}, "unit": dict(weights=ones), "scaled": dict(scaled=True)}

    def unit_stats(out):
        sw = out['sweeps']
        st = {"sweeps_per_unit_mean": float(sw.mean()), "sweeps_per_unit_max": int(sw.max()),
              "status_counts": [int((out['status'] == s).sum()) for s in (0, 1, 2, 3)]}
        if 'outer' in out:
            st.update(outer_per_unit_mean=float(out['outer'].mean()), outer_per_unit_max=int(out['outer'].max()))
        return st

    if args.kernel_only or "kernel" in parts or "scaled" in parts:
        eye = np.broadcast_to(np.eye(p), (B, p, p))
        eng = solver.HipEngine(eye, eye, eye, np.broadcast_to(np.zeros((p, p)), (B, p, p)))
        got = {}
        try:
            eng.set_data_subsets(X, idx, center=True, scale=True)

            def call(name):
                def run():
                    got[name] = eng.neighborhood_stability(lam, 'and', **routes[name])
                return run

            if args.kernel_only:
                for _ in range(args.calls):
                    call(args.kernel_only)()
                print(json.dumps({**shape, "kernel_only": args.kernel_only, **unit_stats(got[args.kernel_only])}), flush=True)
                return
            names = (["plain", "unit"] if "kernel" in parts else []) + (["scaled"] if "scaled" in parts else [])
            if "scaled" in parts and "plain" not in names:
                names.insert(0, "plain")
            times = alternate_ms([call(n) for n in names], args.calls)
        finally:
            eng.close()
        if "kernel" in parts:
            same = np.array_equal(got["plain"]["num"], got["unit"]["num"]) and np.array_equal(got["plain"]["sweeps"], got["unit"]["sweeps"])
            print(json.dumps({**shape, "part": "kernel", "plain_call_ms": times[names.index("plain")],
                              "unit_weights_call_ms": times[names.index("unit")], "same_num_and_sweeps": bool(same),
                              **unit_stats(got["plain"])}), flush=True)
        if "scaled" in parts:
            print(json.dumps({**shape, "part": "scaled", "plain_call_ms": times[names.index("plain")],
                              "scaled_call_ms": times[names.index("scaled")], "plain": unit_stats(got["plain"]),
                              "scaled": unit_stats(got["scaled"])}), flush=True)

    if "precision" in parts:
        out = {}
        S_full = utils.sample_covariance(X, center=True, scale=True)[0]

        def quiet(fn):
            def run():
                with contextlib.redirect_stdout(io.StringIO()):
                    fn()
            return run

        def precision():
            out['scaled'] = utils.scaled_lasso_precision(S_full, n=N)

        def stars():
            out['stars'] = ms.stars_search(X, lam, indices=idx, scale=True, method='mb')

        def cv():
            out['cv'] = ms.cv_search(X, lam, n_folds=5, scale=True, method='mb')

        import warnings
        with warnings.catch_warnings():
            warnings.simplefilter("ignore")
            t_sc, t_st, t_cv = alternate_ms([quiet(precision), quiet(stars), quiet(cv)], args.calls)
        Theta, info = out['scaled']
        edges = lambda A: int(np.count_nonzero(np.triu(A, 1)))
        print(json.dumps({**shape, "part": "precision", "scaled_lasso_precision_ms": t_sc, "stars_search_mb_ms": t_st,
                          "cv_search_mb_ms": t_cv, "lambda0": info['LAMBDA0'], "scaled_edges": edges(Theta != 0),
                          "stars_edges": edges(out['stars'][0]['adjacency']), "stars_lambda": float(out['stars'][0]['lambda1']),
                          "cv_edges": edges(out['cv'][0]['adjacency']), "cv_lambda": float(out['cv'][0]['lambda1']),
                          "scaled_outer_mean": float(info['OUTER'].mean()), "scaled_outer_max": int(info['OUTER'].max()),
                          "scaled_sweeps_mean": float(info['SWEEPS'].mean()),
                          "scaled_status_counts": [int((info['STATUS'] == s).sum()) for s in (0, 1, 2, 3)],
                          "note": "three different statistics: what each costs, not that one replaces the other"}), flush=True)


if __name__ == "__main__":
    main()
