"""Meinshausen-Buhlmann neighbourhood selection under StARS at the size of profiles/stars_selection.txt.

    python tools/bench_neighborhood.py [--shape p,N,B,L] [--calls 5] [--part search,twin] [--twin-nodes 40] [--kernel-only]

One JSON line per part (whole-call times; the routes of a comparison alternate, --calls rounds after one warm-up round,
reported as median, min and max):

* search  ``model_selection.stars_search(method='mb')`` against ``method='glasso'`` on the same data, subsamples and grid
          (``scale=True``: correlations, what huge does for either estimator).  The two estimators are not the same
          statistic; the line also carries both choices.
* twin    the same ``method='mb'`` search against the numpy twin.  The twin's whole search takes minutes at this size, so it
          runs the paths of ``--twin-nodes`` nodes of subsample 0 only and the line carries that time, the node count and the
          plain proportion to all B p nodes; that the twin scales so is not measured.

``--kernel-only``: the subsample matrices once, then --calls calls of ``HipEngine.neighborhood_stability`` and nothing else, for
a run under ``rocprofv3 --kernel-trace --stats``; the line carries the sweeps per (subsample, lambda, node) unit."""
import argparse
import contextlib
import io
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from bench_stars import alternate_ms, make_problem      # noqa: E402  (tools/ is the script's directory)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--shape", default="500,2000,20,10", help="p,N,B,L")
    ap.add_argument("--calls", type=int, default=5)
    ap.add_argument("--part", default="search,twin")
    ap.add_argument("--twin-nodes", type=int, default=40)
    ap.add_argument("--kernel-only", action="store_true")
    ap.add_argument("--beta", type=float, default=0.05)
    args = ap.parse_args()
    from gglasso_amd import model_selection as ms, solver, utils
    p, N, B, L = (int(v) for v in args.shape.split(","))
    X = make_problem(p, N)
    idx = ms.stars_subsamples(N, B)
    lam = np.geomspace(0.6, 0.15, L)
    shape = {"p": p, "N": N, "B": B, "b": int(idx.shape[1]), "L": L, "calls": args.calls}
    parts = args.part.split(",")

    if args.kernel_only:
        eye = np.broadcast_to(np.eye(p), (B, p, p))
        eng = solver.HipEngine(eye, eye, eye, np.broadcast_to(np.zeros((p, p)), (B, p, p)))
        try:
            eng.set_data_subsets(X, idx, center=True, scale=True)
            for _ in range(args.calls):
                out = eng.neighborhood_stability(lam, 'and')
        finally:
            eng.close()
        sw = out['sweeps']
        print(json.dumps({**shape, "kernel_only": True, "units": int(sw.size), "sweeps_per_unit_mean": float(sw.mean()),
                          "sweeps_per_unit_max": int(sw.max()), "sweeps_per_node_path_mean": float(sw.sum(axis=0).mean()),
                          "status_counts": [int((out['status'] == s).sum()) for s in (0, 1, 2)]}), flush=True)
        return

    out = {}

    def search(method):
        def run():
            with contextlib.redirect_stdout(io.StringIO()):
                out[method] = ms.stars_search(X, lam, indices=idx, beta=args.beta, scale=True, method=method)
        return run

    if "search" in parts:
        mb_ms, gl_ms = alternate_ms([search('mb'), search('glasso')], args.calls)
        (_, st_mb), (_, st_gl) = out['mb'], out['glasso']
        print(json.dumps({**shape, "part": "search", "mb_ms": mb_ms, "glasso_ms": gl_ms, "mb_NUM": st_mb["NUM"],
                          "mb_IX": st_mb["IX"], "glasso_NUM": st_gl["NUM"], "glasso_IX": st_gl["IX"]}), flush=True)

    if "twin" in parts:
        nodes = list(range(0, p, max(1, p // args.twin_nodes)))[:args.twin_nodes]
        S0 = utils.sample_covariance_subsets(X, idx[:1], center=True, scale=True)
        S0 = (S0[0] if isinstance(S0, tuple) else S0)[0]

        ones = np.ones(p)

        def twin():
            with np.errstate(all='ignore'):
                for j in nodes:
                    utils._host_mb_node_w(S0, j, lam, ones, False, 1e-7, 10000, 1e-7, 100)

        dev_ms, twin_ms = alternate_ms([search('mb'), twin], args.calls)
        scale = B * p / len(nodes)
        print(json.dumps({**shape, "part": "twin", "device_search_ms": dev_ms, "twin_nodes": len(nodes), "twin_nodes_ms": twin_ms,
                          "twin_all_nodes_by_proportion_ms": twin_ms["median"] * scale,
                          "note": "the twin ran the paths of twin_nodes nodes of subsample 0; the proportion to B p nodes is "
                                  "arithmetic, its scaling is not measured"}), flush=True)


if __name__ == "__main__":
    main()
