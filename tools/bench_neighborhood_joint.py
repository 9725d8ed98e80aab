"""Joint neighbourhood selection at the size of the GGL benchmark: K = 32 instances, p = 500, five lambda2
chains of ten lambda1.

    python tools/bench_neighborhood_joint.py [--shape K,p,N,L1,L2] [--calls 5] [--part search,kernel,twin,admm] [--twin-nodes 4]

One JSON line per part (the routes of a comparison alternate, --calls rounds after one warm-up round, reported as median, min
and max in ms):

* search  the whole ``model_selection.joint_neighborhood_search``: the grid call with the refit (tables only), the score on the
          host, the further call at the chosen point with its coefficient stacks.
* kernel  ``k_mb_joint_path`` alone by HIP events (``ggl_dev_mb_joint_bench``: all chains in one launch, no transfers), the
          tables-only grid call around it, beside ``k_mb_path`` on the same K matrices and the same lambda1 grid (``HipEngine.neighborhood_stability``: the path,
          the symmetrisation and the edge counts, nothing downloaded but tables), as the per-sweep yardstick: K separate lassos
          against K coupled ones, with the sweeps of both.
* twin    the numpy twin on ``--twin-nodes`` nodes of ONE chain, SCALED UP to p nodes and L2 chains (said so in the line).
* admm    ``ADMM_MGL`` with reg='GGL' at ONE grid point on the same stack: a different statistic (the penalised likelihood, not
          the node-wise regressions), timed to say what each costs."""
import argparse
import json
import os
import sys
import time
import warnings

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from bench_stars import alternate_ms, make_problem      # noqa: E402  (tools/ is the script's directory)


def make_stack(K, p, N):
    """K correlation matrices of observations that share the chain of ``make_problem`` and differ in a few long-range edges."""
    S = np.stack([np.corrcoef(make_problem(p, N, seed=k)) for k in range(K)])
    S = 0.5 * (S + np.swapaxes(S, 1, 2))
    S[:, np.arange(p), np.arange(p)] = 1.0
    return np.ascontiguousarray(S)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--shape", default="32,500,2000,10,5", help="K,p,N,L1,L2")
    ap.add_argument("--calls", type=int, default=5)
    ap.add_argument("--part", default="search,kernel,twin,admm")
    ap.add_argument("--twin-nodes", type=int, default=4)
    args = ap.parse_args()
    from gglasso_amd import _lib, model_selection as ms, solver, utils
    K, p, N, L1, L2 = (int(v) for v in args.shape.split(","))
    S = make_stack(K, p, N)
    l1, l2 = np.geomspace(0.4, 0.1, L1), np.geomspace(0.2, 0.02, L2)
    shape = {"K": K, "p": p, "N": N, "L1": L1, "L2": L2, "calls": args.calls}
    parts = args.part.split(",")
    lib = _lib.load()

    if "search" in parts:
        got = {}

        def search():
            got['out'] = ms.joint_neighborhood_search(S, N, l1, l2)
        t, = alternate_ms([search], args.calls)
        sol, st = got['out']
        print(json.dumps({**shape, "part": "search", "joint_neighborhood_search_ms": t, "best": st['BEST'], "ix": list(st['IX']),
                          "edges_per_instance_mean": float(sol['adjacency'].sum(axis=(1, 2)).mean() / 2),
                          "common_edges": int(sol['common_adjacency'].sum() // 2),
                          "status_counts": [int((st['STATUS'] == s).sum()) for s in (0, 1, 2)],
                          "refit_status_counts": [int((st['REFIT_STATUS'] == s).sum()) for s in (0, 1, 2, 3)]}), flush=True)

    if "kernel" in parts:
        got = {}
        Sm, a1, a2, om = utils._mbj_args(S, l1, l2, 'and', None, 1e-7, 10000, False, 1e-8)
        eye = np.broadcast_to(np.eye(p), (K, p, p))
        eng = solver.HipEngine(S, eye, eye, np.broadcast_to(np.zeros((p, p)), (K, p, p)))
        try:
            def joint():
                got['joint'] = utils._joint_run(Sm, a1, a2, om, 'and', 1e-7, 10000, False, 1e-8, 0, False, want_coef=False)

            def single():
                got['single'] = eng.neighborhood_stability(a1, 'and')
            t_j, t_s = alternate_ms([joint, single], args.calls)
        finally:
            eng.close()
        lam1 = np.ascontiguousarray(np.broadcast_to(a1[None, :], (L2, L1)))
        lam2 = np.ascontiguousarray(np.broadcast_to(a2[:, None], (L2, L1)))
        ms_out = np.zeros(args.calls)
        _lib.check(lib.ggl_dev_mb_joint_bench(K, p, _lib.ptr(Sm), L2, L1, _lib.ptr(lam1), _lib.ptr(lam2), 1e-7, 10000, args.calls,
                                              _lib.ptr(ms_out)))
        kms = [float(v) for v in ms_out]
        info = got['joint']['INFO']
        print(json.dumps({**shape, "part": "kernel",
                          "k_mb_joint_path_event_ms": {"median": float(np.median(kms)), "min": min(kms), "max": max(kms)},
                          "joint_call_tables_only_ms": t_j, "k_mb_path_stability_call_ms": t_s,
                          "joint_units": int(L2 * p), "joint_sweeps_per_unit_pair_mean": float(info[..., 0].mean()),
                          "joint_sweeps_max": int(info[..., 0].max()), "joint_newton_max": int(info[..., 2].max()),
                          "joint_status_counts": [int((info[..., 1] == s).sum()) for s in (0, 1, 2)],
                          "single_units": int(K * p), "single_sweeps_per_unit_lambda_mean": float(got['single']['sweeps'].mean()),
                          "single_sweeps_max": int(got['single']['sweeps'].max()),
                          "note": "k_mb_path runs ONE lambda1 chain of K p lassos; k_mb_joint_path L2 chains of p coupled units"}),
              flush=True)

    if "twin" in parts:
        nodes = list(np.linspace(0, p - 1, args.twin_nodes).astype(int))
        dg = np.ascontiguousarray(np.diagonal(S, axis1=1, axis2=2))
        desc = np.sort(l1)[::-1]
        t0 = time.perf_counter()
        with np.errstate(all='ignore'):
            for j in nodes:
                utils._host_mbj_unit(S, np.ones(K), dg, int(j), desc, np.full(L1, l2[L2 // 2]), 1e-7, 10000)
        sec = time.perf_counter() - t0
        print(json.dumps({**shape, "part": "twin", "nodes_timed": len(nodes), "chain_lambda2": float(l2[L2 // 2]),
                          "seconds_timed": sec, "seconds_scaled_to_p_nodes_and_L2_chains": sec / len(nodes) * p * L2,
                          "note": "SCALED UP from the nodes timed, one run"}), flush=True)

    if "admm" in parts:
        got = {}

        def admm():
            with warnings.catch_warnings():
                warnings.simplefilter("ignore")
                got['out'] = solver.ADMM_MGL(S, float(l1[L1 // 2]), float(l2[L2 // 2]), 'GGL', np.tile(np.eye(p), (K, 1, 1)),
                                             tol=1e-7, rtol=1e-7)
        t, = alternate_ms([admm], args.calls)
        print(json.dumps({**shape, "part": "admm", "ADMM_MGL_one_point_ms": t, "lambda1": float(l1[L1 // 2]),
                          "lambda2": float(l2[L2 // 2]), "iterations": int(got['out'][1].get('iter', -1)) if isinstance(got['out'][1], dict) else -1,
                          "note": "a different statistic (penalised likelihood); one grid point, the search has L1 * L2"}), flush=True)


if __name__ == "__main__":
    main()
