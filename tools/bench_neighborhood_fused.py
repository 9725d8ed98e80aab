"""Fused joint neighbourhood selection at the size of the GGL benchmark: K = 32 instances, p = 500, five lambda2
chains of ten lambda1.

    python tools/bench_neighborhood_fused.py [--shape K,p,N,L1,L2] [--calls 5] [--part kernel,sweeps,search]

One JSON line per part:

* kernel  ``k_mb_fused_path`` and ``k_mb_joint_path`` alone by HIP events on the same stack and grid
          (``ggl_dev_mb_fused_bench`` / ``ggl_dev_mb_joint_bench``: all chains in one launch, no transfers).  The two routes
          alternate, ``--calls`` rounds of one launch each after one warm-up round; median, min and max in ms.  The group
          kernel is the yardstick; the two solve different problems, so the sweeps of both are reported beside the times.
* sweeps  sweeps per (unit, pair) of the fused route on the correlation stack (the block step is exact) and on the same stack
          rescaled per (instance, variable) by factors in [1, 1.5] (the block step is majorised): where majorisation shows.
* search  the whole ``model_selection.fused_neighborhood_search``."""
import argparse
import json
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from bench_neighborhood_joint import make_stack          # noqa: E402  (tools/ is the script's directory)
from bench_stars import alternate_ms                     # noqa: E402


def rescaled(S):
    """S rescaled per (instance, variable) by factors in [1, 1.5], bitwise symmetric (the upper triangle mirrored)."""
    K, p, _ = S.shape
    c = np.random.default_rng([31, p, K]).uniform(1.0, 1.5, size=(K, p))
    up = np.triu(S * c[:, :, None] * c[:, None, :])
    return np.ascontiguousarray(up + np.swapaxes(np.triu(up, 1), 1, 2))


def summary(v):
    return {"median": float(np.median(v)), "min": float(np.min(v)), "max": float(np.max(v))}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--shape", default="32,500,2000,10,5", help="K,p,N,L1,L2")
    ap.add_argument("--calls", type=int, default=5)
    ap.add_argument("--part", default="kernel,sweeps,search")
    args = ap.parse_args()
    from gglasso_amd import _lib, model_selection as ms, utils
    K, p, N, L1, L2 = (int(v) for v in args.shape.split(","))
    S = make_stack(K, p, N)
    l1, l2 = np.geomspace(0.4, 0.1, L1), np.geomspace(0.2, 0.02, L2)
    shape = {"K": K, "p": p, "N": N, "L1": L1, "L2": L2, "calls": args.calls}
    parts = args.part.split(",")
    lib = _lib.load()
    Sm, a1, a2, om = utils._mbj_args(S, l1, l2, 'and', None, 1e-7, 10000, False, 1e-8, 'fused')
    lam1 = np.ascontiguousarray(np.broadcast_to(a1[None, :], (L2, L1)))
    lam2 = np.ascontiguousarray(np.broadcast_to(a2[:, None], (L2, L1)))

    def tables(stack, coupling):
        return utils._joint_run(stack, a1, a2, om, 'and', 1e-7, 10000, False, 1e-8, 0, False, want_coef=False, coupling=coupling)['INFO']

    if "kernel" in parts:
        times = {"fused": [], "group": []}
        one = np.zeros(1)
        for rnd in range(-1, args.calls):                                   # (round -1 warms both up)
            for name, entry in (("fused", lib.ggl_dev_mb_fused_bench), ("group", lib.ggl_dev_mb_joint_bench)):
                _lib.check(entry(K, p, _lib.ptr(Sm), L2, L1, _lib.ptr(lam1), _lib.ptr(lam2), 1e-7, 10000, 1, _lib.ptr(one)))
                if rnd >= 0:
                    times[name].append(float(one[0]))
        inf_f, inf_g = tables(Sm, 'fused'), tables(Sm, 'group')
        print(json.dumps({**shape, "part": "kernel", "k_mb_fused_path_event_ms": summary(times["fused"]),
                          "k_mb_joint_path_event_ms": summary(times["group"]), "units": int(L2 * p),
                          "fused_sweeps_per_unit_pair_mean": float(inf_f[..., 0].mean()), "fused_sweeps_max": int(inf_f[..., 0].max()),
                          "group_sweeps_per_unit_pair_mean": float(inf_g[..., 0].mean()), "group_sweeps_max": int(inf_g[..., 0].max()),
                          "fused_status_counts": [int((inf_f[..., 1] == s).sum()) for s in (0, 1, 2)],
                          "group_status_counts": [int((inf_g[..., 1] == s).sum()) for s in (0, 1, 2)],
                          "note": "every timed launch sits in a call of its own that uploads S first; the event pair brackets the launch alone"}),
              flush=True)

    if "sweeps" in parts:
        out = {}
        for name, stack in (("correlation", Sm), ("rescaled", rescaled(Sm))):
            info = tables(stack, 'fused')
            out[name] = {"sweeps_per_unit_pair_mean": float(info[..., 0].mean()), "sweeps_max": int(info[..., 0].max()),
                         "per_lambda2_chain_mean": [float(v) for v in info[..., 0].mean(axis=(0, 2))],
                         "status_counts": [int((info[..., 1] == s).sum()) for s in (0, 1, 2)]}
        print(json.dumps({**shape, "part": "sweeps", **out}), flush=True)

    if "search" in parts:
        got = {}

        def search():
            got['out'] = ms.fused_neighborhood_search(S, N, l1, l2)
        t, = alternate_ms([search], args.calls)
        sol, st = got['out']
        print(json.dumps({**shape, "part": "search", "fused_neighborhood_search_ms": t, "best": st['BEST'], "ix": list(st['IX']),
                          "edges_per_instance_mean": float(sol['adjacency'].sum(axis=(1, 2)).mean() / 2),
                          "changed_edges_total": int(sol['changed_edges'].sum()),
                          "status_counts": [int((st['STATUS'] == s).sum()) for s in (0, 1, 2)],
                          "refit_status_counts": [int((st['REFIT_STATUS'] == s).sum()) for s in (0, 1, 2, 3)]}), flush=True)


if __name__ == "__main__":
    main()
