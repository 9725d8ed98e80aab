"""One SHA-1 per array that the six single-problem neighbourhood-selection entries return, for "same bits before and after"
checks of a change to ``k_mb_path`` or to its host paths: run it from two checkouts, each with its own built library, and
compare the listings byte for byte (profiles/neighborhood_one_body.txt).

    python tools/mb_identity.py [--sizes 5,64,65,257,513] > listing.txt

Per size p (the three matrices of tests/mb_ref.py; the four-lambda grid, at p > 257 two lambdas) and per route -- plain, the
weight tables of tests/mbw_ref.py, scaled without weights:
* ``utils.neighborhood_selection`` with ``return_info``, rules raw / and / or   (ggl_neighborhood_path, _path_w)
* ``HipEngine.neighborhood_stability`` on a ctx that holds the three matrices, counts and stack   (_stability, _stability_w)
* ``HipEngine.neighborhood_cv`` on the same ctx, with and without ``refit``, stack   (_cv, _cv_w)
A line is ``p route entry key dtype shape sha1``; the dict keys are part of the listing, so a key that comes or goes shows."""
import argparse
import hashlib
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sizes", default="5,64,65,257,513")
    args = ap.parse_args()
    import mb_ref
    import mbw_ref
    from gglasso_amd import model_selection as ms, solver, utils

    def show(p, route, entry, out):
        for key in sorted(out):
            a = np.ascontiguousarray(out[key])
            print(p, route, entry, key, a.dtype, "x".join(str(n) for n in a.shape), hashlib.sha1(a.tobytes()).hexdigest(), flush=True)

    for p in (int(v) for v in args.sizes.split(",")):
        S = mb_ref.stack(p)
        lam = np.array(mb_ref.GRID if p <= 257 else (0.2, 0.1))
        X = mb_ref.stars_data(p=p, N=60)
        _, test = ms.cv_folds(60, 3, 4)
        routes = {"plain": {}, "weighted": dict(weights=mbw_ref.weight_stack(p)), "scaled": dict(scaled=True, sig_tol=mbw_ref.SIG_TOL)}
        eye = np.broadcast_to(np.eye(p), (3, p, p))
        eng = solver.HipEngine(S, eye, eye, np.zeros((3, p, p)))
        try:
            for route, kw in routes.items():
                for rule in ('raw', 'and', 'or'):
                    W, info = utils.neighborhood_selection(S, lam, rule, tol=mbw_ref.TOL, return_info=True, **kw)
                    show(p, route, f"selection_{rule}", {"W": W, **info})
                show(p, route, "stability", eng.neighborhood_stability(lam, 'and', tol=mbw_ref.TOL, counts=True, stack=True, **kw))
                for refit in (False, True):
                    show(p, route, f"cv_refit{int(refit)}", eng.neighborhood_cv(X, test, lam, 'or', tol=mbw_ref.TOL, refit=refit,
                                                                                 stack=True, **kw))
        finally:
            eng.close()


if __name__ == "__main__":
    main()
