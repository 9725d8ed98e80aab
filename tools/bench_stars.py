"""StARS stability selection: the device route against the route without the two new kernels, at the size of
profiles/stars_selection.txt.

    python tools/bench_stars.py [--shape p,N,B,L] [--calls 5] [--part cov,edge,search] [--kernel-only]

Three comparisons, one JSON line each (whole-call times; the routes of a comparison alternate, --calls rounds after one
warm-up round, reported as median, min and max):

* cov     the B subset covariances: ``utils.sample_covariance_subsets`` (X up once, gather on the device) against the
          host gather ``X[:, idx[r]]`` of every subset + ``utils.sample_covariance`` of the (B,p,b) stack.
* edge    the edge statistics of K = L * B snapshots: ``HipEngine.edge_stability`` (L integers come back) against the
          download of the Theta stack + numpy.  ``bytes`` is what the kernel has to read, L B p (p-1) / 2 doubles.
* search  the whole ``model_selection.stars_search`` against the same search with the covariances from the host route
          above, ``ADMM_SGL_batch`` on the uploaded stack, the download of every Theta and numpy counts.

The kernels' own times come from running this tool with ``--kernel-only`` (snapshots planted once, then --calls calls of
edge_stability and of the subset covariance, nothing else) under ``rocprofv3 --kernel-trace --stats``: the average of
k_edge_stability over bytes gives its share of the HBM peak (8 TB/s), k_gather_cols is the cost of the gather."""
import argparse
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

HBM_PEAK = 8.0e12      # bytes / s


def alternate_ms(fns, calls):
    """Times of the callables run in turn, ``calls`` rounds after one warm-up round: per callable the median and the
    spread {'median', 'min', 'max'} in ms -- the routes of one comparison see the same machine at the same time."""
    for fn in fns:
        fn()
    t = [[] for _ in fns]
    for _ in range(calls):
        for i, fn in enumerate(fns):
            t0 = time.perf_counter()
            fn()
            t[i].append(1e3 * (time.perf_counter() - t0))
    return [{"median": float(np.median(v)), "min": float(min(v)), "max": float(max(v))} for v in t]


def make_problem(p, N, seed=0):
    """Observations of a chain graph with a few long-range edges (a sparse, well-conditioned precision matrix)."""
    rng = np.random.default_rng(seed)
    Th = np.eye(p)
    i = np.arange(p - 1)
    Th[i, i + 1] = Th[i + 1, i] = 0.4
    for a, b in rng.integers(0, p, (p // 10, 2)):
        if abs(a - b) > 1:
            Th[a, b] = Th[b, a] = 0.1
    return np.linalg.cholesky(np.linalg.inv(Th)) @ rng.standard_normal((p, N))


def host_covariances(X, idx):
    from gglasso_amd import utils
    return utils.sample_covariance(np.stack([X[:, idx[r]] for r in range(idx.shape[0])]))


def host_search(X, lam, idx, beta, tol, rtol):
    """stars_search without the two kernels: host gather, upload of the (L B,p,p) covariances, download of every Theta."""
    from gglasso_amd import model_selection as ms, solver, utils
    from gglasso_amd.batch import ADMM_SGL_batch
    p, (B, _), L = X.shape[0], idx.shape, len(lam)
    S = host_covariances(X, idx)
    res = ADMM_SGL_batch(np.tile(S, (L, 1, 1)), np.repeat(lam, B), Omega_0=np.eye(p), X_0=np.eye(p), tol=tol, rtol=rtol,
                         fetch=('Theta',))
    Th = np.stack([sol['Theta'] for sol, _ in res]).reshape(L, B, p, p)
    _, num = ms._host_edge_counts(Th, 1e-8)
    D = np.array([2 * int(n) / (B * B * (p * (p - 1) // 2)) for n in num])
    ix, _ = ms.stars_select(D, beta)
    sol, _ = solver.ADMM_SGL(utils.sample_covariance(X), lam[ix], np.eye(p), X_0=np.eye(p), tol=tol, rtol=rtol)
    return [int(n) for n in num], ix, sol


def planted_engine(p, K, seed=1):
    """An engine whose K snapshots are sparse symmetric matrices with entries on both sides of the threshold."""
    from gglasso_amd.solver import HipEngine
    rng = np.random.default_rng(seed)
    T = rng.standard_normal((K, p, p)) * (rng.random((K, p, p)) < 0.1)
    T = T + T.transpose(0, 2, 1)
    eye = np.broadcast_to(np.eye(p), (K, p, p))
    eng = HipEngine(eye, eye, eye, 0 * eye)
    eng.set_state(np.ascontiguousarray(eye), T, np.zeros((K, p, p)))
    for k in range(K):
        eng.snapshot_k(k)
    return eng, T


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--shape", default="500,2000,20,10", help="p,N,B,L")
    ap.add_argument("--calls", type=int, default=5)
    ap.add_argument("--part", default="cov,edge,search")
    ap.add_argument("--kernel-only", action="store_true", help="only device calls of the two kernels (for a profiler run)")
    ap.add_argument("--beta", type=float, default=0.05)
    args = ap.parse_args()
    import contextlib
    import io
    from gglasso_amd import model_selection as ms, utils
    p, N, B, L = (int(v) for v in args.shape.split(","))
    X = make_problem(p, N)
    idx = ms.stars_subsamples(N, B)
    b = idx.shape[1]
    lam = np.geomspace(0.6, 0.15, L)
    shape = {"p": p, "N": N, "B": B, "b": b, "L": L, "calls": args.calls}
    parts = args.part.split(",")
    edge_bytes = 8.0 * L * B * p * (p - 1) / 2

    if args.kernel_only:
        eng, _ = planted_engine(p, L * B)
        try:
            for _ in range(args.calls):
                eng.edge_stability(B)
                eng.edge_stability(B, counts=True)
                utils.sample_covariance_subsets(X, idx)
        finally:
            eng.close()
        print(json.dumps({**shape, "kernel_only": True, "edge_bytes": edge_bytes}), flush=True)
        return

    if "cov" in parts:
        S_dev, S_host = utils.sample_covariance_subsets(X, idx), host_covariances(X, idx)
        dev, host = alternate_ms([lambda: utils.sample_covariance_subsets(X, idx), lambda: host_covariances(X, idx)], args.calls)
        print(json.dumps({**shape, "part": "cov", "same_bits": bool(np.array_equal(S_dev, S_host)), "device_gather_ms": dev,
                          "host_gather_ms": host}), flush=True)

    if "edge" in parts:
        eng, T = planted_engine(p, L * B)
        try:
            def host():
                Th = eng.snapshots(names=('Theta',))['Theta']
                return ms._host_edge_counts(Th.reshape(L, B, p, p), 1e-8)[1]
            same = bool(np.array_equal(eng.edge_stability(B), host()))
            dev_ms, dev_counts_ms, host_ms = alternate_ms([lambda: eng.edge_stability(B),
                                                           lambda: eng.edge_stability(B, counts=True), host], args.calls)
        finally:
            eng.close()
        print(json.dumps({**shape, "part": "edge", "same_integers": same, "bytes": edge_bytes, "device_call_ms": dev_ms,
                          "device_call_with_counts_ms": dev_counts_ms, "download_numpy_ms": host_ms}), flush=True)

    if "search" in parts:
        out = {}

        def device():
            with contextlib.redirect_stdout(io.StringIO()):
                out["dev"] = ms.stars_search(X, lam, indices=idx, beta=args.beta)

        def host():
            with contextlib.redirect_stdout(io.StringIO()):
                out["host"] = host_search(X, lam, idx, args.beta, 1e-7, 1e-7)

        dev_ms, host_ms = alternate_ms([device, host], args.calls)
        sol, st = out["dev"]
        num, ix, sol_h = out["host"]
        print(json.dumps({**shape, "part": "search", "device_route_ms": dev_ms, "host_route_ms": host_ms,
                          "same_NUM": st["NUM"] == num, "same_IX": st["IX"] == ix,
                          "same_solution_bits": bool(np.array_equal(sol["Theta"], sol_h["Theta"])),
                          "NUM": st["NUM"], "IX": st["IX"], "lambda1": float(st["BEST"]["lambda1"]),
                          "instability": [float(v) for v in st["INSTABILITY"]]}), flush=True)


if __name__ == "__main__":
    main()
