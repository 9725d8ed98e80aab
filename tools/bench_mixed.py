"""The latent correlation matrix of mixed binary / continuous data: ``utils.mixed_correlation`` (the counts on the int8 matrix
cores, one wave per root of a bridge function) at the size of profiles/mixed_correlation.txt.

    python tools/bench_mixed.py [--shape p,N,B] [--calls 5] [--part single,subsets] [--host-calls 5,1] [--kernel-only]

Data: the chain-graph observations of tools/bench_stars.py as the latent normal; the even variables dichotomised at the
quantiles of U(0.2, 0.8), the odd ones passed through exp.  Two workloads, one JSON line each (whole-call times from the
observations on the host to the matrices on the host; the routes of a workload alternate, --calls rounds after one warm-up
round, reported as median, min and max):

* single    one matrix of all N observations.
* subsets   the B subsample matrices of StARS (``model_selection.stars_subsamples``: b = int(10 sqrt(N))).

Routes:

* device    ``utils.mixed_correlation``: dense ranks on the host, one upload, k_kendall_counts, k_bridge_zero_counts,
            k_bridge_invert.
* skeptic   ``utils.skeptic_correlation`` of the same data: what the counts alone cost (the same upload and download).
* host      ``utils.host_mixed_correlation`` GIVEN the device's counts (its own brute-force counts take minutes at this size
            and are not what is compared): the thresholds and the p (p - 1) / 2 roots in numpy.  Timed in a loop of its own,
            --host-calls rounds for the two workloads.

``--kernel-only`` makes --calls device calls of each workload and nothing else, for a run under ``rocprofv3 --kernel-trace
--stats`` (the time of k_bridge_invert itself)."""
import argparse
import json
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from tools.bench_stars import alternate_ms, make_problem      # noqa: E402


def make_mixed(p, N, seed=0):
    Z = make_problem(p, N, seed)
    Z /= Z.std(axis=1, keepdims=True)
    share = np.random.default_rng(seed + 1).uniform(0.2, 0.8, p)
    X = np.exp(Z)
    for i in range(0, p, 2):
        X[i] = (Z[i] > np.quantile(Z[i], share[i])).astype(np.float64)
    return X


def bridge_residuals(S, G, n0, types, n, clip=0.999):
    """|F(S_ij) - tau| of every bridged pair that is not clipped, F by the twin's quadrature (``utils._bridge_H``), and F'
    there: S, G (p,p), n0 (p,) of one subset of n samples.  Where F is flat (F' tiny: thresholds far apart, r towards -1 or 1)
    the root is ill-conditioned, and two solvers that both meet the equation to rounding differ in r."""
    from gglasso_amd import utils
    p = S.shape[0]
    iu, ju = np.triu_indices(p, 1)
    ti, tj = types[iu] == 1, types[ju] == 1
    mix = (ti | tj) & (np.abs(S[iu, ju]) < clip)
    iu, ju, ti, tj = iu[mix], ju[mix], ti[mix], tj[mix]
    delta = np.array([utils._bridge_delta(n0[i], n) if types[i] else 0.0 for i in range(p)])
    bb = ti & tj
    h, k = np.where(ti, delta[iu], delta[ju]), np.where(bb, delta[ju], 0.0)
    c, amp = np.where(bb, 1 / np.pi, 2 / np.pi), np.where(bb, 1.0, np.sqrt(2.0))
    x = np.arcsin(S[iu, ju] / amp)
    res = np.abs(utils._bridge_H(x, h * h + k * k, 2 * h * k, c) - G[iu, ju] / float(n * (n - 1) // 2))
    slope = c * np.exp(-(h * h + k * k - 2 * h * k * np.sin(x)) / (2 * np.cos(x) ** 2)) / (amp * np.cos(x))
    return res, slope, (iu, ju)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--shape", default="500,2000,20", help="p,N,B")
    ap.add_argument("--calls", type=int, default=5)
    ap.add_argument("--part", default="single,subsets")
    ap.add_argument("--host-calls", default="5,1", help="rounds of the host route for single,subsets (0: skip)")
    ap.add_argument("--kernel-only", action="store_true", help="only device calls (for a profiler run)")
    args = ap.parse_args()
    from gglasso_amd import model_selection as ms, utils
    p, N, B = (int(v) for v in args.shape.split(","))
    X = make_mixed(p, N)
    types = utils.variable_types(X)
    idx = ms.stars_subsamples(N, B)
    b = idx.shape[1]
    work = {"single": (None, N, 1), "subsets": (idx, b, B)}
    host_calls = dict(zip(("single", "subsets"), (int(v) for v in args.host_calls.split(","))))
    for part in args.part.split(","):
        sub, n, nB = work[part]
        shape = {"part": part, "p": p, "N": N, "B": nB, "b": n, "binary": int(types.sum()), "calls": args.calls}
        if args.kernel_only:
            for _ in range(args.calls):
                utils.mixed_correlation(X, types, sub)
            print(json.dumps({**shape, "kernel_only": True}), flush=True)
            continue
        S_dev, info = utils.mixed_correlation(X, types, sub, return_info=True)
        dev_ms, skeptic_ms = alternate_ms([lambda: utils.mixed_correlation(X, types, sub),
                                           lambda: utils.skeptic_correlation(X, sub)], args.calls)
        out = {**shape, "device_ms": dev_ms, "skeptic_ms": skeptic_ms, "clipped": int(np.sum(info['clipped'])),
               "bridged_pairs": nB * int(p * (p - 1) // 2 - (p - types.sum()) * (p - types.sum() - 1) // 2)}
        if host_calls.get(part, 0) > 0:
            G = utils.kendall_counts(X, sub)
            host = lambda: utils.host_mixed_correlation(X, types, sub, counts=G)
            S_host = host()
            out["host_given_counts_ms"] = alternate_ms([host], host_calls[part])[0]
            out["host_calls"] = host_calls[part]
            # the two solvers against the equation itself, and their distance in r scaled by F' (both in units of F)
            Sd, Sh, Gs, n0s = (a.reshape((nB,) + a.shape[-2:]) for a in (S_dev, S_host, G, info['zero_counts'][..., None]))
            rd, rh, scaled = 0.0, 0.0, 0.0
            for r in range(nB):
                res_d, slope, (iu, ju) = bridge_residuals(Sd[r], Gs[r], n0s[r, :, 0], types, n)
                res_h = bridge_residuals(Sh[r], Gs[r], n0s[r, :, 0], types, n)[0]
                rd, rh = max(rd, float(res_d.max())), max(rh, float(res_h.max()))
                scaled = max(scaled, float((np.abs(Sd[r] - Sh[r])[iu, ju] * slope).max()))
            out.update(max_residual_device=rd, max_residual_host=rh, max_abs_device_minus_host=float(np.abs(S_dev - S_host).max()),
                       max_abs_device_minus_host_times_slope=scaled)
        print(json.dumps(out), flush=True)


if __name__ == "__main__":
    main()
