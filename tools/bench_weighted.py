"""Kernel-weighted covariance stack of one series (ggl_covariance_weighted) at p = 500, N = 2000, K = 50, Gaussian kernel at
three bandwidths: supports of N (no zero weight), about N/4 and about N/10 -- as recorded in profiles/weighted_covariance.txt.

    python tools/bench_weighted.py [--p 500] [--N 2000] [--K 50] [--rounds 5] [--device-only]

Whole calls from host data to host stack, every route once per round with the routes alternating, after one warm-up round:
median (min - max) of --rounds.

  weighted   (a) utils.kernel_covariance: one upload of X and of the weights, the stack computed on the device
  scaled     (b) what the library offered before: K host-built arrays sqrt(N w_k / W_k) (X - m_k), all N columns each, through
             utils.sample_covariance(center=False) -- K times the data on the host and over the bus
  support    (b') the same with every array cut to the columns of its support (a ragged list): the best a caller could do
  numpy      (c) a loop of numpy.cov(X, aweights=w_k, bias=True) on the host's threads

Then the time of k_gram_nt_weighted alone with and without GGL_COV_FULL_RANGE, from the event timeline of a ctx
(ggl_trace_start / ggl_trace_read around ggl_set_S_from_weighted: the events 30 and 31 in front of and behind the launch),
median (min - max) of --rounds after one warm-up call.  One JSON line per support."""
import argparse
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def rounds_ms(routes, rounds):
    """{name: [ms per round]}: one warm-up round, then every route once per round, in turn."""
    for fn in routes.values():
        fn()
    t = {name: [] for name in routes}
    for _ in range(rounds):
        for name, fn in routes.items():
            t0 = time.perf_counter()
            fn()
            t[name].append(1e3 * (time.perf_counter() - t0))
    return t


def summary(ms):
    return {"median_ms": float(np.median(ms)), "min_ms": float(np.min(ms)), "max_ms": float(np.max(ms))}


def scaled_copies(X, w, cut):
    """The K arrays whose raw second moment (1/N_k) Y Y^T is the weighted covariance of row k."""
    out = []
    for wk in w:
        cols = slice(None)
        if cut:
            nz = np.flatnonzero(wk)
            cols = slice(nz[0], nz[-1] + 1)
        wt = wk[cols] / wk.sum()
        Xs = X[:, cols]
        m = Xs @ wt
        out.append(np.sqrt(Xs.shape[1] * wt) * (Xs - m[:, None]))
    return out


def gram_kernel_us(eng, X, w, flags, rounds):
    """Microseconds of k_gram_nt_weighted per call, from the ctx's event timeline."""
    from gglasso_amd._lib import check, ptr
    us = []
    for it in range(rounds + 1):
        check(eng.lib.ggl_trace_start(eng.h, 16))
        check(eng.lib.ggl_set_S_from_weighted(eng.h, ptr(X), X.shape[1], ptr(w), flags))
        rows = np.zeros((16, 4))
        n = check(eng.lib.ggl_trace_read(eng.h, ptr(rows), 16))
        t = {int(r[2]): r[3] for r in rows[:n] if r[0] == 0.0}
        if it:
            us.append(t[31] - t[30])
    return us


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--p", type=int, default=500)
    ap.add_argument("--N", type=int, default=2000)
    ap.add_argument("--K", type=int, default=50)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--device-only", action="store_true", help="skip the host routes")
    args = ap.parse_args()
    from gglasso_amd import _lib, utils
    from gglasso_amd.solver import HipEngine
    p, N, K = args.p, args.N, args.K
    rng = np.random.default_rng(0)
    X = np.ascontiguousarray(rng.standard_normal((p, N)) + rng.uniform(-10, 10, (p, 1)))
    times, at = np.arange(float(N)), np.linspace(0, N - 1, K)
    width = 2.0 * np.sqrt(2.0 * 53.0 * np.log(2.0))               # support of the Gaussian at the default cutoff, in bandwidths
    eye = np.broadcast_to(np.eye(p), (K, p, p))
    eng = HipEngine(eye, eye, eye, 0 * eye)
    try:
        for what, h, cutoff in (("N", float(N), 0.0), ("N/4", N / 4 / width, 2.0 ** -53), ("N/10", N / 10 / width, 2.0 ** -53)):
            w = utils.kernel_weights(times, at, h, cutoff=cutoff)
            lens = [int(np.flatnonzero(r)[-1] - np.flatnonzero(r)[0] + 1) for r in w]
            routes = {"weighted": lambda: utils.kernel_covariance(X, at=at, bandwidth=h, cutoff=cutoff),
                      "scaled": lambda: utils.sample_covariance(scaled_copies(X, w, False), center=False),
                      "support": lambda: utils.sample_covariance(scaled_copies(X, w, True), center=False)}
            if not args.device_only:
                routes["numpy"] = lambda: np.stack([np.cov(X, aweights=wk, bias=True) for wk in w])
            out = {"support": what, "bandwidth": h, "K": K, "p": p, "N": N, "rounds": args.rounds,
                   "mean_support": float(np.mean(lens)), "max_support": int(np.max(lens))}
            for name, ms in rounds_ms(routes, args.rounds).items():
                out[name] = summary(ms)
            for name, flags in (("gram_us", _lib.COV_CENTER), ("gram_full_range_us", _lib.COV_CENTER | _lib.COV_FULL_RANGE)):
                us = gram_kernel_us(eng, X, w, flags, args.rounds)
                out[name] = {"median": float(np.median(us)), "min": float(np.min(us)), "max": float(np.max(us))}
            S = utils.kernel_covariance(X, at=at, bandwidth=h, cutoff=cutoff)[0]
            B = np.stack(list(utils.sample_covariance(scaled_copies(X, w, True), center=False).values()))
            out["max_abs_diff_weighted_vs_support"] = float(np.abs(S - B).max())
            print(json.dumps(out), flush=True)
    finally:
        eng.close()


if __name__ == "__main__":
    main()
