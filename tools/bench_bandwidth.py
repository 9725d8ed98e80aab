"""Measurements behind DESIGN 25 (profiles/bandwidth_selection.txt): the leave-one-out bandwidth search on the device against
its numpy twin, k_chol_predict against the vendor's batched Cholesky + triangular solve, and the block update on the matrix
cores against the same kernel with the update on the VALU.

    python tools/bench_bandwidth.py [--rounds 5] [--host-eval 200] [--once]

Routes alternate within a round; every figure is the median (min-max) of the rounds.  --once runs one device search at
p = 100 and nothing else (the run a kernel trace is taken from)."""
import argparse
import ctypes
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))


def series(p, N, seed=0):
    rng = np.random.default_rng(seed)
    A = np.eye(p) + 0.3 * rng.standard_normal((p, p)) / np.sqrt(p)
    return A @ rng.standard_normal((p, N))


def fmt(v, unit="ms"):
    v = np.asarray(v, dtype=float)
    return f"{np.median(v):.3f} ({v.min():.3f}-{v.max():.3f}) {unit}"


def wall(fn):
    t0 = time.perf_counter()
    fn()
    return (time.perf_counter() - t0) * 1e3


def chol_bench(K, p, iters):
    from gglasso_amd import _lib
    out = (ctypes.c_double * 3)()
    _lib.check(_lib.load().ggl_dev_chol_bench(K, p, iters, out))
    return out[0], out[1], out[2]


def torch_chol(K, p, iters):
    """cholesky_ex + solve_triangular + the two reductions on a device stack, torch events, ms per call"""
    import torch
    g = torch.Generator(device="cpu").manual_seed(0)
    A = torch.rand((p, p), generator=g, dtype=torch.float64) - 0.5
    A = (0.5 * (A + A.T) + (1.0 + p) * torch.eye(p, dtype=torch.float64)).cuda().expand(K, p, p).contiguous()
    d = (torch.rand((K, p, 1), generator=g, dtype=torch.float64) - 0.5).cuda()

    def run():
        L, info = torch.linalg.cholesky_ex(A)
        y = torch.linalg.solve_triangular(L, d, upper=False)
        return 2.0 * torch.log(torch.diagonal(L, dim1=1, dim2=2)).sum(dim=1), (y * y).sum(dim=(1, 2)), info
    for _ in range(3):
        run()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    e0.record()
    for _ in range(iters):
        run()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / iters


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--host-eval", type=int, default=200)
    ap.add_argument("--once", action="store_true")
    a = ap.parse_args()
    from gglasso_amd import utils
    hs = [400.0, 200.0, 100.0, 60.0, 40.0, 30.0]
    X = series(100, 2000)
    if a.once:
        SC, ST = utils.loo_bandwidth_scores(X, hs)
        print("one search p=100 N=2000 H=6 M=2000: CV", SC.mean(axis=1), "not PD", int((ST >= 0).sum()))
        return
    utils.loo_bandwidth_scores(X, hs[:1], eval_index=50)                      # warm-up: library, context
    dev, dev_sub, host_sub = [], [], []
    for _ in range(a.rounds):
        dev.append(wall(lambda: utils.loo_bandwidth_scores(X, hs)))
        host_sub.append(wall(lambda: utils.host_loo_bandwidth_scores(X, hs, eval_index=a.host_eval)))
        dev_sub.append(wall(lambda: utils.loo_bandwidth_scores(X, hs, eval_index=a.host_eval)))
    print(f"search p=100 N=2000 H=6, all 2000 samples, device:           {fmt(dev)}")
    print(f"search p=100 N=2000 H=6, {a.host_eval} samples, device:               {fmt(dev_sub)}")
    print(f"search p=100 N=2000 H=6, {a.host_eval} samples, numpy twin:           {fmt(host_sub)}")
    X5 = series(500, 2000, 1)
    h5 = [400.0, 200.0, 100.0, 60.0, 40.0, 30.0]
    t5 = [wall(lambda: utils.loo_bandwidth_scores(X5, h5, eval_index=200, ridge=1e-2)) for _ in range(a.rounds)]
    SC, ST = utils.loo_bandwidth_scores(X5, h5, eval_index=200, ridge=1e-2)
    print(f"search p=500 N=2000 H=6, 200 samples, ridge 1e-2, device:    {fmt(t5)}   not PD: {int((ST >= 0).sum())}")
    for K, p, iters in ((2000, 100, 20), (200, 500, 10)):
        mf, va, cp, tc = [], [], [], []
        for _ in range(a.rounds):
            m, v, c = chol_bench(K, p, iters)
            mf.append(m), va.append(v), cp.append(c)
            tc.append(torch_chol(K, p, iters))
        print(f"k_chol_predict K={K} p={p}: matrix cores {fmt(mf)}   VALU update {fmt(va)}   (restoring copy {fmt(cp)})")
        print(f"torch cholesky_ex + solve_triangular + reductions K={K} p={p}: {fmt(tc)}")


if __name__ == "__main__":
    main()
