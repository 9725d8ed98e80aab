"""ADMM_FSGL against its yardstick ADMM_SGL on one MI355X: median ADMM iterations per second over 7 regions and the per-phase
device profile of both, on covariances of the same recipe (same Omega-step, same bytes in the Theta-step).

    python tools/bench_fsgl.py [--p 100] [--M 10] [--steps 30] [--warmup 10]

FSGL at (p, M), i.e. dimension p*M; SGL at dimension p*M.  Prints one JSON line at the end."""
import argparse
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def make_S(p, M, N, seed=7):
    rng = np.random.default_rng(seed)
    pM = p * M
    adj = np.triu(rng.random((p, p)) < 3.0 / p, 1)
    Th = np.zeros((pM, pM))
    for i, j in zip(*np.nonzero(adj)):
        Th[i * M:(i + 1) * M, j * M:(j + 1) * M] = 0.3 * rng.standard_normal((M, M))
    Th = Th + Th.T
    Th += (0.5 - np.linalg.eigvalsh(Th).min()) * np.eye(pM)
    Sigma = np.linalg.inv(Th)
    X = rng.multivariate_normal(np.zeros(pM), 0.5 * (Sigma + Sigma.T), size=N, method="cholesky")
    return np.cov(X.T, bias=True)


def run(reg, S, lam, M, steps, warmup, regions=7):
    from gglasso_amd import solver
    pM = S.shape[0]
    I = np.eye(pM)[None]
    eng = solver.HipEngine(S[None], I, I, np.zeros_like(I))
    try:
        if reg == "FSGL":
            eng.set_block_size(M)
        nk = np.ones(1)
        eng.save_state()
        rates = []
        for _ in range(regions):
            eng.restore_state()
            for _ in range(warmup):
                eng.step(1.0, lam, 0.0, reg, False, None, nk)
            eng.sync()
            t0 = time.perf_counter()
            for _ in range(steps):
                eng.step(1.0, lam, 0.0, reg, False, None, nk)
            eng.sync()
            rates.append(steps / (time.perf_counter() - t0))
        eng.restore_state()
        eng.profile(1)
        for _ in range(steps):
            eng.step(1.0, lam, 0.0, reg, False, None, nk)
        prof = {k: {"ms_per_step": v[0] / steps, "launches": v[1]} for k, v in eng.profile_read().items() if v[1]}
        eng.profile(0)
        return {"it_per_s_median": float(np.median(rates)), "it_per_s": [float(r) for r in rates], "profile": prof,
                "theta_kernel": eng.last_dispatch()["theta_kernel"]}
    finally:
        eng.close()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--p", type=int, default=100)
    ap.add_argument("--M", type=int, default=10)
    ap.add_argument("--steps", type=int, default=30)
    ap.add_argument("--warmup", type=int, default=10)
    ap.add_argument("--only", choices=("FSGL", "SGL"), default=None, help="one side only (for a profiler run)")
    a = ap.parse_args()
    pM = a.p * a.M
    S = make_S(a.p, a.M, 3 * pM)
    from gglasso_amd import utils
    lam_f = 0.3 * utils.lambda_max_fsgl(S, a.M)
    off = np.abs(S - np.diag(np.diag(S)))
    lam_s = 0.3 * off.max()
    out = {"pM": pM, "p": a.p, "M": a.M, "steps": a.steps, "warmup": a.warmup}
    for reg, lam in (("FSGL", lam_f), ("SGL", lam_s)):
        if a.only and reg != a.only:
            continue
        out[reg] = run(reg, S, float(lam), a.M, a.steps, a.warmup)
        th = out[reg]["profile"].get("theta", {}).get("ms_per_step", float("nan"))
        # Theta-step traffic of the non-latent step: Omega, X, Omega_prev read, Theta, X written: 5 stacks of pM^2 doubles
        gbs = 5 * pM * pM * 8 / (th * 1e-3) / 1e9
        out[reg]["theta_GBps"] = gbs
        print(f"{reg:5s} pM={pM}: {out[reg]['it_per_s_median']:.1f} it/s (median of 7), Theta phase {th * 1e3:.1f} us "
              f"= {gbs:.0f} GB/s" + (f", Theta kernel code {out[reg]['theta_kernel']}" if reg == "FSGL" else ""))
        for k, v in out[reg]["profile"].items():
            print(f"      {k:12s} {v['ms_per_step'] * 1e3:9.1f} us/step  {v['launches']} launches")
    if not a.only:
        out["fsgl_over_sgl"] = out["FSGL"]["it_per_s_median"] / out["SGL"]["it_per_s_median"]
        print(f"FSGL / SGL rate: {out['fsgl_over_sgl']:.3f}")
    print(json.dumps(out))


if __name__ == "__main__":
    main()
