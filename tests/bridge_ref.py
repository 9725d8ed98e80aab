"""TEST-ONLY reference of the latent correlation of mixed binary / continuous data (Fan, Liu, Ning, Zou 2017): the bridge
functions by scipy's adaptive quadrature, the thresholds by scipy's normal quantile, the roots by Brent's method, tau-a from
the brute-force counts of kendall_ref.  Nothing here shares code with the package.

    g(t; h, k) = exp(-(h^2 + k^2 - 2 h k sin t) / (2 cos^2 t))
    binary, binary:      F(r) = (1/pi) int_0^{asin r}         g(t; D_i, D_j) dt = 2 (Phi_2(D_i, D_j; r) - Phi(D_i) Phi(D_j))
    binary, continuous:  F(r) = (2/pi) int_0^{asin(r/sqrt 2)} g(t; D, 0) dt     = 4 Phi_2(D, 0; r / sqrt 2) - 2 Phi(D)
"""
import math
import warnings

import numpy as np
from scipy import integrate, optimize, special

from kendall_ref import counts_ref

CLIP = 0.999


def F_ref(r, h, k, bb):
    """The bridge function at r: ``bb`` both binary (thresholds h, k), else binary / continuous (threshold h)."""
    if not bb:
        k = 0.0
    h, k = float(h), float(k)                            # (python floats and the math module: quad calls g point by point)
    g = lambda t: math.exp(-(h * h + k * k - 2.0 * h * k * math.sin(t)) / (2.0 * math.cos(t) ** 2))
    top = math.asin(r) if bb else math.asin(r / math.sqrt(2.0))
    with warnings.catch_warnings():
        warnings.simplefilter("ignore", integrate.IntegrationWarning)      # (1e-15 is at the rounding level: quad says so)
        val = integrate.quad(g, 0.0, top, epsabs=1e-15, epsrel=1e-15)[0]
    return val / np.pi if bb else 2.0 * val / np.pi


def dF_ref(r, h, k, bb):
    """F'(r), analytic."""
    if bb:
        return np.exp(-(h * h + k * k - 2.0 * h * k * r) / (2.0 * (1.0 - r * r))) / (np.pi * np.sqrt(1.0 - r * r))
    s = r / np.sqrt(2.0)
    return (2.0 / np.pi) * np.exp(-h * h / (2.0 * (1.0 - s * s))) / np.sqrt(2.0 - r * r)


def delta_ref(n0, n):
    return float(special.ndtri(n0 / n))


def r_ref(tau, h, k, bb, clip=CLIP):
    """(the root of F = tau in [-clip, clip], whether it was clipped)."""
    if tau <= F_ref(-clip, h, k, bb):
        return -clip, True
    if tau >= F_ref(clip, h, k, bb):
        return clip, True
    return optimize.brentq(lambda r: F_ref(r, h, k, bb) - tau, -clip, clip, xtol=1e-15, rtol=8.9e-16), False


def types_ref(X):
    return np.array([len(set(x.tolist())) == 2 for x in X], dtype=np.int32)


def pair_table(X, types=None, clip=CLIP):
    """Every pair i < j of X (p,N) that involves a binary variable: a list of dicts with i, j, tau (tau-a), h, k, bb, r
    (the reference root), clipped -- and the (p,) zero counts and the counts G."""
    X = np.asarray(X, dtype=np.float64)
    p, n = X.shape
    t = types_ref(X) if types is None else np.asarray(types)
    G = counts_ref(X)
    n0 = np.array([int(np.sum(x == x.min())) for x in X])
    d = [delta_ref(n0[i], n) if t[i] else 0.0 for i in range(p)]
    rows = []
    for i in range(p):
        for j in range(i + 1, p):
            if not (t[i] or t[j]):
                continue
            bb = bool(t[i] and t[j])
            h, k = (d[i], d[j]) if bb else ((d[i] if t[i] else d[j]), 0.0)
            tau = G[i, j] / (n * (n - 1) // 2)
            r, cl = r_ref(tau, h, k, bb, clip)
            rows.append(dict(i=i, j=j, tau=tau, h=h, k=k, bb=bb, r=r, clipped=cl))
    return rows, n0, G


def latent_truth(p, rho=0.6):
    return rho ** np.abs(np.subtract.outer(np.arange(p), np.arange(p)))


def make_mixed(p, N, n_binary, seed):
    """(p,N) mixed data of a Gaussian copula with AR(1) latent correlation 0.6: n_binary rows dichotomised at the cut points
    ndtri(U(0.2, 0.8)) and interleaved with the continuous rows, which are passed through exp."""
    rng = np.random.default_rng([20250607, p, N, n_binary, seed])
    Z = np.linalg.cholesky(latent_truth(p)) @ rng.standard_normal((p, N))
    cut = special.ndtri(rng.uniform(0.2, 0.8, p))
    X = np.exp(Z)
    for i in sorted(range(p), key=lambda i: (i % 2, i))[:n_binary]:         # the even rows first: binary beside continuous
        X[i] = (Z[i] > cut[i]).astype(np.float64)
    return X
