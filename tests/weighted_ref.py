"""Comparison value and derived error bound of the weighted covariance (csrc/covariance_weighted.hip, utils.weighted_covariance,
utils.host_weighted_covariance), shared by test_cpu_weighted.py and test_gpu_weighted_cov.py.

Comparison value: the two-pass formula in numpy.longdouble,

    W = sum_n w_n,   m = (1/W) sum_n w_n x_n,   S = (1/W) sum_n w_n (x_n - m)(x_n - m)^T.

Bound.  u = 2^-53, wt = w / W, xc = x - m, n = the length of the support of w (last minus first positive weight, plus one),
A_ij = sum_n wt_n |xc_in| |xc_jn|, M_i = sum_n wt_n |x_in|:

    |S_dev - S_ref|_ij <= (2 n + 12) u A_ij + ((2 n + 2) u)^2 M_i M_j

Derivation against what the kernels do (first order in u; entries outside the support are exact zeros and round nothing):

* k_weight_prepare: W^ = W (1 + t1), |t1| <= (n - 1) u for a sum of n non-negative terms in any order (here: per lane, then
  the xor tree); r^_n = sqrt(w_n) (1 + d), |d| <= u.
* k_row_means_weighted: the numerator sum_n w_n x_in is n fused multiply-adds in any order, error <= n u sum w |x_i|; the
  division by W^ adds (n - 1) u + u.  So |m^_i - m_i| <= 2 n u M_i, taken as (2 n + 2) u M_i.
* k_gram_nt_weighted stages a_in = fl(r^_n fl(x_in - m^_i)): one square root, one subtraction, one product per operand, so
  a_in a_jn = w_n (x_in - m^_i)(x_jn - m^_j)(1 + 6 d).  The matrix cores sum n such products in a fixed order (<= n u), the
  epilogue divides by W^ ((n - 1) u + u).  Together (2 n + 6) u; the comparison value's own rounding and the terms of higher
  order take the rest of the 12.  That is the first term.
* With dm = m^ - m: sum wt (xc_i - dm_i)(xc_j - dm_j) = S_ij + dm_i dm_j, because sum wt xc = 0 -- the rounded mean enters in
  second order only, |dm_i dm_j| <= ((2 n + 2) u)^2 M_i M_j.  That is the second term.  (Mixed terms, a rounding of the first
  kind times dm, are of order (n u)^2 M_i sum wt |xc_j|; they are left to the slack of the constants above.)
* center=False: m^ = m = 0 exactly, the subtraction rounds nothing: the first term alone, with xc = x.

host_weighted_covariance (numpy: x - m, times w, a BLAS product, one division) rounds fewer times per term (no square
roots) and sums in another order; the same bound covers it.
"""
import numpy as np

U = 2.0 ** -53


def make_data(p, N, seed):
    """mean + std * z with per-row means in [-1e3, 1e3] and std in [0.1, 10] (as test_gpu_covariance.make_data): a wrong or
    unweighted mean is ~1e6 against a bound of ~1e-13."""
    rng = np.random.default_rng([20241018, p, N, seed])
    mean = rng.uniform(-1e3, 1e3, (p, 1))
    std = rng.uniform(0.1, 10.0, (p, 1))
    return mean + std * rng.standard_normal((p, N))


def support(w):
    """[lo, hi) of one weight row: first and one-past-last index with w > 0."""
    nz = np.flatnonzero(np.asarray(w) > 0)
    return int(nz[0]), int(nz[-1]) + 1


def reference(X, w, center=True):
    """(S in longdouble, elementwise bound) of one weight row w (N,)."""
    Xl, wl = X.astype(np.longdouble), np.asarray(w).astype(np.longdouble)
    lo, hi = support(w)
    n = hi - lo
    wt = wl / wl.sum()
    m = (Xl * wt).sum(axis=1, keepdims=True) if center else np.zeros((X.shape[0], 1), dtype=np.longdouble)
    Xc = Xl - m
    S = (Xc * wt) @ Xc.T
    A = (np.abs(Xc) * wt) @ np.abs(Xc).T
    bound = (2 * n + 12) * U * A
    if center:
        M = (np.abs(Xl) * wt).sum(axis=1)
        bound = bound + ((2 * n + 2) * U) ** 2 * np.outer(M, M)
    return S, bound


def ratio(S, X, w, center=True, ref=None):
    """max over the entries of |S - S_ref| / bound (0 / 0 counts as 0: an entry that must be, and is, exact); ref: what
    ``reference(X, w, center)`` returned, where several results share it."""
    ref, bound = reference(X, w, center) if ref is None else ref
    err = np.abs(S.astype(np.longdouble) - ref)
    with np.errstate(divide='ignore', invalid='ignore'):
        r = np.where(err == 0, 0.0, err / bound)
    return float(r.max())


def check(S, X, w, center, what, ref=None):
    """S (p,p) within the bound of row w, and exactly symmetric; prints and returns max(err / bound)."""
    r = ratio(S, X, w, center, ref)
    print(what, "max err/bound", r)
    assert r <= 1.0, (what, r)
    assert np.array_equal(S, S.T), what
    return r
