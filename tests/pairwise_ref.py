"""Reference, error bound and test data of the pairwise-complete covariance (tests/test_cpu_pairwise_ref.py,
tests/test_gpu_pairwise_cov.py).

Definition (X (p,N), variables in rows, NaN = missing, O_ij the samples where x_i and x_j are both observed, n_ij = |O_ij|):

    S_ij = (1/n_ij) sum_{O_ij} (x_in - m_i|j)(x_jn - m_j|i),   m_i|j = (1/n_ij) sum_{O_ij} x_in        center=True
    S_ij = (1/n_ij) sum_{O_ij} x_in x_jn                                                               center=False

``reference`` evaluates it in numpy.longdouble straight from the masks, pair by pair, without the four-product identity.

Bound (u = 2^-53): with y = x - (mean of the observed entries of the row) for center=True -- the operand the kernel forms --
and y = x for center=False, and D_ij = (1/n_ij) sqrt(sum_{O_ij} y_i^2 sum_{O_ij} y_j^2),

    |S_dev - S_ref|_ij <= (3 n_ij + 16) u D_ij.

To first order: P = sum y_i y_j, A = sum y_i, B = sum y_j over O_ij are sums of at most n_ij terms in any order, each with
error <= n_ij u sum |terms|; sum |y_i y_j| <= n_ij D and |A| |B| / n_ij^2 <= D by Cauchy-Schwarz (three times n_ij u D); the
rest is the rounding of x - c, of the product A B, of the two divisions and of the subtraction, and the comparison value's
own rounding (16 u D covers them).  For center=False only the first term and the division exist.
"""
import numpy as np

U = 2.0 ** -53
PATTERNS = ("none", "r30", "r60", "lastcol", "lastrow", "slab", "eqmean", "minpairs")


def reference(X, center=True):
    """(S longdouble (p,p), n_ij int64 (p,p), D longdouble (p,p)); a pair without a shared sample gets NaN in S and D."""
    X = np.asarray(X, dtype=np.float64)
    p, N = X.shape
    obs = ~np.isnan(X)
    Xl = np.where(obs, X, 0.0).astype(np.longdouble)
    n = obs.astype(np.int64) @ obs.astype(np.int64).T
    if center:
        row_n = np.maximum(obs.sum(axis=1, keepdims=True), 1)
        Yl = np.where(obs, Xl - Xl.sum(axis=1, keepdims=True) / row_n, 0).astype(np.longdouble)
    else:
        Yl = Xl
    S = np.full((p, p), np.nan, dtype=np.longdouble)
    D = np.full((p, p), np.nan, dtype=np.longdouble)
    for i in range(p):
        both = obs[i][None, :] & obs                                   # (p,N): O_ij for every j
        nij = both.sum(axis=1).astype(np.longdouble)
        ok = nij > 0
        nn = np.where(ok, nij, 1)
        xi = np.where(both, Xl[i][None, :], 0)
        xj = np.where(both, Xl, 0)
        if center:
            xi = np.where(both, xi - (xi.sum(axis=1) / nn)[:, None], 0)
            xj = np.where(both, xj - (xj.sum(axis=1) / nn)[:, None], 0)
        s = (xi * xj).sum(axis=1) / nn
        yi = np.where(both, Yl[i][None, :], 0)
        yj = np.where(both, Yl, 0)
        d = np.sqrt((yi * yi).sum(axis=1) * (yj * yj).sum(axis=1)) / nn
        S[i, ok], D[i, ok] = s[ok], d[ok]
    return S, n, D


def bound(n, D):
    return (3 * n.astype(np.longdouble) + 16) * U * D


def ratio(S, ref):
    """Largest |S - S_ref| / bound over the pairs that share a sample (0 / 0 counts as 0: an exact result at a zero bound);
    inf where the result misses a zero bound or is not finite."""
    Sr, n, D = ref
    ok = n > 0
    err = np.abs(np.asarray(S, dtype=np.longdouble) - Sr)[ok]
    b = bound(n, D)[ok]
    if not np.all(np.isfinite(err.astype(np.float64))):
        return np.inf
    r = np.where(err == 0, 0, err / np.where(b > 0, b, 1))
    r = np.where((b == 0) & (err > 0), np.inf, r)
    return float(r.max()) if r.size else 0.0


def make_data(p, N, seed):
    """The generator of tests/test_gpu_covariance.py: row means in +-1e3, std in 0.1-10, so a wrong centring or a padded column
    that leaks is ~1e6 against a bound of ~1e-13."""
    rng = np.random.default_rng([20241018, p, N, seed])
    mean = rng.uniform(-1e3, 1e3, (p, 1))
    std = rng.uniform(0.1, 10.0, (p, 1))
    return mean + std * rng.standard_normal((p, N))


def make_case(p, N, pattern, seed=0):
    """Complete data with the holes of ``pattern`` punched in, or None where the shape has no room for it.  The first two
    columns stay observed in every row (min_pairs = 2 then holds for every pair), except where the pattern says otherwise."""
    X = make_data(p, N, seed)
    rng = np.random.default_rng([7, p, N, seed, PATTERNS.index(pattern)])
    if pattern == "none":
        return X
    if pattern in ("r30", "r60"):
        if N < 3:
            return None
        hole = rng.random((p, N)) < (0.3 if pattern == "r30" else 0.6)
        hole[:, :2] = False
        X[hole] = np.nan
        return X
    if pattern == "lastcol":                 # the clamped fetch past the last sample reads this column
        if N < 3 or N % 16 == 0:
            return None
        X[:, N - 1] = np.nan
        return X
    if pattern == "lastrow":                 # the clamped fetch past the last variable reads this row
        if N < 3 or p % 32 == 0 or p < 2:
            return None
        X[p - 1, 2:] = np.nan
        return X
    if pattern == "slab":                    # a whole k-slab of one operand is missing
        if N < 35:
            return None
        X[p // 2, 2:34] = np.nan
        return X
    if pattern == "eqmean":                  # observed entries EQUAL to the row's observed mean: y = 0 with w = 1
        if N < 4:
            return None
        r = p // 3
        X[r] = 7.0
        X[r, 0], X[r, 1] = 6.0, 8.0
        X[r, N - 1] = np.nan
        assert np.nanmean(X[r]) == 7.0
        return X
    if pattern == "minpairs":                # variables 0 and 1 share exactly the first two samples
        if N < 4 or p < 2:
            return None
        half = 2 + (N - 2) // 2
        X[0, half:] = np.nan
        X[1, 2:half] = np.nan
        return X
    raise ValueError(pattern)
