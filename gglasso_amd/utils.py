"""Utilities on the device: the block norms of the Functional Graphical Lasso (reference: helper/utils.py:69-107 of
fabian-sp/GGLasso) and the sample covariance of observations (what helper/data_generation.py:221,234 gets from numpy.cov)."""
import ctypes

import numpy as np

from . import _lib
from ._lib import as_c, check, ptr


def frob_norm_per_block(S, M, off_diag=False):
    """helper/utils.py:69-87: the (p,p) table of Frobenius norms of the M x M blocks of the (pM,pM) matrix S (the upper
    blocks decide, the lower ones mirror them); ``off_diag``: zero diagonal."""
    S = as_c(S)
    assert S.ndim == 2 and S.shape[0] == S.shape[1]
    pM = S.shape[0]
    assert pM % M == 0
    p = pM // int(M)
    out = np.empty((p, p))
    _lib.require_gpu()
    check(_lib.load().ggl_frob_norm_per_block(pM, int(M), ptr(S), int(bool(off_diag)), ptr(out)))
    return out


def lambda_max_fsgl(S, M):
    """helper/utils.py:89-107: the smallest lambda1 for which every off-diagonal block of the FSGL solution is zero,
    max_{j != l} |S^M_jl|_F."""
    return frob_norm_per_block(S, M, off_diag=True).max()


def _covariance_call(Xs, flags, device=0):
    """One ``ggl_covariance`` call: ``Xs`` a list of C-contiguous float64 (p, N_k) arrays of one p.  Returns
    (S (K,p,p), variances (K,p) or None)."""
    K, p = len(Xs), Xs[0].shape[0]
    N = (ctypes.c_int * K)(*[x.shape[1] for x in Xs])
    Xp = (_lib._dp * K)(*[ptr(x) for x in Xs])
    S = np.empty((K, p, p))
    var = np.empty((K, p)) if flags & _lib.COV_SCALE else None
    _lib.require_gpu()
    check(_lib.load().ggl_covariance(int(device), K, p, N, Xp, int(flags), ptr(S), ptr(var)))
    return S, var


def _data_list(X):
    """(kind, list of C-contiguous float64 (p_k, N_k) arrays) of what ``sample_covariance`` accepts."""
    if isinstance(X, dict):
        assert sorted(X.keys()) == list(range(len(X))), "a dict of data needs the keys 0,...,K-1"
        kind, Xs = "dict", [X[k] for k in range(len(X))]
    elif isinstance(X, (list, tuple)):
        kind, Xs = "dict", list(X)
    else:
        X = np.asarray(X)
        assert X.ndim in (2, 3), f"The specified data has shape {X.shape}, use (p,N), (K,p,N) or a list/dict of (p_k,N_k) arrays"
        kind, Xs = ("2d", [X]) if X.ndim == 2 else ("3d", list(X))
    assert len(Xs) >= 1, "no data"
    Xs = [as_c(x) for x in Xs]
    for k, x in enumerate(Xs):
        assert x.ndim == 2 and x.shape[0] >= 1 and x.shape[1] >= 1, \
            f"instance {k}: data must be a (p,N) array with variables in rows, has shape {x.shape}"
    return kind, Xs


def sample_covariance(X, center=True, scale=False, device=0, missing=None, min_pairs=2, return_counts=False):
    """``numpy.cov(X_k, bias=True)`` of every instance on the device (FP64 matrix cores; bitwise symmetric and reproducible).

    X: (p,N), (K,p,N), or a list / dict (keys 0..K-1) of (p_k,N_k) arrays, variables in rows (the reference's ``sample[k]``).
    Returns S of the matching kind -- (p,p), (K,p,p), or a dict with keys 0..K-1.  ``center=False``: the raw second moment.
    ``scale=True``: the correlations, and as a second return value the variances (same kind, (p,), (K,p) or dict).
    Instances of different dimension take one library call per distinct p_k.

    ``missing='pairwise'``: a NaN in X is a missing value and S is the pairwise-complete covariance
    (``ggl_covariance_pairwise``): entry (i,j) is the covariance of x_i and x_j over the ``n_ij`` samples where both are
    observed, normalised by ``1/n_ij`` -- ``pandas.DataFrame(X.T).cov() * (n - 1) / n``.  S can be indefinite and is returned
    as it is.  A variable without observations, or a pair with ``n_ij < min_pairs``, is refused, naming it.  ``scale=True``
    divides by the diagonal of this S (each variable's variance over all its observed entries): unit diagonal, but an
    off-diagonal entry can exceed 1 in magnitude.  ``return_counts=True``: the int32 ``n_ij`` come back as one more value of the
    matching kind.  ``missing=None`` (default) is the complete-data path, where a NaN spreads over its row and column."""
    assert missing in (None, 'pairwise'), "missing must be None (complete data) or 'pairwise'"
    if missing == 'pairwise':
        return _sample_covariance_pairwise(X, center, scale, device, min_pairs, return_counts)
    assert not return_counts, "return_counts needs missing='pairwise' (on complete data every count is N)"
    kind, Xs = _data_list(X)
    flags = (_lib.COV_CENTER if center else 0) | (_lib.COV_SCALE if scale else 0)
    S, var = [None] * len(Xs), [None] * len(Xs)
    for p in sorted({x.shape[0] for x in Xs}):
        idx = [k for k, x in enumerate(Xs) if x.shape[0] == p]
        Sp, vp = _covariance_call([Xs[k] for k in idx], flags, device)
        for j, k in enumerate(idx):
            S[k] = Sp[j]
            var[k] = vp[j] if scale else None
    if kind == "2d":
        S, var = S[0], var[0]
    elif kind == "3d":
        S, var = np.stack(S), (np.stack(var) if scale else None)
    else:
        S = {k: np.array(S[k]) for k in range(len(Xs))}
        var = {k: np.array(var[k]) for k in range(len(Xs))} if scale else None
    return (S, var) if scale else S


def _subset_indices(indices):
    """The (B, b) int32 array of column indices of ``sample_covariance_subsets`` (the library checks B, b and the range)."""
    idx = np.asarray(indices)
    assert idx.ndim == 2 and np.issubdtype(idx.dtype, np.integer), \
        f"indices must be a (B, b) integer array, is {idx.dtype} of shape {idx.shape}"
    assert idx.size == 0 or (idx.min() >= -2 ** 31 and idx.max() < 2 ** 31), "indices do not fit 32 bits"
    return np.ascontiguousarray(idx, dtype=np.int32)


def _covariance_subsets_call(X, idx, flags, device=0):
    """One ``ggl_covariance_subsets`` call: X C-contiguous float64 (p, N), idx C-contiguous int32 (B, b).  Returns
    (S (B,p,p), variances (B,p) or None)."""
    (p, N), (B, b) = X.shape, idx.shape
    S = np.empty((B, p, p))
    var = np.empty((B, p)) if flags & _lib.COV_SCALE else None
    _lib.require_gpu()
    check(_lib.load().ggl_covariance_subsets(int(device), p, N, ptr(X), B, b, idx.ctypes.data_as(_lib._ip), int(flags), ptr(S),
                                             ptr(var)))
    return S, var


def sample_covariance_subsets(X, indices, center=True, scale=False, device=0, missing=None, min_pairs=2, return_counts=False):
    """``numpy.cov(X[:, indices[r]], bias=True)`` for every row r of ``indices`` (B, b) on the device: X (p, N), variables in
    rows, goes up once and the columns are gathered there -- the subsamples of ``model_selection.stars_search``.  Duplicate
    indices are allowed (a bootstrap draw).  Returns S (B,p,p), bitwise what ``sample_covariance`` gives for the B gathered
    arrays as one (B,p,b) stack; ``scale=True``: each subset's own correlations, and as a second value the variances (B,p).
    ``missing='pairwise'``, ``min_pairs``, ``return_counts``: as in ``sample_covariance`` (the counts are (B,p,p) int32)."""
    assert missing in (None, 'pairwise'), "missing must be None (complete data) or 'pairwise'"
    X = as_c(X)
    assert X.ndim == 2 and X.shape[0] >= 1 and X.shape[1] >= 1, \
        f"data must be a (p,N) array with variables in rows, has shape {X.shape}"
    flags = (_lib.COV_CENTER if center else 0) | (_lib.COV_SCALE if scale else 0)
    if missing == 'pairwise':
        S, var, cnt = _covariance_pairwise_subsets_call(X, _subset_indices(indices), flags, min_pairs, return_counts, device)
        out = (S,) + ((var,) if scale else ()) + ((cnt,) if return_counts else ())
        return out if len(out) > 1 else S
    assert not return_counts, "return_counts needs missing='pairwise' (on complete data every count is b)"
    S, var = _covariance_subsets_call(X, _subset_indices(indices), flags, device)
    return (S, var) if scale else S


# -----------------------------------------------------------------------------------------------------------------
# Pairwise-complete covariance of data with missing values (NaN): csrc/covariance_missing.hip behind ggl_covariance_pairwise
# -----------------------------------------------------------------------------------------------------------------
def _covariance_pairwise_call(Xs, flags, min_pairs=2, counts=True, device=0):
    """One ``ggl_covariance_pairwise`` call: ``Xs`` a list of C-contiguous float64 (p, N_k) arrays of one p.  Returns
    (S (K,p,p), variances (K,p) or None, counts (K,p,p) int32 or None)."""
    K, p = len(Xs), Xs[0].shape[0]
    N = (ctypes.c_int * K)(*[x.shape[1] for x in Xs])
    Xp = (_lib._dp * K)(*[ptr(x) for x in Xs])
    S = np.empty((K, p, p))
    var = np.empty((K, p)) if flags & _lib.COV_SCALE else None
    cnt = np.empty((K, p, p), dtype=np.int32) if counts else None
    _lib.require_gpu()
    check(_lib.load().ggl_covariance_pairwise(int(device), K, p, N, Xp, int(flags), int(min_pairs), ptr(S), ptr(var),
                                              None if cnt is None else cnt.ctypes.data_as(_lib._ip)))
    return S, var, cnt


def _covariance_pairwise_subsets_call(X, idx, flags, min_pairs=2, counts=True, device=0):
    """One ``ggl_covariance_pairwise_subsets`` call: X C-contiguous float64 (p, N), idx C-contiguous int32 (B, b).  Returns
    (S (B,p,p), variances (B,p) or None, counts (B,p,p) int32 or None)."""
    (p, N), (B, b) = X.shape, idx.shape
    S = np.empty((B, p, p))
    var = np.empty((B, p)) if flags & _lib.COV_SCALE else None
    cnt = np.empty((B, p, p), dtype=np.int32) if counts else None
    _lib.require_gpu()
    check(_lib.load().ggl_covariance_pairwise_subsets(int(device), p, N, ptr(X), B, b, idx.ctypes.data_as(_lib._ip), int(flags),
                                                      int(min_pairs), ptr(S), ptr(var),
                                                      None if cnt is None else cnt.ctypes.data_as(_lib._ip)))
    return S, var, cnt


def _sample_covariance_pairwise(X, center, scale, device, min_pairs, return_counts):
    """``sample_covariance(..., missing='pairwise')``: one library call per distinct p_k, results of the matching kind."""
    kind, Xs = _data_list(X)
    flags = (_lib.COV_CENTER if center else 0) | (_lib.COV_SCALE if scale else 0)
    S, var, cnt = [None] * len(Xs), [None] * len(Xs), [None] * len(Xs)
    for p in sorted({x.shape[0] for x in Xs}):
        idx = [k for k, x in enumerate(Xs) if x.shape[0] == p]
        Sp, vp, cp = _covariance_pairwise_call([Xs[k] for k in idx], flags, min_pairs, return_counts, device)
        for j, k in enumerate(idx):
            S[k] = Sp[j]
            var[k] = vp[j] if scale else None
            cnt[k] = cp[j] if return_counts else None
    out = [S] + ([var] if scale else []) + ([cnt] if return_counts else [])
    if kind == "2d":
        out = [a[0] for a in out]
    elif kind == "3d":
        out = [np.stack(a) for a in out]
    else:
        out = [{k: np.array(a[k]) for k in range(len(Xs))} for a in out]
    return tuple(out) if len(out) > 1 else out[0]


def host_pairwise_covariance(X, center=True, indices=None):
    """numpy counterpart of ``sample_covariance(..., missing='pairwise', return_counts=True)`` for one (p,N) array (engines
    without the device route): the four products of the kernel, ``P = Y Y^T, A = Y W^T, B = W Y^T, C = W W^T`` with ``y = x - c``
    (c: the mean of a row's observed entries) where observed and 0 where missing, ``w`` the mask, and
    ``S = (P - A B / C) / C`` (``center=False``: ``y = x``, ``S = P / C``).  Returns ``(S, counts)``: (p,p) arrays, or (B,p,p) with
    ``indices`` (B,b).  A pair without a shared sample gives NaN; nothing is refused here."""
    X = np.asarray(X, dtype=np.float64)
    assert X.ndim == 2, f"data must be a (p,N) array with variables in rows, has shape {X.shape}"
    subsets = [X] if indices is None else [X[:, np.asarray(ix)] for ix in np.asarray(indices)]
    S, cnt = [], []
    for Xr in subsets:
        obs = ~np.isnan(Xr)
        W = obs.astype(np.float64)
        n_row = np.maximum(W.sum(axis=1, keepdims=True), 1.0)
        X0 = np.where(obs, Xr, 0.0)
        Y = np.where(obs, Xr - X0.sum(axis=1, keepdims=True) / n_row, 0.0) if center else X0
        C = W @ W.T
        with np.errstate(invalid='ignore', divide='ignore'):
            S.append((Y @ Y.T - (Y @ W.T) * (W @ Y.T) / C) / C if center else (Y @ Y.T) / C)
        cnt.append(np.rint(C).astype(np.int32))
    S, cnt = np.stack(S), np.stack(cnt)
    return (S[0], cnt[0]) if indices is None else (S, cnt)


# -----------------------------------------------------------------------------------------------------------------
# Rank correlation: Kendall's tau-b and the nonparanormal skeptic matrix sin(pi/2 tau) (Liu, Han, Yuan, Lafferty, Wasserman
# 2012; the other input statistic of R's huge).  With Z[i,(a,b)] = sgn(x_ia - x_ib) over the sample pairs a < b, G = Z Z^T
# holds exact integers, G_ij = concordant - discordant pairs and G_ii = the pairs not tied in i, and tau-b = G_ij / sqrt(G_ii
# G_jj) with ties handled.  The library forms G on the int8 matrix cores from dense ranks (csrc/kendall.hip).
# -----------------------------------------------------------------------------------------------------------------
_llp = ctypes.POINTER(ctypes.c_longlong)


def dense_ranks(X):
    """The (p,N) int32 array of dense ranks of every row of ``X`` (p,N): equal values get equal ranks, 0 for the smallest.
    The sign of a rank difference is the sign of the value difference.  NaN and inf are refused."""
    X = np.asarray(X, dtype=np.float64)
    assert X.ndim == 2 and X.shape[0] >= 1 and X.shape[1] >= 1, \
        f"data must be a (p,N) array with variables in rows, has shape {X.shape}"
    assert np.isfinite(X).all(), "rank correlation needs finite data (NaN or inf found)"
    R = np.empty(X.shape, dtype=np.int32)
    for i in range(X.shape[0]):
        R[i] = np.unique(X[i], return_inverse=True)[1].reshape(-1)
    return R


def _kendall_call(R, idx, skeptic, device=0):
    """One ``ggl_kendall_counts`` / ``ggl_kendall_skeptic`` call: R C-contiguous int32 (p,N) dense ranks, idx C-contiguous
    int32 (B,b) or None (all samples, B = 1).  Returns (G (B,p,p) int64, S (B,p,p) or None)."""
    p, N = R.shape
    B, b = (1, N) if idx is None else idx.shape
    G = np.empty((B, p, p), dtype=np.int64)
    S = np.empty((B, p, p)) if skeptic else None
    ip = None if idx is None else idx.ctypes.data_as(_lib._ip)
    _lib.require_gpu()
    lib = _lib.load()
    if skeptic:
        check(lib.ggl_kendall_skeptic(int(device), p, N, R.ctypes.data_as(_lib._ip), B, b, ip, ptr(S), G.ctypes.data_as(_llp)))
    else:
        check(lib.ggl_kendall_counts(int(device), p, N, R.ctypes.data_as(_lib._ip), B, b, ip, G.ctypes.data_as(_llp)))
    return G, S


def host_kendall_counts(X, indices=None, chunk=1 << 22):
    """numpy counterpart of ``kendall_counts`` for one (p,N) array (engines without the device route): a brute force over the
    sample pairs, ``chunk`` sign entries at a time, summed in int64.  Returns (B,p,p), or (p,p) without ``indices``."""
    X = np.asarray(X, dtype=np.float64)
    assert X.ndim == 2 and np.isfinite(X).all(), "rank correlation needs a finite (p,N) array"
    p = X.shape[0]
    subsets = [X] if indices is None else [X[:, np.asarray(ix)] for ix in np.asarray(indices)]
    out = np.zeros((len(subsets), p, p), dtype=np.int64)
    for r, Xr in enumerate(subsets):
        n = Xr.shape[1]
        rows = max(1, int(chunk // max(1, p * n)))                    # a-samples per chunk
        for a0 in range(0, n - 1, rows):
            a = np.arange(a0, min(n - 1, a0 + rows))
            Z = np.sign(Xr[:, a, None] - Xr[:, None, :])               # (p, a, b)
            Z *= (np.arange(n)[None, :] > a[:, None])[None]            # pairs a < b only
            Z = Z.reshape(p, -1).astype(np.int64)
            out[r] += Z @ Z.T
    return out[0] if indices is None else out


def _tau_from_counts(G, skeptic):
    """tau-b (or sin(pi/2 tau-b)) from the integers, diagonal exactly 1; a constant variable is refused."""
    G = np.asarray(G)
    d = np.diagonal(G, axis1=-2, axis2=-1).astype(np.float64)
    assert np.all(d > 0), "rank correlation: a variable is constant (no untied pair of samples)"
    T = G / np.sqrt(d[..., :, None] * d[..., None, :])
    if skeptic:
        T = np.sin(np.pi / 2 * T)
    i = np.arange(G.shape[-1])
    T[..., i, i] = 1.0
    return T


def host_skeptic_correlation(X, indices=None):
    """numpy counterpart of ``skeptic_correlation`` for one (p,N) array."""
    return _tau_from_counts(host_kendall_counts(X, indices), True)


def _kendall_per_instance(X, indices, fn):
    """``fn(ranks of instance, idx)`` for every instance of what ``sample_covariance`` accepts, returned as the same kind (with
    ``indices`` every result carries a leading axis of B subsets)."""
    kind, Xs = _data_list(X)
    idx = None if indices is None else _subset_indices(indices)
    out = [fn(dense_ranks(x), idx) for x in Xs]
    if indices is None:
        out = [o[0] for o in out]
    if kind == "2d":
        return out[0]
    if kind == "3d":
        return np.stack(out)
    return {k: out[k] for k in range(len(out))}


def kendall_counts(X, indices=None, device=0):
    """The exact int64 matrix ``G = Z Z^T`` of Kendall's tau on the device (int8 matrix cores):
    ``G[i,j] = sum_{a<b} sgn(x_ia - x_ib) sgn(x_ja - x_jb)`` -- concordant minus discordant pairs of (i,j) off the diagonal,
    the pairs not tied in i on it.  Exactly symmetric, the same bits on every call, and invariant under any increasing
    transform of a variable.

    X: (p,N), (K,p,N), or a list / dict (keys 0..K-1) of (p_k,N_k) arrays, variables in rows; one kernel call per instance.
    ``indices`` (B,b): G of the column subsets ``X[:, indices[r]]`` (one upload of the ranks; duplicates allowed) -- every
    instance's result then is (B,p,p)."""
    return _kendall_per_instance(X, indices, lambda R, idx: _kendall_call(R, idx, False, device)[0])


def kendall_tau(X, indices=None, device=0):
    """Kendall's tau-b between every pair of variables, ``G_ij / sqrt(G_ii G_jj)`` of ``kendall_counts`` (ties handled; what
    ``scipy.stats.kendalltau`` returns per pair); the diagonal is 1.  A constant variable is refused.  Arguments and the kind
    of the result as ``kendall_counts``."""
    return _kendall_per_instance(X, indices, lambda R, idx: _tau_from_counts(_kendall_call(R, idx, False, device)[0], False))


def skeptic_correlation(X, indices=None, device=0):
    """The nonparanormal skeptic matrix ``sin(pi/2 tau-b)`` on the device: a correlation estimate that is invariant under
    monotone transforms of the variables and robust to outliers and ties.  Diagonal exactly 1, exactly symmetric; it need not
    be positive semidefinite.  A variable that is constant (over a subset) is refused, naming it.  Arguments and the kind of
    the result as ``kendall_counts``."""
    return _kendall_per_instance(X, indices, lambda R, idx: _kendall_call(R, idx, True, device)[1])
