"""Utilities on the device: the block norms of the Functional Graphical Lasso (reference: helper/utils.py:69-107 of
fabian-sp/GGLasso), the sample covariance of observations (what helper/data_generation.py:221,234 gets from numpy.cov), its
rank-based, pairwise-complete and weighted forms, the kernel-smoothed covariance stack of a time series, and -- the output
side -- the debiased graphical lasso with the edge-wise tests and confidence intervals built on it."""
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


# -----------------------------------------------------------------------------------------------------------------
# Latent correlation of mixed binary / continuous data: the Gaussian copula model of Fan, Liu, Ning, Zou (2017), the
# estimator of R's mixedCCA / latentcor.  A binary variable is 1{Z > Delta} of a latent normal Z, a continuous one an
# increasing transform of it.  With Kendall's tau-a = G_ij / (n (n - 1) / 2) of the counts above and Delta = the normal
# quantile of the share of a binary variable's smaller value, the latent correlation r of a pair solves F(r) = tau:
#     binary, binary:       F(r) = (1/pi) int_0^{asin r}          g(t; Delta_i, Delta_j) dt
#     binary, continuous:   F(r) = (2/pi) int_0^{asin(r/sqrt 2)}  g(t; Delta, 0) dt
#     continuous pair:      r = sin(pi/2 tau)
#     g(t; h, k) = exp(-(h^2 + k^2 - 2 h k sin t) / (2 cos^2 t))
# The library evaluates the integral by a 64-node Gauss-Legendre rule, one node per lane (csrc/bridge.hip).
# -----------------------------------------------------------------------------------------------------------------
# the 64-node Gauss-Legendre rule on [0, 1] (nodes (1 + x) / 2, weights w / 2): the table of csrc/bridge.hip
_GL64_U = np.array([
    0.0003474791321139303, 0.0018299416140223604, 0.00449331426162784, 0.008331873057687022,
    0.013336586105044517, 0.01949560017397314, 0.026794312570798593, 0.035215413934030215,
    0.044738931460748595, 0.055342277002442944, 0.06700030092295359, 0.07968535187370981,
    0.09336734243860122, 0.1080138205283293, 0.12359004636973406, 0.1400590749141946,
    0.15738184347288336, 0.17551726437267132, 0.19442232241380336, 0.21405217689868297,
    0.23436026799005272, 0.2552984271464735, 0.27681699137326793, 0.2988649210180042,
    0.32138992083116596, 0.34433856400489454, 0.3676564188956163, 0.39128817812999644,
    0.41517778978800357, 0.4392685903519397, 0.4635034391061005, 0.48782485366828776,
    0.5121751463317122, 0.5364965608938995, 0.5607314096480602, 0.5848222102119964,
    0.6087118218700035, 0.6323435811043837, 0.6556614359951055, 0.6786100791688341,
    0.7011350789819958, 0.723183008626732, 0.7447015728535265, 0.7656397320099473,
    0.7859478231013171, 0.8055776775861966, 0.8244827356273287, 0.8426181565271166,
    0.8599409250858054, 0.876409953630266, 0.8919861794716707, 0.9066326575613988,
    0.9203146481262902, 0.9329996990770464, 0.944657722997557, 0.9552610685392514,
    0.9647845860659698, 0.9732056874292014, 0.9805043998260269, 0.9866634138949555,
    0.991668126942313, 0.9955066857383722, 0.9981700583859776, 0.999652520867886])
_GL64_V = np.array([
    0.0008916403608482165, 0.002073516630281234, 0.0032522289844891814, 0.0044233799131819735,
    0.005584069730065564, 0.006731523948359321, 0.007863015238012359, 0.008975857887848672,
    0.010067411576765104, 0.011135086904191627, 0.012176351284355437, 0.01318873485752733,
    0.014169836307129742, 0.015117328536201239, 0.016028964177425775, 0.016902580918570803,
    0.017736106628441193, 0.018527564270120023, 0.019275076589307813, 0.01997687056636017,
    0.020631281621311764, 0.021236757561826795, 0.021791862264661725, 0.022295279081878283,
    0.02274581396370907, 0.023142398290657208, 0.02348409140810501, 0.023770082857415154,
    0.023999694298229155, 0.024172381117401477, 0.024287733720751714, 0.024345478504569862,
    0.024345478504569862, 0.024287733720751714, 0.024172381117401477, 0.023999694298229155,
    0.023770082857415154, 0.02348409140810501, 0.023142398290657208, 0.02274581396370907,
    0.022295279081878283, 0.021791862264661725, 0.021236757561826795, 0.020631281621311764,
    0.01997687056636017, 0.019275076589307813, 0.018527564270120023, 0.017736106628441193,
    0.016902580918570803, 0.016028964177425775, 0.015117328536201239, 0.014169836307129742,
    0.01318873485752733, 0.012176351284355437, 0.011135086904191627, 0.010067411576765104,
    0.008975857887848672, 0.007863015238012359, 0.006731523948359321, 0.005584069730065564,
    0.0044233799131819735, 0.0032522289844891814, 0.002073516630281234, 0.0008916403608482165])


def variable_types(X):
    """The (p,) int32 array of variable types of ``X`` (p,N) for ``mixed_correlation``: 1 (binary) where a row takes exactly
    two distinct values, whatever their coding, 0 (continuous) elsewhere."""
    X = np.asarray(X, dtype=np.float64)
    assert X.ndim == 2, f"data must be a (p,N) array with variables in rows, has shape {X.shape}"
    return np.array([len(np.unique(x)) == 2 for x in X], dtype=np.int32)


def _mixed_types(R, types):
    """``types`` as the C-contiguous int32 (p,) array the library takes; None: from the dense ranks R (binary: top rank 1)."""
    if types is None:
        return (R.max(axis=1) == 1).astype(np.int32)
    t = np.ascontiguousarray(types, dtype=np.int32)
    assert t.shape == (R.shape[0],), f"types must have shape ({R.shape[0]},), has {t.shape}"
    return t


def _normal_quantile_lower(q):
    """The standard normal quantile of 0 < q <= 1/2: Newton on Phi(x) - q from x = 0.  Phi is convex on the negative axis,
    so the iterates decrease to the root."""
    import math
    x = 0.0
    for _ in range(200):
        xn = x - (0.5 * math.erfc(-x / math.sqrt(2.0)) - q) * math.sqrt(2.0 * math.pi) * math.exp(0.5 * x * x)
        if not xn < x:
            break
        x = xn
    return x


def _bridge_delta(n0, n):
    """Delta = the normal quantile of n0 / n, 0 < n0 < n, taken from the lower tail (as the kernel does)."""
    n0, n = int(n0), int(n)
    return _normal_quantile_lower(n0 / n) if 2 * n0 <= n else -_normal_quantile_lower((n - n0) / n)


def _bridge_H(x, h2k2, hk2, c):
    """H(x) = c x sum_n v_n g(x u_n) for arrays of pairs: the kernel's br_H."""
    t = x[:, None] * _GL64_U[None]
    co = np.cos(t)
    return c * x * ((_GL64_V[None] * np.exp(-(h2k2[:, None] - hk2[:, None] * np.sin(t)) / (2.0 * co * co))).sum(axis=1))


def _bridge_solve(tau, h, k, bb, clip, max_iter=64, ftol=2.0 ** -51):
    """The roots of the bridge functions for arrays of pairs, by the kernel's safeguarded Newton iteration in the angle.
    ``bb``: both variables binary (thresholds h, k), else binary / continuous (threshold h, k = 0).  Returns (r, clipped)."""
    k = np.where(bb, k, 0.0)
    h2k2, hk2 = h * h + k * k, 2.0 * h * k
    c = np.where(bb, 1.0 / np.pi, 2.0 / np.pi)
    amp = np.where(bb, 1.0, np.sqrt(2.0))
    pos = tau >= 0.0
    xe = np.where(pos, 1.0, -1.0) * np.arcsin(clip / amp)
    Fe = _bridge_H(xe, h2k2, hk2, c)
    clipped = np.where(pos, tau >= Fe, tau <= Fe)
    lo, hi = np.minimum(0.0, xe), np.maximum(0.0, xe)
    with np.errstate(all='ignore'):
        x = tau / (c * np.exp(-0.5 * h2k2))
        x = np.where((x > lo) & (x < hi), x, 0.5 * (lo + hi))
        act = np.flatnonzero(~clipped)
        for _ in range(max_iter):
            if act.size == 0:
                break
            xa = x[act]
            f = _bridge_H(xa, h2k2[act], hk2[act], c[act]) - tau[act]
            go = np.abs(f) > ftol
            act, xa, f = act[go], xa[go], f[go]
            hi[act] = np.where(f > 0.0, xa, hi[act])
            lo[act] = np.where(f > 0.0, lo[act], xa)
            co = np.cos(xa)
            d = c[act] * np.exp(-(h2k2[act] - hk2[act] * np.sin(xa)) / (2.0 * co * co))
            xn = xa - f / d
            xn = np.where((xn > lo[act]) & (xn < hi[act]), xn, 0.5 * (lo[act] + hi[act]))
            x[act] = xn
            act = act[xn != xa]
    r = np.clip(amp * np.sin(x), -clip, clip)
    return np.where(clipped, np.where(pos, clip, -clip), r), clipped


def host_mixed_correlation(X, types=None, indices=None, clip=0.999, return_info=False, counts=None):
    """numpy counterpart of ``mixed_correlation`` for one (p,N) array (engines without the device route): the counts of
    ``host_kendall_counts`` (or ``counts``, where the caller has them), the same 64-node rule and the same safeguarded Newton
    iteration.  Returns (p,p), or (B,p,p) with ``indices`` (B,b); with ``return_info`` also the dict ``mixed_correlation``
    describes."""
    X = np.asarray(X, dtype=np.float64)
    assert X.ndim == 2 and np.isfinite(X).all(), "rank correlation needs a finite (p,N) array"
    assert 0.0 < clip < 1.0, f"clip = {clip}, outside (0, 1)"
    p = X.shape[0]
    R = dense_ranks(X)
    t = _mixed_types(R, types)
    assert np.isin(t, (0, 1)).all(), "types: a variable is continuous (0) or binary (1)"
    top = R.max(axis=1)
    assert np.all(top > 0), f"variable {int(np.argmin(top > 0))} is constant"
    assert np.all(top[t == 1] == 1), "a variable marked binary takes more than two values"
    G = host_kendall_counts(X, indices) if counts is None else np.asarray(counts)
    G = G[None] if indices is None else G
    subsets = [R] if indices is None else [R[:, np.asarray(ix)] for ix in np.asarray(indices)]
    iu, ju = np.triu_indices(p, 1)
    ti, tj = t[iu] == 1, t[ju] == 1
    S = np.empty(G.shape)
    n0 = np.empty((len(subsets), p), dtype=np.int32)
    clipped = np.zeros(len(subsets), dtype=np.int32)
    for r, Rr in enumerate(subsets):
        n = Rr.shape[1]
        n0[r] = (Rr == 0).sum(axis=1)
        flat = Rr.min(axis=1) == Rr.max(axis=1)
        assert not flat.any(), f"variable {int(np.argmax(flat))} is constant over subset {r}"
        delta = np.array([_bridge_delta(n0[r, i], n) if t[i] else 0.0 for i in range(p)])
        tau = G[r][iu, ju] / float(n * (n - 1) // 2)
        val = np.sin(np.pi / 2 * tau)
        mix = ti | tj
        if mix.any():
            h = np.where(ti, delta[iu], delta[ju])[mix]
            val[mix], cl = _bridge_solve(tau[mix], h, delta[ju][mix], (ti & tj)[mix], clip)
            clipped[r] = int(cl.sum())
        S[r] = np.eye(p)
        S[r][iu, ju] = val
        S[r][ju, iu] = val
    info = {'types': t, 'zero_counts': n0, 'clipped': clipped}
    if indices is None:
        S, info = S[0], {'types': t, 'zero_counts': n0[0], 'clipped': int(clipped[0])}
    return (S, info) if return_info else S


def _mixed_call(R, types, idx, clip, device=0):
    """One ``ggl_mixed_correlation`` call: R, idx as ``_kendall_call``, types C-contiguous int32 (p,).  Returns (S (B,p,p), G
    (B,p,p) int64, zero counts (B,p) int32, clipped (B,) int32)."""
    p, N = R.shape
    B, b = (1, N) if idx is None else idx.shape
    S = np.empty((B, p, p))
    G = np.empty((B, p, p), dtype=np.int64)
    n0 = np.empty((B, p), dtype=np.int32)
    cl = np.empty(B, dtype=np.int32)
    _lib.require_gpu()
    check(_lib.load().ggl_mixed_correlation(int(device), p, N, R.ctypes.data_as(_lib._ip), types.ctypes.data_as(_lib._ip), B, b,
                                            None if idx is None else idx.ctypes.data_as(_lib._ip), float(clip), ptr(S),
                                            G.ctypes.data_as(_llp), n0.ctypes.data_as(_lib._ip), cl.ctypes.data_as(_lib._ip)))
    return S, G, n0, cl


def mixed_correlation(X, types=None, indices=None, clip=0.999, device=0, return_info=False):
    """The latent correlation matrix of mixed binary / continuous data on the device (Fan, Liu, Ning, Zou 2017): Kendall's
    tau-a of every pair from the exact counts of ``kendall_counts``, inverted through the bridge function of the pair's types
    (one root per pair: ``ggl_mixed_correlation``).  ``types`` (p,): 1 binary, 0 continuous (default ``variable_types(X)``: a
    variable with exactly two distinct values is binary, whatever their coding; the same ``types`` serve every instance).
    The roots are sought in ``[-clip, clip]``; a pair of continuous variables gets ``sin(pi/2 tau-a)``, unclipped -- on data
    without ties the entry of ``skeptic_correlation``.

    Diagonal exactly 1, exactly symmetric, the same bits on every call, invariant under increasing transforms of any variable
    (a recoding of a binary one included); it need not be positive semidefinite.  A variable that is constant (over a subset)
    is refused, naming it.  X, ``indices`` and the kind of the result as ``kendall_counts``.

    ``return_info``: also a dict (one per instance for several instances) of ``types`` (p,), ``zero_counts`` -- the samples at
    every variable's smaller value, (p,) or (B,p) int32 -- and ``clipped``, the pairs that ended on ``+-clip`` (int, or (B,))."""
    infos = []

    def one(R, idx):
        t = _mixed_types(R, types)
        S, _, n0, cl = _mixed_call(R, t, idx, clip, device)
        infos.append({'types': t, 'zero_counts': n0, 'clipped': cl} if indices is not None else
                     {'types': t, 'zero_counts': n0[0], 'clipped': int(cl[0])})
        return S

    S = _kendall_per_instance(X, indices, one)
    if not return_info:
        return S
    return S, (infos[0] if isinstance(S, np.ndarray) and S.ndim == (2 if indices is None else 3) else infos)


# -----------------------------------------------------------------------------------------------------------------
# Weighted covariance of one data array under K weight rows, and the kernel-smoothed covariance stack of a time series
# (Zhou, Lafferty, Wasserman 2010; Monti et al. 2014 "SINGLE"): csrc/covariance_weighted.hip behind ggl_covariance_weighted.
#     W_k = sum_n w_kn,  m_k = (1/W_k) sum_n w_kn x_n,  S_k = (1/W_k) sum_n w_kn (x_n - m_k)(x_n - m_k)^T
# -----------------------------------------------------------------------------------------------------------------
def _weights_2d(weights, N):
    """(the C-contiguous float64 (K,N) array of ``weights``, whether it was given as one (N,) row)."""
    w = as_c(weights)
    assert w.ndim in (1, 2) and w.shape[-1] == N and w.size >= 1, \
        f"weights must be (N,) or (K,N) with N = {N}, have shape {w.shape}"
    return (w[None], True) if w.ndim == 1 else (w, False)


def _covariance_weighted_call(X, w, flags, device=0):
    """One ``ggl_covariance_weighted`` call: X C-contiguous float64 (p,N), w C-contiguous float64 (K,N).  Returns
    (S (K,p,p), variances (K,p) or None, W (K,))."""
    (p, N), K = X.shape, w.shape[0]
    S = np.empty((K, p, p))
    var = np.empty((K, p)) if flags & _lib.COV_SCALE else None
    wsum = np.empty(K)
    _lib.require_gpu()
    check(_lib.load().ggl_covariance_weighted(int(device), p, N, ptr(X), K, ptr(w), int(flags), ptr(S), ptr(var), ptr(wsum)))
    return S, var, wsum


def weighted_covariance(X, weights, center=True, scale=False, device=0, return_wsum=False):
    """``numpy.cov(X, aweights=weights[k], bias=True)`` for every row of ``weights`` on the device (FP64 matrix cores):
    ``S_k = (1/W_k) sum_n w_kn (x_n - m_k)(x_n - m_k)^T`` with ``W_k = sum_n w_kn`` and the weighted mean ``m_k``.

    X: (p,N), variables in rows; it goes up once and is shared by all rows.  ``weights``: (N,) gives (p,p), (K,N) gives (K,p,p);
    non-negative and finite, every row with a positive sum (anything else is refused, naming row and sample).  Only the
    samples between a row's first and last positive weight are visited.  S is exactly symmetric, positive semidefinite up to
    rounding, and the same bits on every call.  ``center=False``: the weighted raw second moment.  ``scale=True``: the
    correlations, and as a second value the weighted variances ((p,) or (K,p)).  ``return_wsum=True``: the ``W_k`` the kernels
    used as one more value."""
    X = as_c(X)
    assert X.ndim == 2 and X.shape[0] >= 1 and X.shape[1] >= 1, \
        f"data must be a (p,N) array with variables in rows, has shape {X.shape}"
    w, one = _weights_2d(weights, X.shape[1])
    flags = (_lib.COV_CENTER if center else 0) | (_lib.COV_SCALE if scale else 0)
    S, var, wsum = _covariance_weighted_call(X, w, flags, device)
    out = (S,) + ((var,) if scale else ()) + ((wsum,) if return_wsum else ())
    if one:
        out = tuple(a[0] for a in out)
    return out if len(out) > 1 else out[0]


def host_weighted_covariance(X, weights, center=True):
    """numpy counterpart of ``weighted_covariance`` (engines without the device route): the same formula, two passes.
    Returns (p,p) for (N,) weights, (K,p,p) for (K,N).  Nothing is refused here but a shape."""
    X = np.asarray(X, dtype=np.float64)
    assert X.ndim == 2, f"data must be a (p,N) array with variables in rows, has shape {X.shape}"
    w, one = _weights_2d(weights, X.shape[1])
    S = []
    for wk in w:
        W = wk.sum()
        Xc = X - (X @ wk / W)[:, None] if center else X
        S.append((Xc * wk) @ Xc.T / W)
    return S[0] if one else np.stack(S)


def kernel_weights(times, at, bandwidth, kernel='gaussian', cutoff=2.0 ** -53):
    """The (K,N) weights ``w_kn = kappa((times[n] - at[k]) / h_k)`` of kernel smoothing at the K points ``at``.

    ``kernel``: 'gaussian' ``exp(-u^2/2)``, 'epanechnikov' ``max(0, 1 - u^2)``, 'uniform' ``|u| <= 1``.  ``bandwidth``: one
    positive number, or one per point of ``at``.  An entry below ``cutoff * max_n w_kn`` becomes exactly 0: that gives the
    Gaussian a finite support (about 8.6 h wide at the default), which is what ``weighted_covariance`` visits.  ``times`` need
    not be sorted, but a row's support -- first to last positive weight, as positions in ``times`` -- is only tight when it is:
    with shuffled times every row spans nearly all samples and the device visits them all."""
    t = np.asarray(times, dtype=np.float64)
    a = np.atleast_1d(np.asarray(at, dtype=np.float64))
    assert t.ndim == 1 and t.size >= 1 and a.ndim == 1 and a.size >= 1, "times must be (N,), at must be (K,)"
    assert np.isfinite(t).all() and np.isfinite(a).all(), "times and at must be finite"
    h = np.broadcast_to(np.asarray(bandwidth, dtype=np.float64), a.shape)
    assert np.all(h > 0) and np.isfinite(h).all(), "bandwidth must be positive and finite"
    assert kernel in ('gaussian', 'epanechnikov', 'uniform'), "kernel must be 'gaussian', 'epanechnikov' or 'uniform'"
    assert 0 <= cutoff < 1, "cutoff must lie in [0, 1)"
    u = (t[None, :] - a[:, None]) / h[:, None]
    if kernel == 'gaussian':
        w = np.exp(-0.5 * u * u)
    elif kernel == 'epanechnikov':
        w = np.maximum(0.0, 1.0 - u * u)
    else:
        w = (np.abs(u) <= 1.0).astype(np.float64)
    w[w < cutoff * w.max(axis=1, keepdims=True)] = 0.0
    return w


def effective_sample_size(weights):
    """Kish's effective sample size ``W_k^2 / sum_n w_kn^2`` of every weight row, as floats: (K,) for (K,N) weights, a float for
    (N,).  N for equal weights, 1 for a single non-zero weight."""
    w = np.asarray(weights, dtype=np.float64)
    assert w.ndim in (1, 2), f"weights must be (N,) or (K,N), have shape {w.shape}"
    n = w.sum(axis=-1) ** 2 / (w * w).sum(axis=-1)
    return float(n) if w.ndim == 1 else n


def _kernel_setup(N, at, bandwidth, times, kernel, cutoff):
    """(times, evaluation points, weights (K,N)) of ``kernel_covariance``."""
    assert bandwidth is not None, "kernel_covariance needs a bandwidth"
    assert at is not None, "kernel_covariance needs the evaluation points: at = K, or an array of times"
    t = np.arange(N, dtype=np.float64) if times is None else np.asarray(times, dtype=np.float64)
    assert t.shape == (N,), f"times must have one entry per column of X, ({N},), has shape {t.shape}"
    if isinstance(at, (int, np.integer)) and not isinstance(at, bool):
        assert at >= 1, "at = K needs K >= 1"
        a = np.linspace(t.min(), t.max(), int(at)) if at > 1 else np.array([0.5 * (t.min() + t.max())])
    else:
        a = np.atleast_1d(np.asarray(at, dtype=np.float64))
    return t, a, kernel_weights(t, a, bandwidth, kernel, cutoff)


def kernel_covariance(X, at=None, bandwidth=None, times=None, kernel='gaussian', cutoff=2.0 ** -53, center=True, scale=False,
                      device=0):
    """The kernel-smoothed covariance stack of a time series on the device: ``S_k = weighted_covariance(X, w_k)`` with
    ``w_k = kernel_weights(times, at, bandwidth, kernel, cutoff)[k]`` -- the input of a Fused Graphical Lasso for time-varying
    networks (Zhou, Lafferty, Wasserman 2010; Monti et al. 2014).

    X: (p,N), one column per observation; ``times`` (N,) its time stamps, default ``0..N-1``.  ``at``: an integer K (that many
    equally spaced points over the range of ``times``) or an array of evaluation times.  ``bandwidth`` is required (one number
    or one per point); choosing it is left to the caller.  Returns ``(S (K,p,p), n_eff (K,))`` with Kish's effective sample size
    per point, and with ``scale=True`` ``(S, n_eff, variances (K,p))``."""
    X = as_c(X)
    assert X.ndim == 2 and X.shape[0] >= 1 and X.shape[1] >= 1, \
        f"data must be a (p,N) array with variables in rows, has shape {X.shape}"
    _, _, w = _kernel_setup(X.shape[1], at, bandwidth, times, kernel, cutoff)
    out = weighted_covariance(X, w, center=center, scale=scale, device=device)
    n_eff = effective_sample_size(w)
    return (out[0], n_eff, out[1]) if scale else (out, n_eff)


# -----------------------------------------------------------------------------------------------------------------
# Leave-one-out choice of the bandwidth by the Gaussian predictive likelihood (Yin, Geng, Li, Wang 2010; Monti et al. 2014;
# DESIGN 25).  For a bandwidth h and the observation i at time tau_i
#     w_n = kappa((tau_n - tau_i) / h) for n != i,  w_i = 0;    m, S = the weighted mean and covariance of X under w
#     score_i(h) = log det S + (x_i - m)^T S^-1 (x_i - m)        (-2 log-density of x_i, up to p log 2 pi)
# On the device: the launches of the weighted covariance, then csrc/cholesky.hip (a batched Cholesky that returns the log
# det and the quadratic form), behind ggl_weighted_predictive_scores; the covariances never leave the device.
# -----------------------------------------------------------------------------------------------------------------
def _chol_args(S, d, ridge):
    """(S (K,p,p), d (K,p) or None, single) of what ``cholesky_predict`` accepts, C-contiguous float64."""
    Sm = np.asarray(S, dtype=np.float64)
    assert Sm.ndim in (2, 3) and Sm.shape[-1] == Sm.shape[-2] and Sm.shape[-1] >= 1 and Sm.shape[0] >= 1, \
        f"cholesky_predict needs a square (p,p) matrix or a (K,p,p) stack of them, S has shape {Sm.shape}"
    single = Sm.ndim == 2
    Sm = as_c(Sm[None] if single else Sm)
    if d is not None:
        d = np.asarray(d, dtype=np.float64)
        d = as_c(d[None] if single and d.ndim == 1 else d)
        assert d.shape == Sm.shape[:2], f"d must have shape {Sm.shape[1:2] if single else Sm.shape[:2]}, has {d.shape}"
    assert ridge >= 0 and np.isfinite(ridge), f"ridge = {ridge}: it must be non-negative and finite"
    return Sm, d, single


def _chol_result(out, single):
    res = (out[:, 0].copy(), out[:, 1].copy(), out[:, 2].copy(), out[:, 3].astype(np.int64))
    return tuple(a[0] for a in res) if single else res


def cholesky_predict(S, d=None, ridge=0.0, device=0):
    """Batched Cholesky factorisation ``S + ridge I = L L^T`` on the device (``ggl_cholesky_predict``, one workgroup per
    matrix, the block updates on the FP64 matrix cores).  S: (p,p) or (K,p,p), symmetric, only the lower triangle is read;
    d: (p,) / (K,p) or None.  Returns ``(logdet, quad, min_pivot, status)``, floats for one matrix and (K,) arrays for a stack:
    ``logdet = 2 sum_j log l_jj``, ``quad = d^T (S + ridge I)^-1 d`` (0 without d), ``min_pivot`` the smallest ``l_jj^2``, and
    ``status`` -1, or the first column whose pivot was not positive and finite -- then ``logdet = -inf``, ``quad = nan`` and
    ``min_pivot`` the smallest pivot up to and including that one.  A matrix that is not positive definite is not an error.
    The same bits on every call, instance k's independent of the others."""
    Sm, dm, single = _chol_args(S, d, ridge)
    K, p = Sm.shape[0], Sm.shape[1]
    out = np.empty((K, 4))
    _lib.require_gpu()
    check(_lib.load().ggl_cholesky_predict(int(device), K, p, ptr(Sm), ptr(dm), float(ridge), ptr(out)))
    return _chol_result(out, single)


def host_cholesky_predict(S, d=None, ridge=0.0):
    """numpy counterpart of ``cholesky_predict``: the plain column Cholesky with d as a border row and the same failure
    rule, so the first failing column is the same."""
    Sm, dm, single = _chol_args(S, d, ridge)
    K, p = Sm.shape[0], Sm.shape[1]
    out = np.empty((K, 4))
    for k in range(K):
        A = np.tril(Sm[k])
        A[np.arange(p), np.arange(p)] += ridge
        L, y = np.zeros_like(A), np.zeros(p)
        lsum, minpiv, status = 0.0, np.inf, -1
        with np.errstate(all='ignore'):
            for j in range(p):
                piv = A[j, j] - L[j, :j] @ L[j, :j]
                minpiv = piv if (piv < minpiv or piv != piv) else minpiv
                if not (piv > 0 and np.isfinite(piv)):
                    status = j
                    break
                L[j, j] = np.sqrt(piv)
                lsum += np.log(L[j, j])
                L[j + 1:, j] = (A[j + 1:, j] - L[j + 1:, :j] @ L[j, :j]) / L[j, j]
                if dm is not None:                               # the border row: y = L^-1 d, one entry per column
                    y[j] = (dm[k, j] - y[:j] @ L[j, :j]) / L[j, j]
        if status >= 0:
            out[k] = (-np.inf, np.nan, minpiv, status)
        else:
            out[k] = (2.0 * lsum, float(y @ y), minpiv, -1)
    return _chol_result(out, single)


def _loo_setup(X, bandwidths, times, eval_index):
    """(X (p,N), bandwidths (H,) as given, times (N,), evaluation samples (M,) int32) of the bandwidth search."""
    X = as_c(X)
    assert X.ndim == 2 and X.shape[0] >= 1 and X.shape[1] >= 2, \
        f"data must be a (p,N) array with variables in rows and N >= 2, has shape {X.shape}"
    N = X.shape[1]
    h = np.atleast_1d(np.asarray(bandwidths, dtype=np.float64)).reshape(-1)
    assert h.size >= 1 and np.all(h > 0) and np.isfinite(h).all(), "bandwidths must be positive and finite"
    t = np.arange(N, dtype=np.float64) if times is None else np.asarray(times, dtype=np.float64)
    assert t.shape == (N,), f"times must have one entry per column of X, ({N},), has shape {t.shape}"
    if eval_index is None:
        ev = np.arange(N)
    elif isinstance(eval_index, (int, np.integer)) and not isinstance(eval_index, bool):
        assert 1 <= eval_index <= N, f"eval_index = {eval_index}: between 1 and N = {N} samples can be evaluated"
        ev = np.unique(np.round(np.linspace(0, N - 1, int(eval_index))).astype(np.int64))
    else:
        ev = np.asarray(eval_index)
        assert ev.ndim == 1 and ev.size >= 1 and np.issubdtype(ev.dtype, np.integer), "eval_index must be a 1-d integer array"
        assert ev.min() >= 0 and ev.max() < N, f"eval_index must lie in [0, {N})"
    return X, h, t, np.ascontiguousarray(ev, dtype=np.int32)


def loo_weights(times, eval_index, bandwidth, kernel='gaussian', cutoff=2.0 ** -53):
    """The (M,N) leave-one-out weights of one bandwidth: ``kernel_weights(times, times[eval_index], bandwidth, kernel,
    cutoff)`` with the own column of every row set to exactly 0.  A row left without a positive weight is a ValueError naming
    the bandwidth and the sample."""
    ev = np.asarray(eval_index)
    w = kernel_weights(times, np.asarray(times, dtype=np.float64)[ev], float(bandwidth), kernel, cutoff)
    w[np.arange(ev.size), ev] = 0.0
    alone = ~(w > 0).any(axis=1)
    if alone.any():
        raise ValueError(f"bandwidth {float(bandwidth):g}: the evaluation sample {int(ev[np.flatnonzero(alone)[0]])} has no "
                         f"neighbour with a positive weight ({kernel} kernel); the bandwidth is too narrow for these times")
    return w


def _loo_scores(X, bandwidths, times, kernel, cutoff, center, ridge, eval_index, device, chunk, host):
    """(SCORE (H,M), STATUS (H,M), N_EFF (H,), evaluation samples) in the order of ``bandwidths``."""
    X, h, t, ev = _loo_setup(X, bandwidths, times, eval_index)
    assert ridge >= 0 and np.isfinite(ridge), f"ridge = {ridge}: it must be non-negative and finite"
    assert isinstance(chunk, (int, np.integer)) and chunk >= 0, f"chunk = {chunk}: a non-negative integer (0: by memory budget)"
    (p, N), M = X.shape, ev.size
    keep = h.size * M * N <= 1 << 26                             # the weights of the grid, kept where they take <= 512 MiB
    Ws = [loo_weights(t, ev, hb, kernel, cutoff) for hb in h] if keep else None
    if not keep:
        for hb in h:                                             # every refusal before anything is uploaded
            loo_weights(t, ev, hb, kernel, cutoff)
    SCORE, STATUS, N_EFF = np.empty((h.size, M)), np.empty((h.size, M), dtype=np.int64), np.empty(h.size)
    flags = _lib.COV_CENTER if center else 0
    if not host:
        _lib.require_gpu()
    for b, hb in enumerate(h):
        w = Ws[b] if keep else loo_weights(t, ev, hb, kernel, cutoff)
        N_EFF[b] = effective_sample_size(w).min()
        out = np.empty((M, 4))
        if host:
            for r in range(M):
                n = np.flatnonzero(w[r])
                S = host_weighted_covariance(X[:, n], w[r, n], center)
                d = X[:, ev[r]] - (X[:, n] @ w[r, n] / w[r, n].sum() if center else 0.0)
                out[r] = host_cholesky_predict(S, d, ridge)
        else:
            check(_lib.load().ggl_weighted_predictive_scores(int(device), p, N, ptr(X), M, ptr(w), ev.ctypes.data_as(_lib._ip),
                                                             float(ridge), flags, int(chunk), ptr(out)))
        STATUS[b] = out[:, 3].astype(np.int64)
        SCORE[b] = np.where(STATUS[b] < 0, out[:, 0] + out[:, 1], np.inf)
    return SCORE, STATUS, N_EFF, ev


def loo_bandwidth_scores(X, bandwidths, times=None, kernel='gaussian', cutoff=2.0 ** -53, center=True, ridge=0.0,
                         eval_index=None, device=0, chunk=0):
    """Leave-one-out Gaussian predictive scores of a time series under kernel smoothing, on the device:
    ``SCORE[b,r] = log det S + (x_i - m)^T S^-1 (x_i - m)`` for ``i = eval_index[r]``, with ``m, S`` the weighted mean and
    covariance of X (p,N) under ``loo_weights(times, eval_index, bandwidths[b], kernel, cutoff)[r]`` -- minus twice the log
    density of ``x_i`` under the estimate that never saw it, up to ``p log 2 pi``.  The smaller, the better the bandwidth predicts.

    ``times`` (N,) default ``0..N-1``; ``kernel`` and ``cutoff`` as ``kernel_covariance``.  ``eval_index``: None (all N
    samples), an integer m (m equally spaced samples) or an index array.  ``center=False``: ``m = 0`` and the weighted raw second
    moment.  ``ridge >= 0`` is added to every diagonal before the factorisation.  ``chunk``: weight rows per device pass, 0
    sizing it from a memory budget; the result does not depend on it.  A bandwidth that leaves an evaluation sample without a
    neighbour is refused (ValueError) before anything is uploaded.  Returns ``SCORE (H,M)`` and ``STATUS (H,M)`` in the order
    of ``bandwidths``: status -1, or the first column at which the covariance was found not positive definite -- its score is
    +inf.  The same bits on every call."""
    return _loo_scores(X, bandwidths, times, kernel, cutoff, center, ridge, eval_index, device, chunk, False)[:2]


def host_loo_bandwidth_scores(X, bandwidths, times=None, kernel='gaussian', cutoff=2.0 ** -53, center=True, ridge=0.0,
                              eval_index=None):
    """numpy counterpart of ``loo_bandwidth_scores`` (engines without the device route): the same weights, the same formula
    through ``host_weighted_covariance`` and ``host_cholesky_predict``, the same refusals."""
    return _loo_scores(X, bandwidths, times, kernel, cutoff, center, ridge, eval_index, 0, 0, True)[:2]


# -----------------------------------------------------------------------------------------------------------------
# Nearest-correlation projection of an indefinite S (Higham 2002, with Dykstra's correction; what R's Matrix::nearPD does
# behind latentcor / mixedCCA).  The skeptic, pairwise-complete and latent matrices above need not be positive semidefinite,
# and the graphical lasso objective is unbounded below for small lambda1 when S is not.  Per matrix, on D^-1/2 S D^-1/2 with
# the diagonal set to exactly 1, starting from Y = S, dS = 0:
#     R = Y - dS;   X = V max(lambda, eps) V^T of R = V lambda V^T;   dS = X - R;   Y' = X with the diagonal set to 1
#     r1 = |Y' - Y|_F / |Y'|_F,   delta = |Y' - X|_F,   r2 = delta / |Y'|_F;   stop when max(r1, r2) <= tol
# and then always nu = delta / (1 - eps + delta), result (1 - nu) Y' off the diagonal and 1 on it, scaled back by sqrt(d_i d_j):
# lambda_min(Y') >= eps - delta, so the smallest eigenvalue of the result is at least eps min_i d_i, converged or not.
# -----------------------------------------------------------------------------------------------------------------
_NC_KEYS = ("iterations", "converged", "residual", "distance", "shrink")


def _nc_args(S, eps, tol, max_iter):
    """(A (B,p,p) C-contiguous float64, single) of what ``nearest_correlation`` accepts; the scalar arguments checked."""
    A = np.asarray(S, dtype=np.float64)
    assert A.ndim in (2, 3) and A.shape[-1] == A.shape[-2] and A.shape[-1] >= 1, \
        f"nearest correlation needs a square (p,p) matrix or a (B,p,p) stack of them, S has shape {A.shape}"
    single = A.ndim == 2
    A = as_c(A[None] if single else A)
    assert A.shape[0] >= 1, "nearest correlation: the stack is empty"
    assert 0.0 <= eps <= 0.5, f"eps = {eps}, the eigenvalue floor lies in [0, 0.5]"
    assert 1e-14 <= tol <= 1e-2, f"tol = {tol}, the tolerance lies in [1e-14, 1e-2]"
    assert int(max_iter) >= 1, f"max_iter = {max_iter}, at least one iteration is needed"
    return A, single


def _nc_result(out, single, iters, res, dist, nu, max_iter, return_info, what):
    import warnings
    conv = iters > 0
    if not conv.all():
        bad = np.flatnonzero(~conv)
        warnings.warn(f"{what}: no convergence within {max_iter} iterations for the matrices {bad.tolist()} (residuals "
                      f"{[float(r) for r in res[bad]]}); their results are positive definite but not the nearest",
                      RuntimeWarning, stacklevel=3)
    if not return_info:
        return out[0] if single else out
    vals = (np.abs(iters), conv, res, dist, nu)
    info = {k: (v[0].item() if single else v) for k, v in zip(_NC_KEYS, vals)}
    return (out[0] if single else out), info


def host_nearest_correlation(S, eps=1e-8, tol=1e-10, max_iter=500, return_info=False):
    """numpy counterpart of ``nearest_correlation`` (engines without the device route): the same recursion, stopping test,
    pass-through rule and final shrink, with ``numpy.linalg.eigh`` as the eigen route."""
    A, single = _nc_args(S, eps, tol, max_iter)
    B, p = A.shape[0], A.shape[1]
    out = np.empty_like(A)
    iters = np.zeros(B, dtype=np.int64)
    res, dist, nus = np.zeros(B), np.zeros(B), np.zeros(B)
    di = np.arange(p)
    for b in range(B):
        Ab = A[b]
        bad = ~np.isfinite(Ab).all(axis=1)
        assert not bad.any(), \
            f"nearest correlation: the row of variable {int(np.flatnonzero(bad)[0])} of matrix {b} holds a non-finite entry (NaN or inf)"
        d = np.diagonal(Ab).copy()
        assert (d > 0).all(), (f"nearest correlation: the diagonal entry of variable {int(np.flatnonzero(~(d > 0))[0])} of matrix {b} "
                               f"is {d[~(d > 0)][0]}, not positive")
        sc = np.sqrt(d[:, None] * d[None, :])
        Y = (Ab + Ab.T) * 0.5 / sc
        Y[di, di] = 1.0
        dS = np.zeros_like(Y)
        delta, r, it, done = 0.0, np.inf, 0, False
        while it < int(max_iter) and not done:
            it += 1
            R = Y - dS
            w, V = np.linalg.eigh(R)
            X = (V * np.maximum(w, eps)) @ V.T
            X = np.triu(X) + np.triu(X, 1).T          # one value for (i,j) and (j,i)
            dS = X - R
            Yn = X.copy()
            Yn[di, di] = 1.0
            ny = np.sqrt(np.sum(Yn * Yn))
            delta = np.sqrt(np.sum((1.0 - X[di, di]) ** 2))
            r = max(np.sqrt(np.sum((Yn - Y) ** 2)) / ny, delta / ny)
            Y = Yn
            done = r <= tol
        if done and it == 1:
            out[b] = Ab                                # the input needed no projection: bit for bit
        else:
            nus[b] = delta / (1.0 - eps + delta)
            O = Y * (1.0 - nus[b]) * sc
            O[di, di] = d
            out[b] = O
        iters[b] = it if done else -int(max_iter)
        res[b] = r
        dist[b] = np.sqrt(np.sum((out[b] - Ab) ** 2))
    return _nc_result(out, single, iters, res, dist, nus, int(max_iter), return_info, "host_nearest_correlation")


def nearest_correlation(S, eps=1e-8, tol=1e-10, max_iter=500, device=0, return_info=False):
    """The nearest (Frobenius norm) matrix to ``S`` with the same diagonal whose correlation matrix has no eigenvalue below
    ``eps``, on the device: Higham's alternating projections with Dykstra's correction, the projection onto the cone running
    as the L-step's ``(C - mu I)_+`` on the FP64 matrix cores, a (B,p,p) stack in lock-step.

    S: (p,p) or (B,p,p), symmetric with a positive diagonal ``d`` (``(S + S^T) / 2`` is used); with ``d != 1`` the iteration
    runs on ``D^-1/2 S D^-1/2`` and the result is scaled back, so variances are kept.  The result is exactly symmetric, has
    the diagonal of ``S`` and ``lambda_min >= eps min(d)`` -- also when ``max_iter`` ended the iteration (a ``RuntimeWarning``
    names those matrices; their result is feasible, only not nearest).  A matrix that already meets the stopping test in the
    first iteration is returned bit for bit (then ``lambda_min >= eps - tol |S|_F``).  The same bits on every call.

    ``return_info=True``: also a dict with, per matrix, ``iterations``, ``converged``, ``residual`` (max(r1, r2) of the last
    iteration), ``distance`` (``|out - S|_F``) and ``shrink`` (the final nu); and ``fallbacks``, the eigendecomposition
    fallbacks of the L-step over the call.  NaN / inf entries and non-positive diagonal entries are refused, naming matrix and
    variable.  ``device`` must be 0 (a ctx on another device projects its own ``S``: ``HipEngine.project_S``)."""
    A, single = _nc_args(S, eps, tol, max_iter)
    assert int(device) == 0, "nearest_correlation runs on device 0; use HipEngine.project_S for a ctx on another device"
    B, p = A.shape[0], A.shape[1]
    out = np.empty_like(A)
    iters = np.zeros(B, dtype=np.int32)
    info = np.zeros((B, 4))
    _lib.require_gpu()
    check(_lib.load().ggl_nearest_correlation(B, p, ptr(A), ptr(out), float(eps), float(tol), int(max_iter),
                                              iters.ctypes.data_as(_lib._ip), ptr(info)))
    r = _nc_result(out, single, iters.astype(np.int64), info[:, 0].copy(), info[:, 1].copy(), info[:, 2].copy(), int(max_iter),
                   return_info, "nearest_correlation")
    if return_info:
        r[1]["fallbacks"] = int(info[0, 3])
    return r


# -----------------------------------------------------------------------------------------------------------------
# Inference on a fitted precision matrix: the debiased graphical lasso (Jankova & van de Geer 2015; D-S_GL of R's
# SILGGM), edge-wise tests and confidence intervals, differential tests between instances
# -----------------------------------------------------------------------------------------------------------------
def _debias_args(Theta, S, N):
    """(Theta (K,p,p), S (K,p,p), n (K,), single) of what ``debiased_precision`` accepts, C-contiguous float64."""
    Th, Sm = np.asarray(Theta, dtype=np.float64), np.asarray(S, dtype=np.float64)
    assert Th.ndim in (2, 3) and Th.shape[-1] == Th.shape[-2] and Th.shape[-1] >= 1, \
        f"debiased precision needs a square (p,p) matrix or a (K,p,p) stack of them, Theta has shape {Th.shape}"
    assert Sm.shape == Th.shape, f"Theta has shape {Th.shape}, S has shape {Sm.shape}: they must match"
    single = Th.ndim == 2
    Th, Sm = as_c(Th[None] if single else Th), as_c(Sm[None] if single else Sm)
    K = Th.shape[0]
    assert K >= 1, "debiased precision: the stack is empty"
    n = np.asarray(N, dtype=np.float64)
    assert n.ndim == 0 or n.shape == (K,), f"N must be one number or an array of length K = {K}, has shape {n.shape}"
    n = as_c(np.broadcast_to(n, (K,)))
    return Th, Sm, n, single


def _debias_call(Theta, S, n, flags=0, device=0):
    """One ``ggl_debias`` call on C-contiguous float64 (K,p,p) stacks and n (K,).  Returns (T, SE)."""
    K, p = Theta.shape[0], Theta.shape[1]
    T, SE = np.empty_like(Theta), np.empty_like(Theta)
    _lib.require_gpu()
    check(_lib.load().ggl_debias(int(device), K, p, ptr(Theta), ptr(S), ptr(n), int(flags), ptr(T), ptr(SE)))
    return T, SE


def debiased_precision(Theta, S, N, device=0, return_se=True):
    """The de-sparsified graphical lasso of an estimate ``Theta`` fitted to the covariance ``S`` of ``N`` observations, on
    the device (``ggl_debias``: two products per instance on the FP64 matrix cores, the second over the upper tile pairs
    only with both results fused into its epilogue):

        T  = 2 Theta - Theta S Theta                       (not sparse; the lasso's shrinkage is taken out)
        SE = sqrt((Theta_ii Theta_jj + Theta_ij^2) / N)    (the asymptotic standard error of T_ij)

    so that ``(T_ij - Theta0_ij) / SE_ij`` is asymptotically standard normal (``edge_tests``).  Theta, S: (p,p) or (K,p,p),
    symmetric; N: one number or (K,), not necessarily integers (effective sample sizes).  Returns ``T, SE`` of the shape of
    Theta (``return_se=False``: T alone), both bitwise symmetric, the same bits on every call, instance k's independent of the
    others.  A non-finite entry of Theta or S, a non-positive diagonal entry of Theta and an N that is not positive and
    finite are refused (AssertionError), naming the instance and the variable."""
    Th, Sm, n, single = _debias_args(Theta, S, N)
    T, SE = _debias_call(Th, Sm, n, 0, device)
    if single:
        T, SE = T[0], SE[0]
    return (T, SE) if return_se else T


def host_debiased_precision(Theta, S, N):
    """numpy counterpart of ``debiased_precision``: the same formula, the same refusals, and the same rule that the upper
    triangle (of the product, and of Theta in the two epilogues) decides and the lower one mirrors it."""
    Th, Sm, n, single = _debias_args(Theta, S, N)
    K, p = Th.shape[0], Th.shape[1]
    for k in range(K):
        assert n[k] > 0 and np.isfinite(n[k]), f"debiased precision: N of instance {k} is {n[k]}, not positive and finite"
        for name, A in (("Theta", Th[k]), ("S", Sm[k])):
            bad = ~np.isfinite(A).all(axis=1)
            assert not bad.any(), \
                f"debiased precision: {name} of instance {k}, variable {int(np.flatnonzero(bad)[0])} holds a non-finite entry"
        d = np.diagonal(Th[k])
        assert (d > 0).all(), (f"debiased precision: Theta of instance {k}, variable {int(np.flatnonzero(~(d > 0))[0])}: the "
                               f"diagonal entry is {d[~(d > 0)][0]}, not positive")
    T, SE = np.empty_like(Th), np.empty_like(Th)
    for k in range(K):
        U = np.triu(Th[k])
        d = np.diagonal(Th[k])
        t = np.triu(2.0 * U - (Th[k] @ Sm[k]) @ Th[k].T)
        se = np.triu(np.sqrt((d[:, None] * d[None, :] + U * U) / n[k]))
        T[k] = t + np.triu(t, 1).T
        SE[k] = se + np.triu(se, 1).T
    return (T[0], SE[0]) if single else (T, SE)


def _special():
    """(erfc, ndtri): scipy's, or torch's where scipy is missing."""
    try:
        from scipy.special import erfc, ndtri
        return erfc, ndtri
    except ImportError:
        import torch
        return (lambda x: torch.special.erfc(torch.as_tensor(np.asarray(x, dtype=np.float64))).numpy(),
                lambda q: torch.special.ndtri(torch.as_tensor(np.asarray(q, dtype=np.float64))).numpy())


_ADJUSTMENTS = ('bh', 'bonferroni', 'none')


def adjust_pvalues(pv, alpha=0.05, method='bh'):
    """(adjusted p-values, rejections at level ``alpha``) of one family of p-values ``pv`` (1-d).  ``'bh'``: the step-up
    procedure of Benjamini & Hochberg -- with m = len(pv) and p_(1) <= ... <= p_(m), every hypothesis with p <= p_(k) is
    rejected for the largest k with p_(k) <= k alpha / m; the adjusted value of p_(i) is min_{j >= i} min(1, m p_(j) / j), monotone
    in p.  ``'bonferroni'``: min(1, m p) <= alpha.  ``'none'``: p <= alpha."""
    assert method in _ADJUSTMENTS, f"method must be one of {_ADJUSTMENTS}, is {method!r}"
    assert 0.0 < alpha < 1.0, f"alpha = {alpha}, a level lies in (0, 1)"
    pv = np.asarray(pv, dtype=np.float64)
    m = pv.size
    if m == 0:
        return pv.copy(), np.zeros(0, dtype=bool)
    if method == 'none':
        return pv.copy(), pv <= alpha
    if method == 'bonferroni':
        adj = np.minimum(1.0, m * pv)
        return adj, adj <= alpha
    order = np.argsort(pv, kind='stable')
    ps = pv[order]
    ranks = np.arange(1, m + 1)
    adj = np.empty(m)
    adj[order] = np.minimum.accumulate(np.minimum(1.0, m * ps / ranks)[::-1])[::-1]
    ok = np.flatnonzero(ps <= ranks * alpha / m)
    reject = pv <= ps[ok[-1]] if ok.size else np.zeros(m, dtype=bool)
    return adj, reject


def _tests_of_z(z, alpha, method):
    """p-values and their adjustment over the off-diagonal pairs of every (p,p) matrix of the stack ``z`` (K,p,p): (pvalue,
    pvalue_adj, reject), symmetric; on the diagonal the raw p-value, NaN as the adjusted one (it is in no family) and no
    rejection."""
    erfc, _ = _special()
    K, p = z.shape[0], z.shape[1]
    pv = np.asarray(erfc(np.abs(z) / np.sqrt(2.0)), dtype=np.float64)
    adj = np.full(z.shape, np.nan)
    rej = np.zeros(z.shape, dtype=bool)
    iu = np.triu_indices(p, 1)
    for k in range(K):
        a, r = adjust_pvalues(pv[k][iu], alpha, method)
        adj[k][iu], rej[k][iu] = a, r
        adj[k].T[iu], rej[k].T[iu] = a, r
    return pv, adj, rej


def _stat_args(T, SE, what):
    T, SE = np.asarray(T, dtype=np.float64), np.asarray(SE, dtype=np.float64)
    assert T.ndim in (2, 3) and T.shape[-1] == T.shape[-2], f"{what} needs (p,p) matrices or (K,p,p) stacks, T has shape {T.shape}"
    assert SE.shape == T.shape, f"T has shape {T.shape}, SE has shape {SE.shape}: they must match"
    return T, SE


def edge_tests(T, SE, alpha=0.05, method='bh', null=0.0):
    """Edge-wise two-sided tests of ``Theta0_ij = null`` and confidence intervals from the debiased estimate and its
    standard errors (``debiased_precision``); host only.  T, SE: (p,p) or (K,p,p).

    ``z = (T - null) / SE``, ``pvalue = erfc(|z| / sqrt 2)``; the adjustment (``method``: 'bh' Benjamini-Hochberg, 'bonferroni',
    'none') runs over the p (p - 1) / 2 off-diagonal pairs of every instance on its own.  Returns a dict of arrays of the shape
    of T: ``z``, ``pvalue``, ``pvalue_adj`` (NaN on the diagonal, which is in no family), ``reject`` (bool, symmetric, False on
    the diagonal: the edges significant at level ``alpha`` after adjustment), ``ci_low``, ``ci_high`` (``T -+ ndtri(1 - alpha / 2)
    SE``: level ``1 - alpha`` per entry, not adjusted)."""
    T, SE = _stat_args(T, SE, "edge_tests")
    single = T.ndim == 2
    with np.errstate(divide='ignore', invalid='ignore'):
        z = (T - null) / SE
    pv, adj, rej = _tests_of_z(z[None] if single else z, alpha, method)
    _, ndtri = _special()
    half = float(ndtri(1.0 - alpha / 2.0)) * SE
    pick = (lambda a: a[0]) if single else (lambda a: a)
    return dict(z=z, pvalue=pick(pv), pvalue_adj=pick(adj), reject=pick(rej), ci_low=T - half, ci_high=T + half)


def differential_tests(T, SE, pairs=None, alpha=0.05, method='bh'):
    """Which entries differ between two instances fitted on independent samples: for every listed pair (a, b) of instances of
    the (K,p,p) stacks T, SE, ``z_ab = (T_a - T_b) / sqrt(SE_a^2 + SE_b^2)`` with p-values and their adjustment as in
    ``edge_tests``, per pair; host only.  ``pairs=None``: the consecutive pairs (k, k + 1) -- where the graph of a Fused
    Graphical Lasso stack changes in time.  Returns a list with one dict per pair: ``pair``, ``z``, ``pvalue``, ``pvalue_adj``,
    ``reject``."""
    T, SE = _stat_args(T, SE, "differential_tests")
    assert T.ndim == 3 and T.shape[0] >= 2, f"differential tests compare the instances of a (K,p,p) stack, K >= 2; T has shape {T.shape}"
    K = T.shape[0]
    pairs = [(k, k + 1) for k in range(K - 1)] if pairs is None else [tuple(int(v) for v in pr) for pr in pairs]
    out = []
    for pr in pairs:
        assert len(pr) == 2 and 0 <= pr[0] < K and 0 <= pr[1] < K and pr[0] != pr[1], \
            f"a pair names two different instances in [0, {K}), got {pr}"
        a, b = pr
        with np.errstate(divide='ignore', invalid='ignore'):
            z = (T[a] - T[b]) / np.sqrt(SE[a] * SE[a] + SE[b] * SE[b])
        pv, adj, rej = _tests_of_z(z[None], alpha, method)
        out.append(dict(pair=(a, b), z=z, pvalue=pv[0], pvalue_adj=adj[0], reject=rej[0]))
    return out


# -----------------------------------------------------------------------------------------------------------------
# Meinshausen-Buhlmann neighbourhood selection (2006; ``method = "mb"`` of R's huge, the default of SpiecEasi): one lasso per
# node on a shared matrix, the graph from the supports.  For a symmetric S with positive diagonal, node j and lambda > 0
#     beta^(j) = argmin over beta with beta_j = 0 of  1/2 beta' S beta - s_j' beta + lambda sum_{k != j} |beta_k|
# (with S = X X' / n the lasso of variable j on the others, lambda = glmnet's / scikit-learn's alpha).  On the device:
# csrc/neighborhood.hip, one wave per (matrix, node), the whole descending grid in one launch; DESIGN 26.
# -----------------------------------------------------------------------------------------------------------------
_MB_RULES = {'raw': 0, 'and': 1, 'or': 2}


def _mb_args(S, lambda_range, rule, tol, max_sweeps):
    """(S (M,p,p) C-contiguous, the grid in descending order, single) of what ``neighborhood_selection`` accepts."""
    Sm = np.asarray(S, dtype=np.float64)
    assert Sm.ndim in (2, 3) and Sm.shape[-1] == Sm.shape[-2] and Sm.shape[-1] >= 1 and Sm.shape[0] >= 1, \
        f"neighborhood_selection needs a square (p,p) matrix or a (M,p,p) stack of them, S has shape {Sm.shape}"
    single = Sm.ndim == 2
    lam = np.sort(np.atleast_1d(np.asarray(lambda_range, dtype=np.float64)).reshape(-1))[::-1].copy()
    assert lam.size >= 1 and np.all(lam > 0) and np.all(np.isfinite(lam)), "every lambda must be positive and finite"
    assert np.all(np.diff(lam) < 0), "the lambdas of a grid must differ"
    assert rule in _MB_RULES, f"rule = {rule!r}: 'and', 'or' or 'raw'"
    assert tol >= 0 and np.isfinite(tol), f"tol = {tol}: it must be non-negative and finite"
    assert int(max_sweeps) >= 1, f"max_sweeps = {max_sweeps}: at least one sweep is needed"
    return as_c(Sm[None] if single else Sm), lam, single


def neighborhood_graph(coef, rule='and'):
    """The symmetric matrix of a (...,p,p) stack of raw coefficients (column j holds ``beta^(j)``): for i < j, of
    ``a = beta^(j)_i`` and ``b = beta^(i)_j`` the one of smaller (``'and'``) or larger (``'or'``) magnitude, ``a`` on a tie,
    at (i,j) and (j,i).  Bitwise symmetric, zero diagonal; its non-zero pattern is the AND / OR graph.  Host only: a
    selection, no arithmetic, so it is bit for bit what ``k_mb_symmetrize`` writes."""
    assert rule in ('and', 'or'), f"rule = {rule!r}: 'and' or 'or'"
    a = np.asarray(coef, dtype=np.float64)
    b = np.swapaxes(a, -1, -2)
    with np.errstate(invalid='ignore'):
        take_b = (np.abs(b) < np.abs(a)) if rule == 'and' else (np.abs(b) > np.abs(a))
    up = np.triu(np.where(take_b, b, a), 1)
    return up + np.swapaxes(up, -1, -2)


def _mb_result(W, raw, resvar, info, lam, single, return_info, scaled=False):
    pick = (lambda a: a[0]) if single else (lambda a: a)
    if not return_info:
        return pick(W)
    out = {'LAMBDA': lam, 'COEF': pick(raw), 'RESVAR': pick(resvar), 'SWEEPS': pick(info[..., 0].astype(np.int64)),
           'STATUS': pick(info[..., 1].astype(np.int64))}
    if info.shape[-1] == 3:                                             # the weighted / scaled route
        out['OUTER'] = pick(info[..., 2].astype(np.int64))
        if scaled:
            with np.errstate(invalid='ignore'):
                out['SIGMA'] = np.sqrt(out['RESVAR'])
    return pick(W), out


def _mbw_args(weights, scaled, sig_tol, max_outer, M, p):
    """(Wt C-contiguous (p,p) or (M,p,p) or None, per_matrix) of the arguments of the weighted / scaled route; its refusals."""
    assert np.isfinite(sig_tol) and sig_tol >= 0, f"sig_tol = {sig_tol}: it must be non-negative and finite"
    assert int(max_outer) >= 1, f"max_outer = {max_outer}: at least one outer iteration is needed"
    if weights is None:
        return None, False
    Wt = np.asarray(weights, dtype=np.float64)
    assert Wt.shape in ((p, p), (M, p, p)), \
        f"weights must have shape ({p},{p}), one table for every matrix, or ({M},{p},{p}), one per matrix; got {Wt.shape}"
    bad = np.argwhere(~(Wt >= 0))
    if bad.size:
        ix = tuple(int(v) for v in bad[0])
        raise ValueError(f"weights{list(ix)} = {Wt[ix]}: a penalty weight must lie in [0, +inf] (row j holds node j's weights)")
    return as_c(Wt), Wt.ndim == 3


def adaptive_weights(coef, gamma=1.0, eps=0.0):
    """The weights of the adaptive lasso's second stage (Zou 2006): ``w = 1 / (|coef| + eps)^gamma`` from first-stage raw
    coefficients ``coef`` ([M,]p,p: column j holds ``beta^(j)``, the ``COEF`` of ``neighborhood_selection`` at one lambda),
    laid out as the ``weights`` argument wants them: ``Wt[..., j, k]`` is node j's weight of variable k.  A zero coefficient
    with ``eps = 0`` gives ``+inf``: the coordinate is excluded and the second stage keeps the first stage's support."""
    C = np.asarray(coef, dtype=np.float64)
    assert C.ndim in (2, 3) and C.shape[-1] == C.shape[-2], f"coef must be (p,p) or (M,p,p), got {C.shape}"
    assert gamma > 0 and np.isfinite(gamma) and eps >= 0 and np.isfinite(eps), "gamma must be positive, eps non-negative, both finite"
    assert np.all(np.isfinite(C)), "adaptive_weights: coef holds a non-finite value (a node that was not solved)"
    with np.errstate(divide='ignore'):
        w = 1.0 / (np.abs(np.swapaxes(C, -1, -2)) + eps) ** gamma
    return np.ascontiguousarray(w)


def scaled_lasso_lambda(p, n):
    """The universal penalty of the scaled lasso, ``sqrt(2 log(p) / n)`` (Sun & Zhang 2012): one value for every node,
    whatever its noise level.  ``p = 1`` has no regression to penalise; any positive number serves, 1.0 is returned."""
    assert int(p) >= 1 and int(n) >= 1, f"scaled_lasso_lambda needs p >= 1 and n >= 1, got p = {p}, n = {n}"
    return float(np.sqrt(2.0 * np.log(int(p)) / int(n))) if int(p) > 1 else 1.0


def neighborhood_selection(S, lambda_range, rule='and', tol=1e-7, max_sweeps=10000, device=0, return_info=False, weights=None,
                           scaled=False, sig_tol=1e-7, max_outer=100):
    """Meinshausen-Buhlmann neighbourhood selection on the device (``ggl_neighborhood_path``).  S: (p,p) or (M,p,p),
    symmetric with a positive diagonal, p <= 2048; the grid is used in descending order, every lambda warm-started from the
    one before.  Returns the (L,p,p) or (M,L,p,p) stack of symmetrised coefficient matrices (``neighborhood_graph``;
    ``rule='raw'``: the raw columns); its non-zero pattern is the graph.

    The method is cyclic coordinate descent with covariance updates on an active set (glmnet, huge).  ``tol`` bounds a sweep's
    ``max_k |change of beta_k| S_kk``; a (node, lambda) is finished only once the gradient recomputed from beta, one further
    sweep and one further screen of all variables change nothing beyond ``tol`` and find no violator.  ``max_sweeps`` caps
    the sweeps of one (node, lambda).

    ``return_info``: also a dict with ``LAMBDA`` (L,), ``COEF`` ([M,]L,p,p: column j is ``beta^(j)``), ``RESVAR`` ([M,]L,p: the
    residual variances ``S_jj - 2 s_j' beta + beta' S beta``), ``SWEEPS`` and ``STATUS`` ([M,]L,p: 0 converged, 1 a cap was
    reached, 2 a non-finite value -- that node's coefficients are NaN from that lambda on).  (The raw columns are a second
    call of the library; the bits of a call do not change.)  The same bits on every call, matrix m's independent of the
    others, a lambda's independent of those behind it.

    ``weights`` ((p,p) shared or (M,p,p), entries in [0, +inf]): node j's penalty of variable k is ``lambda *
    weights[j,k]`` (glmnet's ``penalty.factor``; ``adaptive_weights``); 0 leaves a coordinate unpenalised, ``+inf`` excludes
    it.  ``scaled``: the scaled / square-root lasso (Sun & Zhang 2012; Belloni et al. 2011), ``min sqrt(tau^2(beta)) + lambda
    sum_k w_k |beta_k|``, by alternation: the lasso at ``lambda sigma w_k``, ``sigma = sqrt(tau^2)`` of its result, until
    sigma moves by at most ``sig_tol`` relative, at most ``max_outer`` times; ``RESVAR`` is then ``sigma_j^2`` and
    ``scaled_lasso_lambda`` the one penalty that serves every node.  With either, ``ggl_neighborhood_path_w`` is called
    (one kernel serves both) and the info gains ``OUTER`` (outer iterations, 0 without ``scaled``) and,
    with ``scaled``, ``SIGMA``; status 1 also means ``max_outer`` was reached and status 3 that ``tau^2 <= 1e-10 S_jj``, a
    degenerate square-root problem (a duplicated variable, a perfect fit): NaN from there on, as for status 2.  Without
    both, the call and its bits are what they were."""
    Sm, lam, single = _mb_args(S, lambda_range, rule, tol, max_sweeps)
    M, p, L = Sm.shape[0], Sm.shape[1], lam.size
    weighted = weights is not None or bool(scaled)
    extra, ninfo = (), 2                                                # the five further arguments of the _w entry, ints of info
    if weighted:
        Wt, per_matrix = _mbw_args(weights, scaled, sig_tol, max_outer, M, p)
        extra, ninfo = (ptr(Wt), int(per_matrix), int(bool(scaled)), float(sig_tol), int(max_outer)), 3
    _lib.require_gpu()
    lib = _lib.load()
    fn = lib.ggl_neighborhood_path_w if weighted else lib.ggl_neighborhood_path

    def call(r, with_resvar):
        coef, info = np.empty((M, L, p, p)), np.empty((M, L, p, ninfo), dtype=np.int32)
        resvar = np.empty((M, L, p)) if with_resvar else None
        check(fn(int(device), M, p, ptr(Sm), L, ptr(lam), _MB_RULES[r], float(tol), int(max_sweeps), *extra, ptr(coef),
                 ptr(resvar), info.ctypes.data_as(_lib._ip)))
        return coef, resvar, info

    if not return_info:
        return _mb_result(call(rule, False)[0], None, None, None, lam, single, False)
    raw, resvar, info = call('raw', True)
    W = raw if rule == 'raw' else call(rule, False)[0]
    return _mb_result(W, raw, resvar, info, lam, single, True, bool(scaled))


def _host_mb_node_w(S, j, lam, w, scaled, tol, max_sweeps, sig_tol, max_outer, max_rounds=100):
    """The path of node j with the weights w (p,): (beta (L,p), resvar (L,), sweeps, status, outer (L,)) -- ``k_mb_path``'s
    unit of work, step by step: the threshold of coordinate k is ``ls * w[k]``, ``ls = lambda`` or ``lambda * sigma``, and
    around the procedure runs the alternation on sigma.  ``w = 1`` and ``scaled = False`` is the unweighted lasso
    (``lambda * 1.0`` is exact)."""
    p, L = S.shape[0], lam.size
    beta, g = np.zeros(p), S[j].copy()
    member = np.zeros(p, dtype=bool)
    act = np.zeros(0, dtype=np.int64)
    out_b, out_r = np.zeros((L, p)), np.zeros(L)
    out_s, out_st, out_o = np.zeros(L, dtype=np.int64), np.zeros(L, dtype=np.int64), np.zeros(L, dtype=np.int64)
    sjj = S[j, j]
    tau, dead, dead_status = sjj, False, 2

    def sweep(ls):
        dmax = 0.0
        for k in act:
            skk, bk = S[k, k], beta[k]
            z = g[k] + skk * bk
            b = np.sign(z) * max(abs(z) - ls * w[k], 0.0) / skk
            d = b - bk
            if d != 0.0:
                g[:] -= d * S[k]
                beta[k] = b
            c = abs(d) * skk
            dmax = c if c > dmax else dmax
        return dmax

    def screen(ls):
        viol = ~member & (np.abs(g) > ls * w)
        viol[j] = False
        member[viol] = True
        return int(viol.sum())

    def bad():
        return not (np.all(np.isfinite(g)) and np.all(np.isfinite(beta[act])))

    def tau2():
        return sjj - float(np.sum(beta[act] * (S[j, act] + g[act])))

    for l in range(L):
        lamv, sweeps, status, outer = lam[l], 0, 1, 0
        if dead:
            status = dead_status
        elif bad():
            status = 2
        else:
            sig = np.sqrt(tau) if scaled else 1.0
            for it in range(max_outer if scaled else 1):
                ls = lamv * sig if scaled else lamv
                st, d1 = 1, 0.0
                for rnd in range(max_rounds):
                    nviol = screen(ls)
                    act = np.flatnonzero(member)
                    if nviol == 0 and (not (d1 > tol) if rnd > 0 else act.size == 0):
                        st = 0
                        break
                    conv = False
                    while sweeps < max_sweeps:
                        dm = sweep(ls)
                        sweeps += 1
                        if not (dm > tol):
                            conv = True
                            break
                    if not conv:
                        break
                    g[:] = S[j]
                    for k in act:
                        if beta[k] != 0.0:
                            g[:] -= beta[k] * S[k]
                    if sweeps >= max_sweeps:
                        break
                    d1 = sweep(ls)
                    sweeps += 1
                    if bad():
                        st = 2
                        break
                if st == 1 and bad():
                    st = 2
                outer += 1
                if not scaled:
                    status = st
                    break
                if st == 2:
                    status = 2
                    break
                tau = tau2()
                if not (tau > 1e-10 * sjj):
                    status = 3
                    break
                if st == 1:
                    break
                sn = np.sqrt(tau)
                done = abs(sn - sig) <= sig_tol * sn
                sig = sn
                if done:
                    status = 0
                    break
        if status >= 2:
            dead, dead_status = True, status
        if dead:
            out_b[l], out_r[l] = np.nan, np.nan
            out_b[l, j] = 0.0
        else:
            out_b[l] = beta
            out_r[l] = tau if scaled else tau2()
        out_s[l], out_st[l], out_o[l] = sweeps, status, outer if scaled else 0
    return out_b, out_r, out_s, out_st, out_o


def host_neighborhood_selection(S, lambda_range, rule='and', tol=1e-7, max_sweeps=10000, return_info=False, weights=None,
                                scaled=False, sig_tol=1e-7, max_outer=100):
    """numpy twin of ``neighborhood_selection``: the same algorithm in the same order (screen, sweeps over the ascending
    active set, the gradient recomputed in ascending order, one further sweep, one further screen; the same caps and the same
    statuses), in float64 without fused multiply-adds, so its last bits differ from the device's.  For engines without the
    device route and for tests without a GPU.  ``weights``, ``scaled``, ``sig_tol``, ``max_outer`` as there: the same
    alternation in the same order; without them the one node function runs with unit weights and ``OUTER`` is dropped."""
    Sm, lam, single = _mb_args(S, lambda_range, rule, tol, max_sweeps)
    M, p, L = Sm.shape[0], Sm.shape[1], lam.size
    raw, resvar = np.zeros((M, L, p, p)), np.zeros((M, L, p))
    weighted = weights is not None or bool(scaled)
    Wt, per_matrix = _mbw_args(weights, scaled, sig_tol, max_outer, M, p) if weighted else (None, False)
    ones = np.ones(p)
    info = np.zeros((M, L, p, 3), dtype=np.int32)
    with np.errstate(all='ignore'):
        for m in range(M):
            for j in range(p):
                w = ones if Wt is None else (Wt[m, j] if per_matrix else Wt[j])
                b, r, s, st, o = _host_mb_node_w(Sm[m], j, lam, w, bool(scaled), float(tol), int(max_sweeps), float(sig_tol),
                                                 int(max_outer))
                raw[m, :, :, j], resvar[m, :, j], info[m, :, j, 0], info[m, :, j, 1], info[m, :, j, 2] = b, r, s, st, o
    W = raw if rule == 'raw' else neighborhood_graph(raw, rule)
    return _mb_result(W, raw, resvar, info if weighted else info[..., :2], lam, single, return_info, bool(scaled))


def scaled_lasso_precision(S, n=None, lambda0=None, weights='sd', rule='min', device=0, host=False, tol=1e-7, sig_tol=1e-7,
                           max_outer=100):
    """The scaled-lasso precision matrix (Sun & Zhang 2013; TIGER, Liu & Wang 2017): one scaled path per node at ONE penalty,
    no search.  ``lambda0`` defaults to the universal ``scaled_lasso_lambda(p, n)``, which needs the sample size ``n``.
    ``weights='sd'``: ``w_jk = sqrt(S_kk)``, the penalty on the scale of the predictors, with which the estimator commutes with
    rescaling the variables (on a correlation matrix the weights are 1); ``None``: none; or a (p,p) table.  Returns
    ``(Theta, info)``: ``neighborhood_precision(COEF, RESVAR, rule)[0]`` of the path and the path's info with ``LAMBDA0``;
    ``RESVAR`` holds ``sigma_j^2``.  ``host``: through the numpy twin."""
    Sm = np.asarray(S, dtype=np.float64)
    assert Sm.ndim == 2 and Sm.shape[0] == Sm.shape[1] and Sm.shape[0] >= 1, f"scaled_lasso_precision needs one (p,p) matrix, S has shape {Sm.shape}"
    p = Sm.shape[0]
    if lambda0 is None:
        assert n is not None, "scaled_lasso_precision: the universal penalty sqrt(2 log(p) / n) needs the sample size n"
        lambda0 = scaled_lasso_lambda(p, n)
    assert np.isfinite(lambda0) and lambda0 > 0, f"lambda0 = {lambda0}: it must be positive and finite"
    if isinstance(weights, str):
        assert weights == 'sd', f"weights = {weights!r}: 'sd', None or a (p,p) table"
        Wt = np.ascontiguousarray(np.broadcast_to(np.sqrt(np.diagonal(Sm))[None, :], (p, p)))
    else:
        Wt = weights
    kw = dict(rule='raw', tol=tol, return_info=True, weights=Wt, scaled=True, sig_tol=sig_tol, max_outer=max_outer)
    _, info = host_neighborhood_selection(Sm, [lambda0], **kw) if host else neighborhood_selection(Sm, [lambda0], device=device, **kw)
    info = {k: (v if k == 'LAMBDA' else v[0]) for k, v in info.items()}
    info['LAMBDA0'] = float(lambda0)
    return neighborhood_precision(info['COEF'], info['RESVAR'], rule)[0], info


# -----------------------------------------------------------------------------------------------------------------
# Refit of neighbourhood selection on its graph: with the graph held fixed every node is regressed on its neighbours by
# ordinary least squares -- the relaxed lasso (Meinshausen 2007) and the regression-based precision estimator of Yuan (2010)
# and Zhou, Ruetimann, Xu, Buehlmann (2011).  It takes the lasso's shrinkage out of the coefficients, gives a precision matrix
# (``neighborhood_precision``) and, scored on held-out data, the prediction error that tunes lambda (``cv_search(method='mb')``).
# On the device: csrc/mb_refit.hip; DESIGN 28.
# -----------------------------------------------------------------------------------------------------------------
MB_REFIT_MAX_P = 2048
MB_REFIT_MAX_DEG = 128          # MBR_MAX_DEG of csrc/kernels.hpp; the twin applies the same cap


def mb_refit_max_degree():
    """The largest degree the device refit solves, as the library reports it (``ggl_mb_refit_limits``)."""
    out = (ctypes.c_int * 2)()
    _lib.load().ggl_mb_refit_limits(out)
    return int(out[0])


def _refit_args(S, W, t, S_test):
    Sm = np.asarray(S, dtype=np.float64)
    assert Sm.ndim in (2, 3) and Sm.shape[-1] == Sm.shape[-2] and Sm.shape[-1] >= 1 and Sm.shape[0] >= 1, \
        f"neighborhood_refit needs a square (p,p) matrix or a (M,p,p) stack of them, S has shape {Sm.shape}"
    single = Sm.ndim == 2
    Sm = as_c(Sm[None] if single else Sm)
    M, p = Sm.shape[0], Sm.shape[1]
    assert p <= MB_REFIT_MAX_P, f"p = {p}: the refit serves p <= {MB_REFIT_MAX_P}"
    Wm = np.asarray(W, dtype=np.float64)
    assert Wm.ndim >= 2 and Wm.shape[-2:] == (p, p), f"W must end in ({p},{p}), has shape {Wm.shape}"
    if single:
        assert Wm.ndim in (2, 3), f"with one matrix S, W is (p,p) or (G,p,p); it has shape {Wm.shape}"
        one_graph = Wm.ndim == 2
        Wm = Wm.reshape((1, -1, p, p))
    else:
        assert Wm.ndim in (3, 4) and Wm.shape[0] == M, f"with a (M,p,p) stack S, W is (M,p,p) or (M,G,p,p); it has shape {Wm.shape}"
        one_graph = Wm.ndim == 3
        Wm = Wm.reshape((M, -1, p, p))
    assert Wm.shape[1] >= 1, "W holds no graph"
    assert np.isfinite(t) and t >= 0, f"t = {t}: the edge threshold must be finite and not negative"
    Tm = None
    if S_test is not None:
        Tm = np.asarray(S_test, dtype=np.float64)
        assert Tm.shape == ((p, p) if single else (M, p, p)), f"S_test must have the shape of S, has {Tm.shape}"
        Tm = as_c(Tm[None] if single else Tm)
    if not np.all(np.isfinite(Sm)):
        m, i, k = np.argwhere(~np.isfinite(Sm))[0]
        raise ValueError(f"neighborhood_refit: S of matrix {int(m)}: the entry ({int(i)}, {int(k)}) is not finite")
    dg = np.diagonal(Sm, axis1=1, axis2=2)
    if not np.all(dg > 0):
        m, i = np.argwhere(~(dg > 0))[0]
        raise ValueError(f"neighborhood_refit: S of matrix {int(m)}, variable {int(i)}: the diagonal entry is {dg[m, i]}; it must be positive")

    def pick(a):
        a = a[:, 0] if one_graph else a
        return a[0] if single else a
    return Sm, as_c(Wm), Tm, pick


def _refit_result(coef, resvar, heldout, info, pick):
    return {'COEF': pick(coef), 'RESVAR': pick(resvar), 'HELDOUT': None if heldout is None else pick(heldout),
            'DEGREE': pick(info[..., 0].astype(np.int64)), 'STATUS': pick(info[..., 1].astype(np.int64))}


def neighborhood_refit(S, W, t=1e-8, S_test=None, device=0):
    """Least-squares refit of every node on its neighbours in a given graph, on the device (``ggl_neighborhood_refit``).

    S: (p,p) or (M,p,p), symmetric, finite, positive diagonal, p <= 2048.  W: ([M,][G,]p,p), the graphs: node j's neighbours
    are ``A = {i != j : |W[.., j, i]| >= t}``, ROW j (the edge definition of ``stars_search``; a NaN is no edge).  W need not
    be symmetric: the AND / OR matrices of ``neighborhood_selection`` give graph refits, a raw coefficient matrix transposed
    (row j = node j's support) the per-node relaxed lasso.  With ``d = |A|``: ``beta = S_AA^-1 s_A`` by Cholesky,
    ``tau^2 = S_jj - 2 s_A' beta + beta' S_AA beta``, and with ``S_test`` (the shape of S) the same form on it: the held-out
    residual sum of squares per test sample.

    Returns a dict: ``COEF`` (..,p,p: column j holds node j's coefficients), ``RESVAR``, ``HELDOUT`` (None without ``S_test``),
    ``DEGREE``, ``STATUS`` (..,p): 0 solved; 1 a pivot was not positive and finite (``S_AA`` is not positive definite: a
    duplicated variable, more neighbours than observations); 2 a non-finite value in ``S_test``; 3 the degree exceeds
    ``MB_REFIT_MAX_DEG`` = 128.  For 1-3 that node's coefficients (its diagonal entry aside), ``RESVAR`` and ``HELDOUT``
    are NaN; no other node is touched and nothing is an error.  The same bits on every call; those of one (matrix, graph) do not
    depend on the others in the call."""
    Sm, Wm, Tm, pick = _refit_args(S, W, t, S_test)
    M, G, p = Wm.shape[0], Wm.shape[1], Wm.shape[2]
    _lib.require_gpu()
    lib = _lib.load()
    coef, resvar = np.empty((M, G, p, p)), np.empty((M, G, p))
    heldout = None if Tm is None else np.empty((M, G, p))
    info = np.empty((M, G, p, 2), dtype=np.int32)
    check(lib.ggl_neighborhood_refit(int(device), M, p, ptr(Sm), G, ptr(Wm), float(t), ptr(Tm), ptr(coef), ptr(resvar),
                                     ptr(heldout), info.ctypes.data_as(_lib._ip)))
    return _refit_result(coef, resvar, heldout, info, pick)


def _host_quad(Mat, j, A, beta):
    """``q(M; beta) = M_jj - 2 m_A' beta + beta' M_AA beta`` in the device's arrangement ``M_jj + sum_i beta_i (w_i - 2 m_i)``."""
    if A.size == 0:
        return Mat[j, j]
    x = Mat[np.ix_(A, A)] @ beta - 2.0 * Mat[A, j]
    return Mat[j, j] + float(beta @ x)


def _host_refit_node(S, T, w_row, j, t, cap):
    """(beta (p,), tau2, r, degree, status) of one node: the device's steps and the order of its tests (3, 2 on S, 1, 2 on T)."""
    p = S.shape[0]
    with np.errstate(invalid='ignore'):
        e = np.abs(w_row) >= t
    e[j] = False
    A = np.flatnonzero(e)
    d = int(A.size)
    bad = np.full(p, np.nan)
    bad[j] = 0.0
    if d > cap:
        return bad, np.nan, np.nan, d, 3
    SAA, sA = S[np.ix_(A, A)], S[A, j]
    if not (np.all(np.isfinite(SAA)) and np.all(np.isfinite(sA)) and np.isfinite(S[j, j])):
        return bad, np.nan, np.nan, d, 2
    beta = np.zeros(0)
    if d:
        try:
            Lf = np.linalg.cholesky(SAA)
        except np.linalg.LinAlgError:
            return bad, np.nan, np.nan, d, 1
        if not (np.all(np.isfinite(Lf)) and np.all(np.diagonal(Lf) > 0)):
            return bad, np.nan, np.nan, d, 1
        y = np.zeros(d)
        for k in range(d):
            y[k] = (sA[k] - Lf[k, :k] @ y[:k]) / Lf[k, k]
        beta = np.zeros(d)
        for k in range(d - 1, -1, -1):
            beta[k] = (y[k] - Lf[k + 1:, k] @ beta[k + 1:]) / Lf[k, k]
    tau = _host_quad(S, j, A, beta)
    r = np.nan
    if T is not None:
        if not (np.all(np.isfinite(T[np.ix_(A, A)])) and np.all(np.isfinite(T[A, j])) and np.isfinite(T[j, j])):
            return bad, np.nan, np.nan, d, 2
        r = _host_quad(T, j, A, beta)
    out = np.zeros(p)
    out[A] = beta
    return out, tau, r, d, 0


def host_neighborhood_refit(S, W, t=1e-8, S_test=None):
    """numpy twin of ``neighborhood_refit``: the same steps in float64 -- the neighbour list from row j,
    ``numpy.linalg.cholesky`` per node (a failure, or a factor that is not finite with a positive diagonal, is status 1), the
    two triangular solves by substitution, the quadratic forms -- the same degree cap and the same statuses, in numpy's own
    summation orders and without fused multiply-adds, so its last bits differ from the device's.  For engines without the
    device route and tests without a GPU."""
    Sm, Wm, Tm, pick = _refit_args(S, W, t, S_test)
    M, G, p = Wm.shape[0], Wm.shape[1], Wm.shape[2]
    cap = MB_REFIT_MAX_DEG
    coef, resvar = np.zeros((M, G, p, p)), np.zeros((M, G, p))
    heldout = None if Tm is None else np.zeros((M, G, p))
    info = np.zeros((M, G, p, 2), dtype=np.int32)
    with np.errstate(all='ignore'):
        for m in range(M):
            for g in range(G):
                for j in range(p):
                    b, tau, r, d, st = _host_refit_node(Sm[m], None if Tm is None else Tm[m], Wm[m, g, j], j, float(t), cap)
                    coef[m, g, :, j], resvar[m, g, j], info[m, g, j] = b, tau, (d, st)
                    if heldout is not None:
                        heldout[m, g, j] = r
    return _refit_result(coef, resvar, heldout, info, pick)


def neighborhood_precision(coef, resvar, rule='min'):
    """The precision matrix of a set of node-wise regressions (Yuan 2010; Zhou et al. 2011), on the host (O(p^2)):
    ``Theta_jj = 1 / resvar_j``, column j off the diagonal ``-coef[:, j] / resvar_j``, then symmetrised -- ``rule='min'``: of
    ``Theta_ij`` and ``Theta_ji`` the one of smaller magnitude (the (i,j) entry with i < j on a tie) goes to both places, so a
    pair that only one regression selects is zero; ``rule='average'``: their mean.  Bitwise symmetric.  ``coef`` (p,p) with
    column j node j's coefficients, ``resvar`` (p,): ``COEF`` / ``RESVAR`` of ``neighborhood_refit`` (or of the lasso itself).

    Returns ``(Theta, lambda_min(Theta))``.  The estimator is NOT positive definite by construction -- the node-wise
    regressions are not tied to one another -- and a ``RuntimeWarning`` says so when the smallest eigenvalue is not positive
    (or the inputs hold a NaN: a node whose refit failed).  A positive definite estimate on the same graph needs the
    constrained maximum-likelihood refit, which is not implemented."""
    import warnings
    assert rule in ('min', 'average'), f"rule = {rule!r}: 'min' or 'average'"
    C = np.asarray(coef, dtype=np.float64)
    tau = np.asarray(resvar, dtype=np.float64).reshape(-1)
    assert C.ndim == 2 and C.shape[0] == C.shape[1] == tau.size, f"coef (p,p) and resvar (p,) do not fit: {C.shape}, {tau.shape}"
    p = tau.size
    with np.errstate(all='ignore'):
        raw = -C / tau[None, :]
        a, b = np.triu(raw, 1), np.triu(raw.T, 1)                           # Theta_ij from node j, from node i (i < j)
        up = np.where(np.abs(b) < np.abs(a), b, a) if rule == 'min' else 0.5 * (a + b)
        up = np.triu(up, 1)
        Theta = up + up.T
        Theta[np.arange(p), np.arange(p)] = 1.0 / tau
    if not np.all(np.isfinite(Theta)):
        warnings.warn("neighborhood_precision: the regressions hold a non-finite value (a node whose refit failed, a residual "
                      "variance of zero); the matrix is returned as it is", RuntimeWarning, stacklevel=2)
        return Theta, float('nan')
    lmin = float(np.linalg.eigvalsh(Theta)[0])
    if not lmin > 0:
        warnings.warn(f"neighborhood_precision: the smallest eigenvalue is {lmin:.3g}; the regression-based estimator is not "
                      f"positive definite by construction", RuntimeWarning, stacklevel=2)
    return Theta, lmin


def mb_cv_scores(resvar, heldout, bad, score='pseudo'):
    """(L,F) scores of a neighbourhood cross-validation from its per-node arrays (L,F,p), summed on the host:
    ``'pseudo'``: ``sum_j log tau_j^2 + r_j / tau_j^2`` (the negative Gaussian pseudo-log-likelihood per held-out observation, up
    to a constant), +inf for a (lambda, fold) with a node marked in ``bad`` (L,F,p: a refit status 1-3, a non-finite path) or
    whose tau^2 is not positive; ``'mse'``:
    ``sum_j r_j`` (NaN where a node has none)."""
    import math
    assert score in ('pseudo', 'mse'), f"score = {score!r}: 'pseudo' or 'mse'"
    tau, r, bad = np.asarray(resvar, dtype=np.float64), np.asarray(heldout, dtype=np.float64), np.asarray(bad, dtype=bool)
    L, F = tau.shape[:2]
    out = np.zeros((L, F))
    for l in range(L):
        for f in range(F):
            if score == 'mse':
                out[l, f] = math.fsum(r[l, f]) if np.all(np.isfinite(r[l, f])) else np.nan
            elif np.any(bad[l, f]) or not np.all(tau[l, f] > 0) or not np.all(np.isfinite(r[l, f])):
                out[l, f] = np.inf
            else:
                out[l, f] = math.fsum(np.log(tau[l, f]) + r[l, f] / tau[l, f])
    return out


# -----------------------------------------------------------------------------------------------------------------
# Joint neighbourhood selection of K instances that share structure: the regression counterpart of the GGL penalty
# (Chiquet, Grandvalet, Ambroise 2011, R's simone; the penalty of Danaher, Wang, Witten 2014).  For node j
#     min_B  sum_k omega_k [ 1/2 beta^(k)' S^(k) beta^(k) - s_j^(k)' beta^(k) ]
#            + lambda1 sum_k sum_{i != j} |beta^(k)_i| + lambda2 sum_{i != j} ||(beta^(1)_i, ..., beta^(K)_i)||_2
# by block coordinate descent (one block: the K coefficients of one variable; Simon, Friedman, Hastie, Tibshirani 2013).
# On the device: csrc/neighborhood_joint.hip, one workgroup per (chain, node); DESIGN 30.
# -----------------------------------------------------------------------------------------------------------------
_MBJ_MAX_ROUNDS = 100
_MBJ_NEWTON_CAP = 64
_MBJ_COUPLINGS = {'group': 'joint_neighborhood_selection', 'fused': 'fused_neighborhood_selection'}     # coupling -> front end


def mb_joint_limits():
    """(largest K, largest p) of the device route, as the library reports them (``ggl_mb_joint_limits``)."""
    out = (ctypes.c_int * 2)()
    _lib.load().ggl_mb_joint_limits(out)
    return int(out[0]), int(out[1])


def _mbj_args(S, lambda1, lambda2, rule, instance_weights, tol, max_sweeps, refit, t, coupling='group'):
    """(S (K,p,p) C-contiguous, lambda1 descending (L1,), lambda2 (L2,), omega (K,) or None) of what
    ``joint_neighborhood_selection`` (``coupling='group'``) and ``fused_neighborhood_selection`` (``'fused'``) accept; their
    refusals, which name the caller."""
    assert coupling in _MBJ_COUPLINGS, f"coupling = {coupling!r}: 'group' or 'fused'"
    who = _MBJ_COUPLINGS[coupling]
    Sm = np.asarray(S, dtype=np.float64)
    assert Sm.ndim == 3 and Sm.shape[-1] == Sm.shape[-2] and Sm.shape[-1] >= 1 and Sm.shape[0] >= 1, \
        f"{who} needs a (K,p,p) stack of square matrices, S has shape {Sm.shape}"
    K, p = Sm.shape[0], Sm.shape[1]
    l1 = np.sort(np.atleast_1d(np.asarray(lambda1, dtype=np.float64)).reshape(-1))[::-1].copy()
    l2 = np.atleast_1d(np.asarray(lambda2, dtype=np.float64)).reshape(-1).copy()
    assert l1.size >= 1 and l2.size >= 1, "lambda1 and lambda2 need at least one value each"
    assert np.all(np.isfinite(l1)) and np.all(l1 >= 0), "every lambda1 must be non-negative and finite"
    assert np.all(np.isfinite(l2)) and np.all(l2 >= 0), "every lambda2 must be non-negative and finite"
    assert np.all(np.diff(l1) < 0), "the lambda1 of a grid must differ"
    assert l1.min() + l2.min() > 0, "lambda1 + lambda2 must be positive at every grid point"
    assert rule in _MB_RULES, f"rule = {rule!r}: 'and', 'or' or 'raw'"
    assert not (refit and rule == 'raw'), "refit needs a graph: rule 'and' or 'or'"
    assert tol >= 0 and np.isfinite(tol), f"tol = {tol}: it must be non-negative and finite"
    assert int(max_sweeps) >= 1, f"max_sweeps = {max_sweeps}: at least one sweep is needed"
    assert np.isfinite(t) and t >= 0, f"t = {t}: the edge threshold must be finite and not negative"
    om = None
    if instance_weights is not None:
        om = np.ascontiguousarray(np.asarray(instance_weights, dtype=np.float64).reshape(-1))
        assert om.shape == (K,), f"instance_weights must hold one weight per instance ({K}), has shape {om.shape}"
        if not (np.all(np.isfinite(om)) and np.all(om > 0)):
            k = int(np.flatnonzero(~(np.isfinite(om) & (om > 0)))[0])
            raise ValueError(f"instance_weights[{k}] = {om[k]}: an instance weight must be positive and finite")
    if not np.all(np.isfinite(Sm)):
        k, i, q = np.argwhere(~np.isfinite(Sm))[0]
        raise ValueError(f"{who}: S of instance {int(k)}: the entry ({int(i)}, {int(q)}) is not finite")
    dg = np.diagonal(Sm, axis1=1, axis2=2)
    if not np.all(dg > 0):
        k, i = np.argwhere(~(dg > 0))[0]
        raise ValueError(f"{who}: S of instance {int(k)}, variable {int(i)}: the diagonal entry is "
                         f"{dg[k, i]}; it must be positive")
    asym = np.argwhere(Sm != np.swapaxes(Sm, 1, 2))
    if asym.size:
        k, i, q = asym[0]
        raise ValueError(f"{who}: S of instance {int(k)} is not bitwise symmetric: the entries "
                         f"({int(i)}, {int(q)}) and ({int(q)}, {int(i)}) differ")
    return as_c(Sm), l1, l2, om


def _condat_tv(y, lam):
    """Condat's direct 1-D total-variation prox of ``y`` (N >= 2) at ``lam`` in float64: ``mbf_condat``'s decisions and
    arithmetic in its order (``condat_inplace`` of the Theta-step), the trip cap N (N + 1) / 2 and NaN behind it included."""
    N, x = len(y), y.copy()
    k = k0 = kplus = kminus = 0
    vmin, vmax, umin, umax = y[0] - lam, y[0] + lam, lam, -lam
    for _ in range(N * (N + 1) // 2):
        if k == N - 1:
            if umin < 0.0:
                x[k0:kminus + 1] = vmin
                kminus += 1
                k = k0 = kminus
                umin, vmin = lam, y[k]
                umax = vmin + lam - vmax
                if k == N - 1:
                    x[k] = vmin + umin
                    return x
            elif umax > 0.0:
                x[k0:kplus + 1] = vmax
                kplus += 1
                k = k0 = kplus
                umax, vmax = -lam, y[k]
                umin = vmax - lam - vmin
                if k == N - 1:
                    x[k] = vmin + umin
                    return x
            else:
                x[k0:] = vmin + umin / float(k - k0 + 1)
                return x
        else:
            yn = y[k + 1]
            if yn + umin - vmin < -lam:
                x[k0:kminus + 1] = vmin
                kminus += 1
                k = kplus = k0 = kminus
                vmin = y[k]
                vmax, umin, umax = vmin + 2 * lam, lam, -lam
            elif yn + umax - vmax > lam:
                x[k0:kplus + 1] = vmax
                kplus += 1
                k = kminus = k0 = kplus
                vmax = y[k]
                vmin, umin, umax = vmax - 2 * lam, lam, -lam
            else:
                k += 1
                umin, umax = umin + yn - vmin, umax + yn - vmax
                if umin >= lam:
                    vmin += (umin - lam) / float(k - k0 + 1)
                    umin, kminus = lam, k
                if umax <= -lam:
                    vmax += (umax + lam) / float(k - k0 + 1)
                    umax, kplus = -lam, k
    return np.full(N, np.nan)


def _host_mbj_unit(S, om, dg, j, l1s, l2s, tol, max_sweeps, coupling='group'):
    """The chain of node j: (B (L,K,p), resvar (L,K), sweeps (L,), status (L,), newton (L,)) -- the unit of work of
    ``k_mb_joint_path`` (``coupling='group'``) or ``k_mb_fused_path`` (``'fused'``: the majorised fused-lasso block update and
    the dual feasibility screen), step by step."""
    fused = coupling == 'fused'
    K, p, L = S.shape[0], S.shape[1], len(l1s)
    B, g = np.zeros((K, p)), om[:, None] * S[:, j, :]
    member = np.zeros(p, dtype=bool)
    act = np.zeros(0, dtype=np.int64)
    out_b, out_r = np.zeros((L, K, p)), np.zeros((L, K))
    out_s, out_st, out_n = np.zeros(L, dtype=np.int64), np.zeros(L, dtype=np.int64), np.zeros(L, dtype=np.int64)
    state = {'newton': 0, 'nfb': False}
    dead = False

    def sweep(l1, l2):
        dmax = 0.0
        for i in act:
            a, bo = om * dg[:, i], B[:, i].copy()
            b = np.zeros(K)
            if fused:
                a = np.max(a)                                               # one curvature for the block
                v = bo + g[:, i] / a
                x = v if (l2 == 0.0 or K == 1) else _condat_tv(v, l2 / a)
                if not np.all(np.isfinite(x)):
                    state['nfb'] = True
                x = np.where(np.isnan(x), 0.0, x)                           # (the device's soft turns a NaN into 0)
                b = np.sign(x) * np.maximum(np.abs(x) - l1 / a, 0.0)
            else:
                z = g[:, i] + a * bo
                u = np.sign(z) * np.maximum(np.abs(z) - l1, 0.0)
                un = np.sqrt(np.sum(u * u))
                if un > l2:
                    if l2 == 0.0:
                        b = u / a
                    else:
                        nu, it = (un - l2) / np.max(a), 0
                        while it < _MBJ_NEWTON_CAP:
                            tt = 1.0 / (a * nu + l2)
                            ut = u * tt
                            f, fp = np.sum(ut * ut) - 1.0, -2.0 * np.sum(ut * ut * a * tt)
                            nn = nu - f / fp
                            if not (nn > nu):
                                break
                            nu, it = nn, it + 1
                        state['newton'] = max(state['newton'], it)
                        b = u * nu / (a * nu + l2)
            if not np.all(np.isfinite(b)):
                state['nfb'] = True
            d = b - bo
            nz = d != 0.0
            if np.any(nz):
                g[nz] -= (om[nz] * d[nz])[:, None] * S[nz, i, :]
                B[nz, i] = b[nz]
            cm = np.fmax.reduce(np.abs(d) * a)
            dmax = cm if cm > dmax else dmax
        return dmax

    def screen(l1, l2):
        if fused:
            # 0 solves the fused-lasso prox of g_i exactly if the dual is feasible: the interval of admissible t_k, walked along k
            lo, hi, ok = np.zeros(p), np.zeros(p), np.ones(p, dtype=bool)
            for k in range(K - 1):
                lo, hi = lo + g[k] - l1, hi + g[k] + l1
                lo, hi = np.where(lo < -l2, -l2, lo), np.where(hi > l2, l2, hi)
                ok &= lo <= hi
            out = ~(ok & (lo + g[K - 1] - l1 <= 0.0) & (hi + g[K - 1] + l1 >= 0.0))
        else:
            sg = np.maximum(np.abs(g) - l1, 0.0)
            out = np.sqrt(np.sum(sg * sg, axis=0)) > l2
        viol = ~member & out
        viol[j] = False
        member[viol] = True
        return int(viol.sum())

    def bad():
        return state['nfb'] or not np.all(np.isfinite(g))

    for l in range(L):
        l1, l2, sweeps, status = l1s[l], l2s[l], 0, 1
        state['newton'] = 0
        if dead or bad():
            status = 2
        else:
            d1 = 0.0
            for rnd in range(_MBJ_MAX_ROUNDS):
                nviol = screen(l1, l2)
                act = np.flatnonzero(member)
                if nviol == 0 and (not (d1 > tol) if rnd > 0 else act.size == 0):
                    status = 0
                    break
                conv = False
                while sweeps < max_sweeps:
                    dm = sweep(l1, l2)
                    sweeps += 1
                    if not (dm > tol):
                        conv = True
                        break
                if not conv:
                    break
                g[:] = om[:, None] * S[:, j, :]
                for i in act:
                    nz = B[:, i] != 0.0
                    if np.any(nz):
                        g[nz] -= (om[nz] * B[nz, i])[:, None] * S[nz, i, :]
                if sweeps >= max_sweeps:
                    break
                d1 = sweep(l1, l2)
                sweeps += 1
                if bad():
                    status = 2
                    break
            if status == 1 and bad():
                status = 2
        dead = status == 2
        if dead:
            out_b[l], out_r[l] = np.nan, np.nan
            out_b[l, :, j] = 0.0
        else:
            out_b[l] = B
            out_r[l] = dg[:, j] - np.sum(B[:, act] * (S[:, j, act] + g[:, act] / om[:, None]), axis=1)
        out_s[l], out_st[l], out_n[l] = sweeps, status, state['newton']
    return out_b, out_r, out_s, out_st, out_n


def _joint_run(Sm, l1, l2, om, rule, tol, max_sweeps, refit, t, device, host, want_coef=True, last_only=False, coupling='group'):
    """The grid ``l1`` (L1, descending) x ``l2`` (L2) as L2 chains of L1 pairs, on the device or through the twin.  Returns a
    dict of arrays in grid layout (L1,L2,...): W (None without ``want_coef``), RESVAR, INFO (L1,L2,p,3) and, with ``refit``,
    REFIT_COEF (None without ``want_coef``), REFIT_RESVAR, REFIT_INFO (L1,L2,K,p,2).  ``last_only``: W and REFIT_COEF are
    (L2,K,p,p), the LAST pair of every chain (``ggl_neighborhood_joint_last``: nothing else is downloaded); the tables stay
    whole.  ``coupling``: 'group' (``k_mb_joint_path``) or 'fused' (``k_mb_fused_path``, through the ``_fused_`` entries)."""
    K, p, L, C = Sm.shape[0], Sm.shape[1], l1.size, l2.size
    lam1 = np.ascontiguousarray(np.broadcast_to(l1[None, :], (C, L)))
    lam2 = np.ascontiguousarray(np.broadcast_to(l2[:, None], (C, L)))
    out = {'W': None, 'REFIT_COEF': None}
    if host:
        omv = np.ones(K) if om is None else om
        dg = np.ascontiguousarray(np.diagonal(Sm, axis1=1, axis2=2))
        raw, resvar = np.zeros((C, L, K, p, p)), np.zeros((C, L, K, p))
        info = np.zeros((C, L, p, 3), dtype=np.int32)
        with np.errstate(all='ignore'):
            for c in range(C):
                for j in range(p):
                    b, r, s, st, nw = _host_mbj_unit(Sm, omv, dg, j, lam1[c], lam2[c], float(tol), int(max_sweeps), coupling)
                    raw[c, :, :, :, j], resvar[c, :, :, j] = b, r
                    info[c, :, j, 0], info[c, :, j, 1], info[c, :, j, 2] = s, st, nw
        W = raw if rule == 'raw' else neighborhood_graph(raw, rule)
        out.update(W=W, RESVAR=resvar, INFO=info)
        if refit:
            rf = host_neighborhood_refit(Sm, np.ascontiguousarray(np.moveaxis(W.reshape(C * L, K, p, p), 1, 0)), t=t)
            out['REFIT_COEF'] = np.moveaxis(rf['COEF'], 0, 1).reshape(C, L, K, p, p)
            out['REFIT_RESVAR'] = np.moveaxis(rf['RESVAR'], 0, 1).reshape(C, L, K, p)
            out['REFIT_INFO'] = np.stack([np.moveaxis(rf['DEGREE'], 0, 1), np.moveaxis(rf['STATUS'], 0, 1)], axis=-1) \
                .reshape(C, L, K, p, 2).astype(np.int32)
    else:
        _lib.require_gpu()
        lib = _lib.load()
        cshape = (C, K, p, p) if last_only else (C, L, K, p, p)
        coef = np.empty(cshape) if want_coef else None
        resvar, info = np.empty((C, L, K, p)), np.empty((C, L, p, 3), dtype=np.int32)
        rcoef = np.empty(cshape) if (refit and want_coef) else None
        rres = np.empty((C, L, K, p)) if refit else None
        rinfo = np.empty((C, L, K, p, 2), dtype=np.int32) if refit else None
        ip = lambda a: None if a is None else a.ctypes.data_as(_lib._ip)
        entry = getattr(lib, f"ggl_neighborhood_{'fused' if coupling == 'fused' else 'joint'}_{'last' if last_only else 'path'}")
        check(entry(int(device), K, p, ptr(Sm), ptr(om), C, L, ptr(lam1), ptr(lam2), _MB_RULES[rule], float(tol), int(max_sweeps),
                    int(bool(refit)), float(t), ptr(coef), ptr(resvar), ip(info), ptr(rcoef), ptr(rres), ip(rinfo)))
        out.update(W=coef, RESVAR=resvar, INFO=info)
        if refit:
            out.update(REFIT_COEF=rcoef, REFIT_RESVAR=rres, REFIT_INFO=rinfo)
    sw = lambda a: None if a is None else np.ascontiguousarray(np.swapaxes(a, 0, 1))        # (C,L,...) -> (L1,L2,...)
    res = {k: sw(v) for k, v in out.items()}
    if last_only:
        for k in ('W', 'REFIT_COEF'):
            if out[k] is not None:
                res[k] = np.ascontiguousarray(out[k][:, L - 1]) if host else out[k]
    return res


def _joint_result(out, l1, l2, refit, return_info):
    if not return_info:
        return out['W']
    info = {'LAMBDA1': l1, 'LAMBDA2': l2, 'RESVAR': out['RESVAR'], 'SWEEPS': out['INFO'][..., 0].astype(np.int64),
            'STATUS': out['INFO'][..., 1].astype(np.int64), 'NEWTON': out['INFO'][..., 2].astype(np.int64)}
    if refit:
        info.update(REFIT_COEF=out['REFIT_COEF'], REFIT_RESVAR=out['REFIT_RESVAR'],
                    DEGREE=out['REFIT_INFO'][..., 0].astype(np.int64), REFIT_STATUS=out['REFIT_INFO'][..., 1].astype(np.int64))
    return out['W'], info


def joint_neighborhood_selection(S, lambda1, lambda2, rule='and', instance_weights=None, tol=1e-7, max_sweeps=10000, refit=False,
                                 t=1e-8, device=0, return_info=False):
    """Joint neighbourhood selection of K instances on the device (``ggl_neighborhood_joint_path``): every node's K
    regressions are coupled by a group penalty across the instances (``lambda2``) beside the lasso penalty of each
    (``lambda1``) -- ``reg='GGL'`` for neighbourhood selection.  S: (K,p,p), every ``S[k]`` bitwise symmetric with a positive
    diagonal; ``instance_weights`` (K,) positive, default all 1.  Limits: ``mb_joint_limits()``, read from the library.

    ``lambda1`` (L1) x ``lambda2`` (L2): one chain per ``lambda2``, walked along the descending ``lambda1`` with warm starts.
    Returns W (L1,L2,K,p,p): per instance the symmetrised coefficients (``neighborhood_graph``; ``rule='raw'``: column j holds
    ``beta^(k)`` of node j).  With ``lambda1 = 0`` the K supports coincide; with ``lambda2 = 0`` these are K separate lassos.

    ``return_info``: also a dict with ``LAMBDA1`` (descending), ``LAMBDA2``, ``RESVAR`` (L1,L2,K,p: the unweighted residual
    variances), ``SWEEPS``, ``STATUS`` (L1,L2,p: 0 converged, 1 a cap was reached, 2 a non-finite value -- all K columns of that
    node are NaN from that ``lambda1`` on), ``NEWTON`` (the largest number of Newton steps a block's root took) and, with
    ``refit`` (rule 'and' / 'or'): ``REFIT_COEF``, ``REFIT_RESVAR``, ``DEGREE``, ``REFIT_STATUS`` -- every instance refitted on its
    graph (entries with ``|W| >= t``) as ``neighborhood_refit`` does, on the device.  The same bits on every call, a chain's
    independent of the others, a point's independent of the ``lambda1`` below it."""
    Sm, l1, l2, om = _mbj_args(S, lambda1, lambda2, rule, instance_weights, tol, max_sweeps, refit, t)
    out = _joint_run(Sm, l1, l2, om, rule, tol, max_sweeps, bool(refit), t, device, False)
    return _joint_result(out, l1, l2, bool(refit), return_info)


def host_joint_neighborhood_selection(S, lambda1, lambda2, rule='and', instance_weights=None, tol=1e-7, max_sweeps=10000,
                                      refit=False, t=1e-8, return_info=False):
    """numpy twin of ``joint_neighborhood_selection``: the same procedure in the same order (screen of the groups, sweeps of
    block updates over the ascending active list with the same Newton iteration, all gradients recomputed in ascending order,
    one further sweep, one further screen; the same caps and statuses) in float64 with numpy's own summation orders, so its
    last bits differ from the device's.  The refit goes through ``host_neighborhood_refit``.  For engines without the device
    route and for tests without a GPU."""
    Sm, l1, l2, om = _mbj_args(S, lambda1, lambda2, rule, instance_weights, tol, max_sweeps, refit, t)
    out = _joint_run(Sm, l1, l2, om, rule, tol, max_sweeps, bool(refit), t, 0, True)
    return _joint_result(out, l1, l2, bool(refit), return_info)


def mb_fused_limits():
    """(largest K, largest p) of the fused device route, as the library reports them (``ggl_mb_fused_limits``)."""
    out = (ctypes.c_int * 2)()
    _lib.load().ggl_mb_fused_limits(out)
    return int(out[0]), int(out[1])


def fused_neighborhood_selection(S, lambda1, lambda2, rule='and', instance_weights=None, tol=1e-7, max_sweeps=10000, refit=False,
                                 t=1e-8, device=0, return_info=False):
    """Fused joint neighbourhood selection of K ORDERED instances on the device (``ggl_neighborhood_fused_path``): every
    node's K regressions are coupled by the total variation of each coefficient along the instances' given order
    (``lambda2 sum_k |beta^(k+1)_i - beta^(k)_i|``) beside the lasso penalty of each (``lambda1``) -- ``reg='FGL'`` for
    neighbourhood selection, time-varying neighbourhood selection (Kolar, Song, Ahmed, Xing 2010).  The arguments and the
    results of ``joint_neighborhood_selection``; ``NEWTON`` is all 0.  Limits: ``mb_fused_limits()``, read from the library.

    With ``lambda2 = 0`` these are K separate lassos; with ``lambda2`` large enough the K coefficient vectors of a node
    coincide and are the lasso on ``sum_k omega_k S^(k)`` at ``K lambda1``; with K = 1 ``lambda2`` is inert.  A block (the K
    coefficients of one variable) is updated by the fused-lasso prox under the one curvature ``max_k omega_k S^(k)_ii``: exact
    block minimisation where these are equal (correlation stacks, equal weights), a majorise-minimise step with the same fixed
    points otherwise, which takes more sweeps.  The same bits on every call, a chain's independent of the others, a point's
    independent of the ``lambda1`` below it."""
    Sm, l1, l2, om = _mbj_args(S, lambda1, lambda2, rule, instance_weights, tol, max_sweeps, refit, t, 'fused')
    out = _joint_run(Sm, l1, l2, om, rule, tol, max_sweeps, bool(refit), t, device, False, coupling='fused')
    return _joint_result(out, l1, l2, bool(refit), return_info)


def host_fused_neighborhood_selection(S, lambda1, lambda2, rule='and', instance_weights=None, tol=1e-7, max_sweeps=10000,
                                      refit=False, t=1e-8, return_info=False):
    """numpy twin of ``fused_neighborhood_selection``: the same procedure in the same order (the dual feasibility screen,
    sweeps of majorised block updates over the ascending active list with the same Condat scan, all gradients recomputed in
    ascending order, one further sweep, one further screen; the same caps and statuses) in float64 with numpy's own summation
    orders, so its last bits differ from the device's.  The refit goes through ``host_neighborhood_refit``."""
    Sm, l1, l2, om = _mbj_args(S, lambda1, lambda2, rule, instance_weights, tol, max_sweeps, refit, t, 'fused')
    out = _joint_run(Sm, l1, l2, om, rule, tol, max_sweeps, bool(refit), t, 0, True, coupling='fused')
    return _joint_result(out, l1, l2, bool(refit), return_info)


def joint_neighborhood_precision(coef, resvar, rule='min'):
    """``neighborhood_precision`` per instance: ``coef`` (K,p,p) with column j node j's coefficients in instance k, ``resvar``
    (K,p).  Returns ``(Theta (K,p,p), lambda_min (K,))``."""
    C, tau = np.asarray(coef, dtype=np.float64), np.asarray(resvar, dtype=np.float64)
    assert C.ndim == 3 and C.shape[1] == C.shape[2] and tau.shape == C.shape[:2], \
        f"coef (K,p,p) and resvar (K,p) do not fit: {C.shape}, {tau.shape}"
    res = [neighborhood_precision(C[k], tau[k], rule) for k in range(C.shape[0])]
    return np.stack([r[0] for r in res]), np.array([r[1] for r in res])
