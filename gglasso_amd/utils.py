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


def sample_covariance(X, center=True, scale=False, device=0):
    """``numpy.cov(X_k, bias=True)`` of every instance on the device (FP64 matrix cores; bitwise symmetric and reproducible).

    X: (p,N), (K,p,N), or a list / dict (keys 0..K-1) of (p_k,N_k) arrays, variables in rows (the reference's ``sample[k]``).
    Returns S of the matching kind -- (p,p), (K,p,p), or a dict with keys 0..K-1.  ``center=False``: the raw second moment.
    ``scale=True``: the correlations, and as a second return value the variances (same kind, (p,), (K,p) or dict).
    Instances of different dimension take one library call per distinct p_k."""
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


def sample_covariance_subsets(X, indices, center=True, scale=False, device=0):
    """``numpy.cov(X[:, indices[r]], bias=True)`` for every row r of ``indices`` (B, b) on the device: X (p, N), variables in
    rows, goes up once and the columns are gathered there -- the subsamples of ``model_selection.stars_search``.  Duplicate
    indices are allowed (a bootstrap draw).  Returns S (B,p,p), bitwise what ``sample_covariance`` gives for the B gathered
    arrays as one (B,p,b) stack; ``scale=True``: each subset's own correlations, and as a second value the variances (B,p)."""
    X = as_c(X)
    assert X.ndim == 2 and X.shape[0] >= 1 and X.shape[1] >= 1, \
        f"data must be a (p,N) array with variables in rows, has shape {X.shape}"
    flags = (_lib.COV_CENTER if center else 0) | (_lib.COV_SCALE if scale else 0)
    S, var = _covariance_subsets_call(X, _subset_indices(indices), flags, device)
    return (S, var) if scale else S
