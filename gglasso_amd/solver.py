"""Drop-in ADMM solvers: ``ADMM_MGL``, ``ADMM_SGL`` and ``ADMM_FSGL`` with the reference's keyword signatures and
return contracts (solver/admm_solver.py:13-313, solver/single_admm_solver.py:15-275, solver/functional_sgl_admm.py:12-238
of fabian-sp/GGLasso), usable as the ``solver`` callable of ``grid_search`` (helper/model_selection.py:55,222).

What stays on the host (as in the reference): iteration count, the rho rule, the stopping decision,
status strings, verbose printing, exit warnings.  What moves to the MI355X: every array operation of
the loop body.  S, Omega, Theta, L, X live in HBM for the whole solve; per iteration two scalars go
down (rho, lambda/rho) and five squared norms come back.

There is no CPU fallback: constructing the engine raises if libggl_hip.so or a GPU is missing.
"""
import math
import time
import warnings

import numpy as np

from . import _lib
from ._lib import as_c, check, ptr

_REG = {"SGL": _lib.REG_SGL, "GGL": _lib.REG_GGL, "FGL": _lib.REG_FGL, "FSGL": _lib.REG_FSGL}


# ctx options (include/ggl_hip.h GGL_OPT_*, names in _lib.OPTIONS) every engine is created with.  Empty in normal
# use: the library's defaults are the measured best.  The parity tests set entries to drive the iteration through
# every dispatch (speculation hits and forced misses, both Newton-Schulz product modes, the mirroring Theta kernels).
ENGINE_OPTIONS = {}


# Rank of the latent component in the model-selection tables (helper/model_selection.py:256, :638 call
# numpy.linalg.matrix_rank(L), i.e. #{|lambda_i| > p * eps * max|lambda|}).  That rule fits an L rebuilt from an
# eigendecomposition (null space at 1e-16 |L|), and every L this library RETURNS is one: up to p = 8 (GGL_NS_MIN_P; rounds
# 1-3: 128) the L-step is the LDS Jacobi eigensolver, above it the per-iteration L-step is the sign iteration (null space at
# 4e-14 .. 7e-13 |L|, which numpy's rule counts as rank: 22 for 6 on a p = 500 SGL problem, tools/probe_rank_noise.py) and the
# solve's LAST L-step is redone as an eigendecomposition before the solution is handed out (HipEngine.finalize_L, round 4).  So
# the rule is numpy's, on every route; RANK_REL_TOL (rounds 1-3: a 1e-9 cut for the sign iteration's L) is kept for callers
# that look at an L mid-solve.
RANK_REL_TOL = 1e-9


def latent_rank(L, rel_tol=0.0):
    """numpy.linalg.matrix_rank of one symmetric (p,p) L (rel_tol 0: numpy's p * eps; host counterpart of
    ``HipEngine.selection_rank``)."""
    a = np.abs(np.linalg.eigvalsh(L))
    return int(np.count_nonzero(a > a.max() * max(rel_tol, L.shape[0] * np.finfo(np.float64).eps)))


def _host_period(A, K=None, p=None):
    """(C-contiguous host array to upload, period): a numpy.broadcast_to VIEW (stride 0 along its first axis) of one (p,p)
    matrix as (K,p,p), or of one (K',p,p) stack as (G,K',p,p), is uploaded once -- period 1 resp. K' -- and replicated on
    the device (ggl_set_S_ex / ggl_set_state_ex); anything else travels whole (period 0).  With K and p given the shape is
    CHECKED against the ctx's stack -- the C side copies period * p * p (or K * p * p) doubles out of the buffer it is handed
     -- and a single matrix, (p,p) or (1,p,p), for K > 1 instances is taken as shared (period 1)."""
    if K is not None:
        assert A.ndim in (2, 3, 4) and A.shape[-2:] == (p, p), \
            f"array of shape {A.shape} does not fit a stack of {K} ({p},{p}) matrices"
        if A.ndim == 2:
            return as_c(A), (1 if K > 1 else 0)
        lead = int(np.prod(A.shape[:-2]))
        if A.ndim == 3 and A.shape[0] == 1 and K > 1:
            return as_c(A[0]), 1
        assert lead == K, f"array of shape {A.shape} does not fit a stack of {K} ({p},{p}) matrices"
    if A.ndim == 3 and A.shape[0] > 1 and A.strides[0] == 0:
        return as_c(A[0]), 1
    if A.ndim == 4:
        if A.shape[0] > 1 and A.strides[0] == 0:
            return as_c(A[0]), int(A.shape[1])
        return as_c(A).reshape(-1, A.shape[2], A.shape[3]), 0
    return as_c(A), 0


class HipEngine:
    """Device-resident ADMM state behind the C ABI (one ggl_ctx)."""
    _S_scaled = False       # True while the ctx holds variances beside its S: after set_data(scale=True), until S is set anew

    def __init__(self, S, Omega_0, Theta_0, X_0, L_0=None, eig=_lib.EIG_AUTO, device=0, stream=None, options=None):
        """stream: None (the ctx creates a private stream) or an int HIP stream handle -- 0 is the legacy default
        stream itself, not "none" (a NULL handle used to be read as "create one")."""
        _lib.require_gpu()
        self.lib = _lib.load()
        S = np.asarray(S, dtype=np.float64)
        self.K, self.p = int(np.prod(S.shape[:-2])), int(S.shape[-1])      # (K,p,p), or (G,K',p,p) for a grid of problems
        h = _lib._vp()
        flags = int(eig) | (0 if stream is None else _lib.CTX_STREAM_GIVEN)
        check(self.lib.ggl_ctx_create(int(device), self.K, self.p, flags, stream, h))
        self.h = h
        self.device = int(device)
        self.stream_handle = None if stream is None else int(stream)
        for name, value in {**ENGINE_OPTIONS, **(options or {})}.items():
            self.set_option(name, value)
        # broadcast VIEWS (what the batched grids pass for S, Omega_0, X_0) are uploaded once and replicated on the device
        # instead of being materialised on the host: _host_period
        import ctypes
        assert S.ndim in (3, 4) and S.shape[-2] == S.shape[-1], f"S must be (K,p,p) or (G,K,p,p), is {S.shape}"
        Sh, s_period = _host_period(S, self.K, self.p)
        check(self.lib.ggl_set_S_ex(self.h, ptr(Sh), s_period))
        arrs, periods = [], (ctypes.c_int * 4)(0, 0, 0, 0)
        for slot, A in enumerate((Omega_0, Theta_0, L_0, X_0)):
            if A is None:
                arrs.append(None)
                continue
            Ah, periods[slot] = _host_period(np.asarray(A, dtype=np.float64), self.K, self.p)
            arrs.append(Ah)
        check(self.lib.ggl_set_state_ex(self.h, ptr(arrs[0]), ptr(arrs[1]), ptr(arrs[2]), ptr(arrs[3]), periods))
        self._norms = np.zeros(5)
        self._norms_p = ptr(self._norms)
        self._ptr_cache = {}

    def set_data(self, X, N=None, center=True, scale=False, missing=None, min_pairs=2):
        """The ctx's S computed on the device from observations and left there (``ggl_set_S_from_data``): X a (K,p,N)
        array or a list of K (p,N_k) arrays, variables in rows; N (optional) the K sample counts, checked against the
        data.  ``scale``: S becomes the correlations, ``get_S`` then also returns the variances.
        ``missing='pairwise'``: NaN is a missing value and S the pairwise-complete covariance
        (``ggl_set_S_from_data_pairwise``, see ``utils.sample_covariance``); a refused call (a variable without observations, a
        pair sharing fewer than ``min_pairs`` samples) leaves the ctx's S and variances as they were."""
        import ctypes
        assert missing in (None, 'pairwise'), "missing must be None (complete data) or 'pairwise'"
        Xs = [as_c(x) for x in (X if isinstance(X, (list, tuple)) else np.asarray(X))]
        assert len(Xs) == self.K and all(x.ndim == 2 and x.shape[0] == self.p for x in Xs), \
            f"data must be {self.K} arrays of shape ({self.p}, N_k)"
        Nk = [x.shape[1] for x in Xs]
        if N is not None:
            assert list(np.broadcast_to(np.asarray(N, dtype=int), (self.K,))) == Nk, f"N = {N} does not match the data ({Nk})"
        flags = (_lib.COV_CENTER if center else 0) | (_lib.COV_SCALE if scale else 0)
        if missing == 'pairwise':
            check(self.lib.ggl_set_S_from_data_pairwise(self.h, (_lib._dp * self.K)(*[ptr(x) for x in Xs]),
                                                        (ctypes.c_int * self.K)(*Nk), flags, int(min_pairs)))
            self._S_scaled = bool(scale)
            return
        self._S_scaled = False              # the call drops the ctx's variances first, also where it fails
        check(self.lib.ggl_set_S_from_data(self.h, (_lib._dp * self.K)(*[ptr(x) for x in Xs]), (ctypes.c_int * self.K)(*Nk),
                                           flags))
        self._S_scaled = bool(scale)

    def set_data_subsets(self, X, indices, center=True, scale=False, missing=None, min_pairs=2):
        """The ctx's S from column subsets of ONE data array, computed on the device (``ggl_set_S_from_subsets``): X (p,N),
        variables in rows, ``indices`` (B,b) ints with B a divisor of K; instance k gets ``cov(X[:, indices[k % B]])``.
        A refused call (an index outside [0,N), say) leaves S as it was.  ``missing='pairwise'``: every subset's
        pairwise-complete covariance (``ggl_set_S_from_subsets_pairwise``), as in ``set_data``."""
        from .utils import _subset_indices
        assert missing in (None, 'pairwise'), "missing must be None (complete data) or 'pairwise'"
        X = as_c(X)
        assert X.ndim == 2 and X.shape[0] == self.p, f"data must be a ({self.p}, N) array"
        idx = _subset_indices(indices)
        flags = (_lib.COV_CENTER if center else 0) | (_lib.COV_SCALE if scale else 0)
        if missing == 'pairwise':
            check(self.lib.ggl_set_S_from_subsets_pairwise(self.h, ptr(X), X.shape[1], idx.shape[0], idx.shape[1],
                                                           idx.ctypes.data_as(_lib._ip), flags, int(min_pairs)))
        else:
            check(self.lib.ggl_set_S_from_subsets(self.h, ptr(X), X.shape[1], idx.shape[0], idx.shape[1],
                                                  idx.ctypes.data_as(_lib._ip), flags))
        self._S_scaled = bool(scale)

    def set_data_weighted(self, X, weights, center=True, scale=False):
        """The ctx's S as weighted covariances of ONE data array, computed on the device (``ggl_set_S_from_weighted``): X (p,N),
        variables in rows, ``weights`` (K,N) non-negative; instance k gets ``numpy.cov(X, aweights=weights[k], bias=True)`` --
        with ``utils.kernel_weights`` the kernel-smoothed stack of a time series.  X goes up once.  A refused call (a negative
        weight, a row of zeros, a constant variable under ``scale``) leaves the ctx's S and variances as they were."""
        X = as_c(X)
        assert X.ndim == 2 and X.shape[0] == self.p, f"data must be a ({self.p}, N) array"
        w = as_c(weights)
        assert w.shape == (self.K, X.shape[1]), f"weights must be ({self.K}, {X.shape[1]}), have shape {w.shape}"
        flags = (_lib.COV_CENTER if center else 0) | (_lib.COV_SCALE if scale else 0)
        check(self.lib.ggl_set_S_from_weighted(self.h, ptr(X), X.shape[1], ptr(w), flags))
        self._S_scaled = bool(scale)

    def set_kendall_subsets(self, X, indices=None):
        """The ctx's S as skeptic matrices ``sin(pi/2 tau-b)`` of column subsets of ONE data array, computed on the device
        (``ggl_set_S_from_kendall``): X (p,N), variables in rows, ``indices`` (B,b) ints with B a divisor of K (None: all
        samples, B = 1); instance k gets the matrix of ``X[:, indices[k % B]]``.  A refused call (a variable constant over a
        subset, an index outside [0,N)) leaves S as it was."""
        from .utils import _subset_indices, dense_ranks
        X = as_c(X)
        assert X.ndim == 2 and X.shape[0] == self.p, f"data must be a ({self.p}, N) array"
        R = dense_ranks(X)
        idx = None if indices is None else _subset_indices(indices)
        B, b = (1, X.shape[1]) if idx is None else idx.shape
        check(self.lib.ggl_set_S_from_kendall(self.h, R.ctypes.data_as(_lib._ip), X.shape[1], B, b,
                                              None if idx is None else idx.ctypes.data_as(_lib._ip)))
        self._S_scaled = False

    def set_mixed_subsets(self, X, indices=None, types=None, clip=0.999):
        """The ctx's S as latent correlation matrices of mixed binary / continuous data (``utils.mixed_correlation``) of column
        subsets of ONE data array, computed on the device (``ggl_set_S_from_mixed``): X, ``indices`` and the layout as
        ``set_kendall_subsets``; ``types`` (p,) 1 binary / 0 continuous (None: a variable with two distinct values is binary).
        A refused call (a variable constant over a subset, a bad ``types`` or ``clip``) leaves S as it was."""
        from .utils import _mixed_types, _subset_indices, dense_ranks
        X = as_c(X)
        assert X.ndim == 2 and X.shape[0] == self.p, f"data must be a ({self.p}, N) array"
        R = dense_ranks(X)
        t = _mixed_types(R, types)
        idx = None if indices is None else _subset_indices(indices)
        B, b = (1, X.shape[1]) if idx is None else idx.shape
        check(self.lib.ggl_set_S_from_mixed(self.h, R.ctypes.data_as(_lib._ip), t.ctypes.data_as(_lib._ip), X.shape[1], B, b,
                                            None if idx is None else idx.ctypes.data_as(_lib._ip), float(clip)))
        self._S_scaled = False

    def project_S(self, period=None, eps=1e-8, tol=1e-10, max_iter=500):
        """The ctx's S replaced, where it lies, by its nearest-correlation projection (``ggl_project_S``, see
        ``utils.nearest_correlation``): every matrix keeps its diagonal and ends with ``lambda_min >= eps min(diagonal)``.
        ``period=B``, a divisor of K: S holds B distinct matrices, instance k carrying matrix ``k % B`` (what the
        ``set_*_subsets`` calls install); the B are projected once and replicated on the device.  None: all K.  Returns the
        info dict of ``utils.nearest_correlation`` (arrays over the matrices projected); a ``RuntimeWarning`` names those that
        did not converge.  A refused call (a non-finite entry, a non-positive diagonal) leaves S as it was."""
        from .utils import _nc_result
        B = self.K if period is None else int(period)
        assert 0.0 <= eps <= 0.5, f"eps = {eps}, the eigenvalue floor lies in [0, 0.5]"
        assert 1e-14 <= tol <= 1e-2, f"tol = {tol}, the tolerance lies in [1e-14, 1e-2]"
        assert int(max_iter) >= 1, f"max_iter = {max_iter}, at least one iteration is needed"
        assert 1 <= B <= self.K and self.K % B == 0, f"period = {period} must be a divisor of K = {self.K}"
        iters = np.zeros(B, dtype=np.int32)
        info = np.zeros((B, 4))
        check(self.lib.ggl_project_S(self.h, 0 if period is None else B, float(eps), float(tol), int(max_iter),
                                     iters.ctypes.data_as(_lib._ip), ptr(info)))
        _, out = _nc_result(None, False, iters.astype(np.int64), info[:, 0].copy(), info[:, 1].copy(), info[:, 2].copy(),
                            int(max_iter), True, "project_S")
        out["fallbacks"] = int(info[0, 3])
        return out

    def edge_stability(self, B, t=1e-8, counts=False):
        """StARS over the Theta snapshots of a batch of K = L * B points (instance l * B + r: subsample r at lambda l):
        the (L,) int64 array ``sum_{i<j} c (B - c)`` of the selection counts ``c[l,i,j] = #{r : |Theta| >= t}``, exact; with
        ``counts`` also the (L,p,p) int32 tables of c (mirrored, zero diagonal)."""
        import ctypes
        L = self.K // int(B) if int(B) >= 1 and self.K % int(B) == 0 else 1        # (otherwise the library refuses the call)
        num = np.zeros(L, dtype=np.int64)
        tab = np.empty((L, self.p, self.p), dtype=np.int32) if counts else None
        check(self.lib.ggl_edge_stability(self.h, int(B), float(t), None if tab is None else tab.ctypes.data_as(_lib._ip),
                                          num.ctypes.data_as(ctypes.POINTER(ctypes.c_longlong))))
        return (num, tab) if counts else num

    def neighborhood_stability(self, lambda_range, rule='and', tol=1e-7, max_sweeps=10000, t=1e-8, counts=False, stack=False,
                               weights=None, scaled=False, sig_tol=1e-7, max_outer=100):
        """Meinshausen-Buhlmann neighbourhood selection on the K matrices the ctx's S holds -- the B = K subsample matrices
        a ``set_*_subsets`` call wrote -- along the descending grid ``lambda_range`` (``ggl_neighborhood_stability``, see
        ``utils.neighborhood_selection``), and the edge stability of the result: the symmetrised (L,K,p,p) stack stays on the
        device and is reduced as in ``edge_stability``.  Returns a dict: ``num`` (L,) int64, ``sweeps`` and ``status``
        (L,K,p), with ``counts`` the (L,p,p) int32 tables, with ``stack`` the stack itself.  ``weights`` ((p,p) shared or
        (K,p,p)), ``scaled``, ``sig_tol``, ``max_outer`` as in ``utils.neighborhood_selection``: with ``weights`` or ``scaled``
        the call goes to ``ggl_neighborhood_stability_w`` and the dict gains ``outer`` (L,K,p); without, it is the call it
        was."""
        import ctypes
        from .utils import _MB_RULES, _mbw_args
        lam = as_c(np.asarray(lambda_range, dtype=np.float64).reshape(-1))
        assert rule in ('and', 'or'), f"rule = {rule!r}: 'and' or 'or'"
        L = lam.size
        num = np.zeros(L, dtype=np.int64)
        tab = np.empty((L, self.p, self.p), dtype=np.int32) if counts else None
        W = np.empty((L, self.K, self.p, self.p)) if stack else None
        fn, extra, ni = self.lib.ggl_neighborhood_stability, (), 2
        if weights is not None or scaled:
            Wt, per_matrix = _mbw_args(weights, scaled, sig_tol, max_outer, self.K, self.p)
            fn, ni = self.lib.ggl_neighborhood_stability_w, 3
            extra = (ptr(Wt), int(per_matrix), int(bool(scaled)), float(sig_tol), int(max_outer))
        info = np.empty((L, self.K, self.p, ni), dtype=np.int32)
        check(fn(self.h, L, ptr(lam), _MB_RULES[rule], float(tol), int(max_sweeps), float(t), *extra,
                 num.ctypes.data_as(ctypes.POINTER(ctypes.c_longlong)), None if tab is None else tab.ctypes.data_as(_lib._ip),
                 ptr(W), info.ctypes.data_as(_lib._ip)))
        out = {'num': num, 'sweeps': info[..., 0].astype(np.int64), 'status': info[..., 1].astype(np.int64)}
        if ni == 3:
            out['outer'] = info[..., 2].astype(np.int64)
        if counts:
            out['counts'] = tab
        if stack:
            out['stack'] = W
        return out

    def neighborhood_cv(self, X, test_idx, lambda_range, rule='and', tol=1e-7, max_sweeps=10000, t=1e-8, refit=True,
                        center=True, stack=False, weights=None, scaled=False, sig_tol=1e-7, max_outer=100):
        """One cross-validation step of neighbourhood selection on the K = F train matrices the ctx's S holds (a
        ``set_*_subsets`` call with the train indices wrote them), ``ggl_neighborhood_cv``: the path along the descending grid,
        symmetrised by ``rule``; the F test covariances of ``X[:, test_idx[f]]`` built on the device as ``heldout_scores``
        builds them; then with ``refit`` every node regressed on its neighbours by least squares on the train matrix
        (``utils.neighborhood_refit``) and scored on the test matrix, without it the lasso's own coefficients scored there.
        Returns a dict of (L,K,p) arrays: ``resvar`` (tau^2), ``heldout`` (r), ``status``, and ``degree`` (with ``refit``) or
        ``sweeps`` (without); with ``stack`` the symmetrised (L,K,p,p) stack.  ``weights`` ((p,p) shared or (K,p,p)),
        ``scaled``, ``sig_tol``, ``max_outer`` as in ``utils.neighborhood_selection``: with ``weights`` or ``scaled`` the call
        goes to ``ggl_neighborhood_cv_w`` (without ``refit`` the dict gains ``outer``); without, it is the call it was."""
        from .utils import _MB_RULES, _mbw_args, _subset_indices
        X = as_c(X)
        assert X.ndim == 2 and X.shape[0] == self.p, f"data must be a ({self.p}, N) array"
        idx = _subset_indices(test_idx)
        lam = as_c(np.asarray(lambda_range, dtype=np.float64).reshape(-1))
        assert rule in ('and', 'or'), f"rule = {rule!r}: 'and' or 'or'"
        L = lam.size
        resvar, heldout = np.empty((L, self.K, self.p)), np.empty((L, self.K, self.p))
        W = np.empty((L, self.K, self.p, self.p)) if stack else None
        fn, extra, ni = self.lib.ggl_neighborhood_cv, (), 2
        if weights is not None or scaled:
            Wt, per_matrix = _mbw_args(weights, scaled, sig_tol, max_outer, self.K, self.p)
            fn, ni = self.lib.ggl_neighborhood_cv_w, 3
            extra = (ptr(Wt), int(per_matrix), int(bool(scaled)), float(sig_tol), int(max_outer))
        buf = np.empty(L * self.K * self.p * ni, dtype=np.int32)
        check(fn(self.h, ptr(X), X.shape[1], idx.shape[0], idx.shape[1], idx.ctypes.data_as(_lib._ip),
                 _lib.COV_CENTER if center else 0, L, ptr(lam), _MB_RULES[rule], float(tol), int(max_sweeps), float(t),
                 1 if refit else 0, *extra, ptr(resvar), ptr(heldout), buf.ctypes.data_as(_lib._ip), ptr(W)))
        if refit:
            ni = 2                                                      # the refit's info: two ints per node, in front
        info = buf[:L * self.K * self.p * ni].reshape(L, self.K, self.p, ni)
        out = {'resvar': resvar, 'heldout': heldout, 'status': info[..., 1].astype(np.int64),
               ('degree' if refit else 'sweeps'): info[..., 0].astype(np.int64)}
        if ni == 3:
            out['outer'] = info[..., 2].astype(np.int64)
        if stack:
            out['stack'] = W
        return out

    def heldout_scores(self, X, test_idx, center=True, out=None):
        """K-fold cross-validation over the Theta snapshots of a batch of K = L * F points (instance l * F + f: fold f at
        lambda l): (K,4) = ``<S_test[k % F], Theta_k>``, log det Theta_k, count_nonzero(Theta_k), lambda_min(Theta_k), with
        ``S_test[f]`` the covariance of ``X[:, test_idx[f]]`` (``test_idx`` (F,m) ints) built on the device beside the ctx's S
        (``ggl_heldout_scores``).  The last three columns are the bits of ``selection_stats``.  ``out``: a (K,4) array to
        write into; a refused call leaves it alone."""
        from .utils import _subset_indices
        X = as_c(X)
        assert X.ndim == 2 and X.shape[0] == self.p, f"data must be a ({self.p}, N) array"
        idx = _subset_indices(test_idx)
        if out is None:
            out = np.zeros((self.K, 4))
        assert out.shape == (self.K, 4) and out.dtype == np.float64 and out.flags.c_contiguous
        check(self.lib.ggl_heldout_scores(self.h, ptr(X), X.shape[1], idx.shape[0], idx.shape[1],
                                          idx.ctypes.data_as(_lib._ip), _lib.COV_CENTER if center else 0, ptr(out)))
        return out

    def get_S(self):
        """S (K,p,p) as it lies on the device; after ``set_data(..., scale=True)`` the pair (S, variances (K,p))."""
        S = np.empty((self.K, self.p, self.p))
        var = np.empty((self.K, self.p)) if self._S_scaled else None
        check(self.lib.ggl_get_S(self.h, ptr(S), ptr(var)))
        return S if var is None else (S, var)

    def set_state(self, Omega, Theta, X, L=None):
        """Overwrite the iterate (admm_solver.py:142-150 semantics: L None zeroes it)."""
        for A in (Omega, Theta, X, L):
            assert A is None or np.shape(A) == (self.K, self.p, self.p), f"state arrays must be {(self.K, self.p, self.p)}"
        check(self.lib.ggl_set_state(self.h, ptr(as_c(Omega)), ptr(as_c(Theta)), ptr(None if L is None else as_c(L)),
                                     ptr(as_c(X))))

    def save_state(self):
        """Keep a device copy of the iterate (a start point several solves / benchmark regions return to)."""
        check(self.lib.ggl_state_snapshot(self.h, 0))

    def restore_state(self):
        """Back to the saved iterate, device to device (set_state with the same arrays, without the upload)."""
        check(self.lib.ggl_state_snapshot(self.h, 1))

    def set_option(self, name, value):
        check(self.lib.ggl_ctx_set_option(self.h, _lib.OPTIONS[name], float(value)))

    def get_option(self, name):
        out = np.zeros(1)
        check(self.lib.ggl_ctx_get_option(self.h, _lib.OPTIONS[name], ptr(out)))
        return float(out[0])

    # -- iteration pieces ------------------------------------------------------------------
    def set_lambda1_mask(self, lam_pp):
        check(self.lib.ggl_set_lambda1_mask(self.h, ptr(None if lam_pp is None else as_c(lam_pp))))

    def set_lambda1_mask_k(self, lam_Kpp):
        """One (p,p) threshold array lambda1 * lambda1_mask per instance (K,p,p); None clears it."""
        check(self.lib.ggl_set_lambda1_mask_k(self.h, ptr(None if lam_Kpp is None else as_c(lam_Kpp))))

    def set_instance_dims(self, pk):
        """Instances of different dimension in identity-padded slots: the stopping-test sums of ``sgl_batch_step`` run
        over the leading (pk[k],pk[k]) blocks only; None: all of dimension p."""
        import ctypes
        if pk is None:
            check(self.lib.ggl_set_instance_dims(self.h, None))
            return
        pk = np.ascontiguousarray(pk, dtype=np.int32)
        assert pk.shape == (self.K,)
        check(self.lib.ggl_set_instance_dims(self.h, pk.ctypes.data_as(ctypes.POINTER(ctypes.c_int))))

    def set_block_size(self, M):
        """Functional SGL (functional_sgl_admm.py:14): the Theta-step of ``step(..., 'FSGL', ...)`` and of the batched
        single problems shrinks M x M blocks by their Frobenius norm (prox_sum_Frob, ggl_helper.py:45-66); 0 / None clears."""
        check(self.lib.ggl_set_block_size(self.h, int(M or 0)))

    def fsgl_stats(self):
        """{'M': block size, 'pair_steps': FSGL Theta-steps as one launch over tile pairs (M <= 32), 'table_steps': behind the
        table of block sums (M > 32), 'fused_sgl_steps': fused one-launch SGL iterations (p <= 64) this ctx ran}."""
        import ctypes
        out = (ctypes.c_longlong * 4)()
        check(self.lib.ggl_fsgl_stats(self.h, out))
        return dict(zip(("M", "pair_steps", "table_steps", "fused_sgl_steps"), (int(v) for v in out)))

    def _cptr(self, a):
        """ctypes pointer of a parameter vector, cached per array object (this sits on the per-iteration path)."""
        if a is None:
            return None
        hit = self._ptr_cache.get(id(a))
        if hit is None or hit[0] is not a:
            hit = (a, ptr(a))
            self._ptr_cache[id(a)] = hit
        return hit[1]

    def step(self, rho, lambda1, lambda2, reg, latent, mu1, nk):
        rc = self.lib.ggl_admm_step(self.h, rho, lambda1, lambda2, _REG[reg], int(latent), self._cptr(mu1),
                                    self._cptr(nk), self._norms_p)
        if rc != 0:
            # ggl_admm_step repeats a rejected speculative step itself; a positive code here would mean the
            # repeat (which does not speculate) was rejected as well
            if rc > 0:
                raise RuntimeError(f"ggl_admm_step: unexpected return code {rc} (speculative step rejected twice)")
            check(rc)
        return self._norms

    def hint_last_step(self):
        """The next ``step`` is the last one of the caller's loop: no chain is pre-launched behind it."""
        self.lib.ggl_hint_last_step(self.h)

    def step_omega(self, rho, latent, nk, speculate=False):
        fn = self.lib.ggl_step_omega_spec if speculate else self.lib.ggl_step_omega
        check(fn(self.h, rho, int(latent), ptr(nk)))

    def step_group_partial(self, rho, lambda1):
        check(self.lib.ggl_step_group_partial(self.h, rho, lambda1))

    def step_finish(self, rho, lambda1, lambda2, reg, latent, mu1, groupsq_ready, defer_norms=False):
        """defer_norms: leave the five local sums on the device (BUF_NORMS) for an on-device all-reduce; fetch
        them with ``read_norms`` afterwards."""
        rc = check(self.lib.ggl_step_finish(self.h, rho, lambda1, lambda2, _REG[reg], int(latent), ptr(mu1),
                                            int(groupsq_ready) | (2 if defer_norms else 0), ptr(self._norms)))
        if defer_norms:
            return None
        # 1 = the speculative Omega-step of this iteration was rejected (the iterate is untouched, Omega un-flipped):
        # there are no norms; the caller repeats the iteration with step_omega(speculate=False)
        return None if rc == 1 else self._norms.copy()

    def read_norms(self):
        """The five sums, or None when a speculative Omega-step failed validation on some rank (repeat the step)."""
        rc = self.lib.ggl_norms_read(self.h, ptr(self._norms))
        if rc == 1:
            return None
        check(rc)
        return self._norms.copy()

    def scale_X(self, f):
        check(self.lib.ggl_scale_X(self.h, f))

    # -- RCCL behind the C ABI (K-sharded GGL: the whole iteration incl. both all-reduces is one call) -----------
    def comm_init(self, rank, nranks, unique_id):
        check(self.lib.ggl_comm_init(self.h, int(rank), int(nranks), bytes(unique_id)))

    def comm_count(self):
        """ncclCommCount of the ctx's communicator: the ranks RCCL itself sees."""
        import ctypes
        n = ctypes.c_int(0)
        check(self.lib.ggl_comm_count(self.h, ctypes.byref(n)))
        return int(n.value)

    def step_sharded(self, rho, lambda1, lambda2, nk, latent=False, mu1=None):
        """One K-sharded GGL iteration on this rank's slab; returns the five GLOBAL sums (same on every rank)."""
        check(self.lib.ggl_admm_step_sharded_latent(self.h, rho, lambda1, lambda2, int(latent), self._cptr(mu1),
                                                    self._cptr(nk), self._norms_p))
        return self._norms

    # -- K independent single problems (batched lambda path) ----------------------------------
    def sgl_batch_step(self, rho, lambda1, latent, mu1):
        out = np.zeros((self.K, 5))
        check(self.lib.ggl_sgl_batch_step(self.h, ptr(as_c(rho)), ptr(as_c(lambda1)), int(latent),
                                          ptr(None if mu1 is None else as_c(mu1)), ptr(out)))
        return out

    def scale_X_batch(self, factors):
        check(self.lib.ggl_scale_X_batch(self.h, ptr(as_c(factors))))

    def batch_run(self, n_iters, rho, last, status, fin_iter, it_base, dims, tol, rtol, update_rho, snap=None, stop_after=0,
                  *, lambda1, lambda2=None, reg=None, latent=False, mu1=None, nk=None, G=None):
        """Up to ``n_iters`` batch iterations in ONE C call (ggl_sgl_batch_run; ggl_mgl_batch_run when ``G`` problems of K/G
        instances are given): per-point stopping test, rho rule and X rescale taken in C, bit for bit ``batch._decide``.
        rho (n,) float64, last (n,4) float64, status (n,) int32 (0 live, 1 converged, 2 failed), fin_iter (n,) int32 are
        updated IN PLACE.  snap = (engine, slots int32 per instance slot): finishing points are snapshotted there on the
        device, failed ones parked, and the loop goes on until all are finished, ``stop_after`` are (> 0), or n_iters;
        None: returns after the first iteration with an event.  Returns the iterations run."""
        ip = _lib._ip
        n = self.K if G is None else int(G)
        for a, dt, shp in ((rho, np.float64, (n,)), (last, np.float64, (n, 4)), (status, np.int32, (n,)),
                           (fin_iter, np.int32, (n,))):
            assert a.dtype == dt and a.flags.c_contiguous and a.shape == shp, (a.dtype, a.shape, shp)
        sh, si = (None, None)
        if snap is not None:
            sh = snap[0].h
            si = np.ascontiguousarray(snap[1], dtype=np.int32)
            assert si.shape == (self.K,)
        sip = None if si is None else si.ctypes.data_as(ip)
        mu = ptr(None if mu1 is None else as_c(mu1))
        if G is None:
            rc = self.lib.ggl_sgl_batch_run(self.h, int(n_iters), ptr(rho), ptr(as_c(lambda1)), int(latent), mu,
                                            ptr(as_c(dims)), float(tol), float(rtol), int(bool(update_rho)), ptr(last),
                                            status.ctypes.data_as(ip), fin_iter.ctypes.data_as(ip), int(it_base), sh, sip,
                                            int(stop_after))
        else:
            rc = self.lib.ggl_mgl_batch_run(self.h, n, int(n_iters), ptr(rho), ptr(as_c(lambda1)), ptr(as_c(lambda2)),
                                            _REG[reg], int(latent), mu, ptr(None if nk is None else as_c(nk)),
                                            ptr(as_c(dims)), float(tol), float(rtol), int(bool(update_rho)), ptr(last),
                                            status.ctypes.data_as(ip), fin_iter.ctypes.data_as(ip), int(it_base), sh, sip,
                                            int(stop_after))
        return int(check(rc))

    def snapshot_state_from(self, kd, src, ks):
        """Omega, Theta, L, X of instance ``ks`` of the engine ``src`` (may be this one) into slot ``kd``'s device snapshot."""
        check(self.lib.ggl_snapshot_state_from(self.h, int(kd), src.h, int(ks)))

    def snapshots(self, latent=False, names=None):
        """{'Omega','Theta','X'[,'L']}: the (K,p,p) snapshot stacks, one download each; ``names``: only these."""
        shape = (self.K, self.p, self.p)
        want = [nm for nm in ('Omega', 'Theta', 'X') + (('L',) if latent else ()) if names is None or nm in names]
        arr = {nm: np.empty(shape) for nm in want}
        check(self.lib.ggl_get_snapshots(self.h, ptr(arr.get('Omega')), ptr(arr.get('Theta')), ptr(arr.get('L')),
                                         ptr(arr.get('X'))))
        return arr

    def snapshot_state_k(self, k):
        """(Omega, X) of instance k's snapshot."""
        Om, X = np.empty((self.p, self.p)), np.empty((self.p, self.p))
        check(self.lib.ggl_get_snapshot_state_k(self.h, int(k), ptr(Om), ptr(X)))
        return Om, X

    # -- G independent multiple-graph problems in one stack (batched lambda1 x lambda2 grid) -------------------
    def mgl_batch_step(self, G, rho, lambda1, lambda2, reg, latent, mu1, nk):
        """One ADMM_MGL iteration of all G problems (problem g = instances g*K/G ..); returns the (G,5) sums."""
        out = np.zeros((int(G), 5))
        rc = self.lib.ggl_mgl_batch_step(self.h, int(G), ptr(as_c(rho)), ptr(as_c(lambda1)), ptr(as_c(lambda2)),
                                         _REG[reg], int(latent), ptr(None if mu1 is None else as_c(mu1)),
                                         ptr(None if nk is None else as_c(nk)), ptr(out))
        if rc > 0:
            raise RuntimeError(f"ggl_mgl_batch_step: unexpected return code {rc} (speculative step rejected twice)")
        check(rc)
        return out

    def state_k(self, k, latent=False):
        shape = (self.p, self.p)
        Om, Th, X = np.empty(shape), np.empty(shape), np.empty(shape)
        L = np.empty(shape) if latent else None
        check(self.lib.ggl_get_state_k(self.h, int(k), ptr(Om), ptr(Th), ptr(L), ptr(X)))
        sol = {'Omega': Om, 'Theta': Th, 'X': X}
        if latent:
            sol['L'] = L
        return sol

    def snapshot_k(self, k):
        check(self.lib.ggl_snapshot_k(self.h, int(k)))

    def snapshot_from(self, kd, src, ks):
        """Snapshot instance ``ks`` of the engine ``src`` (a compacted batch, ``subset``) into slot ``kd`` of this one."""
        check(self.lib.ggl_snapshot_from(self.h, int(kd), src.h, int(ks)))

    def selection_stats(self):
        """(K,4): <S,Theta>, log det Theta (-inf if lambda_min <= 1e-12), count_nonzero(Theta), lambda_min(Theta)
        of every instance's snapshot."""
        out = np.zeros((self.K, 4))
        check(self.lib.ggl_selection_stats(self.h, ptr(out)))
        return out

    def threshold_scan(self, tau_range):
        """(K, len(tau_range), 4): the four selection statistics of every snapshot thresholded at every tau
        (helper/model_selection.py:698-737); second value: eigenvalue problems solved for them."""
        import ctypes
        tau = as_c(np.asarray(tau_range, dtype=np.float64))
        out = np.zeros((self.K, tau.size, 4))
        n_eig = ctypes.c_int(0)
        check(self.lib.ggl_threshold_scan(self.h, ptr(tau), int(tau.size), ptr(out), ctypes.byref(n_eig)))
        return out, int(n_eig.value)

    def selection_rank(self, rel_tol=0.0):
        """(K,4): rank of every L snapshot at the relative tolerance (<= 0: numpy.linalg.matrix_rank's p*eps),
        max|lambda|, the largest |lambda| left out and the smallest one counted."""
        out = np.zeros((self.K, 4))
        check(self.lib.ggl_selection_rank(self.h, float(rel_tol), ptr(out)))
        return out

    # -- batches of independent problems: fault isolation and compaction (include/ggl_hip.h, GGL_OPT_ISOLATE) ----------------
    def failed_instances(self):
        """(K,) 0/1: instances the library marked (non-finite data, eigensolver failure) since the ctx was created."""
        import ctypes
        out = np.zeros(self.K, dtype=np.int32)
        check(self.lib.ggl_failed_instances(self.h, out.ctypes.data_as(ctypes.POINTER(ctypes.c_int))))
        return out

    _FAIL_WHY = {1: "a spectral / norm bound that is not finite or not positive", 2: "an eigensolver that did not converge",
                 3: "a non-finite residual in the L-step's sign iteration", 4: "marked inside a fused batch iteration"}

    def failed_reason(self, k):
        """Why the library marked instance k (ggl_failed_reason), as text, or None if it did not."""
        out = np.zeros(2)
        check(self.lib.ggl_failed_reason(self.h, int(k), ptr(out)))
        if out[0] == 0:
            return None
        return f"{self._FAIL_WHY.get(int(out[0]), 'marked')} (value {out[1]!r})"

    def reset_instance(self, k):
        """Park instance k on the identity problem (S = Omega = Theta = I, L = X = 0)."""
        check(self.lib.ggl_reset_instance(self.h, int(k)))

    def subset(self, idx):
        """A NEW engine holding the instances ``idx`` of this one (device to device: S, iterate, masks, dimensions, options);
        this engine stays valid."""
        import ctypes
        idx = np.ascontiguousarray(idx, dtype=np.int32)
        h = _lib._vp()
        check(self.lib.ggl_ctx_create_subset(self.h, idx.ctypes.data_as(ctypes.POINTER(ctypes.c_int)), int(idx.size),
                                             ctypes.byref(h)))
        new = object.__new__(type(self))
        new.lib, new.h, new.K, new.p = self.lib, h, int(idx.size), self.p
        new.device, new.stream_handle = self.device, None
        new._norms = np.zeros(5)
        new._norms_p = ptr(new._norms)
        new._ptr_cache = {}
        return new

    def finalize_L(self, which=0):
        """Rebuild the L a solve returns from one eigendecomposition of the last L-step's input where that step was the
        sign iteration (ggl_finalize_L; which 0: live iterate, 1: snapshots).  Returns (instances rebuilt, (K,) ranks:
        #{eig(C_k) > mu1_k/rho} for the rebuilt instances, -1 for the others)."""
        import ctypes
        rk = np.full(self.K, -1, dtype=np.int32)
        n = check(self.lib.ggl_finalize_L(self.h, int(which), rk.ctypes.data_as(ctypes.POINTER(ctypes.c_int))))
        return int(n), rk

    def finalize_stats(self):
        """{'calls': eigendecompositions ggl_finalize_L ran on this ctx, 'retries': of those repeated because their eigenvalues
        did not add up to trace(C)} (the check of round 6)."""
        import ctypes
        out = (ctypes.c_longlong * 2)()
        check(self.lib.ggl_finalize_stats(self.h, out))
        return {'calls': int(out[0]), 'retries': int(out[1])}

    def snapshot_L_k(self, k):
        L = np.empty((self.p, self.p))
        check(self.lib.ggl_get_snapshot_k(self.h, int(k), None, ptr(L)))
        return L

    def objective(self, lambda1, lambda2, reg):
        out = np.zeros(3)
        check(self.lib.ggl_objective(self.h, lambda1, lambda2, _REG[reg], ptr(out)))
        return out

    def kkt_residual(self, rho, lambda1, lambda2, reg, latent, mu1, nk):
        out = np.zeros(1)
        check(self.lib.ggl_kkt_residual(self.h, rho, lambda1, lambda2, _REG[reg], int(latent), ptr(mu1), ptr(nk),
                                        ptr(out)))
        return float(out[0])

    def kkt_terms(self, rho, lambda1, lambda2, reg, latent, mu1, nk):
        """(4,): the terms ``kkt_residual`` is the maximum of, in the reference's order (admm_solver.py:343-371); term 4 is 0
        when not latent."""
        out = np.zeros(4)
        check(self.lib.ggl_kkt_terms(self.h, rho, lambda1, lambda2, _REG[reg], int(latent), ptr(mu1), ptr(nk), ptr(out)))
        return out

    def diag_stats(self):
        """{'logdet_w', 'logdet_chol', 'logdet_eig': ``objective`` calls by the route their log det took (eigenvalues of W from
        the last Omega-step, Cholesky factor of Omega, eigenvalues of Omega behind a failed factorisation); 'kkt_jacobi',
        'kkt_rocsolver': KKT calls by eigensolver; 'kkt_mask', 'kkt_mask_k': KKT calls with the shared / per-instance mask}."""
        import ctypes
        out = (ctypes.c_longlong * 8)()
        check(self.lib.ggl_diag_stats(self.h, out))
        return dict(zip(("logdet_w", "logdet_chol", "logdet_eig", "kkt_jacobi", "kkt_rocsolver", "kkt_mask", "kkt_mask_k"),
                        (int(v) for v in out)))

    def exit_checks(self, latent):
        out = np.zeros(5)
        check(self.lib.ggl_exit_checks(self.h, int(latent), ptr(out)))
        return out

    def exit_checks_fast(self, latent, shift_l, shift_tl=0.0):
        """(K,5): the three asymmetries and the two DECISIONS of the exit checks -- Theta_k - L_k - shift_tl I positive definite,
        L_k + shift_l I positive definite (1 / 0) -- by batched Cholesky factorisations, no eigenvalues (ggl_exit_checks_fast_k)."""
        out = np.zeros((self.K, 5))
        check(self.lib.ggl_exit_checks_fast_k(self.h, int(latent), float(shift_tl), float(shift_l), ptr(out)))
        return out

    def exit_checks_k(self, latent):
        out = np.zeros((self.K, 5))
        check(self.lib.ggl_exit_checks_k(self.h, int(latent), ptr(out)))
        return out

    # -- ext_ADMM_MGL: instances of different dimension in one padded stack (gglasso_amd/ext_solver.py) -----------
    def ext_setup(self, pk, G):
        import ctypes
        pk = np.ascontiguousarray(pk, dtype=np.int32)
        G = np.ascontiguousarray(G, dtype=np.int32)
        assert G.ndim == 3 and G.shape[0] == 2 and G.shape[2] == self.K
        ip = ctypes.POINTER(ctypes.c_int)
        check(self.lib.ggl_ext_setup(self.h, pk.ctypes.data_as(ip), G.ctypes.data_as(ip), int(G.shape[1])))

    def ext_setup_batch(self, nprob, pk, G):
        """nprob problems of K/nprob instances each with the dimensions pk and the bookkeeping array G of ONE problem."""
        import ctypes
        pk = np.ascontiguousarray(pk, dtype=np.int32)
        G = np.ascontiguousarray(G, dtype=np.int32)
        assert self.K % int(nprob) == 0 and G.ndim == 3 and G.shape[0] == 2 and G.shape[2] == self.K // int(nprob)
        ip = ctypes.POINTER(ctypes.c_int)
        check(self.lib.ggl_ext_setup_batch(self.h, int(nprob), pk.ctypes.data_as(ip), G.ctypes.data_as(ip), int(G.shape[1])))

    def ext_batch_step(self, nprob, rho, lambda1K, lambda2G, latent, mu1):
        """One iteration of all problems; returns the (nprob,5) sums."""
        out = np.zeros((int(nprob), 5))
        rc = self.lib.ggl_ext_batch_step(self.h, rho, ptr(as_c(lambda1K)), ptr(as_c(lambda2G)), int(latent),
                                         ptr(None if mu1 is None else as_c(mu1)), ptr(out))
        if rc > 0:
            raise RuntimeError(f"ggl_ext_batch_step: unexpected return code {rc} (speculative step rejected twice)")
        check(rc)
        return out

    def ext_state_k(self, k):
        """Lambda and X1 of one instance slot (snapshot of a converged problem of a batch)."""
        st = self.ext_state()          # (the ext state has no per-slot download; batches are small)
        return {'Lambda': st['Lambda'][k], 'X1': st['X1'][k]}

    def ext_set_state(self, Lambda, X1):
        check(self.lib.ggl_ext_set_state(self.h, ptr(as_c(Lambda)), ptr(None if X1 is None else as_c(X1))))

    def ext_state(self):
        shape = (self.K, self.p, self.p)
        Lam, X1 = np.empty(shape), np.empty(shape)
        check(self.lib.ggl_ext_get_state(self.h, ptr(Lam), ptr(X1)))
        return {'Lambda': Lam, 'X1': X1}

    def ext_step(self, rho, lambda1K, lambda2, latent, mu1):
        rc = self.lib.ggl_ext_admm_step(self.h, rho, self._cptr(lambda1K), lambda2, int(latent), self._cptr(mu1),
                                        self._norms_p)
        if rc != 0:
            if rc > 0:
                raise RuntimeError(f"ggl_ext_admm_step: unexpected return code {rc} (speculative step rejected twice)")
            check(rc)
        return self._norms

    def ext_kkt(self, rho, lambda1K, lambda2, latent, mu1):
        out = np.zeros(1)
        check(self.lib.ggl_ext_kkt_residual(self.h, rho, ptr(lambda1K), lambda2, int(latent), ptr(mu1), ptr(out)))
        return float(out[0])

    def state(self):
        shape = (self.K, self.p, self.p)
        Om, Th, L, X = (np.empty(shape) for _ in range(4))
        check(self.lib.ggl_get_state(self.h, ptr(Om), ptr(Th), ptr(L), ptr(X)))
        return {'Omega': Om, 'Theta': Th, 'L': L, 'X': X}

    def profile(self, on=1):
        """0 off, 1 every phase, 2 only the eigen / matrix-function phases (cheapest live timing)."""
        check(self.lib.ggl_profile_enable(self.h, int(on)))

    def profile_read(self, reset=True):
        """{phase: (total_ms, launches)} measured with HIP events on the ctx stream."""
        import ctypes
        ms = np.zeros(len(_lib.PHASES))
        cnt = (ctypes.c_longlong * len(_lib.PHASES))()
        check(self.lib.ggl_profile_read(self.h, ptr(ms), cnt, int(reset)))
        return {name: (float(ms[i]), int(cnt[i])) for i, name in enumerate(_lib.PHASES)}

    def ns_stats(self):
        import ctypes
        out = (ctypes.c_longlong * 16)()
        check(self.lib.ggl_ns_stats(self.h, out))
        return dict(zip(("calls", "steps", "stable_calls", "units", "launches", "rank_calls", "rank_retries",
                         "rank_fallbacks", "rank_launches", "spec_calls", "spec_misses", "spin_timeouts", "last_parts",
                         "last_variant", "eigh_fallbacks", "pre_dropped"), (int(v) for v in out)))

    def poly_stats(self):
        """GGL_OPT_OMEGA_POLY: {'seqs': Omega-step launch sequences that ran the direct polynomial, 'seqs_total': all of them,
        'last_deg': degree of the last direct polynomial}."""
        import ctypes
        out = (ctypes.c_longlong * 3)()
        check(self.lib.ggl_omega_poly_stats(self.h, out))
        return dict(zip(("seqs", "seqs_total", "last_deg"), (int(v) for v in out)))

    def rank_stats(self):
        import ctypes
        out = (ctypes.c_longlong * 4)()
        check(self.lib.ggl_rank_stats(self.h, out))
        st = dict(zip(("calls", "continued_calls", "continued_instances", "eigh_fallbacks"), (int(v) for v in out)))
        d = (ctypes.c_longlong * 2)()
        check(self.lib.ggl_deflate_stats(self.h, d))
        st["deflated_calls"], st["deflated_instances"] = int(d[0]), int(d[1])
        return st

    def group_stats(self):
        """GGL_OPT_GROUP_SCHED: {'steps': Omega-steps that ran as groups with their own schedules, 'groups': of the last step,
        'len', 'units': of its groups, 'units_sum': per group slot over all grouped steps}."""
        import ctypes
        out = (ctypes.c_longlong * 11)()
        us = np.zeros(4)
        check(self.lib.ggl_group_stats(self.h, out, ptr(us)))
        g = int(out[1])
        return {'steps': int(out[0]), 'groups': g, 'changes': int(out[10]), 'len': [int(out[2 + i]) for i in range(g)] if g > 1 else [],
                'units': [int(out[6 + i]) for i in range(g)] if g > 1 else [], 'units_sum': us.tolist()}

    def spectral_bounds(self):
        """(c, beta), K each: c_k >= lambda_max(W_k^2 + 4 beta_k I) of the last validated Omega-step, or None."""
        cb, be = np.zeros(self.K), np.zeros(self.K)
        if check(self.lib.ggl_spectral_bounds(self.h, ptr(cb), ptr(be))) == 0:
            return None
        return cb, be

    def lds_stats(self):
        """The LDS-resident Omega-step (p <= 64): launches, launches repeated on the launch chain, products and steps
        summed over all instances."""
        import ctypes
        out = (ctypes.c_longlong * 4)()
        check(self.lib.ggl_lds_stats(self.h, out))
        return dict(zip(("calls", "misses", "products", "steps"), (int(v) for v in out)))

    def pipeline_stats(self):
        import ctypes
        out = (ctypes.c_longlong * 10)()
        check(self.lib.ggl_pipeline_stats(self.h, out))
        return dict(zip(("prelaunched", "dropped", "early_launched", "early_used", "part_streams_tried", "w_fused", "w_fused_used",
                         "bound_rides", "copy_rides", "reduce_rides"),
                        (int(v) for v in out)))

    def eig_info(self):
        """(K,) sweeps of the LDS Jacobi kernel in the last step (-1: not converged), or rocSOLVER's info."""
        import ctypes
        out = np.zeros(self.K, dtype=np.int32)
        check(self.lib.ggl_eig_info(self.h, out.ctypes.data_as(ctypes.POINTER(ctypes.c_int))))
        return out

    def last_dispatch(self):
        import ctypes
        out = (ctypes.c_longlong * 4)()
        check(self.lib.ggl_last_dispatch(self.h, out))
        return dict(zip(("parts", "variant", "theta_kernel", "finalize_calls"), (int(v) for v in out)))

    def device_ptr(self, which):
        return self.lib.ggl_device_ptr(self.h, which)

    def sync(self):
        check(self.lib.ggl_ctx_sync(self.h))

    def close(self):
        if getattr(self, "h", None) is not None and self.h:
            self.lib.ggl_ctx_destroy(self.h)
            self.h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


# The engine class the solvers instantiate.  Tests of the host logic may substitute a class with
# the same methods; the shipped value is the HIP engine and nothing else.
ENGINE = HipEngine


def residuals_from_norms(sq, rho, tol, rtol, dim):
    """ADMM_stopping_criterion (solver/admm_solver.py:316-331) from the five squared norms."""
    n_om, n_thl, n_x, n_r, n_s = (math.sqrt(v) for v in sq)
    e_pri = dim * tol + rtol * max(n_om, n_thl)
    e_dual = dim * tol + rtol * rho * n_x
    return n_r, rho * n_s, e_pri, e_dual


def next_rho(rho, r_t, s_t):
    """Residual balancing (solver/admm_solver.py:227-233)."""
    if r_t >= 10 * s_t:
        return 2 * rho
    if s_t >= 10 * r_t:
        return 0.5 * rho
    return 1. * rho


def _run_admm(eng, reg, K_total, p, lambda1, lambda2, latent, mu1, nk, rho, tol, rtol, stopping_criterion,
              update_rho, max_iter, verbose, measure, title, comm=None, want_objective=False, show_rho=False):
    """Host control flow shared by ADMM_MGL / ADMM_SGL / ADMM_FSGL / the K-sharded driver.
    comm: None or an object with ``allreduce_groupsq(engine)`` and ``allreduce_norms(np.ndarray)``.
    show_rho: the verbose table carries a rho column (functional_sgl_admm.py:129-131, :188)."""
    runtime = np.zeros(max_iter)
    residual = np.zeros(max_iter)
    objective = np.zeros(max_iter)
    status = ''
    dim = K_total * ((p ** 2 + p) / 2)
    sharded_ggl = comm is not None and reg == 'GGL'
    device_norms = sharded_ggl and getattr(comm, "device_norms", False) and hasattr(eng, "read_norms")

    if ((measure and want_objective) or stopping_criterion != 'boyd') and hasattr(eng, "set_option") and comm is None:
        # the objective / the KKT residual are evaluated between the iterations and use the scratch a pre-launched
        # Omega-step chain would be working in: no pipelining across iterations here (include/ggl_hip.h, GGL_OPT_PIPELINE)
        eng.set_option("pipeline", 0)

    if verbose:
        print(f"------------ADMM Algorithm for {title} Graphical Lasso----------------")
        if stopping_criterion == 'boyd' and show_rho:
            print("%4s\t%10s\t%10s\t%10s\t%10s\t%10s" % ("iter", "r_t", "s_t", "eps_pri", "eps_dual", "rho"))
        elif stopping_criterion == 'boyd':
            print("%4s\t%10s\t%10s\t%10s\t%10s" % ("iter", "r_t", "s_t", "eps_pri", "eps_dual"))
        else:
            print("%4s\t%10s" % ("iter", "kkt residual"))

    r_t = s_t = e_pri = e_dual = 0.0
    iter_t = -1
    for iter_t in range(max_iter):
        if measure:
            start = time.time()
        if sharded_ggl and getattr(comm, "capi", False):
            # RCCL behind the C ABI: Omega-step, both all-reduces, Theta-step and the norms in one call
            if iter_t == max_iter - 1:
                eng.hint_last_step()
            sq = eng.step_sharded(rho, lambda1, lambda2, nk, latent, mu1)
        elif sharded_ggl:
            # device_norms: HIP engine over RCCL.  The Omega-step may then run speculatively; its validation flag
            # rides on the (p,p) all-reduce, so either every rank accepts the step or every rank repeats it.
            def sharded_pass(speculate):
                eng.step_omega(rho, latent, nk, *((True,) if speculate else ()))
                eng.step_group_partial(rho, lambda1)
                comm.allreduce_groupsq(eng)
                if device_norms:
                    # the five sums are all-reduced where they are (HBM) and cross PCIe once, already global
                    eng.step_finish(rho, lambda1, lambda2, reg, latent, mu1, 1, defer_norms=True)
                    return comm.allreduce_norms_device(eng)
                loc = eng.step_finish(rho, lambda1, lambda2, reg, latent, mu1, 1)
                return None if loc is None else comm.allreduce_norms(loc)

            sq = sharded_pass(device_norms)
            if sq is None:
                # the reduced validation flag says some rank's speculative schedule did not cover its spectrum: every
                # rank left its iterate alone; same iteration again, bounds first
                sq = sharded_pass(False)
                if sq is None:
                    raise RuntimeError("K-sharded ADMM: the non-speculative repeat of an iteration was rejected")
        else:
            if iter_t == max_iter - 1 and hasattr(eng, "hint_last_step"):
                eng.hint_last_step()
            sq = eng.step(rho, lambda1, lambda2, reg, latent, mu1, nk)
            if comm is not None:
                sq = comm.allreduce_norms(sq)
        if measure:
            runtime[iter_t] = time.time() - start
            if want_objective:
                o = eng.objective(lambda1, lambda2, reg)
                if comm is not None:
                    o[:2] = comm.allreduce_norms(o[:2])
                objective[iter_t] = o.sum()

        if stopping_criterion == 'boyd':
            r_t, s_t, e_pri, e_dual = residuals_from_norms(sq, rho, tol, rtol, dim)
            if update_rho:
                rho_new = next_rho(rho, r_t, s_t)
                if rho_new != rho:
                    eng.scale_X(rho / rho_new)       # solver/admm_solver.py:236
                rho = rho_new
            residual[iter_t] = max(r_t, s_t)
            if verbose and show_rho:
                print("%4d\t%10.4g\t%10.4g\t%10.4g\t%10.4g\t%10.4g" % (iter_t, r_t, s_t, e_pri, e_dual, rho))
            elif verbose:
                print("%4d\t%10.4g\t%10.4g\t%10.4g\t%10.4g" % (iter_t, r_t, s_t, e_pri, e_dual))
            if (r_t <= e_pri) and (s_t <= e_dual):
                status = 'optimal'
                break
        else:
            eta_A = eng.kkt_residual(rho, lambda1, lambda2, reg, latent, mu1, nk)
            residual[iter_t] = eta_A
            if verbose:
                print("%4d\t%10.4g" % (iter_t, eta_A))
            if eta_A <= tol:
                status = 'optimal'
                break

    if status != 'optimal':
        if stopping_criterion == 'boyd':
            if r_t <= e_pri:
                status = 'primal optimal'
            elif s_t <= e_dual:
                status = 'dual optimal'
            else:
                status = 'max iterations reached'
        else:
            status = 'max iterations reached'

    print(f"ADMM terminated after {iter_t+1} iterations with status: {status}.")
    info = {'status': status}
    if measure:
        info['runtime'] = runtime[:iter_t + 1]
        info['residual'] = residual[:iter_t + 1]
        if want_objective:
            info['objective'] = objective[:iter_t + 1]
    return info, rho


def _exit_report(eng, latent, psd_tol, verbose_min_ev):
    """Symmetry / definiteness checks after the loop (solver/admm_solver.py:284-301,
    solver/single_admm_solver.py:244-263)."""
    if hasattr(eng, "exit_checks_fast"):
        # the reference's DECISIONS first (two batched Cholesky factorisations); its eigenvalues only when a warning has to be
        # printed: they cost as much as the whole solve (20 ms behind 25 ms of iterations at (32,500), tools/time_exit_checks.py)
        f = eng.exit_checks_fast(latent, psd_tol)
        a_om, a_th, a_l = f[:, 0].max(), f[:, 1].max(), f[:, 2].max()
        for name, dev in (("Omega", a_om), ("Theta", a_th), ("L", a_l)):
            if dev > 1e-5:
                warnings.warn(f"{name} variable is not symmetric, largest deviation is {dev}.")
        if f[:, 3].min() > 0 and f[:, 4].min() > 0:
            return
    a_om, a_th, a_l, min_tl, min_l = eng.exit_checks(latent)
    for name, dev in (("Omega", a_om), ("Theta", a_th), ("L", a_l)):
        if dev > 1e-5 and not hasattr(eng, "exit_checks_fast"):
            warnings.warn(f"{name} variable is not symmetric, largest deviation is {dev}.")
    if min_tl <= 0:
        extra = f" (min EV is {min_tl})" if verbose_min_ev else ""
        print("WARNING: Theta (Theta - L resp.) is not positive definite. Solve to higher accuracy!" + extra)
    if latent and min_l < -psd_tol:
        extra = f" (min EV is {min_l})" if verbose_min_ev else ""
        print("WARNING: L is not positive semidefinite. Solve to higher accuracy!" + extra)


def ADMM_MGL(S, lambda1, lambda2, reg, Omega_0, Theta_0=np.array([]), X_0=np.array([]), n_samples=None,
             tol=1e-5, rtol=1e-4, stopping_criterion='boyd', update_rho=True, rho=1., max_iter=1000,
             verbose=False, measure=False, latent=False, mu1=None):
    """Multiple Graphical Lasso by ADMM on the MI355X -- same arguments, defaults, asserts, status
    strings and return dicts as the reference's ``ADMM_MGL`` (solver/admm_solver.py:13-313).

    Returns ``(sol, info)`` with ``sol = {'Omega','Theta','L','X'}`` (each (K,p,p), X the scaled dual)
    and ``info = {'status'}`` (+ ``runtime``, ``residual``, ``objective`` when ``measure``)."""
    assert Omega_0.shape == S.shape
    assert S.shape[1] == S.shape[2]
    assert reg in ['GGL', 'FGL']
    assert min(lambda1, lambda2) > 0
    (K, p, p) = S.shape
    assert rho > 0, "ADMM penalization parameter must be positive."
    assert stopping_criterion in ('boyd', 'kkt')

    if latent:
        if isinstance(mu1, float):
            mu1 = mu1 * np.ones(K)
        assert mu1 is not None
        assert np.all(mu1 > 0)
        mu1 = as_c(mu1)
    else:
        mu1 = None

    # admm_solver.py:129-139: None -> ones, int -> same weight for every instance, else (K,) array
    if n_samples is None:
        nk = np.ones(K)
    elif isinstance(n_samples, (int, np.integer)):
        nk = float(n_samples) * np.ones(K)
    else:
        nk = as_c(n_samples).reshape(-1)
        assert len(nk) == K

    if len(Theta_0) == 0:
        Theta_0 = Omega_0
    if len(X_0) == 0:
        X_0 = np.zeros((K, p, p))

    eng = ENGINE(S, Omega_0, Theta_0, X_0)
    try:
        info, _ = _run_admm(eng, reg, K, p, float(lambda1), float(lambda2), bool(latent), mu1, nk, float(rho),
                            tol, rtol, stopping_criterion, update_rho, max_iter, verbose, measure, "Multiple",
                            want_objective=True)
        if latent:
            eng.finalize_L()        # the returned L: one eigendecomposition where the L-steps were sign iterations
        _exit_report(eng, latent, 1e-5, False)
        sol = eng.state()
    finally:
        eng.close()
    return sol, info


def ADMM_SGL(S, lambda1, Omega_0, Theta_0=np.array([]), X_0=np.array([]), rho=1., max_iter=1000, tol=1e-7,
             rtol=1e-4, stopping_criterion='boyd', update_rho=True, verbose=False, measure=False, latent=False,
             mu1=None, lambda1_mask=None):
    """Single Graphical Lasso by ADMM on the MI355X -- the reference's ``ADMM_SGL``
    (solver/single_admm_solver.py:15-275): same arguments, asserts and return contract (``sol`` has
    no 'L' unless ``latent``)."""
    assert Omega_0.shape == S.shape
    assert S.shape[0] == S.shape[1]
    (p, p) = S.shape
    assert lambda1 > 0, ("lambda1 should be positive, otherwise using Graphical Lasso is redundant. "
                         "Specify entries with zero regularization using lambda1_mask.")
    lam_pp = None
    if lambda1_mask is not None:
        assert lambda1_mask.shape == (p, p), f"lambda1_mask needs to be of shape (p,p), but is {lambda1_mask.shape}."
        assert np.all(lambda1_mask >= 0), "lambda1_mask needs to be non-negative."
        assert np.all(np.abs(lambda1_mask.T - lambda1_mask) <= 1e-5), "lambda1_mask needs to be symmetric."
        lam_pp = lambda1 * lambda1_mask           # single_admm_solver.py:114
    assert stopping_criterion in ["boyd", "kkt"]
    if latent:
        assert mu1 is not None
        assert mu1 > 0
    assert rho > 0, "ADMM penalization parameter must be positive."

    if len(Theta_0) == 0:
        Theta_0 = Omega_0
    if len(X_0) == 0:
        X_0 = np.zeros((p, p))

    eng = ENGINE(S[None], np.asarray(Omega_0)[None], np.asarray(Theta_0)[None], np.asarray(X_0)[None])
    try:
        eng.set_lambda1_mask(lam_pp)
        mu = as_c(np.array([mu1])) if latent else None
        info, _ = _run_admm(eng, 'SGL', 1, p, float(lambda1), 0.0, bool(latent), mu, np.ones(1), float(rho), tol,
                            rtol, stopping_criterion, update_rho, max_iter, verbose, measure, "Single")
        if latent:
            eng.finalize_L()
        _exit_report(eng, latent, 1e-8, True)
        st = eng.state()
    finally:
        eng.close()
    sol = {'Omega': st['Omega'][0], 'Theta': st['Theta'][0], 'X': st['X'][0]}
    if latent:
        sol['L'] = st['L'][0]
    return sol, info


def ADMM_FSGL(S, lambda1, M, Omega_0, Theta_0=np.array([]), X_0=np.array([]), rho=1., max_iter=1000, tol=1e-7,
              rtol=1e-4, update_rho=True, verbose=False, measure=False, latent=False, mu1=None):
    """(Latent variable) Functional Single Graphical Lasso by ADMM on the MI355X -- the reference's ``ADMM_FSGL``
    (solver/functional_sgl_admm.py:12-238): each of the p variables has an M-dimensional functional representation, S is
    (p*M,p*M), and the penalty is lambda1 * sum_{j != l} |Theta^M_jl|_F.  Same arguments, defaults, asserts, prints, exit
    warnings and return contract: ``sol = {'Omega','Theta','X'}`` (+ 'L' when ``latent``), ``info = {'status'}``
    (+ ``runtime``, ``residual`` with ``measure``).  The Omega-step is the SGL Omega-step at dimension p*M, the Theta-step
    prox_sum_Frob (solver/ggl_helper.py:45-66) as one HIP kernel with the dual update and the stopping-test sums."""
    assert Omega_0.shape == S.shape
    assert S.shape[0] == S.shape[1]
    assert lambda1 > 0
    if latent:
        assert mu1 is not None
        assert mu1 > 0
    (pM, pM) = S.shape
    assert pM % M == 0
    p = int(pM / M)
    if verbose:
        print(f"Derived a Functional SGL problem of dimensionality p={p}.")
    assert rho > 0, "ADMM penalization parameter must be positive."

    if len(Theta_0) == 0:
        Theta_0 = Omega_0
    if len(X_0) == 0:
        X_0 = np.zeros((pM, pM))

    eng = ENGINE(np.asarray(S)[None], np.asarray(Omega_0)[None], np.asarray(Theta_0)[None], np.asarray(X_0)[None])
    try:
        eng.set_block_size(int(M))
        mu = as_c(np.array([mu1])) if latent else None
        # (dim = (pM^2 + pM) / 2, functional_sgl_admm.py:248: the single-problem test at dimension pM)
        info, _ = _run_admm(eng, 'FSGL', 1, pM, float(lambda1), 0.0, bool(latent), mu, np.ones(1), float(rho), tol,
                            rtol, 'boyd', update_rho, max_iter, verbose, measure, "Functional Single", show_rho=True)
        if latent:
            eng.finalize_L()
        # functional_sgl_admm.py:207-226: warnings, not prints, with the eigenvalue in the message
        definite = False
        if hasattr(eng, "exit_checks_fast"):
            # the decisions by two Cholesky factorisations; the eigenvalues only for the text of a warning (as _exit_report)
            f = eng.exit_checks_fast(latent, 1e-8)
            a_om, a_th, a_l = f[:, 0].max(), f[:, 1].max(), f[:, 2].max()
            definite = f[:, 3].min() > 0 and f[:, 4].min() > 0
            min_tl, min_l = 1.0, 0.0
        if not definite:
            a_om, a_th, a_l, min_tl, min_l = eng.exit_checks(latent)
        for name, dev in (("Omega", a_om), ("Theta", a_th), ("L", a_l)):
            if dev > 1e-5:
                warnings.warn(f"{name} variable is not symmetric, largest deviation is {dev}.")
        if min_tl <= 0:
            warnings.warn(f"Theta (Theta - L resp.) is not positive definite. Solve to higher accuracy! (min EV is {min_tl})")
        if latent and min_l < -1e-8:
            warnings.warn(f"L is not positive semidefinite. Solve to higher accuracy! (min EV is {min_l})")
        st = eng.state()
    finally:
        eng.close()
    sol = {'Omega': st['Omega'][0], 'Theta': st['Theta'][0], 'X': st['X'][0]}
    if latent:
        sol['L'] = st['L'][0]
    return sol, info


def get_connected_components(S, lambda1):
    """Connected components of the graph |S_ij| > lambda1_ij with the diagonal kept
    (solver/single_admm_solver.py:478-490)."""
    from scipy.sparse.csgraph import connected_components
    A = (np.abs(S) > lambda1).astype(int)
    np.fill_diagonal(A, 1)
    numC, labels = connected_components(A, directed=False, return_labels=True)
    return numC, [np.flatnonzero(labels == i) for i in range(numC)]


# upper edges of the size classes whose connected components share one padded stack in block_SGL (ratio ~1.5: a component
# is padded by at most that factor; 128 was the LDS-Jacobi limit when the edges were chosen -- since round 4 every bucket above 8
# runs the matrix-function route, the edges only bound the padding)
BLOCK_BUCKETS = (4, 6, 9, 13, 19, 28, 42, 63, 94, 128, 192, 288, 432, 648, 972, 1458, 2187, 3281, 4922, 7383, 11075)


def block_bucket(size):
    for edge in BLOCK_BUCKETS:
        if size <= edge:
            return edge
    return int(size)


def block_SGL(S, lambda1, Omega_0, Theta_0=None, X_0=None, rho=1., max_iter=1000, tol=1e-7, rtol=1e-3,
              stopping_criterion="boyd", update_rho=True, verbose=False, measure=False, lambda1_mask=None):
    """The reference's ``block_SGL`` (solver/single_admm_solver.py:326-475; what ``glasso_problem.solve()``
    calls for non-latent SGL, problem.py:443-450): split S into the connected components of |S| > lambda1,
    solve singletons in closed form 1/S_ii and every larger block with ADMM, reassemble.  Returns ``sol`` only,
    like the reference.

    The graph split stays on the host (SciPy).  The components are solved TOGETHER on the GPU: every component is the
    leading block of an identity-padded slot of one stack (gglasso_amd.batch.ADMM_SGL_batch with ``dims``: each component
    keeps its own rho, residuals over its own block and stopping iteration, its own slice of ``lambda1_mask``, so the
    result equals the reference's component-by-component loop).  Components of very different size do not share a stack
    (padding a 5 x 5 block to 900 x 900 would cost more than it saves): sizes are bucketed geometrically (edges
    ``BLOCK_BUCKETS``, ratio 1.5), one batch per bucket.  With the KKT criterion or ``measure`` the components go through
    ``ADMM_SGL`` one by one exactly as in the reference."""
    from scipy.linalg import block_diag
    from .batch import ADMM_SGL_batch
    assert Omega_0.shape == S.shape
    assert S.shape[0] == S.shape[1]
    (p, p) = S.shape
    assert lambda1 > 0, ("lambda1 should be positive, otherwise using Graphical Lasso is redundant. "
                         "Specify entries with zero regularization using lambda1_mask.")
    has_mask = lambda1_mask is not None
    if has_mask:
        assert lambda1_mask.shape == (p, p), f"lambda1_mask needs to be of shape (p,p), but is {lambda1_mask.shape}."
        assert np.all(lambda1_mask >= 0), "lambda1_mask needs to be non-negative."
        assert np.all(np.abs(lambda1_mask.T - lambda1_mask) <= 1e-5), "lambda1_mask needs to be symmetric."
    else:
        lambda1_mask = np.ones((p, p))
    if Theta_0 is None:
        Theta_0 = Omega_0.copy()
    if X_0 is None:
        X_0 = np.zeros((p, p))

    numC, allC = get_connected_components(S, lambda1 * lambda1_mask)
    sols = [None] * numC
    by_bucket = {}
    for i, C in enumerate(allC):
        if len(C) == 1:
            v = 1 / S[C, C]                     # off-diagonal penalty: 1/S_ii, not 1/(S_ii + lambda1)
            sols[i] = (v, v, np.array([0]))
        else:
            by_bucket.setdefault(block_bucket(len(C)), []).append(i)

    batched = stopping_criterion == "boyd" and not measure
    for _, idx in sorted(by_bucket.items()):
        if batched:
            from .batch import pad_blocks
            ixs = [np.ix_(allC[i], allC[i]) for i in idx]
            dims = np.array([len(allC[i]) for i in idx])
            P = int(dims.max())
            res = ADMM_SGL_batch(pad_blocks([S[ix] for ix in ixs], P, True), lambda1,
                                 Omega_0=pad_blocks([Omega_0[ix] for ix in ixs], P, True),
                                 Theta_0=pad_blocks([Theta_0[ix] for ix in ixs], P, True),
                                 X_0=pad_blocks([X_0[ix] for ix in ixs], P, False), rho=rho, max_iter=max_iter, tol=tol,
                                 rtol=rtol, update_rho=update_rho, verbose=verbose, dims=dims,
                                 lambda1_mask=pad_blocks([lambda1_mask[ix] for ix in ixs], P, False) if has_mask else None)
            for i, (bs, binfo) in zip(idx, res):
                print(f"ADMM terminated after {binfo['iterations']} iterations with status: {binfo['status']}.")
                sols[i] = (bs['Omega'], bs['Theta'], bs['X'])
        else:
            for i in idx:
                ix = np.ix_(allC[i], allC[i])
                bs, _ = ADMM_SGL(S[ix], lambda1, Omega_0[ix], Theta_0=Theta_0[ix], X_0=X_0[ix], tol=tol, rtol=rtol,
                                 stopping_criterion=stopping_criterion, update_rho=update_rho, rho=rho,
                                 max_iter=max_iter, verbose=verbose, measure=measure, lambda1_mask=lambda1_mask[ix])
                sols[i] = (bs['Omega'], bs['Theta'], bs['X'])

    per = np.hstack(allC)
    inv = np.empty_like(per)
    inv[per] = np.arange(per.size)
    ixp = np.ix_(inv, inv)
    return {'Omega': block_diag(*[s[0] for s in sols])[ixp], 'Theta': block_diag(*[s[1] for s in sols])[ixp],
            'X': block_diag(*[s[2] for s in sols])[ixp]}
