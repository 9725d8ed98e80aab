"""``glasso_problem`` and ``GGLassoEstimator``: the front end a GGLasso user types (problem.py of fabian-sp/GGLasso), on
this package's solvers and batched model-selection drivers -- no reference package, no numba.

Public names, signatures, defaults, assertion messages and warnings are the reference class's; the
implementation is this package's own:

* ``solve()`` runs ``ADMM_SGL`` / ``block_SGL`` / ``ADMM_MGL`` / ``ext_ADMM_MGL`` of this package (the MI355X).
* ``model_selection()`` calls this package's ``single_grid_search`` / ``K_single_grid`` / ``grid_search``, so a grid is
  solved as batches (``ADMM_SGL_batch`` / ``ADMM_MGL_batch`` / ``ext_ADMM_MGL_batch``) instead of a sequential walk.
* ``do_scaling`` (covariances -> correlations, and Theta, L back) goes through the device kernel (``ggl_scale_by_diagonal``).
* ``glasso_problem.from_data(X, ...)`` starts from observations: S comes from ``utils.sample_covariance``, or with
  ``correlation='kendall'`` from ``utils.skeptic_correlation`` (rank based), with ``correlation='mixed'`` from
  ``utils.mixed_correlation`` (binary beside continuous variables).
* ``glasso_problem.from_time_series(X, at, bandwidth, ...)`` starts from ONE series with time stamps: S is the stack of
  kernel-smoothed covariances (``utils.kernel_covariance``), the input of the Fused Graphical Lasso for time-varying networks;
  ``from_time_series_cv(X, at, bandwidths, ...)`` chooses the bandwidth from the series first (``bandwidth_search``).
* ``edge_inference()`` tests the edges of the solution at hand and gives confidence intervals: the debiased graphical lasso
  (``utils.debiased_precision`` on the device, ``utils.edge_tests`` / ``utils.differential_tests`` on the host).
"""
import numbers
import warnings
from collections import namedtuple

import numpy as np

from . import ops, utils
from . import model_selection as _ms
from . import solver as _solver
from . import ext_solver as _ext

assert_tol = 1e-5

# What the input says about the problem.  kind: 'single' (one (p,p) matrix), 'stack' ((K,p,p), one dimension) or 'dict'
# (instances of different dimension, keys 0..K-1); p is an int, or the K dimensions for 'dict'.
_Formulation = namedtuple("_Formulation", "kind K p S N")

# messages of the shape / symmetry checks per kind of checked array
_INPUT_MESSAGES = {
    'single': ("Dimensions are not correct, 1st and 2nd dimension have to match but shape is {shape}. "
               "Specify covariance data in format(p,p)!", "Covariance data is not symmetric."),
    'stack': ("Dimensions are not correct, 2nd and 3rd dimension have to match but shape is {shape}. "
              "Specify covariance data in format(K,p,p)!", "Covariance data is not symmetric."),
    'dict': ("Dimensions are not correct, 1st and 2nd dimension have to match but do not match for instance {k}.",
             "Covariance data for instance {k} is not symmetric."),
}

# kind (and, for a single problem, latent) -> (module, solver, entries of reg_params it takes, attributes it takes)
_SOLVE_ROUTES = {
    ('single', False): (_solver, 'block_SGL', ('lambda1_mask',), ()),
    ('single', True): (_solver, 'ADMM_SGL', ('lambda1_mask', 'mu1'), ('latent',)),
    'stack': (_solver, 'ADMM_MGL', ('lambda2', 'mu1'), ('reg', 'latent')),
    'dict': (_ext, 'ext_ADMM_MGL', ('lambda2', 'mu1'), ('reg', 'latent', 'G')),
}

_SCALING_WARNINGS = (
    "NOTE: Input data S is rescaled to correlations, this has impact on the scale of the regularization parameters!",
    "The output/solution is rescaled to covariances. All model selection output, in particular the optimal regularization "
    "parameters in self.reg_params are corresponding to the correlations.",
)


def _is_number(x):
    return isinstance(x, numbers.Real)


def _per_instance(A, fn):
    """fn over the instances of a dict, or on the array itself."""
    return {k: fn(A[k]) for k in A} if isinstance(A, dict) else fn(A)


def _square_and_symmetric(A, kind, **where):
    not_square, not_symmetric = _INPUT_MESSAGES[kind]
    assert A.shape[-2] == A.shape[-1], not_square.format(shape=A.shape, **where)
    assert np.abs(A - np.swapaxes(A, -1, -2)).max() <= assert_tol, not_symmetric.format(**where)


def _formulate(S, N, G):
    """The ``_Formulation`` of the input (a copy of S, N per instance for multiple problems), or the reference's complaint."""
    if isinstance(S, np.ndarray):
        assert S.ndim in (2, 3), f"The specified covariance data has shape {S.shape}, GGLasso can only handle 2 or 3dim-input"
        kind = 'single' if S.ndim == 2 else 'stack'
        _square_and_symmetric(S, kind)
        K, p, S = (1 if kind == 'single' else S.shape[0]), S.shape[-1], S.copy()
        if kind == 'single':
            assert _is_number(N), "For SGL problems, N needs to be a single number, float or int."
    elif isinstance(S, (list, dict)):
        assert len(S) > 1, \
            "Covariance data is a list/dict with only one entry. This is a Single Graphical Lasso problem. Specify S as 2d-array."
        assert G is not None, \
            "For non-conforming dimensions, the input G has to be specified for bookeeping the overlapping variables."
        kind, K = 'dict', len(S)
        for k in range(K):
            _square_and_symmetric(S[k], kind, k=k)
        S = {k: np.array(S[k]) for k in range(K)}
        p = np.array([S[k].shape[0] for k in range(K)], dtype=int)
        _ext.check_G(G, p)
    else:
        raise TypeError(f"Incorrect input type of S. You input {type(S)}, but np.ndarray or list/dict is expected.")
    if kind != 'single' and _is_number(N):
        N = N * np.ones(K)
    assert np.all(np.asarray(N) > 0), "N must be positive."
    return _Formulation(kind, K, p, S, N)


def adjacency_matrix(S, t=1e-10):
    """|S| >= t off the diagonal as an int array, for a matrix or a stack (helper/basic_linalg.py:35)."""
    A = (np.abs(S) >= t).astype(int)
    i = np.arange(A.shape[-1])
    A[..., i, i] = 0
    return A


class glasso_problem:
    """A Graphical Lasso problem; the formulation is derived from the input (print the object to see it):

    * ``S`` a (p,p) array: Single Graphical Lasso (``multiple = False``).
    * ``S`` a (K,p,p) array: Group (``reg='GGL'``) or Fused (``reg='FGL'``) Graphical Lasso, ``conforming = True``.
    * ``S`` a list / dict of (p_k,p_k) arrays with the bookkeeping array ``G``: Group Graphical Lasso over instances of
      different dimension (``conforming = False``); S becomes a dict with keys 0..K-1.

    ``N``: the number of samples, one number or an array of length K.  ``reg_params``: dict with ``lambda1``, ``lambda2``,
    ``mu1`` (``latent=True``), ``lambda1_mask`` (single problems).  ``latent``: model Theta - L (sparse minus low rank).
    After ``solve()`` or ``model_selection()`` the estimates are in ``self.solution`` (a ``GGLassoEstimator``).

    ``do_scaling``: S is scaled to correlations before solving.  For a single matrix and for a list / dict the variances are
    kept in ``_scale`` and the solution is scaled back to the covariances' scale.  For a (K,p,p) stack the reference's
    ``_scale`` is all ones (it holds views of the stack it then scales in place), so its solution stays on the CORRELATIONS'
    scale whatever its second warning says; that observable behaviour is kept here, and the variances are in ``_variances``."""

    def __init__(self, S, N, reg="GGL", reg_params=None, latent=False, G=None, do_scaling=False):
        form = _formulate(S, N, G)
        self._kind = form.kind
        self.S, self.N, self.K, self.p = form.S, form.N, form.K, form.p
        self.multiple, self.conforming = form.kind != 'single', form.kind != 'dict'
        self.latent, self.G, self.do_scaling = latent, G, do_scaling
        self.reg = None
        if self.multiple:
            assert reg in ["GGL", "FGL"], \
                "Specify 'GGL' for Group Graphical Lasso or 'FGL' for Fused Graphical Lasso (or None for Single Graphical Lasso)"
            self.reg = reg
        self.reg_params = self._default_reg_params()
        self.set_reg_params(reg_params)
        self.modelselect_params = self._default_modelselect_params()
        # the estimator keeps the input on its own scale
        self.solution = GGLassoEstimator(S=self.S, N=self.N, p=self.p, K=self.K, multiple=self.multiple, latent=self.latent,
                                         conforming=self.conforming)
        if do_scaling:
            for text in _SCALING_WARNINGS:
                warnings.warn(text)
            self._to_correlations()

    @classmethod
    def from_data(cls, X, *, reg="GGL", reg_params=None, latent=False, G=None, do_scaling=False, center=True, correlation=None,
                  missing=None, min_pairs=2, project=False):
        """The problem of observations ``X``: (p,N), (K,p,N) or a list / dict of (p_k,N_k) arrays, variables in rows.
        ``N`` is read off the data and S is computed on the device (``utils.sample_covariance``).

        ``correlation='kendall'``: S is every instance's nonparanormal skeptic matrix ``sin(pi/2 tau-b)``
        (``utils.skeptic_correlation``: Kendall's tau-b on the int8 matrix cores) -- for data that are not Gaussian (counts,
        skewed or heavy-tailed measurements, ties).  It is a correlation matrix (unit diagonal; ``center`` has no meaning and
        must be left at its default) and it can be indefinite: the ADMM's log-det prox does not need a positive semidefinite
        input, so the matrix is used as it is and no projection is applied.  ``project=True`` (below) projects it.

        ``missing='pairwise'``: a NaN in X is a missing value and S is every instance's pairwise-complete covariance
        (``utils.sample_covariance(..., missing='pairwise', min_pairs=min_pairs)``); it can be indefinite as well and is used
        as it is.  ``N`` stays the number of columns of the data, whatever is missing; the numbers of samples every pair
        shares are kept in ``problem.pair_counts`` (of the kind of S).  Not with ``correlation='kendall'`` or ``'mixed'``.

        ``correlation='mixed'``: S is every instance's latent correlation matrix of mixed binary / continuous data
        (``utils.mixed_correlation``: a variable with exactly two distinct values is binary; Kendall's tau-a inverted through
        the bridge function of each pair's types) -- for presence / absence or yes / no variables beside continuous ones, where
        Pearson attenuates and the skeptic bridge is wrong.  ``center`` as with ``'kendall'``; the matrix can be indefinite and
        is used as it is.

        ``project=True``: S (every instance of a stack) is replaced by its nearest-correlation projection
        (``utils.nearest_correlation`` with its defaults: same diagonal, no eigenvalue of its correlation matrix below 1e-8),
        after any ``correlation=`` and ``missing=`` choice, Pearson included.  With an indefinite S the objective is unbounded
        below once lambda1 is small, which is where a regularisation path starts.  What the projection did is kept as
        ``problem.projection`` (the info dict; per instance for a list / dict of different dimensions), and
        ``stability_selection`` projects every subsample's matrix as well."""
        assert correlation in (None, 'kendall', 'mixed'), "correlation must be None (Pearson), 'kendall' or 'mixed'"
        assert missing in (None, 'pairwise'), "missing must be None (complete data) or 'pairwise'"
        if missing == 'pairwise' and correlation in ('kendall', 'mixed'):
            raise ValueError(f"missing='pairwise' with correlation='{correlation}': ranks of data with holes are not implemented")
        _, Xs = utils._data_list(X)
        N = np.array([x.shape[1] for x in Xs])
        counts = None
        if correlation == 'kendall':
            assert center is True, "correlation='kendall' has no use for center: leave it at its default"
            S = cls._skeptic(X)
        elif correlation == 'mixed':
            assert center is True, "correlation='mixed' has no use for center: leave it at its default"
            S = cls._mixed(X)
        elif missing == 'pairwise':
            S, counts = cls._pairwise(X, center, min_pairs)
        else:
            S = utils.sample_covariance(X, center=center)
        if isinstance(S, dict) and G is None and len({s.shape[0] for s in S.values()}) == 1:
            S = np.stack([S[k] for k in range(len(S))])       # a list of instances of ONE dimension is a conforming stack
            counts = None if counts is None else np.stack([counts[k] for k in range(len(counts))])
        projection = None
        if project:
            S, projection = cls._project(S)
        if isinstance(S, np.ndarray) and S.ndim == 2:
            N = int(N[0])
        prob = cls(S, N, reg=reg, reg_params=reg_params, latent=latent, G=G, do_scaling=do_scaling)
        prob._observations, prob._center = Xs, center       # kept for resampling (stability_selection)
        prob._correlation = correlation
        prob._missing, prob._min_pairs = missing, min_pairs
        prob.pair_counts = counts
        prob._project_S, prob.projection = bool(project), projection
        return prob

    @classmethod
    def from_time_series(cls, X, at, bandwidth, *, times=None, kernel='gaussian', cutoff=2.0 ** -53, reg='FGL', reg_params=None,
                         latent=False, do_scaling=False, center=True):
        """The time-varying problem of ONE series ``X`` (p,N), a column per observation with time stamps ``times`` (default
        ``0..N-1``): S is the stack of kernel-smoothed covariances at the K points ``at`` (an integer K, or an array of times)
        with bandwidth ``bandwidth`` (``utils.kernel_covariance``, computed on the device from one upload of X), and ``N`` the
        vector of Kish's effective sample sizes -- kernel smoothing followed by the Fused Graphical Lasso (Zhou, Lafferty,
        Wasserman 2010; Monti et al. 2014).  ``problem.weights`` (K,N) and ``problem.eval_times`` (K,) are kept.  K = 1 gives a
        Single Graphical Lasso problem.  The observations are not kept: ``stability_selection`` needs ``from_data``."""
        Xc = utils.as_c(X)
        assert Xc.ndim == 2 and Xc.shape[0] >= 1 and Xc.shape[1] >= 1, \
            f"data must be a (p,N) array with variables in rows, has shape {Xc.shape}"
        _, eval_times, w = utils._kernel_setup(Xc.shape[1], at, bandwidth, times, kernel, cutoff)
        if hasattr(_solver.ENGINE, "set_data_weighted"):
            S = utils.weighted_covariance(Xc, w, center=center)
        else:
            S = utils.host_weighted_covariance(Xc, w, center)
        n_eff = utils.effective_sample_size(w)
        if S.shape[0] == 1:
            S, n_eff = S[0], float(n_eff[0])
        prob = cls(S, n_eff, reg=reg, reg_params=reg_params, latent=latent, do_scaling=do_scaling)
        prob.weights, prob.eval_times = w, eval_times
        return prob

    @classmethod
    def from_time_series_cv(cls, X, at, bandwidths, *, rule='min', ridge=0.0, eval_index=None, times=None, kernel='gaussian',
                            cutoff=2.0 ** -53, reg='FGL', reg_params=None, latent=False, do_scaling=False, center=True):
        """``from_time_series`` with the bandwidth chosen from the series: ``model_selection.bandwidth_search(X, bandwidths,
        rule, ...)`` scores the grid by the leave-one-out Gaussian predictive likelihood (``rule``: ``'min'`` or ``'one_se'``;
        ``ridge``, ``eval_index`` as there; ``times``, ``kernel``, ``cutoff``, ``center`` are shared by the search and the
        stack), then the problem is built with the chosen bandwidth.  ``problem.bandwidth_`` is that bandwidth and
        ``problem.bandwidth_stats`` the statistics of the search."""
        h, stats = _ms.bandwidth_search(X, bandwidths, rule=rule, times=times, kernel=kernel, cutoff=cutoff, center=center,
                                        ridge=ridge, eval_index=eval_index)
        prob = cls.from_time_series(X, at, h, times=times, kernel=kernel, cutoff=cutoff, reg=reg, reg_params=reg_params,
                                    latent=latent, do_scaling=do_scaling, center=center)
        prob.bandwidth_, prob.bandwidth_stats = h, stats
        return prob

    @staticmethod
    def _project(S):
        """(projected S, info) of a matrix, a stack or a dict of matrices; an engine without the device route (``project_S``)
        takes the numpy twin."""
        fn = utils.nearest_correlation if hasattr(_solver.ENGINE, "project_S") else utils.host_nearest_correlation
        if isinstance(S, dict):
            out = {k: fn(S[k], return_info=True) for k in range(len(S))}
            return {k: o for k, (o, _) in out.items()}, {k: i for k, (_, i) in out.items()}
        return fn(S, return_info=True)

    @staticmethod
    def _pairwise(X, center, min_pairs):
        """(S, counts) of the pairwise-complete covariance, of the kind ``utils.sample_covariance`` returns; an engine without
        the device route (``set_data_subsets``) takes the numpy products and refuses what the library refuses."""
        if hasattr(_solver.ENGINE, "set_data_subsets"):
            return utils.sample_covariance(X, center=center, missing='pairwise', min_pairs=min_pairs, return_counts=True)
        kind, Xs = utils._data_list(X)
        out = [utils.host_pairwise_covariance(x, center) for x in Xs]
        assert int(min_pairs) >= 1 and all(c.min() >= int(min_pairs) for _, c in out), \
            f"a pair of variables shares fewer than min_pairs = {min_pairs} samples"
        S, C = [s for s, _ in out], [c for _, c in out]
        if kind == "2d":
            return S[0], C[0]
        return (np.stack(S), np.stack(C)) if kind == "3d" else (dict(enumerate(S)), dict(enumerate(C)))

    @staticmethod
    def _skeptic(X):
        """The skeptic matrices of the observations, of the kind ``utils.sample_covariance`` returns; an engine without the
        device route (``set_kendall_subsets``) takes the numpy brute force."""
        if hasattr(_solver.ENGINE, "set_kendall_subsets"):
            return utils.skeptic_correlation(X)
        kind, Xs = utils._data_list(X)
        S = [utils.host_skeptic_correlation(x) for x in Xs]
        return S[0] if kind == "2d" else (np.stack(S) if kind == "3d" else dict(enumerate(S)))

    @staticmethod
    def _mixed(X):
        """The latent correlation matrices of mixed data, of the kind ``utils.sample_covariance`` returns; an engine without
        the device route (``set_mixed_subsets``) takes the numpy twin."""
        if hasattr(_solver.ENGINE, "set_mixed_subsets"):
            return utils.mixed_correlation(X)
        kind, Xs = utils._data_list(X)
        S = [utils.host_mixed_correlation(x) for x in Xs]
        return S[0] if kind == "2d" else (np.stack(S) if kind == "3d" else dict(enumerate(S)))

    def __repr__(self):
        name = {None: "SINGLE", "GGL": "GROUP", "FGL": "FUSED"}[self.reg]
        tail = "WITH LATENT VARIABLES" if self.latent else ""
        return f" \n{name} GRAPHICAL LASSO PROBLEM {tail}\nRegularization parameters:\n{self.reg_params}"

    # -- scaling (device kernel) -----------------------------------------------------------------------------------------
    def _to_correlations(self):
        if self._kind == 'dict':
            scaled = [ops._scale_by_diagonal(self.S[k]) for k in range(self.K)]
            self.S = {k: c for k, (c, _) in enumerate(scaled)}
            self._scale = [d for _, d in scaled]
            return
        self.S, d = ops._scale_by_diagonal(self.S)
        if self._kind == 'single':
            self._scale = d
        else:                                                   # see the class docstring
            self._variances = list(d)
            self._scale = [np.ones(self.p) for _ in range(self.K)]

    def _from_correlations(self, X):
        """An estimate of an inverse covariance goes back to the covariances' scale by the same division, X_ij /
        sqrt(scale_i scale_j); nothing to do where the scale is one."""
        if self._kind == 'stack':
            return X
        if self._kind == 'single':
            return ops.scale_array_by_diagonal(X, d=self._scale)
        return {k: ops.scale_array_by_diagonal(X[k], d=self._scale[k]) for k in range(self.K)}

    # -- defaults ----------------------------------------------------------------------------------------------------------
    def _default_reg_params(self):
        return dict.fromkeys(('lambda1', 'lambda2', 'mu1') if self.multiple else ('lambda1', 'mu1'))

    def _default_start_point(self):
        if self._kind == 'dict':
            return {k: np.eye(self.p[k]) for k in range(self.K)}
        return np.eye(self.p) if self._kind == 'single' else np.tile(np.eye(self.p), (self.K, 1, 1))

    def _default_solver_params(self):
        params = dict(verbose=False, measure=False, rho=1., max_iter=1000, update_rho=True)
        if self._kind == 'dict':
            del params['update_rho']                          # ext_ADMM_MGL has no such argument
        return params

    def _default_modelselect_params(self):
        grid = [('lambda1_range', np.logspace(0, -3, 10))]
        if self.multiple:
            grid.append(('lambda2_range', np.logspace(-1, -4, 5)))
        grid.append(('mu1_range', np.logspace(2, -1, 10) if self.latent else None))
        if not self.multiple:
            grid.append(('lambda1_mask', None))
        return dict(grid)

    def set_reg_params(self, reg_params=None):
        """Set or update (a subset of) ``lambda1``, ``lambda2``, ``mu1``, ``lambda1_mask``; other entries are kept."""
        assert reg_params is None or type(reg_params) == dict
        self.reg_params.update(reg_params or {})

    def set_start_point(self, Omega_0=None):
        """Start point of the solver, of the same kind as S; default the identity."""
        self.Omega_0 = self._default_start_point() if Omega_0 is None else Omega_0.copy()

    def set_modelselect_params(self, modelselect_params=None):
        """Set or update (a subset of) ``lambda1_range``, ``lambda2_range``, ``mu1_range``, ``lambda1_mask``."""
        if modelselect_params is None:
            warnings.warn("No grid for model selection is specified and thus default (or previous) values are used. A grid can be specified with the argument modelselect_params.")
            return
        assert isinstance(modelselect_params, dict)
        self.modelselect_params.update(modelselect_params)

    # -- solving -----------------------------------------------------------------------------------------------------------
    def solve(self, Omega_0=None, solver_params=dict(), tol=1e-8, rtol=1e-7, solver='admm', verbose=False):
        """Solve at ``self.reg_params``; the estimates go to ``self.solution``, the solver's info to ``self.solver_info``."""
        assert solver in ["admm"], "Currently only the ADMM solver is supported as it is implemented for all cases."
        assert self.reg_params.get('lambda1') is not None, \
            "Regularization parameters need to be set first (at least lambda1), see function glasso_problem.set_reg_params()"
        self.set_start_point(Omega_0)
        self.tol, self.rtol = tol, rtol
        self.solver_params = {**self._default_solver_params(), **solver_params, 'verbose': verbose}

        module, name, from_reg, from_self = _SOLVE_ROUTES[(self._kind, bool(self.latent)) if self._kind == 'single' else self._kind]
        kw = dict(S=self.S, lambda1=self.reg_params['lambda1'], Omega_0=self.Omega_0, tol=self.tol, rtol=self.rtol)
        kw.update({key: self.reg_params.get(key) for key in from_reg})
        kw.update({key: getattr(self, key) for key in from_self})
        if name == 'block_SGL':
            kw['rtol'] = self.tol       # the reference hands block_SGL its absolute tolerance as the relative one (problem.py:447)
        out = getattr(module, name)(**kw, **self.solver_params)
        sol, info = out if isinstance(out, tuple) else (out, {})        # block_SGL returns no info
        self._keep(sol)
        self.solver_info = dict(info)

    def _keep(self, sol):
        """A solver's result, on the input's scale, into ``self.solution``."""
        Theta, L = sol['Theta'], (sol['L'] if self.latent else None)
        if self.do_scaling:
            Theta, L = self._from_correlations(Theta), (None if L is None else self._from_correlations(L))
        self.solution._set_solution(Theta=Theta, L=L)

    # -- model selection ---------------------------------------------------------------------------------------------------
    def model_selection(self, modelselect_params=None, method='eBIC', gamma=0.1, tol=1e-7, rtol=1e-7, store_all=False):
        """Pick the regularization parameters on a grid by eBIC or AIC; every grid is solved as batches on the device.

        * single problem: the ``lambda1`` path, or the ``(lambda1, mu1)`` grid if ``latent``;
        * multiple, not latent: the ``(lambda1, lambda2)`` grid;
        * multiple, latent: first the ``(lambda1, mu1)`` grid of every instance on its own, then the ``(lambda1, lambda2)``
          grid with, per ``lambda1`` and instance, the ``mu1`` that stage one preferred.

        ``self.reg_params`` is set to the best point, the tables are in ``self.modelselect_stats``."""
        assert (gamma >= 0) and (gamma <= 1), "gamma needs to be chosen as a parameter in [0,1]."
        assert method in ['eBIC', 'AIC'], "Supported evaluation methods are eBIC and AIC."
        self.set_modelselect_params(modelselect_params)
        lambda1_range = self.modelselect_params['lambda1_range']
        if np.any(np.diff(lambda1_range) > 0):
            warnings.warn("Ideally the lambda1 range is sorted in descending order, so the grid search is performed from sparse to dense.")
        if store_all:
            warnings.warn("Setting store_all=True might cause memory issues as the solution is stored at all grid points.")
        if self.do_scaling and np.max(lambda1_range) > 1:
            warnings.warn("Using do_scaling=True, you can restrict the range for lambda1 to 1. Larger lambdas will result in the zero solution.")
        criterion = dict(method=method, gamma=gamma, tol=tol, rtol=rtol)
        select = self._select_multiple if self.multiple else self._select_single
        sol, stats = select(criterion, store_all)
        self._keep(sol)
        self.modelselect_stats = dict(stats)

    def stability_selection(self, modelselect_params=None, n_subsamples=20, subsample_size=None, beta=0.05, seed=0, tol=1e-7,
                            rtol=1e-7, store_all=False):
        """Pick ``lambda1`` of a Single Graphical Lasso problem built by ``from_data`` by StARS (stability across
        subsamples of the observations, ``model_selection.stars_search``) over ``modelselect_params['lambda1_range']``.
        ``self.reg_params['lambda1']`` is set to the choice, the estimate on all observations goes to ``self.solution`` and
        the instabilities to ``self.modelselect_stats``.  With ``do_scaling`` every subsample is scaled to its own
        correlations and the solution goes back to the covariances' scale, as in ``solve``.  A problem built with
        ``correlation='kendall'`` or ``'mixed'`` resamples that matrix instead (``do_scaling`` has nothing to scale then); one built
        with ``missing='pairwise'`` takes every subsample's, and the final fit's, pairwise-complete covariance; one built with
        ``project=True`` projects each of them (``stars_search(..., project=True)``)."""
        assert getattr(self, '_observations', None) is not None, \
            "Stability selection resamples the observations: build the problem with glasso_problem.from_data(X)."
        assert not self.multiple, "Stability selection is implemented for Single Graphical Lasso problems only."
        assert not self.latent, "Stability selection is not implemented for problems with latent variables."
        self.set_modelselect_params(modelselect_params)
        assert self.modelselect_params.get('lambda1_mask') is None and self.reg_params.get('lambda1_mask') is None, \
            "Stability selection is not implemented with a lambda1_mask."
        how = dict(correlation=self._correlation) if getattr(self, '_correlation', None) in ('kendall', 'mixed') else \
            dict(center=self._center, scale=bool(self.do_scaling))
        if getattr(self, '_missing', None) == 'pairwise':
            how.update(missing='pairwise', min_pairs=self._min_pairs)
        if getattr(self, '_project_S', False):
            how.update(project=True)
        sol, stats = _ms.stars_search(self._observations[0], self.modelselect_params['lambda1_range'],
                                      n_subsamples=n_subsamples, subsample_size=subsample_size, beta=beta, seed=seed,
                                      tol=tol, rtol=rtol, store_all=store_all, **how)
        self.set_reg_params(stats['BEST'])
        self._keep(sol)
        self.modelselect_stats = dict(stats)

    def cross_validation(self, modelselect_params=None, n_folds=5, seed=0, rule='min', tol=1e-7, rtol=1e-7, store_all=False):
        """Pick ``lambda1`` of a Single Graphical Lasso problem built by ``from_data`` by K-fold cross-validation of the
        held-out Gaussian likelihood (``model_selection.cv_search``) over ``modelselect_params['lambda1_range']``;
        ``rule``: 'min' or 'one_se'.  ``self.reg_params['lambda1']`` is set to the choice, the estimate on all observations goes
        to ``self.solution`` and the scores to ``self.modelselect_stats``.  With ``do_scaling`` every variable is scaled once, by
        its standard deviation over all observations, and the solution goes back to the covariances' scale, as in ``solve``.
        A problem built with ``correlation=``, ``missing=`` or ``project=True`` is refused: a held-out Gaussian likelihood
        against such a matrix is a different estimator."""
        assert getattr(self, '_observations', None) is not None, \
            "Cross-validation splits the observations: build the problem with glasso_problem.from_data(X)."
        assert not self.multiple, "Cross-validation is implemented for Single Graphical Lasso problems only."
        assert not self.latent, "Cross-validation is not implemented for problems with latent variables."
        self.set_modelselect_params(modelselect_params)
        assert self.modelselect_params.get('lambda1_mask') is None and self.reg_params.get('lambda1_mask') is None, \
            "Cross-validation is not implemented with a lambda1_mask."
        if getattr(self, '_correlation', None) is not None:
            raise ValueError(f"Cross-validation is not implemented for a problem built with correlation={self._correlation!r}.")
        if getattr(self, '_missing', None) is not None:
            raise ValueError(f"Cross-validation is not implemented for a problem built with missing={self._missing!r}.")
        if getattr(self, '_project_S', False):
            raise ValueError("Cross-validation is not implemented for a problem built with project=True.")
        sol, stats = _ms.cv_search(self._observations[0], self.modelselect_params['lambda1_range'], n_folds=n_folds, seed=seed,
                                   rule=rule, center=self._center, scale=bool(self.do_scaling), tol=tol, rtol=rtol,
                                   store_all=store_all)
        self.set_reg_params(stats['BEST'])
        self._keep(sol)
        self.modelselect_stats = dict(stats)

    def neighborhood_selection(self, lambda_range=None, select='stars', rule='and', refit=True, weights=None, **kw):
        """Meinshausen-Buhlmann neighbourhood selection for a Single Graphical Lasso problem built by ``from_data``: the
        penalty is chosen along ``lambda_range`` by StARS (``select='stars'``, ``model_selection.stars_search(method='mb')``) or
        by cross-validated prediction error (``select='cv'``, ``model_selection.cv_search(method='mb')``); ``rule`` (``'and'`` /
        ``'or'``) symmetrises the supports into the graph; ``kw`` goes to the search (``n_subsamples``, ``beta``, ``n_folds``,
        ``score``, ``seed``, ``tol``, ...; the ``rule`` of ``cv_search``, 'min' / 'one_se', as ``cv_rule``).  With ``refit`` (the
        default) every node is then regressed on its neighbours by least squares (``utils.neighborhood_refit``), and
        ``solution.precision_`` is ``utils.neighborhood_precision`` of those regressions; without it, of the lasso's own
        coefficients.  ``solution.adjacency_`` is the selected graph, ``reg_params['lambda1']`` the chosen penalty,
        ``modelselect_stats`` the search's tables and ``neighborhood_`` the search's ``sol``.  The precision matrix is not
        positive definite by construction (``utils.neighborhood_precision``).  ``solve``, ``model_selection`` and the other
        methods are untouched.  With ``do_scaling`` the method works on correlations and the precision matrix goes back to the
        covariances' scale, as in ``solve``.  ``select='cv'`` refuses what ``cross_validation`` refuses.

        ``weights`` ((p,p): row j holds node j's penalty weights, ``utils.adaptive_weights``) goes to the search and its final
        fit.  ``select='scaled'``: no grid and no search -- the scaled lasso (``utils.scaled_lasso_precision``) on the
        problem's matrix at ONE penalty, ``lambda0=`` in ``kw`` or the universal ``sqrt(2 log(p) / N)``, with the weights
        ``'sd'`` unless given.  ``solution.precision_`` is its precision matrix (``rule='and'``: of the two regressions' entries
        the smaller, ``'or'``: their average), ``adjacency_`` its off-diagonal pattern, ``modelselect_stats`` holds ``LAMBDA0``,
        ``SIGMA`` (the noise levels), ``STATUS``, ``SWEEPS`` and ``OUTER``; ``refit`` is not used.  ``kw``: ``tol``,
        ``sig_tol``, ``max_outer``, ``device``.  The same refusals."""
        from . import utils as _utils
        assert select in ('stars', 'cv', 'scaled'), f"select = {select!r}: 'stars', 'cv' or 'scaled'"
        assert rule in ('and', 'or'), f"rule = {rule!r}: 'and' or 'or'"
        assert select == 'scaled' or lambda_range is not None, f"select = {select!r} searches along lambda_range: give one"
        if weights is not None and select != 'scaled':
            kw = dict(kw, weights=weights)
        assert getattr(self, '_observations', None) is not None, \
            "Neighbourhood selection resamples the observations: build the problem with glasso_problem.from_data(X)."
        assert not self.multiple, "Neighbourhood selection is implemented for Single Graphical Lasso problems only."
        assert not self.latent, "Neighbourhood selection is not implemented for problems with latent variables: a lasso per " \
                                "node has no low-rank component."
        assert self.reg_params.get('lambda1_mask') is None, "Neighbourhood selection is not implemented with a lambda1_mask."
        X = self._observations[0]
        if select == 'scaled':
            assert lambda_range is None, "select='scaled' searches nothing: the penalty is lambda0= (default: sqrt(2 log(p) / N))"
            host = not hasattr(_solver.ENGINE, "neighborhood_stability")
            Theta, info = _utils.scaled_lasso_precision(self.S, n=self.N, weights='sd' if weights is None else weights,
                                                        rule={'and': 'min', 'or': 'average'}[rule], host=host, **kw)
            self.set_reg_params({'lambda1': info['LAMBDA0']})
            self._keep({'Theta': Theta})
            with np.errstate(invalid='ignore'):
                self.solution.adjacency_ = ((Theta != 0) & ~np.eye(self.p, dtype=bool)).astype(int)
            self.neighborhood_ = {'coef': info['COEF'], 'resvar': info['RESVAR'], 'lambda1': info['LAMBDA0'],
                                  'adjacency': self.solution.adjacency_.astype(bool), 'precision': Theta}
            self.modelselect_stats = {'select': 'scaled', 'LAMBDA0': info['LAMBDA0'], 'SIGMA': info['SIGMA'],
                                      'STATUS': info['STATUS'], 'SWEEPS': info['SWEEPS'], 'OUTER': info['OUTER']}
            return
        if select == 'stars':
            how = dict(correlation=self._correlation) if getattr(self, '_correlation', None) in ('kendall', 'mixed') else \
                dict(center=self._center, scale=bool(self.do_scaling))
            if getattr(self, '_missing', None) == 'pairwise':
                how.update(missing='pairwise', min_pairs=self._min_pairs)
            if getattr(self, '_project_S', False):
                how.update(project=True)
            sol, stats = _ms.stars_search(X, lambda_range, method='mb', rule=rule, refit=bool(refit), **how, **kw)
        else:
            for name, val in (('correlation', getattr(self, '_correlation', None)), ('missing', getattr(self, '_missing', None))):
                if val is not None:
                    raise ValueError(f"Neighbourhood selection by cross-validation is not implemented for a problem built with {name}={val!r}.")
            if getattr(self, '_project_S', False):
                raise ValueError("Neighbourhood selection by cross-validation is not implemented for a problem built with project=True.")
            kw = dict(kw)
            if 'cv_rule' in kw:
                kw['rule'] = kw.pop('cv_rule')
            sol, stats = _ms.cv_search(X, lambda_range, method='mb', graph_rule=rule, refit=bool(refit), center=self._center,
                                       scale=bool(self.do_scaling), **kw)
        Theta = sol['precision'] if 'precision' in sol else _utils.neighborhood_precision(sol['coef'], sol['resvar'])[0]
        self.set_reg_params(stats['BEST'])
        self._keep({'Theta': Theta})
        self.solution.adjacency_ = np.asarray(sol['adjacency']).astype(int)
        self.neighborhood_ = dict(sol)
        self.modelselect_stats = dict(stats)

    def joint_neighborhood_selection(self, lambda1_range, lambda2_range, rule='and', method='eBIC', gamma=0.1, **kw):
        """Joint neighbourhood selection for a multiple, conforming problem with ``reg='GGL'``: the regression counterpart of
        the Group Graphical Lasso (``utils.joint_neighborhood_selection``: every node's K regressions coupled by a group penalty
        ``lambda2`` across the instances beside the lasso penalty ``lambda1``), the pair chosen on the grid by the extended BIC of
        the refitted regressions (``model_selection.joint_neighborhood_search``; ``method``: 'eBIC', 'BIC', 'AIC').  It works on
        ``self.S`` (the correlations under ``do_scaling``; the precision goes back as in ``solve``) with ``self.N``; ``kw``:
        ``instance_weights``, ``tol``, ``max_sweeps``, ``t``, ``device``, ``host``.  ``solution.precision_`` is the (K,p,p)
        regression-based precision of the refit (not positive definite by construction, ``utils.neighborhood_precision``),
        ``solution.adjacency_`` the K selected graphs, ``reg_params`` gets ``lambda1`` and ``lambda2``, ``modelselect_stats``
        the search's tables and ``neighborhood_`` the search's ``sol``.  ``neighborhood_selection``, ``solve`` and
        ``model_selection`` are untouched."""
        assert rule in ('and', 'or'), f"rule = {rule!r}: 'and' or 'or'"
        assert self.multiple, "Joint neighbourhood selection couples the instances of a multiple problem; this is a single one " \
                              "(see neighborhood_selection)."
        assert self.conforming, "Joint neighbourhood selection is not implemented for instances of different dimension " \
                                "(non-conforming problems)."
        assert not self.latent, "Joint neighbourhood selection is not implemented for problems with latent variables: a lasso " \
                                "per node has no low-rank component."
        assert self.reg_params.get('lambda1_mask') is None, "Joint neighbourhood selection is not implemented with a lambda1_mask."
        assert self.reg == 'GGL', "Joint neighbourhood selection is implemented for reg='GGL' only: the fused penalty of " \
                                  "reg='FGL' has no such block update (see fused_neighborhood_selection)."
        sol, stats = _ms.joint_neighborhood_search(self.S, self.N, lambda1_range, lambda2_range, rule=rule, method=method,
                                                   gamma=gamma, **kw)
        self._store_neighborhood_search(sol, stats)

    def _store_neighborhood_search(self, sol, stats):
        self.set_reg_params(stats['BEST'])
        self._keep({'Theta': sol['precision']})
        self.solution.adjacency_ = np.asarray(sol['adjacency']).astype(int)
        self.neighborhood_ = dict(sol)
        self.modelselect_stats = dict(stats)

    def fused_neighborhood_selection(self, lambda1_range, lambda2_range, rule='and', method='eBIC', gamma=0.1, **kw):
        """Fused joint neighbourhood selection for a multiple, conforming problem with ``reg='FGL'``: the regression
        counterpart of the Fused Graphical Lasso (``utils.fused_neighborhood_selection``: every node's K regressions coupled
        along the instances' order by ``lambda2 sum_k |beta^(k+1) - beta^(k)|`` beside the lasso penalty ``lambda1``), the pair
        chosen by ``model_selection.fused_neighborhood_search``.  Arguments, ``kw`` and what is stored as for
        ``joint_neighborhood_selection``; ``neighborhood_['changed_edges']`` counts the edges that differ between consecutive
        graphs.  For a time series::

            glasso_problem.from_time_series(X, at, h).fused_neighborhood_selection(l1, l2)
        """
        assert rule in ('and', 'or'), f"rule = {rule!r}: 'and' or 'or'"
        assert self.multiple, "Fused neighbourhood selection couples the instances of a multiple problem; this is a single one " \
                              "(see neighborhood_selection)."
        assert self.conforming, "Fused neighbourhood selection is not implemented for instances of different dimension " \
                                "(non-conforming problems)."
        assert not self.latent, "Fused neighbourhood selection is not implemented for problems with latent variables: a lasso " \
                                "per node has no low-rank component."
        assert self.reg_params.get('lambda1_mask') is None, "Fused neighbourhood selection is not implemented with a lambda1_mask."
        assert self.reg == 'FGL', f"Fused neighbourhood selection is implemented for reg='FGL' only, this problem has " \
                                  f"reg={self.reg!r}" + (" (see joint_neighborhood_selection)." if self.reg == 'GGL' else ".")
        sol, stats = _ms.fused_neighborhood_search(self.S, self.N, lambda1_range, lambda2_range, rule=rule, method=method,
                                                   gamma=gamma, **kw)
        self._store_neighborhood_search(sol, stats)

    # -- inference ---------------------------------------------------------------------------------------------------------
    def edge_inference(self, alpha=0.05, method='bh', differential=None, host=False):
        """Edge-wise tests and confidence intervals for the solution at hand by the debiased graphical lasso (Jankova & van de
        Geer 2015): ``utils.debiased_precision`` of ``solution.precision_`` against the covariance it was fitted to with
        ``self.N`` (on the device; ``host=True``: the numpy twin), then ``utils.edge_tests``.  Stored on ``self.solution``:
        ``debiased_precision_``, ``standard_error_``, ``zscore_``, ``pvalue_``, ``pvalue_adj_`` (``method``: 'bh', 'bonferroni',
        'none', over the off-diagonal pairs of every instance), ``confidence_interval_`` (low, high; level ``1 - alpha`` per
        entry) and ``significant_``, the adjacency of the edges rejected at level ``alpha``.

        Everything is on the scale of ``precision_``.  The z-scores, and with them the p-values and ``significant_``, do not
        depend on ``do_scaling``: with Theta' = D Theta D and S' = D^-1 S D^-1 the debiased estimate is D T D and the standard
        error d_i d_j SE_ij.  (For a (K,p,p) stack ``do_scaling`` leaves the solution on the correlations' scale, see the
        class docstring; the correlations are then what it is debiased against.)

        ``differential``: for multiple problems, also test which entries differ between instances
        (``utils.differential_tests``; the instances' samples must be independent): 'consecutive' (the pairs (k, k + 1), the
        change points of an FGL stack), 'all', or a list of pairs.  ``solution.differential_`` gets one dict per pair.

        Refused with a ValueError: ``latent=True`` (Theta is then not the precision matrix of the observed variables),
        instances of different dimension, and a problem built with ``correlation=``, ``missing=`` or ``project=True`` (the
        variance is that of the Gaussian sample covariance)."""
        assert self.solution.precision_ is not None, \
            "Edge inference needs a solution: call solve(), model_selection(), stability_selection() or cross_validation() first."
        if self.latent:
            raise ValueError("Edge inference is not implemented for problems with latent variables: Theta is then not the "
                             "precision matrix of the observed variables.")
        if not self.conforming:
            raise ValueError("Edge inference is not implemented for instances of different dimension (non-conforming problems).")
        if getattr(self, '_correlation', None) is not None:
            raise ValueError(f"Edge inference is not implemented for a problem built with correlation={self._correlation!r}: "
                             "the variance formula is that of the Gaussian sample covariance.")
        if getattr(self, '_missing', None) is not None:
            raise ValueError(f"Edge inference is not implemented for a problem built with missing={self._missing!r}: "
                             "the variance formula is that of the Gaussian sample covariance.")
        if getattr(self, '_project_S', False):
            raise ValueError("Edge inference is not implemented for a problem built with project=True: "
                             "the variance formula is that of the Gaussian sample covariance.")
        if differential is not None and not self.multiple:
            raise ValueError("differential tests compare the instances of a multiple problem; this is a single one.")
        if isinstance(differential, str) and differential not in ('consecutive', 'all'):
            raise ValueError(f"differential must be None, 'consecutive', 'all' or a list of pairs, is {differential!r}")
        sol = self.solution
        S = self.S if (self.do_scaling and self._kind == 'stack') else sol.sample_covariance_
        debias = utils.host_debiased_precision if host else utils.debiased_precision
        T, SE = debias(sol.precision_, S, self.N)
        tests = utils.edge_tests(T, SE, alpha=alpha, method=method)
        sol.debiased_precision_, sol.standard_error_ = T, SE
        sol.zscore_, sol.pvalue_, sol.pvalue_adj_ = tests['z'], tests['pvalue'], tests['pvalue_adj']
        sol.confidence_interval_ = (tests['ci_low'], tests['ci_high'])
        sol.significant_ = tests['reject'].astype(int)
        sol.differential_ = None
        if differential is not None:
            pairs = differential
            if isinstance(differential, str):
                pairs = None if differential == 'consecutive' else [(a, b) for a in range(self.K) for b in range(a + 1, self.K)]
            sol.differential_ = utils.differential_tests(T, SE, pairs=pairs, alpha=alpha, method=method)

    def _select_single(self, criterion, store_all):
        grid = self.modelselect_params
        sol, Thetas, Ls, stats = _ms.single_grid_search(
            S=self.S, lambda_range=grid['lambda1_range'], N=self.N, latent=self.latent, mu_range=grid['mu1_range'],
            use_block=True, store_all=store_all, lambda1_mask=grid['lambda1_mask'], **criterion)
        self._grid_estimates = {'Theta': Thetas, 'L': Ls}       # every grid point's, with store_all
        self.set_reg_params(stats['BEST'])
        return sol, stats

    def _select_multiple(self, criterion, store_all):
        grid = self.modelselect_params
        mu_choice = None
        if self.latent:
            # stage one: every instance alone over (lambda1, mu1); its ix_mu (K, len(lambda1_range)) is the mu1 each instance
            # prefers at each lambda1
            uniform, individual, stage1 = _ms.K_single_grid(
                S=self.S, lambda_range=grid['lambda1_range'], N=self.N, latent=True, mu_range=grid['mu1_range'],
                use_block=True, store_all=store_all, **criterion)
            self._stage1 = {'uniform': uniform, 'individual': individual, 'stats': stage1}
            mu_choice = stage1['ix_mu']
        stats, best, sol = _ms.grid_search(
            _solver.ADMM_MGL if self.conforming else _ext.ext_ADMM_MGL, S=self.S, N=self.N, p=self.p, reg=self.reg,
            l1=grid['lambda1_range'], l2=grid['lambda2_range'], w2=None, G=self.G, latent=self.latent,
            mu_range=grid['mu1_range'], ix_mu=mu_choice, verbose=False, **criterion)
        self.set_reg_params(stats['BEST'])
        if self.latent:
            # best is (lambda2 index, lambda1 index): the lambda1 column picks every instance's mu1
            self.set_reg_params({'mu1': grid['mu1_range'][mu_choice[:, best[1]]]})
        return sol, stats


class GGLassoEstimator:
    """The estimates of a ``glasso_problem``, scikit-learn style: ``precision_`` (the sparse component Theta),
    ``lowrank_`` (L, with ``latent=True``), ``sample_covariance_`` (the input S), ``adjacency_``, ``n_samples``,
    ``n_features``.  For instances of different dimension every attribute is a dict with keys 0..K-1.
    ``glasso_problem.edge_inference()`` adds ``debiased_precision_``, ``standard_error_``, ``zscore_``, ``pvalue_``,
    ``pvalue_adj_``, ``confidence_interval_``, ``significant_`` and ``differential_``."""

    def __init__(self, S, N, p, K, multiple=True, latent=False, conforming=True):
        self.multiple, self.latent, self.conforming, self.K = multiple, latent, conforming, K
        self.n_samples, self.n_features = N, p
        self.sample_covariance_ = _per_instance(S, np.array)
        self.precision_ = self.lowrank_ = self.adjacency_ = self.ebic_ = None

    def _set_solution(self, Theta, L=None):
        self.precision_ = _per_instance(Theta, np.array)
        self.lowrank_ = None if L is None else _per_instance(L, np.array)
        self.calc_adjacency()

    def calc_ebic(self, gamma=0.5):
        """The eBIC of the estimate against the input S (which differs from the tables of a scaled model selection)."""
        self.ebic_ = _ms.ebic(self.sample_covariance_, self.precision_, self.n_samples, gamma=gamma)
        return self.ebic_

    def calc_adjacency(self, t=1e-8):
        self.adjacency_ = _per_instance(self.precision_, lambda Theta: adjacency_matrix(Theta, t=t))
