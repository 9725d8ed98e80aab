"""K-fold cross-validation of lambda1, host side (no GPU): the folds, the choice on a score curve, and ``cv_search`` on its
host route (numpy covariances, ``math.fsum`` inner products, ``robust_logdet``) with the batch's array work done by the
test-only oracle engine."""
import warnings

import numpy as np
import pytest


def cv_data(p, N, seed, M=2):
    """Observations (p,N) of a sparse precision matrix of gglasso_amd.synth."""
    from gglasso_amd import synth
    Th = synth.make_precisions('SGL', 1, p, M=M, seed=seed)[0]
    Z = np.random.default_rng(seed + 101).standard_normal((p, N))
    return np.ascontiguousarray(np.linalg.solve(np.linalg.cholesky(Th).T, Z)), Th


@pytest.fixture()
def oracle_engine(monkeypatch):
    from gglasso_amd import solver
    from oracle_engine import OracleEngine
    monkeypatch.setattr(solver, "ENGINE", OracleEngine)
    return OracleEngine


@pytest.mark.parametrize("N,F", [(23, 5), (40, 4), (10, 5)])
def test_cv_folds(N, F):
    from gglasso_amd.model_selection import cv_folds
    train, test = cv_folds(N, F, seed=3)
    m = N // F
    assert train.shape == (F, N - m) and test.shape == (F, m)
    assert train.dtype == test.dtype == np.int32
    assert np.all(np.diff(test, axis=1) > 0) and np.all(np.diff(train, axis=1) > 0)        # sorted, no duplicates
    assert len(set(test.ravel().tolist())) == F * m                                        # the test rows are disjoint
    assert test.min() >= 0 and test.max() < N
    for f in range(F):
        assert np.array_equal(train[f], np.setdiff1d(np.arange(N), test[f]))               # the complement
    perm = np.random.default_rng([3, F]).permutation(N)
    for f in range(F):
        assert np.array_equal(test[f], np.sort(perm[f * m:(f + 1) * m]))
    again = cv_folds(N, F, seed=3)
    assert np.array_equal(again[0], train) and np.array_equal(again[1], test)
    assert not np.array_equal(cv_folds(N, F, seed=4)[1], test)
    # the left-over observations are in every train set and in no test set
    left = np.setdiff1d(np.arange(N), test.ravel())
    assert left.size == N - F * m and all(np.isin(left, train[f]).all() for f in range(F))


def test_cv_folds_refusals():
    from gglasso_amd.model_selection import cv_folds
    with pytest.raises(ValueError, match="at least 2 folds"):
        cv_folds(20, 1)
    with pytest.raises(ValueError, match="more than the N"):
        cv_folds(4, 5)
    with pytest.raises(ValueError, match="per test fold"):
        cv_folds(9, 5)                                                  # m = 1


def test_cv_select_on_hand_made_curves():
    from gglasso_amd.model_selection import cv_select
    se = np.full(5, 0.1)
    with warnings.catch_warnings():
        warnings.simplefilter("error")
        assert cv_select([5.0, 3.0, 2.0, 2.5, 4.0], se, 'min') == 2
        assert cv_select([5.0, 2.0, 2.0, 2.5, 4.0], se, 'min') == 1              # a tie: the larger lambda
        # one_se: the largest lambda (smallest index) inside CV[min] + SE[min]
        assert cv_select([5.0, 2.09, 2.0, 2.05, 4.0], se, 'one_se') == 1
        assert cv_select([2.1, 2.11, 2.0, 2.05, 4.0], se, 'one_se') == 0
        assert cv_select([5.0, 2.11, 2.0, 2.05, 4.0], se, 'one_se') == 2
        assert cv_select([5.0, 2.5, 2.0, 2.05, 4.0], [0.1, 0.1, 0.6, 0.1, 0.1], 'one_se') == 1
        # NaN (a failed point) and +inf (a Theta that is not positive definite) are never chosen, by either rule
        assert cv_select([np.nan, 3.0, np.inf, 2.5, 4.0], se, 'min') == 3
        assert cv_select([np.nan, np.inf, 2.0, 2.05, 4.0], se, 'one_se') == 2
        assert cv_select([np.nan, 2.05, np.nan, 2.0, np.inf], se, 'one_se') == 1
        assert cv_select([1.0, np.nan], [np.nan, np.nan], 'one_se') == 0          # (a NaN standard error: the band is empty)
        assert cv_select([2.0], [0.0], 'min') == 0
    for rule in ('min', 'one_se'):
        with pytest.warns(RuntimeWarning, match="no lambda1"):
            assert cv_select([np.nan, np.inf, np.nan], [np.nan] * 3, rule) == 0
    with pytest.raises(ValueError, match="rule"):
        cv_select([1.0], [0.0], 'best')


LAM_SMALL = [0.4, 0.2, 0.1, 0.05]


@pytest.fixture(scope="module")
def host_run():
    """One host-route run shared by the tests below: p = 6, N = 60, F = 3, L = 4."""
    from gglasso_amd import solver, model_selection as ms
    from oracle_engine import OracleEngine
    X, _ = cv_data(6, 60, seed=5)
    keep, solver.ENGINE = solver.ENGINE, OracleEngine
    try:
        sol, stats = ms.cv_search(X, LAM_SMALL[::-1], n_folds=3, seed=1, tol=1e-8, rtol=1e-8, store_all=True)
    finally:
        solver.ENGINE = keep
    return X, sol, stats


def numpy_nll(X, stats, center=True):
    L, F = stats['THETA'].shape[:2]
    NLL = np.zeros((L, F))
    for l in range(L):
        for f in range(F):
            Xt = X[:, stats['TEST'][f]]
            S = np.cov(Xt, bias=True) if center else Xt @ Xt.T / Xt.shape[1]
            sign, ld = np.linalg.slogdet(stats['THETA'][l, f])
            assert sign == 1
            NLL[l, f] = np.sum(S * stats['THETA'][l, f]) - ld
    return NLL


def test_cv_search_host_route(host_run):
    from gglasso_amd import model_selection as ms
    from oracle import ggl_oracle as orc
    X, sol, stats = host_run
    p, N, F, L = 6, 60, 3, 4
    assert np.array_equal(stats['LAMBDA'], LAM_SMALL)                   # sorted in descending order
    train, test = ms.cv_folds(N, F, seed=1)
    assert np.array_equal(stats['TRAIN'], train) and np.array_equal(stats['TEST'], test)
    assert stats['n_folds'] == F and stats['rule'] == 'min' and stats['FAILED'] == [] and stats['NOT_PD'] == []
    assert stats['THETA'].shape == (L, F, p, p) and stats['NLL'].shape == stats['NNZ'].shape == (L, F)
    NLL = numpy_nll(X, stats)
    assert np.all(np.abs(stats['NLL'] - NLL) <= 1e-12 * np.abs(NLL))
    assert np.array_equal(stats['CV'], stats['NLL'].mean(axis=1))
    assert np.array_equal(stats['SE'], stats['NLL'].std(axis=1, ddof=1) / np.sqrt(F))
    assert stats['IX'] == ms.cv_select(NLL.mean(axis=1), NLL.std(axis=1, ddof=1) / np.sqrt(F), 'min')
    assert stats['BEST'] == {'lambda1': LAM_SMALL[stats['IX']]}
    assert np.array_equal(stats['NNZ'], np.count_nonzero(stats['THETA'], axis=(2, 3)))
    # every point is the single solve on the train fold's numpy covariance
    ref, _ = orc.ADMM_SGL(np.cov(X[:, train[1]], bias=True), LAM_SMALL[2], np.eye(p), X_0=np.eye(p), tol=1e-8, rtol=1e-8)
    assert np.abs(stats['THETA'][2, 1] - ref['Theta']).max() <= 1e-10
    # the solution: all observations at the chosen lambda
    from gglasso_amd import solver
    from oracle_engine import OracleEngine
    keep, solver.ENGINE = solver.ENGINE, OracleEngine
    try:
        # (the covariance of all observations as the host route forms it: the gathered columns)
        ref, _ = solver.ADMM_SGL(np.cov(X[:, np.arange(N)], bias=True), stats['BEST']['lambda1'], np.eye(p), X_0=np.eye(p),
                                 tol=1e-8, rtol=1e-8, verbose=False)
    finally:
        solver.ENGINE = keep
    assert sorted(sol) == ['Omega', 'Theta', 'X'] and np.array_equal(sol['Theta'], ref['Theta'])


def test_cv_search_chunks_rule_center_and_scale(oracle_engine, host_run):
    from gglasso_amd import model_selection as ms
    X, sol, stats = host_run
    sol2, st2 = ms.cv_search(X, LAM_SMALL, n_folds=3, seed=1, tol=1e-8, rtol=1e-8, lambdas_per_batch=3, rule='one_se')
    assert np.array_equal(st2['NLL'], stats['NLL']) and 'THETA' not in st2 and st2['rule'] == 'one_se'
    assert st2['IX'] == ms.cv_select(stats['CV'], stats['SE'], 'one_se') <= stats['IX']
    # folds given by the caller
    sol3, st3 = ms.cv_search(X, LAM_SMALL, folds=(stats['TRAIN'], stats['TEST']), tol=1e-8, rtol=1e-8)
    assert np.array_equal(st3['NLL'], stats['NLL']) and np.array_equal(sol3['Theta'], sol['Theta'])
    # without centring: the raw second moments on both sides
    sol4, st4 = ms.cv_search(X + 0.3, LAM_SMALL, n_folds=3, seed=1, center=False, tol=1e-8, rtol=1e-8, store_all=True)
    NLL = numpy_nll(X + 0.3, st4, center=False)
    assert np.all(np.abs(st4['NLL'] - NLL) <= 1e-12 * np.abs(NLL))
    # scale: one scale for all folds, from all observations; the run is that of the scaled data
    Y = X * np.arange(1, 7)[:, None]
    sol5, st5 = ms.cv_search(Y, LAM_SMALL, n_folds=3, seed=1, scale=True, tol=1e-8, rtol=1e-8)
    assert np.array_equal(st5['scale'], Y.var(axis=1))
    sol6, st6 = ms.cv_search(Y / Y.std(axis=1)[:, None], LAM_SMALL, n_folds=3, seed=1, tol=1e-8, rtol=1e-8)
    assert np.array_equal(st5['NLL'], st6['NLL']) and np.array_equal(sol5['Theta'], sol6['Theta']) and 'scale' not in st6
    Y[2] = 4.0
    with pytest.raises(ValueError, match="variable 2 is constant"):
        ms.cv_search(Y, LAM_SMALL, n_folds=3, scale=True)


def test_cv_search_failed_point_and_not_pd(oracle_engine, monkeypatch, host_run):
    """A point of lambda index 1 that ends as 'solver error': that lambda has no score, is named and not chosen.  A Theta
    that is not positive definite scores +inf and is not chosen either."""
    from gglasso_amd import solver, model_selection as ms
    X, sol, stats = host_run
    F = 3

    class Failing(oracle_engine):
        def sgl_batch_step(self, rho, lambda1, latent, mu1):
            out = super().sgl_batch_step(rho, lambda1, latent, mu1)
            out[1 * F + 2] = np.nan
            return out

    monkeypatch.setattr(solver, "ENGINE", Failing)
    with pytest.warns(RuntimeWarning) as rec:
        sol2, st2 = ms.cv_search(X, LAM_SMALL, n_folds=3, seed=1, tol=1e-8, rtol=1e-8)
    assert any("cross-validation: a fold failed at lambda1 = [0.2]" in str(w.message) for w in rec)
    assert st2['FAILED'] == [1] and np.all(np.isnan(st2['NLL'][1])) and np.isnan(st2['CV'][1]) and np.all(np.isnan(st2['NNZ'][1]))
    keep = [0, 2, 3]
    assert np.array_equal(st2['NLL'][keep], stats['NLL'][keep])
    assert st2['IX'] != 1 and st2['IX'] == ms.cv_select(st2['CV'], st2['SE'], 'min')

    monkeypatch.setattr(solver, "ENGINE", oracle_engine)
    real = ms.robust_logdet
    best = (stats['IX'], 0)
    target = stats['THETA'][best]
    monkeypatch.setattr(ms, "robust_logdet", lambda A, t=1e-12: -np.inf if np.array_equal(A, target) else real(A, t))
    sol3, st3 = ms.cv_search(X, LAM_SMALL, n_folds=3, seed=1, tol=1e-8, rtol=1e-8)
    assert st3['NOT_PD'] == [best] and st3['NLL'][best] == np.inf and st3['CV'][best[0]] == np.inf
    assert st3['FAILED'] == [] and st3['IX'] != stats['IX']


def test_cv_curve_has_its_minimum_inside_the_grid(oracle_engine):
    """Data of a sparse precision matrix, p = 12, N = 120: over a grid from the empty graph (lambda1 above every off-diagonal
    |S_ij|) to a nearly dense one, the held-out likelihood is best strictly inside."""
    from gglasso_amd import model_selection as ms
    p, N = 12, 120
    X, Th = cv_data(p, N, seed=11)
    lam = np.geomspace(2.0, 0.002, 9)
    sol, st = ms.cv_search(X, lam, n_folds=4, seed=0, store_all=True)
    assert st['FAILED'] == [] and st['NOT_PD'] == []
    nnz = st['NNZ'].mean(axis=1)
    assert nnz[0] == p                                                  # the empty graph
    assert nnz[-1] >= p + 0.8 * p * (p - 1)                             # nearly dense
    assert 0 < st['IX'] < len(lam) - 1 and st['IX'] == int(np.argmin(st['CV']))
    assert st['CV'][st['IX']] < min(st['CV'][0], st['CV'][-1]) - st['SE'][st['IX']]
    assert np.count_nonzero(sol['Theta']) < p * p


def test_binding_has_the_cv_entry_point():
    from gglasso_amd import _lib
    assert "ggl_heldout_scores" in _lib.EXPORTS
    assert _lib.ABI_VERSION == 300


def test_cv_search_refusals():
    from gglasso_amd import model_selection as ms
    X = np.random.default_rng(0).standard_normal((4, 30))
    for kw, word in ((dict(correlation='kendall'), "correlation"), (dict(missing='pairwise'), "missing"),
                     (dict(project=True), "project"), (dict(latent=True), "latent"),
                     (dict(lambda1_mask=np.ones((4, 4))), "lambda1_mask"), (dict(rule='best'), "rule")):
        with pytest.raises(ValueError, match=word):
            ms.cv_search(X, [0.1], **kw)
    with pytest.raises(ValueError, match="multiple-instance"):
        ms.cv_search(np.stack([X, X]), [0.1])
    with pytest.raises(ValueError, match="multiple-instance"):
        ms.cv_search([X, X], [0.1])


def test_cross_validation_front_end(oracle_engine, monkeypatch):
    """glasso_problem.cross_validation on the host route (numpy stands in for the device covariance of from_data)."""
    from gglasso_amd import model_selection as ms, ops, utils
    from gglasso_amd.problem import glasso_problem

    def host_cov(X_, center=True, scale=False, **kw):
        kind, Xs = utils._data_list(X_)
        S = [ms._host_subset_covariances(x, np.arange(x.shape[1])[None], center, False)[0] for x in Xs]
        return S[0] if kind == "2d" else (np.stack(S) if kind == "3d" else dict(enumerate(S)))

    monkeypatch.setattr(utils, "sample_covariance", host_cov)
    X, _ = cv_data(6, 60, seed=5)
    grid = {'lambda1_range': np.array(LAM_SMALL)}
    P = glasso_problem.from_data(X, reg_params={'lambda1': 0.3})
    P.cross_validation(grid, n_folds=3, seed=1, tol=1e-8, rtol=1e-8)
    sol, st = ms.cv_search(X, LAM_SMALL, n_folds=3, seed=1, tol=1e-8, rtol=1e-8)
    assert P.reg_params['lambda1'] == st['BEST']['lambda1'] == P.modelselect_stats['BEST']['lambda1']
    assert np.array_equal(P.modelselect_stats['NLL'], st['NLL']) and P.modelselect_stats['IX'] == st['IX']
    assert np.array_equal(P.solution.precision_, sol['Theta'])
    # refusals: each before any work
    with pytest.raises(AssertionError, match="from_data"):
        glasso_problem(np.eye(6), 50).cross_validation(grid)
    with pytest.raises(AssertionError, match="Single Graphical Lasso"):
        glasso_problem.from_data(np.stack([X, X])).cross_validation(grid)
    with pytest.raises(AssertionError, match="latent"):
        glasso_problem.from_data(X, latent=True).cross_validation(grid)
    with pytest.raises(AssertionError, match="lambda1_mask"):
        glasso_problem.from_data(X).cross_validation({'lambda1_range': np.array(LAM_SMALL), 'lambda1_mask': np.ones((6, 6))})
    for kw, word in ((dict(correlation='kendall'), "correlation='kendall'"), (dict(missing='pairwise'), "missing='pairwise'"),
                     (dict(project=True), "project=True")):
        Q = glasso_problem.from_data(X)
        # (built as the option leaves a problem: the matrices themselves are the device operators')
        if 'correlation' in kw:
            Q._correlation = 'kendall'
        elif 'missing' in kw:
            Q._missing = 'pairwise'
        else:
            Q._project_S = True
        with pytest.raises(ValueError, match=word):
            Q.cross_validation(grid)
