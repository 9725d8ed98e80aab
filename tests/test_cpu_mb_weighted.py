"""Neighbourhood selection with penalty weights and the scaled lasso without a GPU: the numpy twin
(``utils.host_neighborhood_selection(weights=, scaled=)``) under the checks of tests/mbw_ref.py against the longdouble
comparison value, the bits it keeps without the new arguments, ``adaptive_weights``, ``scaled_lasso_lambda``,
``scaled_lasso_precision`` on the host route, and the refusals."""
import warnings

import numpy as np
import pytest

import mb_ref
import mbw_ref
from mbw_ref import SIG_TOL, TOL

SIZES = (1, 2, 3, 5, 17, 63, 64, 65)


def _twin(p, scaled, rule='and'):
    from gglasso_amd import utils
    return utils.host_neighborhood_selection(mb_ref.stack(p), mb_ref.GRID, rule, tol=TOL, return_info=True,
                                             weights=mbw_ref.weight_stack(p), scaled=scaled, sig_tol=SIG_TOL)


@pytest.mark.parametrize("scaled", (False, True), ids=("plain", "scaled"))
@pytest.mark.parametrize("p", SIZES)
def test_twin_against_the_comparison_value(p, scaled):
    """Checks 1-4 for the stack of three seeds with one weight table per matrix."""
    from gglasso_amd import utils
    W, info = _twin(p, scaled)
    assert W.shape == (3, 4, p, p) and info['OUTER'].shape == (3, 4, p)
    assert np.all(info['OUTER'] >= 1) if scaled else not info['OUTER'].any()
    assert ('SIGMA' in info) == scaled
    if scaled:
        assert np.array_equal(info['SIGMA'], np.sqrt(info['RESVAR']))
    for seed in range(3):
        ok = mbw_ref.check_case(p, seed, scaled, info['COEF'][seed], info['RESVAR'][seed], info['STATUS'][seed], "twin")
        for rule in ('and', 'or'):
            Wr = utils.neighborhood_graph(info['COEF'][seed], rule)
            if rule == 'and':
                assert np.array_equal(Wr, W[seed])
            assert np.array_equal(Wr, mbw_ref.and_or(info['COEF'][seed], rule))
            mbw_ref.check_graphs(p, seed, scaled, Wr, rule, ok)


@pytest.mark.parametrize("p", (5, 17, 65))
def test_unit_weights_keep_the_bits(p):
    """``weights`` of ones without ``scaled`` is the arithmetic of the call without them -- every key of the info but
    ``OUTER`` bit for bit, and ``OUTER`` absent from the unweighted call; a shared table is the same table given per matrix."""
    from gglasso_amd import utils
    S = mb_ref.stack(p)[:2]
    W0, i0 = utils.host_neighborhood_selection(S, mb_ref.GRID, 'or', tol=TOL, return_info=True)
    W1, i1 = utils.host_neighborhood_selection(S, mb_ref.GRID, 'or', tol=TOL, return_info=True, weights=np.ones((p, p)))
    assert np.array_equal(W0, W1) and all(np.array_equal(i0[k], i1[k]) for k in i0)
    assert 'OUTER' not in i0 and sorted(set(i1) - set(i0)) == ['OUTER'] and not i1['OUTER'].any()
    Wt = mbw_ref.weights(p, 0)
    for scaled in (False, True):
        a = utils.host_neighborhood_selection(S, mb_ref.GRID, 'and', tol=TOL, return_info=True, weights=Wt, scaled=scaled)
        b = utils.host_neighborhood_selection(S, mb_ref.GRID, 'and', tol=TOL, return_info=True, weights=np.stack([Wt, Wt]),
                                              scaled=scaled)
        assert np.array_equal(a[0], b[0]) and all(np.array_equal(a[1][k], b[1][k]) for k in a[1])


def test_twin_edges_of_the_method():
    from gglasso_amd import utils
    p = 17
    S, Wt = mb_ref.stack(p)[0], mbw_ref.weights(p, 0)
    off = ~np.eye(p, dtype=bool)
    top = float((np.abs(S) / (Wt * np.sqrt(np.diag(S))[:, None]))[off].max())
    for scaled in (False, True):
        W, info = utils.host_neighborhood_selection(S, (top * 1.01, 0.1), 'or', tol=TOL, return_info=True, weights=Wt, scaled=scaled)
        assert not W[0].any() and not info['SWEEPS'][0].any() and not info['STATUS'].any() and W[1].any()
        assert np.array_equal(info['RESVAR'][0], np.diag(S)) and np.all(info['OUTER'][0] == (1 if scaled else 0))
        # p = 1
        W, info = utils.host_neighborhood_selection(np.array([[2.0]]), mb_ref.GRID, 'and', return_info=True, scaled=scaled,
                                                    weights=np.ones((1, 1)))
        assert W.shape == (4, 1, 1) and not W.any() and not info['STATUS'].any() and np.all(info['RESVAR'] == 2.0)
        # a free column and an excluded one
        Wz = Wt.copy()
        Wz[:, 4], Wz[:, 9] = 0.0, np.inf
        W, info = utils.host_neighborhood_selection(S, mb_ref.GRID, 'and', tol=TOL, return_info=True, weights=Wz, scaled=scaled)
        C = info['COEF']
        assert not info['STATUS'].any() and np.all(C[:, 9, :] == 0) and np.all(C[:, 4, :][:, np.arange(p) != 4] != 0)
        mbw_ref.check_residual(S, mb_ref.GRID, Wz, scaled, C, info['RESVAR'], what="free and excluded columns")
    # one outer iteration at the last lambda alone
    W, info = utils.host_neighborhood_selection(S, mb_ref.GRID[-1:], 'and', tol=TOL, return_info=True, weights=Wt, scaled=True,
                                                max_outer=1)
    assert np.all(info['STATUS'] == 1) and np.all(info['OUTER'] == 1) and np.all(np.isfinite(info['COEF']))
    assert np.all(np.isfinite(info['RESVAR'])) and np.all(np.isfinite(W))


def test_twin_duplicated_variable():
    """The degenerate square-root problem: the floor on tau^2 ends the two nodes, nobody else is touched."""
    from gglasso_amd import utils
    S = mbw_ref.duplicate_case()
    p = S.shape[0]
    W, info = utils.host_neighborhood_selection(S, mb_ref.GRID, 'raw', tol=TOL, return_info=True, scaled=True)
    dup = np.zeros(p, dtype=bool)
    dup[[3, 5]] = True
    assert np.all(info['STATUS'][:, dup] == 3) and np.all(info['OUTER'][0, dup] <= 20) and not info['STATUS'][:, ~dup].any()
    for j in (3, 5):
        col = info['COEF'][:, :, j]
        assert np.all(col[:, j] == 0) and np.all(np.isnan(np.delete(col, j, axis=1))) and np.all(np.isnan(info['RESVAR'][:, j]))
    keep = np.broadcast_to(~dup[None, :], info['STATUS'].shape)
    C = np.where(np.isnan(info['COEF']), 0.0, info['COEF'])
    R = np.where(np.isnan(info['RESVAR']), 1.0, info['RESVAR'])
    mbw_ref.check_residual(S, mb_ref.GRID, np.ones((p, p)), True, C, R, nodes=keep, what="beside a duplicated variable")


def test_twin_non_finite_matrix():
    from gglasso_amd import utils
    p = 5
    S = mb_ref.stack(p).copy()
    S[1, 2, 3] = S[1, 3, 2] = np.nan
    Wt = mbw_ref.weights(p, 0)
    for scaled in (False, True):
        W, info = utils.host_neighborhood_selection(S, mb_ref.GRID, 'raw', tol=TOL, return_info=True, weights=Wt, scaled=scaled)
        Wc, ic = utils.host_neighborhood_selection(S[[0, 2]], mb_ref.GRID, 'raw', tol=TOL, return_info=True, weights=Wt, scaled=scaled)
        assert np.all(info['STATUS'][1][:, [2, 3]] == 2) and set(np.unique(info['STATUS'][1])) <= {0, 2}
        assert np.array_equal(W[[0, 2]], Wc) and np.array_equal(info['RESVAR'][[0, 2]], ic['RESVAR'])


def test_adaptive_weights_and_the_second_stage():
    from gglasso_amd import utils
    p = 17
    S = mb_ref.stack(p)[0]
    _, first = utils.host_neighborhood_selection(S, [0.1], 'raw', tol=TOL, return_info=True)
    C = first['COEF'][0]
    Wt = utils.adaptive_weights(C)
    off = ~np.eye(p, dtype=bool)
    assert Wt.shape == (p, p) and Wt.flags.c_contiguous
    for j, k in ((0, 1), (1, 0), (3, 9), (16, 15)):
        assert Wt[j, k] == (np.inf if C[k, j] == 0 else 1.0 / abs(C[k, j]))
    assert np.array_equal(np.isinf(Wt), C.T == 0)
    assert np.array_equal(utils.adaptive_weights(C, gamma=2.0, eps=0.5), 1.0 / (np.abs(C.T) + 0.5) ** 2.0)
    assert utils.adaptive_weights(np.stack([C, C])).shape == (2, p, p)
    _, second = utils.host_neighborhood_selection(S, [0.02, 0.01], 'raw', tol=TOL, return_info=True, weights=Wt)
    assert not second['STATUS'].any()
    nz2 = second['COEF'] != 0
    assert nz2.any() and not (nz2 & (C == 0)[None]).any()             # inside the first stage's support
    mbw_ref.check_residual(S, [0.02, 0.01], Wt, False, second['COEF'], second['RESVAR'], what="adaptive second stage")
    with pytest.raises(AssertionError):
        utils.adaptive_weights(C, gamma=0.0)
    with pytest.raises(AssertionError):
        utils.adaptive_weights(np.full((3, 3), np.nan))


def test_scaled_lasso_lambda():
    from gglasso_amd import utils
    assert utils.scaled_lasso_lambda(50, 200) == float(np.sqrt(2 * np.log(50) / 200))
    lam1 = utils.scaled_lasso_lambda(1, 10)
    assert lam1 > 0 and np.isfinite(lam1)
    with pytest.raises(AssertionError):
        utils.scaled_lasso_lambda(0, 10)
    with pytest.raises(AssertionError):
        utils.scaled_lasso_lambda(5, 0)


def test_scaled_lasso_precision_on_the_host():
    """One path at the universal penalty; the estimator commutes with rescaling the variables by powers of two."""
    from gglasso_amd import utils
    p, n = 17, 108
    S = mb_ref.stack(p)[1]
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        Theta, info = utils.scaled_lasso_precision(S, n=n, host=True)
        lam0 = utils.scaled_lasso_lambda(p, n)
        _, raw = utils.host_neighborhood_selection(S, [lam0], 'raw', return_info=True, scaled=True, weights=np.ones((p, p)))
        assert info['LAMBDA0'] == lam0 and not info['STATUS'].any() and info['COEF'].shape == (p, p)
        assert np.array_equal(Theta, utils.neighborhood_precision(raw['COEF'][0], raw['RESVAR'][0])[0])
        assert np.array_equal(Theta, Theta.T) and np.all(np.diag(Theta) == 1.0 / info['RESVAR'])
        d = 2.0 ** np.random.default_rng(4).integers(-3, 4, p)
        Sd = S * d[:, None] * d[None, :]
        Theta_d, info_d = utils.scaled_lasso_precision(Sd, n=n, host=True)
    # with weights sqrt(S_kk) the rescaled problem is the same problem in other units (the stopping tests are not: they see
    # d_j d_k tol): both results are held to their own optimality residual, their difference is reported
    mbw_ref.check_rescaled(S, Sd, d, lam0, Theta, info, Theta_d, info_d)
    with pytest.raises(AssertionError, match="sample size"):
        utils.scaled_lasso_precision(S, host=True)
    with pytest.raises(AssertionError):
        utils.scaled_lasso_precision(S, lambda0=-1.0, host=True)
    with pytest.raises(AssertionError):
        utils.scaled_lasso_precision(S, n=n, weights='var', host=True)


def test_arguments_are_refused_on_the_host():
    from gglasso_amd import utils
    p = 5
    S, Wt = mb_ref.stack(p), mbw_ref.weights(p, 0)
    neg, nan = Wt.copy(), np.stack([Wt] * 3)
    neg[2, 3] = -0.5
    nan[1, 4, 0] = np.nan
    for fn in (utils.host_neighborhood_selection, utils.neighborhood_selection):
        with pytest.raises(ValueError, match=r"weights\[2, 3\]"):
            fn(S, mb_ref.GRID, weights=neg)
        with pytest.raises(ValueError, match=r"weights\[1, 4, 0\]"):
            fn(S, mb_ref.GRID, weights=nan)
        with pytest.raises(AssertionError, match="shape"):
            fn(S, mb_ref.GRID, weights=np.ones((2, p, p)))
        with pytest.raises(AssertionError, match="sig_tol"):
            fn(S, mb_ref.GRID, scaled=True, sig_tol=-1.0)
        with pytest.raises(AssertionError, match="sig_tol"):
            fn(S, mb_ref.GRID, scaled=True, sig_tol=np.nan)
        with pytest.raises(AssertionError, match="max_outer"):
            fn(S, mb_ref.GRID, scaled=True, max_outer=0)
    inf = Wt.copy()
    inf[0, 1] = np.inf                                                  # legal
    utils.host_neighborhood_selection(S, mb_ref.GRID, weights=inf)


class _NoDeviceRoute:
    """An engine without the device routes: the drivers take numpy covariances and the twins."""


@pytest.mark.parametrize("scaled", (False, True), ids=("plain", "scaled"))
def test_searches_on_the_host_route(monkeypatch, scaled):
    """``stars_search`` and ``cv_search`` with ``weights`` / ``scaled``: the subsample and fold fits and the final fit are the
    twin's with the same arguments; without them the results are those of the calls that do not name them."""
    from gglasso_amd import model_selection as ms, solver, utils
    monkeypatch.setattr(solver, "ENGINE", _NoDeviceRoute)
    X, lam = mb_ref.stars_data(), np.array(mb_ref.GRID)
    Wt = mbw_ref.weights(17, 0)
    idx = ms.stars_subsamples(X.shape[1], 4, None, seed=5)
    kw = dict(tol=TOL, return_info=True, weights=Wt, scaled=scaled)
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        sol, st = ms.stars_search(X, lam, n_subsamples=4, seed=5, beta=0.1, tol=TOL, store_all=True, method='mb', weights=Wt,
                                  scaled=scaled)
        _, st0 = ms.stars_search(X, lam, n_subsamples=4, seed=5, beta=0.1, tol=TOL, store_all=True, method='mb')
        _, st1 = ms.stars_search(X, lam, n_subsamples=4, seed=5, beta=0.1, tol=TOL, store_all=True, method='mb', weights=None,
                                 scaled=False)
    S_sub = ms._host_subset_covariances(X, idx, True, False)
    W, _ = utils.host_neighborhood_selection(S_sub, lam, 'and', **kw)
    assert np.array_equal(st['THETA'], np.swapaxes(W, 0, 1)) and st['FAILED'] == []
    cnt, num = ms._host_edge_counts(st['THETA'], 1e-8)
    assert np.array_equal(st['COUNTS'], cnt) and st['NUM'] == [int(v) for v in num]
    W0 = utils.host_neighborhood_selection(S_sub, lam, 'and', tol=TOL)
    assert np.array_equal(st0['THETA'], np.swapaxes(W0, 0, 1)) and np.array_equal(st0['THETA'], st1['THETA'])
    assert not np.array_equal(st0['THETA'], st['THETA'])
    ix = st['IX']
    S_full = ms._host_subset_covariances(X, np.arange(X.shape[1])[None], True, False)[0]
    Wf, inff = utils.host_neighborhood_selection(S_full, lam[:ix + 1], 'and', **kw)
    assert np.array_equal(sol['coef'], inff['COEF'][ix]) and np.array_equal(sol['resvar'], inff['RESVAR'][ix])
    assert np.array_equal(sol['adjacency'], Wf[ix] != 0)
    # cross-validation, the lasso's own coefficients scored
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        solc, sc = ms.cv_search(X, lam, n_folds=3, seed=4, method='mb', graph_rule='or', refit=False, store_all=True, weights=Wt,
                                scaled=scaled)
        _, sr = ms.cv_search(X, lam, n_folds=3, seed=4, method='mb', graph_rule='or', refit=True, store_all=True, weights=Wt,
                             scaled=scaled)
    train, test = ms.cv_folds(X.shape[1], 3, 4)
    S_tr, S_te = ms._host_subset_covariances(X, train, True, False), ms._host_subset_covariances(X, test, True, False)
    Wc, ic = utils.host_neighborhood_selection(S_tr, lam, 'or', **kw)
    assert np.array_equal(sc['THETA'], np.swapaxes(Wc, 0, 1)) and np.array_equal(sc['RESVAR'], np.swapaxes(ic['RESVAR'], 0, 1))
    assert np.array_equal(sr['THETA'], sc['THETA'])
    rf = utils.host_neighborhood_refit(S_tr, Wc, 1e-8, S_te)
    assert np.array_equal(sr['RESVAR'], np.swapaxes(rf['RESVAR'], 0, 1)) and np.array_equal(sr['HELDOUT'], np.swapaxes(rf['HELDOUT'], 0, 1))
    assert np.array_equal(sc['SCORE'], utils.mb_cv_scores(sc['RESVAR'], sc['HELDOUT'], np.zeros(sc['STATUS'].shape, bool), 'pseudo'))
    ixc = sc['IX']
    _, infc = utils.host_neighborhood_selection(S_full, lam[:ixc + 1], 'or', **kw)
    assert np.array_equal(solc['coef'], infc['COEF'][ixc])
    assert np.array_equal(solc['precision'], utils.neighborhood_precision(infc['COEF'][ixc], infc['RESVAR'][ixc])[0])


def test_searches_refuse_the_arguments_for_the_glasso():
    from gglasso_amd import model_selection as ms
    X = mb_ref.stars_data(p=6, N=60)
    for kw in (dict(weights=np.ones((6, 6))), dict(scaled=True)):
        with pytest.raises(ValueError, match="lambda1_mask"):
            ms.stars_search(X, (0.4, 0.2), n_subsamples=3, **kw)
        with pytest.raises(ValueError, match="lambda1_mask"):
            ms.cv_search(X, (0.4, 0.2), n_folds=3, **kw)
    with pytest.raises(AssertionError, match="one"):
        ms.stars_search(X, (0.4, 0.2), n_subsamples=3, method='mb', weights=np.ones((3, 6, 6)))
    with pytest.raises(AssertionError, match="one"):
        ms.cv_search(X, (0.4, 0.2), n_folds=3, method='mb', weights=np.ones((5, 6)))


def test_front_end_on_the_host_route(monkeypatch):
    from gglasso_amd import model_selection as ms, solver, utils
    from gglasso_amd.problem import glasso_problem
    import problem_helpers
    problem_helpers.on_host(monkeypatch)
    assert not hasattr(solver.ENGINE, "neighborhood_stability")
    X = mb_ref.stars_data()
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        P = glasso_problem.from_data(X, reg=None)
        P.neighborhood_selection(select='scaled')
        want, winfo = utils.scaled_lasso_precision(P.S, n=X.shape[1], host=True)
    assert np.array_equal(P.solution.precision_, want) and P.reg_params['lambda1'] == utils.scaled_lasso_lambda(17, X.shape[1])
    assert np.array_equal(P.solution.adjacency_, (want != 0) & ~np.eye(17, dtype=bool)) and P.solution.adjacency_.any()
    st = P.modelselect_stats
    assert st['LAMBDA0'] == winfo['LAMBDA0'] and np.array_equal(st['SIGMA'], winfo['SIGMA']) and not st['STATUS'].any()
    assert np.array_equal(P.neighborhood_['coef'], winfo['COEF'])
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        Q = glasso_problem.from_data(X, reg=None, do_scaling=True)
        Q.neighborhood_selection(select='scaled', lambda0=0.3, rule='or')
        wq, _ = utils.scaled_lasso_precision(Q.S, lambda0=0.3, rule='average', host=True)
        Wt = mbw_ref.weights(17, 2)
        P.neighborhood_selection(mb_ref.GRID, select='cv', rule='and', n_folds=3, seed=4, weights=Wt, scaled=True)
        sol, stc = ms.cv_search(X, mb_ref.GRID, n_folds=3, seed=4, method='mb', graph_rule='and', weights=Wt, scaled=True)
    assert np.allclose(np.diag(Q.S), 1.0, rtol=0, atol=1e-14) and Q.reg_params['lambda1'] == 0.3
    assert np.array_equal(Q.solution.precision_, Q._from_correlations(wq))
    assert np.array_equal(P.solution.precision_, sol['precision']) and P.modelselect_stats['IX'] == stc['IX']
    with pytest.raises(AssertionError, match="searches nothing"):
        P.neighborhood_selection(mb_ref.GRID, select='scaled')
    with pytest.raises(AssertionError, match="lambda_range"):
        P.neighborhood_selection(select='cv')
    with pytest.raises(AssertionError, match="select"):
        P.neighborhood_selection(mb_ref.GRID, select='ebic')
    with pytest.raises(AssertionError, match="from_data"):
        glasso_problem(np.eye(4), 50, reg=None).neighborhood_selection(select='scaled')
    with pytest.raises(AssertionError, match="latent"):
        glasso_problem.from_data(X, reg=None, latent=True).neighborhood_selection(select='scaled')


def test_entry_points_are_declared():
    """The three entries stand in the header and in the binding's table with the same number of arguments."""
    import os
    import re
    from conftest import ROOT
    from gglasso_amd import _lib
    header = open(os.path.join(ROOT, "include", "ggl_hip.h")).read()
    assert "#define GGL_VERSION 300" in header and "#define GGL_MB_SCALED 1" in header
    for name in ("ggl_neighborhood_path_w", "ggl_neighborhood_stability_w", "ggl_neighborhood_cv_w"):
        m = re.search(r"\bint " + name + r"\(([^;]*)\);", header)
        assert m, name
        assert len(_lib._SIGNATURES[name][0]) == m.group(1).count(",") + 1, name
