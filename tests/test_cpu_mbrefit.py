"""The refit of neighbourhood selection without a GPU: the numpy twin (``utils.host_neighborhood_refit``) against the
longdouble comparison value and the derived bounds of tests/mbrefit_ref.py (sizes up to 65), the engineered graphs, the
statuses, ``utils.neighborhood_precision``, the assembly of the cross-validation scores, ``cv_search(method='mb')`` /
``stars_search(refit=True)`` / ``glasso_problem.neighborhood_selection`` on their host routes, and the refusals of the Python
layer."""
import warnings

import numpy as np
import pytest

import mb_ref
import mbrefit_ref as ref

T_EDGE = 1e-8
SIZES = (1, 2, 3, 5, 17, 63, 64, 65)


class _NoDeviceRoute:
    """An engine without the device routes: the drivers take numpy covariances and the twins."""


@pytest.mark.parametrize("p", SIZES)
def test_twin_against_the_comparison_value(p):
    """AND, OR and raw supports of the path along the grid, three seeds as one stack, T of other seeds."""
    from gglasso_amd import utils
    S, T, W = mb_ref.stack(p), ref.heldout_stack(p), ref.graphs(p)
    out = utils.host_neighborhood_refit(S, W, T_EDGE, T)
    assert out['COEF'].shape == W.shape and out['RESVAR'].shape == W.shape[:3] == out['HELDOUT'].shape
    ref.check_stack(S, T, W, T_EDGE, out, "twin")
    i = np.arange(p)
    assert np.all(out['COEF'][..., i, i] == 0)


def test_twin_identities_and_shapes():
    from gglasso_amd import utils
    p = 17
    S, W = mb_ref.stack(p), ref.graphs(p)
    a = utils.host_neighborhood_refit(S, W, T_EDGE, S)
    assert np.array_equal(a['HELDOUT'], a['RESVAR'])                        # T = S: one function, the same bits
    b = utils.host_neighborhood_refit(S[1], W[1, 5], T_EDGE)                # one matrix, one graph
    assert b['HELDOUT'] is None and b['COEF'].shape == (p, p) and b['RESVAR'].shape == (p,)
    assert np.array_equal(b['COEF'], a['COEF'][1, 5]) and np.array_equal(b['RESVAR'], a['RESVAR'][1, 5])
    c = utils.host_neighborhood_refit(S[2], W[2, :3], T_EDGE)
    assert c['COEF'].shape == (3, p, p) and np.array_equal(c['DEGREE'], a['DEGREE'][2, :3])
    d = utils.host_neighborhood_refit(S, W[:, 0], T_EDGE)
    assert d['COEF'].shape == (3, p, p) and np.array_equal(d['COEF'], a['COEF'][:, 0])


def test_twin_engineered_graphs():
    from gglasso_amd import utils
    p = 17
    S, T = mb_ref.case(p, 0), mb_ref.case(p, 7)
    # the empty graph: beta = 0, tau^2 = S_jj, r = T_jj
    out = utils.host_neighborhood_refit(S, np.zeros((p, p)), T_EDGE, T)
    assert not out['COEF'].any() and not out['DEGREE'].any() and not out['STATUS'].any()
    assert np.array_equal(out['RESVAR'], np.diagonal(S)) and np.array_equal(out['HELDOUT'], np.diagonal(T))
    # a NaN is no edge; below t is no edge; the sign does not matter
    Wn = np.zeros((p, p))
    Wn[3, 5], Wn[3, 6], Wn[3, 7], Wn[3, 8] = np.nan, 0.5e-8, -1.0, 1e-8
    out = utils.host_neighborhood_refit(S, Wn, T_EDGE)
    assert out['DEGREE'][3] == 2 and sorted(np.flatnonzero(out['COEF'][:, 3])) == [7, 8]
    # a non-symmetric pattern: node 2 regresses on 9, node 9 on nothing
    Wa = np.zeros((p, p))
    Wa[2, 9] = 1.0
    out = utils.host_neighborhood_refit(S, Wa, T_EDGE, T)
    assert out['DEGREE'][2] == 1 and out['DEGREE'][9] == 0 and out['COEF'][9, 2] == S[9, 2] / S[9, 9]
    ref.check_stack(S[None], T[None], Wa[None, None], T_EDGE, {k: v[None, None] for k, v in out.items()}, "twin, one edge")


@pytest.mark.parametrize("p", (17, 65))
def test_twin_complete_graph_is_the_inverse(p):
    from gglasso_amd import utils
    S = mb_ref.case(p, 1)
    W = np.ones((p, p))
    out = utils.host_neighborhood_refit(S, W, T_EDGE)
    assert np.all(out['DEGREE'] == p - 1) and not out['STATUS'].any()
    Theta, lmin = utils.neighborhood_precision(out['COEF'], out['RESVAR'])
    assert np.array_equal(Theta, Theta.T) and lmin > 0
    err = np.abs(Theta.astype(ref.LD) - ref.precision_reference(S)).astype(np.float64)
    bound = ref.precision_bound(S, out['COEF'], out['RESVAR'])
    print(f"twin, complete graph p={p}: {float((err / bound).max()):.3f} of the bound")
    assert np.all(err <= bound)


def test_twin_statuses():
    from gglasso_amd import utils
    cap = utils.MB_REFIT_MAX_DEG
    assert cap == 128
    # 1: a duplicated variable inside one neighbourhood
    p = 9
    S = mb_ref.case(p, 0).copy()
    S[4, :], S[:, 4] = S[3, :], S[:, 3]                                      # variable 4 = variable 3
    S[4, 4] = S[3, 3]
    W = np.zeros((p, p))
    W[0, [3, 4, 6]] = 1.0                                                    # node 0 holds both
    W[3, [0, 6]] = W[4, [0, 6]] = W[6, [0, 3]] = 1.0
    out = utils.host_neighborhood_refit(S, W, T_EDGE, mb_ref.case(p, 7))
    assert list(out['STATUS']) == [1, 0, 0, 0, 0, 0, 0, 0, 0]
    assert np.all(np.isnan(np.delete(out['COEF'][:, 0], 0))) and out['COEF'][0, 0] == 0
    assert np.isnan(out['RESVAR'][0]) and np.isnan(out['HELDOUT'][0])
    assert np.all(np.isfinite(out['COEF'][:, 1:])) and np.all(np.isfinite(out['RESVAR'][1:]))
    # 2: a non-finite value of T reaches the nodes whose gathers meet it
    T = mb_ref.case(p, 7).copy()
    T[6, 3] = T[3, 6] = np.inf
    out = utils.host_neighborhood_refit(mb_ref.case(p, 0), W, T_EDGE, T)
    assert list(out['STATUS']) == [2, 0, 0, 2, 0, 0, 2, 0, 0]                # 0: A = {3,4,6}; 3: A = {0,6}; 6: A = {0,3}
    assert np.isnan(out['HELDOUT'][[0, 3, 6]]).all() and np.isfinite(out['HELDOUT'][[1, 2, 4, 5, 7, 8]]).all()
    # 3: a hub with one neighbour more than the cap; with exactly the cap it is solved
    p = cap + 3
    S = mb_ref.case(p, 2)
    for deg, st in ((cap, 0), (cap + 1, 3)):
        out = utils.host_neighborhood_refit(S, ref.star(p, 1, deg), T_EDGE)
        assert out['DEGREE'][1] == deg and out['STATUS'][1] == st and not np.delete(out['STATUS'], 1).any()
        assert np.isnan(out['RESVAR'][1]) == (st == 3)


def test_precision_matrix():
    from gglasso_amd import utils
    coef = np.array([[0.0, 0.5, 0.0], [0.4, 0.0, 0.3], [0.0, 0.0, 0.0]])      # column j: node j
    tau = np.array([1.0, 2.0, 4.0])
    Th, lmin = utils.neighborhood_precision(coef, tau)
    # (0,1): -0.5/2 from node 1, -0.4/1 from node 0: the smaller magnitude; (1,2): node 2 has 0.3 on 1, node 1 nothing on 2
    assert np.array_equal(Th, np.array([[1.0, -0.25, 0.0], [-0.25, 0.5, 0.0], [0.0, 0.0, 0.25]])) and lmin > 0
    Tha, _ = utils.neighborhood_precision(coef, tau, rule='average')
    assert np.array_equal(Tha, Tha.T) and Tha[0, 1] == 0.5 * (-0.25 - 0.4) and Tha[1, 2] == 0.5 * (-0.3 / 4.0)
    with pytest.warns(RuntimeWarning, match="not positive definite by construction"):
        _, lm = utils.neighborhood_precision(np.array([[0.0, 3.0], [3.0, 0.0]]), np.ones(2))
    assert lm < 0
    with pytest.warns(RuntimeWarning, match="non-finite"):
        Thn, lm = utils.neighborhood_precision(np.array([[0.0, np.nan], [0.1, 0.0]]), np.array([1.0, np.nan]))
    assert np.isnan(lm) and np.array_equal(Thn, Thn.T, equal_nan=True)
    with pytest.raises(AssertionError, match="rule"):
        utils.neighborhood_precision(coef, tau, rule='max')
    with pytest.raises(AssertionError, match="do not fit"):
        utils.neighborhood_precision(coef, tau[:2])


def test_score_assembly():
    import math
    from gglasso_amd import utils
    rng = np.random.default_rng(3)
    tau, r = rng.uniform(0.5, 2, (2, 3, 5)), rng.uniform(0.5, 2, (2, 3, 5))
    bad = np.zeros((2, 3, 5), dtype=bool)
    bad[1, 2, 4] = True
    ps = utils.mb_cv_scores(tau, r, bad, 'pseudo')
    assert ps[0, 1] == math.fsum(np.log(tau[0, 1]) + r[0, 1] / tau[0, 1]) and np.isposinf(ps[1, 2]) and np.isfinite(ps).sum() == 5
    rn = r.copy()
    rn[1, 2, 4] = np.nan
    ms_ = utils.mb_cv_scores(tau, rn, bad, 'mse')
    assert ms_[0, 0] == math.fsum(r[0, 0]) and np.isnan(ms_[1, 2])
    tz = tau.copy()
    tz[0, 0, 0] = 0.0
    assert np.isposinf(utils.mb_cv_scores(tz, r, np.zeros_like(bad), 'pseudo')[0, 0])
    with pytest.raises(AssertionError, match="score"):
        utils.mb_cv_scores(tau, r, bad, 'nll')


def _cv_expected(X, lam, train, test, rule, refit, score):
    """The per-node arrays of one cross-validation from the twins and the comparison value's quadratic forms."""
    from gglasso_amd import model_selection as ms, utils
    S_tr, S_te = ms._host_subset_covariances(X, train, True, False), ms._host_subset_covariances(X, test, True, False)
    W, inf = utils.host_neighborhood_selection(S_tr, lam, rule, tol=1e-7, return_info=True)
    return S_tr, S_te, np.swapaxes(W, 0, 1), inf


@pytest.mark.parametrize("refit", (True, False))
def test_cv_host_route(monkeypatch, refit):
    from gglasso_amd import model_selection as ms, solver, utils
    monkeypatch.setattr(solver, "ENGINE", _NoDeviceRoute)
    X = mb_ref.stars_data()
    lam = np.array(mb_ref.GRID)
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        sol, st = ms.cv_search(X, lam, n_folds=3, seed=4, method='mb', graph_rule='or', refit=refit, store_all=True)
        _, st_mse = ms.cv_search(X, lam, n_folds=3, seed=4, method='mb', graph_rule='or', refit=refit, score='mse')
        _, per1 = ms.cv_search(X, lam, n_folds=3, seed=4, method='mb', graph_rule='or', refit=refit, lambdas_per_batch=1)
    train, test = ms.cv_folds(X.shape[1], 3, 4)
    S_tr, S_te, W, inf = _cv_expected(X, lam, train, test, 'or', refit, 'pseudo')
    assert np.array_equal(st['THETA'], W) and st['FAILED'] == [] and st['NOT_SOLVED'] == []
    # every (lambda, fold, node) from the stack returned, in longdouble
    p = X.shape[0]
    for l in range(lam.size):
        for f in range(3):
            for j in range(p):
                if refit:
                    A = ref.neighbours(W[l, f, j], j, T_EDGE)
                    b = ref.solve_node(S_tr[f], j, A).astype(np.float64)
                    tol_t = 1e-12
                else:
                    b_full = inf['COEF'][f, l][:, j]
                    A = np.flatnonzero(b_full)
                    b, tol_t = b_full[A], 1e-6                               # (the lasso's tau^2 carries the path's tol)
                assert abs(st['RESVAR'][l, f, j] - float(ref.quad(S_tr[f], j, A, b))) <= tol_t
                assert abs(st['HELDOUT'][l, f, j] - float(ref.quad(S_te[f], j, A, b))) <= 1e-12
    SC = utils.mb_cv_scores(st['RESVAR'], st['HELDOUT'], np.zeros(st['STATUS'].shape, dtype=bool), 'pseudo')
    assert np.array_equal(st['SCORE'], SC) and np.array_equal(st['CV'], SC.mean(axis=1))
    assert np.array_equal(st['SE'], SC.std(axis=1, ddof=1) / np.sqrt(3)) and st['IX'] == ms.cv_select(st['CV'], st['SE'], 'min')
    assert np.array_equal(st_mse['SCORE'], utils.mb_cv_scores(st['RESVAR'], st['HELDOUT'], np.zeros(st['STATUS'].shape, bool), 'mse'))
    assert np.array_equal(per1['RESVAR'], st['RESVAR']) == refit             # (a path that starts anew moves the lasso's bits)
    assert per1['IX'] == st['IX']
    # the final fit
    ix = st['IX']
    S_full = ms._host_subset_covariances(X, np.arange(X.shape[1])[None], True, False)[0]
    Wf, inff = utils.host_neighborhood_selection(S_full, lam[:ix + 1], 'or', tol=1e-7, return_info=True)
    assert np.array_equal(sol['adjacency'], Wf[ix] != 0) and np.array_equal(sol['coef'], inff['COEF'][ix])
    if refit:
        rf = utils.host_neighborhood_refit(S_full, Wf[ix], T_EDGE)
        assert np.array_equal(sol['coef_refit'], rf['COEF']) and np.array_equal(sol['resvar_refit'], rf['RESVAR'])
        assert np.array_equal(sol['precision'], utils.neighborhood_precision(rf['COEF'], rf['RESVAR'])[0])
        assert np.array_equal((sol['coef_refit'] != 0), sol['adjacency'])
    else:
        assert 'coef_refit' not in sol and np.array_equal(sol['precision'], sol['precision'].T)


def test_stars_refit_and_the_front_end(monkeypatch):
    from gglasso_amd import model_selection as ms, solver, utils
    from gglasso_amd.problem import glasso_problem
    monkeypatch.setattr(solver, "ENGINE", _NoDeviceRoute)
    X = mb_ref.stars_data()
    kw = dict(n_subsamples=6, seed=5, beta=0.1, scale=True, tol=1e-7, method='mb')
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        sol0, st0 = ms.stars_search(X, mb_ref.GRID, **kw)
        sol1, st1 = ms.stars_search(X, mb_ref.GRID, refit=True, **kw)
    assert sorted(sol0) == ['adjacency', 'coef', 'lambda1', 'resvar']
    assert sorted(sol1) == ['adjacency', 'coef', 'coef_refit', 'lambda1', 'precision', 'resvar', 'resvar_refit']
    assert all(np.array_equal(sol0[k], sol1[k]) for k in sol0) and st0['NUM'] == st1['NUM']
    assert np.array_equal(sol1['coef_refit'] != 0, sol1['adjacency']) and np.array_equal(sol1['precision'], sol1['precision'].T)
    S_full = ms._host_subset_covariances(X, np.arange(X.shape[1])[None], True, True)[0]
    rf = utils.host_neighborhood_refit(S_full, sol1['adjacency'].astype(float), T_EDGE)
    assert np.array_equal(sol1['coef_refit'], rf['COEF']) and np.array_equal(sol1['resvar_refit'], rf['RESVAR'])
    with pytest.raises(AssertionError, match="refit"):
        ms.stars_search(X, mb_ref.GRID, refit=True, n_subsamples=3)
    # the front end (the device calls of the class on numpy, an engine without the device routes of the searches)
    import problem_helpers
    problem_helpers.on_host(monkeypatch)
    assert not hasattr(solver.ENGINE, "neighborhood_cv") and not hasattr(solver.ENGINE, "neighborhood_stability")
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        P = glasso_problem.from_data(X, reg=None)
        P.neighborhood_selection(mb_ref.GRID, select='cv', rule='and', n_folds=3, seed=4)
        sol, st = ms.cv_search(X, mb_ref.GRID, n_folds=3, seed=4, method='mb', graph_rule='and')
    assert np.array_equal(P.solution.precision_, sol['precision']) and np.array_equal(P.solution.adjacency_, sol['adjacency'])
    assert P.reg_params['lambda1'] == st['BEST']['lambda1'] and P.modelselect_stats['IX'] == st['IX']
    assert np.array_equal(P.solution.adjacency_, (P.solution.precision_ != 0) & ~np.eye(17, dtype=bool))
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        P.neighborhood_selection(mb_ref.GRID, select='stars', rule='or', refit=False, n_subsamples=4, seed=1, beta=0.1)
    assert P.modelselect_stats['n_subsamples'] == 4 and np.array_equal(P.solution.precision_, P.solution.precision_.T)
    # refused, with the reason
    with pytest.raises(AssertionError, match="from_data"):
        glasso_problem(np.eye(4), 50, reg=None).neighborhood_selection(mb_ref.GRID)
    with pytest.raises(AssertionError, match="Single Graphical Lasso"):
        glasso_problem.from_data([X, X], reg='GGL').neighborhood_selection(mb_ref.GRID)
    with pytest.raises(AssertionError, match="latent"):
        glasso_problem.from_data(X, reg=None, latent=True).neighborhood_selection(mb_ref.GRID)
    with pytest.raises(AssertionError, match="select"):
        P.neighborhood_selection(mb_ref.GRID, select='ebic')
    with pytest.raises(AssertionError, match="rule"):
        P.neighborhood_selection(mb_ref.GRID, rule='raw')


def test_glasso_cv_route_is_untouched(monkeypatch):
    """``method='glasso'`` and no ``method`` at all: the same keys and bits."""
    from gglasso_amd import model_selection as ms, solver
    from oracle_engine import OracleEngine
    monkeypatch.setattr(solver, "ENGINE", OracleEngine)
    X = mb_ref.stars_data(p=6, N=60)
    kw = dict(n_folds=3, seed=2, store_all=True, tol=1e-6, rtol=1e-6)
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        sol_a, st_a = ms.cv_search(X, (0.4, 0.2), **kw)
        sol_b, st_b = ms.cv_search(X, (0.4, 0.2), method='glasso', graph_rule='or', refit=False, score='mse', **kw)
    assert sorted(st_a) == sorted(st_b) and sorted(sol_a) == sorted(sol_b) and 'SCORE' not in st_a
    for k in ('LAMBDA', 'NLL', 'CV', 'SE', 'TRAIN', 'TEST', 'NNZ', 'THETA'):
        assert np.array_equal(st_a[k], st_b[k], equal_nan=True), k
    for k in ('IX', 'BEST', 'FAILED', 'NOT_PD', 'n_folds', 'rule'):
        assert st_a[k] == st_b[k], k
    for k in sol_a:
        assert np.array_equal(sol_a[k], sol_b[k]), k


def test_arguments_are_refused_on_the_host():
    from gglasso_amd import model_selection as ms, utils
    S, W = mb_ref.case(5, 0), np.ones((5, 5))
    for fn in (utils.host_neighborhood_refit, utils.neighborhood_refit):     # (refused before the library is looked for)
        with pytest.raises(AssertionError, match="square"):
            fn(np.ones((5, 4)), W)
        with pytest.raises(AssertionError, match="W must end in"):
            fn(S, np.ones((4, 4)))
        with pytest.raises(AssertionError, match="with a .M,p,p. stack"):
            fn(np.stack([S, S]), np.ones((3, 5, 5)))
        with pytest.raises(AssertionError, match="threshold"):
            fn(S, W, t=-1.0)
        with pytest.raises(AssertionError, match="threshold"):
            fn(S, W, t=np.inf)
        with pytest.raises(AssertionError, match="S_test must have the shape"):
            fn(S, W, S_test=np.ones((4, 4)))
        bad = S.copy()
        bad[1, 2] = np.nan
        with pytest.raises(ValueError, match=r"matrix 0: the entry \(1, 2\) is not finite"):
            fn(bad, W)
        bad = S.copy()
        bad[3, 3] = 0.0
        with pytest.raises(ValueError, match="matrix 0, variable 3: the diagonal entry"):
            fn(bad, W)
        with pytest.raises(AssertionError, match="p <= 2048"):
            fn(np.eye(2049), np.zeros((2049, 2049)))
    X = mb_ref.stars_data(p=5, N=40)
    for kw, msg in ((dict(method='tiger'), "method"), (dict(method='mb', graph_rule='raw'), "graph_rule"),
                    (dict(method='mb', score='nll'), "score"), (dict(method='mb', t=-1.0), "threshold"),
                    (dict(method='mb', rule='best'), "rule")):
        with pytest.raises(ValueError, match=msg):
            ms.cv_search(X, (0.4, 0.2), n_folds=2, **kw)


def test_entry_points_are_wired():
    from gglasso_amd import _lib, build, utils
    from gglasso_amd.solver import HipEngine
    names = ("ggl_mb_refit_limits", "ggl_neighborhood_refit", "ggl_neighborhood_cv")
    assert all(n in _lib.EXPORTS for n in names)
    assert "mb_refit.hip" in build.SOURCES and hasattr(HipEngine, "neighborhood_cv")
    assert callable(utils.neighborhood_refit) and callable(utils.neighborhood_precision)
