"""Joint neighbourhood selection without a GPU: the numpy twin (utils.host_joint_neighborhood_selection) against the
longdouble comparison value and the derived bounds of mbj_ref, the identities that tie it to the single-problem lasso, the
grid search's score and choice, and the front end (glasso_problem.joint_neighborhood_selection) with its refusals."""
import warnings

import numpy as np
import pytest

import mb_ref
import mbj_ref as ref

TOL = 1e-7
SHAPES = [(p, K) for p in (1, 2, 3, 5, 17, 65) for K in (1, 2, 3, 4)]


def _twin(S, om, l1, l2, **kw):
    from gglasso_amd import utils
    W, info = utils.host_joint_neighborhood_selection(S, [l1], [l2], rule='raw', instance_weights=om, tol=TOL, return_info=True, **kw)
    return W[0, 0], info['RESVAR'][0, 0], info['STATUS'][0, 0], info


@pytest.mark.parametrize("kind", ("corr", "scaled"))
@pytest.mark.parametrize("p,K", SHAPES)
def test_twin_against_the_comparison_value(p, K, kind):
    S, om = ref.stack(p, K, kind)
    for ip, (l1, l2) in enumerate(ref.PAIRS):
        coef, resvar, status, _ = _twin(S, om, l1, l2)
        ref.check_case(p, K, kind, ip, coef, resvar, status, TOL, "twin")


@pytest.mark.parametrize("p,K", ((5, 2), (17, 3)))
def test_twin_with_unequal_instance_weights(p, K):
    S, om = ref.stack(p, K, 'weighted')
    assert om is not None and len(set(om)) == K
    for ip, (l1, l2) in enumerate(ref.PAIRS):
        coef, resvar, status, _ = _twin(S, om, l1, l2)
        ref.check_case(p, K, 'weighted', ip, coef, resvar, status, TOL, "twin")


def _node_norm(a):
    """(p,): per node (last axis) the 2-norm over everything else."""
    a = np.asarray(a, dtype=np.float64)
    return np.sqrt((a * a).reshape(-1, a.shape[-1]).sum(axis=0))


def _lasso(S, lam):
    from gglasso_amd import utils
    W, info = utils.host_neighborhood_selection(S, [lam], rule='raw', tol=TOL, return_info=True)
    assert np.all(info['STATUS'] == 0)
    return W[0], mb_ref.residual_bound(S, W, TOL)[0]


@pytest.mark.parametrize("p", (5, 17))
def test_identities(p):
    """Each within the sum of the two distance bounds (residual bound / strong convexity), not bitwise."""
    # K = 1 is the lasso at lambda1 + lambda2
    S, _ = ref.stack(p, 1, 'scaled')
    l1, l2 = 0.05, 0.1
    coef, _, status, _ = _twin(S, None, l1, l2)
    assert np.all(status == 0)
    lasso, lb = _lasso(S[0], l1 + l2)
    mu = ref.strong_convexity(S, None)
    room = (_node_norm(ref.residual_bound(S, None, coef, l2, TOL)) + _node_norm(lb)) / mu
    assert np.all(_node_norm(coef[0] - lasso) <= room), (_node_norm(coef[0] - lasso) / room).max()
    # lambda2 = 0 is the K separate paths
    S, _ = ref.stack(p, 3, 'scaled')
    coef, _, status, _ = _twin(S, None, 0.1, 0.0)
    assert np.all(status == 0)
    each = [_lasso(S[k], 0.1) for k in range(3)]
    mu = ref.strong_convexity(S, None)
    room = (_node_norm(ref.residual_bound(S, None, coef, 0.0, TOL)) + _node_norm(np.stack([b for _, b in each]))) / mu
    diff = _node_norm(coef - np.stack([c for c, _ in each]))
    assert np.all(diff <= room), (diff / room).max()
    # K identical instances with lambda1 = 0 are the lasso at lambda2 / sqrt(K)
    K = 4
    S1 = mb_ref.case(p, 3)
    S = np.stack([S1] * K)
    coef, _, status, _ = _twin(S, None, 0.0, 0.3)
    assert np.all(status == 0)
    lasso, lb = _lasso(S1, 0.3 / np.sqrt(K))
    mu = ref.strong_convexity(S, None)
    room = (_node_norm(ref.residual_bound(S, None, coef, 0.3, TOL)) + np.sqrt(K) * _node_norm(lb)) / mu
    diff = _node_norm(coef - lasso[None])
    assert np.all(diff <= room), (diff / room).max()


def test_supports():
    # lambda1 = 0: the K supports of every (node, variable) coincide exactly
    for kind in ('corr', 'scaled'):
        S, om = ref.stack(17, 4, kind)
        coef, _, status, _ = _twin(S, om, 0.0, 0.15)
        assert np.all(status == 0) and (coef != 0).any()
        assert np.array_equal(coef != 0, np.broadcast_to((coef != 0)[0], coef.shape))
    # lambda1 > 0: some active group has a zero member
    S, om = ref.stack(17, 4, 'corr')
    coef, _, status, _ = _twin(S, om, 0.1, 0.05)
    nz = coef != 0
    assert np.all(status == 0) and np.any(nz.any(axis=0) & ~nz.all(axis=0))


@pytest.mark.parametrize("kind", ("corr", "weighted"))
def test_the_null_model(kind):
    """lambda2 >= max ||soft(w s_ij, lambda1)||: exact zeros, status 0, no sweep, tau^2 = S_jj."""
    S, om = ref.stack(17, 3, kind)
    w = np.ones(3) if om is None else om
    l1 = 0.05
    sg = np.maximum(np.abs(w[:, None, None] * S) - l1, 0.0)
    nrm = np.sqrt((sg * sg).sum(axis=0))
    nrm[np.arange(17), np.arange(17)] = 0.0
    coef, resvar, status, info = _twin(S, om, l1, float(nrm.max()))
    assert np.all(coef == 0) and np.all(status == 0) and np.all(info['SWEEPS'] == 0)
    assert np.array_equal(resvar, np.diagonal(S, axis1=1, axis2=2))
    coef, _, _, _ = _twin(S, om, l1, float(nrm.max()) * 0.98)
    assert (coef != 0).any()


def test_shapes_rules_and_refit():
    from gglasso_amd import utils
    S, _ = ref.stack(5, 3, 'scaled')
    l1, l2 = (0.05, 0.2, 0.1), (0.1, 0.02)
    raw, info = utils.host_joint_neighborhood_selection(S, l1, l2, rule='raw', return_info=True)
    assert raw.shape == (3, 2, 3, 5, 5) and np.array_equal(info['LAMBDA1'], (0.2, 0.1, 0.05)) and np.array_equal(info['LAMBDA2'], l2)
    assert info['RESVAR'].shape == (3, 2, 3, 5) and info['STATUS'].shape == info['SWEEPS'].shape == info['NEWTON'].shape == (3, 2, 5)
    for rule in ('and', 'or'):
        W, inf = utils.host_joint_neighborhood_selection(S, l1, l2, rule=rule, refit=True, return_info=True)
        assert np.array_equal(W, mb_ref.and_or(raw, rule)) and np.array_equal(W, np.swapaxes(W, -1, -2))
        for a in range(3):
            for c in range(2):
                rf = utils.host_neighborhood_refit(S, W[a, c])
                assert np.array_equal(inf['REFIT_COEF'][a, c], rf['COEF']) and np.array_equal(inf['REFIT_RESVAR'][a, c], rf['RESVAR'])
                assert np.array_equal(inf['DEGREE'][a, c], rf['DEGREE']) and np.array_equal(inf['REFIT_STATUS'][a, c], rf['STATUS'])
    # a chain is walked with warm starts: its leading part does not depend on what follows, a chain not on the others
    lead = utils.host_joint_neighborhood_selection(S, l1[1:2], l2[1:], rule='raw')
    assert np.array_equal(lead[0, 0], raw[0, 1])
    Th, lmin = utils.joint_neighborhood_precision(raw[2, 0], info['RESVAR'][2, 0])
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        for k in range(3):
            one = utils.neighborhood_precision(raw[2, 0, k], info['RESVAR'][2, 0, k])
            assert np.array_equal(Th[k], one[0]) and lmin[k] == one[1]


def _direct_score(tau, deg, N, p, method, gamma):
    total = 0.0
    for k in range(tau.shape[0]):
        for j in range(p):
            pen = {'eBIC': np.log(N[k]) + 2 * gamma * np.log(p - 1), 'BIC': np.log(N[k]), 'AIC': 2.0}[method]
            total += N[k] * np.log(tau[k, j]) + deg[k, j] * pen
    return total


def test_search_score_and_choice(monkeypatch):
    from gglasso_amd import model_selection as ms, utils
    S, _ = ref.stack(17, 3, 'scaled')
    N = np.array([80, 120, 100])
    l1, l2 = (0.3, 0.15, 0.08, 0.04), (0.2, 0.05)
    W, info = utils.host_joint_neighborhood_selection(S, l1, l2, refit=True, return_info=True)
    for method, gamma in (('eBIC', 0.1), ('eBIC', 0.5), ('BIC', 0.3), ('AIC', 0.0)):
        sol, st = ms.joint_neighborhood_search(S, N, l1, l2, method=method, gamma=gamma, host=True)
        want = np.array([[_direct_score(info['REFIT_RESVAR'][a, c], info['DEGREE'][a, c], N, 17, method, gamma) for c in range(2)]
                         for a in range(4)])
        assert np.allclose(st['SCORE'], want, rtol=1e-13, atol=0) and st['IX'] == tuple(np.unravel_index(np.argmin(want), want.shape))
        i1, i2 = st['IX']
        assert st['BEST'] == {'lambda1': sorted(l1)[::-1][i1], 'lambda2': l2[i2]}
        # the chosen point's further call returns that point's part of the grid call
        assert np.array_equal(sol['W'], W[i1, i2]) and np.array_equal(sol['coef'], info['REFIT_COEF'][i1, i2])
        assert np.array_equal(sol['resvar'], info['REFIT_RESVAR'][i1, i2])
        assert np.array_equal(sol['adjacency'], (np.abs(W[i1, i2]) >= 1e-8)) and sol['adjacency'].dtype == bool
        assert np.array_equal(sol['common_adjacency'], sol['adjacency'].all(axis=0))
        assert sol['precision'].shape == (3, 17, 17) and np.array_equal(sol['precision'], np.swapaxes(sol['precision'], 1, 2))
    # one number for N
    assert np.allclose(ms.joint_neighborhood_search(S, 100, l1, l2, host=True)[1]['SCORE'],
                       ms.joint_neighborhood_search(S, [100] * 3, l1, l2, host=True)[1]['SCORE'], rtol=0, atol=0)
    # a point with a node that did not finish scores NaN and is never chosen
    sol, st = ms.joint_neighborhood_search(S, N, l1, l2, host=True)
    i1, i2 = st['IX']
    run = utils._joint_run

    def spoiled(*a, **kw):
        out = run(*a, **kw)
        if out['INFO'].shape[0] == 4:
            out['INFO'][i1, i2, 3, 1] = 1
        return out
    monkeypatch.setattr(utils, "_joint_run", spoiled)
    _, st2 = ms.joint_neighborhood_search(S, N, l1, l2, host=True)
    assert np.isnan(st2['SCORE'][i1, i2]) and st2['IX'] != (i1, i2) and np.isfinite(st2['SCORE'][st2['IX']])
    assert st2['SCORE'][st2['IX']] == np.nanmin(st2['SCORE'])

    def refit_spoiled(*a, **kw):
        out = run(*a, **kw)
        if out['INFO'].shape[0] == 4:
            out['REFIT_INFO'][..., 1] = 1
        return out
    monkeypatch.setattr(utils, "_joint_run", refit_spoiled)
    with pytest.raises(ValueError, match="no grid point"):
        ms.joint_neighborhood_search(S, N, l1, l2, host=True)


def test_front_end_and_its_refusals(monkeypatch):
    import problem_helpers
    from gglasso_amd import model_selection as ms, solver
    from gglasso_amd.problem import glasso_problem
    problem_helpers.on_host(monkeypatch)
    assert not hasattr(solver.ENGINE, "neighborhood_stability")
    S, _ = ref.stack(17, 3, 'corr')
    N = [80, 120, 100]
    l1, l2 = (0.3, 0.15, 0.08), (0.2, 0.05)
    P = glasso_problem(S.copy(), N, reg='GGL')
    P.joint_neighborhood_selection(l1, l2, rule='or', method='eBIC', gamma=0.2)
    sol, st = ms.joint_neighborhood_search(S, N, l1, l2, rule='or', method='eBIC', gamma=0.2, host=True)
    assert np.array_equal(P.solution.precision_, sol['precision']) and np.array_equal(P.solution.adjacency_, sol['adjacency'].astype(int))
    assert P.reg_params['lambda1'] == st['BEST']['lambda1'] and P.reg_params['lambda2'] == st['BEST']['lambda2']
    assert P.modelselect_stats['IX'] == st['IX'] and np.array_equal(P.modelselect_stats['SCORE'], st['SCORE'])
    assert sorted(P.neighborhood_) == sorted(sol) and np.array_equal(P.neighborhood_['common_adjacency'], sol['common_adjacency'])
    # with do_scaling the method works on the correlations
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        Ss, _ = ref.stack(17, 3, 'scaled')
        Q = glasso_problem(Ss.copy(), N, reg='GGL', do_scaling=True)
        Q.joint_neighborhood_selection(l1, l2)
        sol_q, st_q = ms.joint_neighborhood_search(Q.S, N, l1, l2, host=True)
    assert np.array_equal(Q.solution.precision_, sol_q['precision']) and Q.modelselect_stats['IX'] == st_q['IX']
    # refused, by name
    with pytest.raises(AssertionError, match="this is a single one"):
        glasso_problem(S[0].copy(), 80, reg=None).joint_neighborhood_selection(l1, l2)
    with pytest.raises(AssertionError, match="non-conforming"):
        glasso_problem([S[0].copy(), S[1].copy()], [80, 90], reg='GGL', G=_trivial_G(17, 2)).joint_neighborhood_selection(l1, l2)
    with pytest.raises(AssertionError, match="latent"):
        glasso_problem(S.copy(), N, reg='GGL', latent=True).joint_neighborhood_selection(l1, l2)
    with pytest.raises(AssertionError, match="lambda1_mask"):
        glasso_problem(S.copy(), N, reg='GGL', reg_params={'lambda1_mask': np.ones((17, 17))}).joint_neighborhood_selection(l1, l2)
    with pytest.raises(AssertionError, match="reg='FGL'"):
        glasso_problem(S.copy(), N, reg='FGL').joint_neighborhood_selection(l1, l2)
    with pytest.raises(AssertionError, match="rule"):
        P.joint_neighborhood_selection(l1, l2, rule='raw')
    # the single-problem method still refuses a multiple problem as it did
    X = mb_ref.stars_data()
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        with pytest.raises(AssertionError, match="Neighbourhood selection is implemented for Single Graphical Lasso problems only."):
            glasso_problem.from_data([X, X], reg='GGL').neighborhood_selection(mb_ref.GRID)


def _trivial_G(p, K):
    """The bookkeeping array of K instances that share all p variables (a list input is a non-conforming problem)."""
    ij = np.array([(i, j) for j in range(p) for i in range(j)])
    return np.stack([np.repeat(ij[:, 0][:, None], K, axis=1), np.repeat(ij[:, 1][:, None], K, axis=1)]).astype(int)


def test_arguments_are_refused_on_the_host():
    from gglasso_amd import model_selection as ms, utils
    S, _ = ref.stack(5, 2, 'corr')
    for fn in (utils.host_joint_neighborhood_selection, utils.joint_neighborhood_selection):   # (before the library is looked for)
        with pytest.raises(AssertionError, match="K,p,p"):
            fn(S[0], [0.1], [0.1])
        with pytest.raises(AssertionError, match="lambda1 must be non-negative"):
            fn(S, [-0.1], [0.1])
        with pytest.raises(AssertionError, match="lambda2 must be non-negative"):
            fn(S, [0.1], [np.inf])
        with pytest.raises(AssertionError, match="lambda1 . lambda2 must be positive"):
            fn(S, [0.1, 0.0], [0.2, 0.0])
        with pytest.raises(AssertionError, match="rule"):
            fn(S, [0.1], [0.1], rule='xor')
        with pytest.raises(AssertionError, match="refit needs a graph"):
            fn(S, [0.1], [0.1], rule='raw', refit=True)
        with pytest.raises(AssertionError, match="tol"):
            fn(S, [0.1], [0.1], tol=-1.0)
        with pytest.raises(AssertionError, match="max_sweeps"):
            fn(S, [0.1], [0.1], max_sweeps=0)
        with pytest.raises(AssertionError, match="threshold"):
            fn(S, [0.1], [0.1], t=-1.0)
        with pytest.raises(AssertionError, match="one weight per instance"):
            fn(S, [0.1], [0.1], instance_weights=[1.0])
        with pytest.raises(ValueError, match=r"instance_weights\[1\] = 0.0"):
            fn(S, [0.1], [0.1], instance_weights=[1.0, 0.0])
        bad = S.copy()
        bad[1, 2, 3] = bad[1, 3, 2] = np.nan
        with pytest.raises(ValueError, match=r"instance 1: the entry \(2, 3\) is not finite"):
            fn(bad, [0.1], [0.1])
        bad = S.copy()
        bad[0, 4, 4] = -1.0
        with pytest.raises(ValueError, match="instance 0, variable 4: the diagonal entry"):
            fn(bad, [0.1], [0.1])
        bad = S.copy()
        bad[1, 0, 3] = np.nextafter(bad[1, 0, 3], 1.0)
        with pytest.raises(ValueError, match=r"instance 1 is not bitwise symmetric: the entries \(0, 3\) and \(3, 0\)"):
            fn(bad, [0.1], [0.1])
    with pytest.raises(AssertionError, match="method"):
        ms.joint_neighborhood_search(S, 50, [0.1], [0.1], method='CV', host=True)
    with pytest.raises(AssertionError, match="unknown arguments"):
        ms.joint_neighborhood_search(S, 50, [0.1], [0.1], n_folds=3, host=True)
    with pytest.raises(AssertionError, match="N must be"):
        ms.joint_neighborhood_search(S, [50, 60, 70], [0.1], [0.1], host=True)


def test_entry_points_are_wired():
    from gglasso_amd import _lib, build, utils
    from gglasso_amd.problem import glasso_problem
    names = ("ggl_mb_joint_limits", "ggl_neighborhood_joint_path", "ggl_neighborhood_joint_last", "ggl_mb_joint_chunk_budget")
    assert all(n in _lib.EXPORTS for n in names)
    assert "neighborhood_joint.hip" in build.SOURCES and callable(glasso_problem.joint_neighborhood_selection)
    assert callable(utils.mb_joint_limits) and not hasattr(utils, "MB_JOINT_MAX_K")       # the limits are the library's alone
