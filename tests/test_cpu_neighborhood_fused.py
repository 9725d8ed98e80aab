"""Fused joint neighbourhood selection without a GPU: the numpy twin (utils.host_fused_neighborhood_selection) against the
longdouble comparison value and the derived bounds of mbf_ref, the identities that tie it to the single-problem lasso and
tell it from the group route, the grid search's tables and choice, and the front end
(glasso_problem.fused_neighborhood_selection) with its refusals."""
import warnings

import numpy as np
import pytest

import mb_ref
import mbf_ref as ref
import mbj_ref

TOL = 1e-7
SHAPES = [(p, K) for p in (1, 2, 3, 5, 17) for K in (1, 2, 3, 5)]


def _twin(S, om, l1, l2, **kw):
    from gglasso_amd import utils
    W, info = utils.host_fused_neighborhood_selection(S, [l1], [l2], rule='raw', instance_weights=om, tol=TOL, return_info=True, **kw)
    assert np.all(info['NEWTON'] == 0)
    return W[0, 0], info['RESVAR'][0, 0], info['STATUS'][0, 0], info


def test_the_scan_against_its_certificate():
    """The longdouble Condat on vectors with ties, jumps and constant runs, lam = 0 included; tv(v, 0) = v, and a lam beyond the
    largest partial sum gives the mean."""
    rng = np.random.default_rng(5)
    for N in (1, 2, 3, 5, 8, 64):
        V = rng.standard_normal((4000, N))
        V[::3] = np.round(V[::3] * 2) / 2
        lam = rng.choice([0.0, 0.1, 0.5, 1.0, 3.0], size=4000)
        X = ref.condat(V, lam)
        lim = 64 * ref.EPS_LD * (np.abs(V).max(axis=1) + lam) * N
        assert np.all(ref.certificate(V, X, lam) <= lim)
        assert np.array_equal(X[lam == 0], V[lam == 0].astype(ref.LD))
        big = ref.condat(V, np.full(4000, 1e3))
        assert np.all(big == big[:, :1]) and np.allclose(big[:, 0].astype(float), V.mean(axis=1), rtol=0, atol=1e-12)


@pytest.mark.parametrize("kind", ref.KINDS)
@pytest.mark.parametrize("p,K", SHAPES)
def test_twin_against_the_comparison_value(p, K, kind):
    S, om = ref.stack(p, K, kind)
    assert kind == 'corr' or K == 1 or (len(set(om)) == K and len(set(np.diagonal(S, axis1=1, axis2=2)[:, 0])) == K)
    for ip, (l1, l2) in enumerate(ref.PAIRS):
        coef, resvar, status, _ = _twin(S, om, l1, l2)
        ref.check_case(p, K, kind, ip, coef, resvar, status, TOL, "twin")


def _node_norm(a):
    """(p,): per node (last axis) the 2-norm over everything else."""
    a = np.asarray(a, dtype=np.float64)
    return np.sqrt((a * a).reshape(-1, a.shape[-1]).sum(axis=0))


def _room(S, om, coef, l1, l2):
    """(p,): mbf_ref's distance bound of a twin result, from the BOUND of its residual."""
    return ref.distance_bound(ref.residual_bound(S, om, coef, l1, l2, TOL), *ref.constants(S, om))


def _lasso(S, lam):
    """(coef (p,p) of the single-problem twin, its distance bound (p,))."""
    from gglasso_amd import utils
    W, info = utils.host_neighborhood_selection(S, [lam], rule='raw', tol=TOL, return_info=True)
    assert np.all(info['STATUS'] == 0)
    return W[0], _node_norm(mb_ref.residual_bound(S, W, TOL)[0]) / np.linalg.eigvalsh(S)[0]


@pytest.mark.parametrize("p", (5, 17))
def test_identities(p):
    """Each within the sum of the two distance bounds, not bitwise."""
    # K = 1 is neighborhood_selection at lambda1, whatever lambda2
    S, _ = mbj_ref.stack(p, 1, 'scaled')
    coef, _, status, _ = _twin(S, None, 0.05, 0.3)
    assert np.all(status == 0)
    lasso, lb = _lasso(S[0], 0.05)
    room = _room(S, None, coef, 0.05, 0.3) + lb
    assert np.all(_node_norm(coef[0] - lasso) <= room), (_node_norm(coef[0] - lasso) / room).max()
    # lambda2 = 0 is the K separate lassos
    S, _ = mbj_ref.stack(p, 3, 'scaled')
    coef, _, status, _ = _twin(S, None, 0.1, 0.0)
    assert np.all(status == 0)
    each = [_lasso(S[k], 0.1) for k in range(3)]
    room = _room(S, None, coef, 0.1, 0.0) + np.sqrt(sum(b * b for _, b in each))
    diff = _node_norm(coef - np.stack([c for c, _ in each]))
    assert np.all(diff <= room), (diff / room).max()
    # K identical instances give the lasso at lambda1 in each
    K, S1 = 4, mb_ref.case(p, 3)
    S = np.stack([S1] * K)
    coef, _, status, _ = _twin(S, None, 0.08, 0.3)
    assert np.all(status == 0)
    lasso, lb = _lasso(S1, 0.08)
    room = _room(S, None, coef, 0.08, 0.3) + np.sqrt(K) * lb
    diff = _node_norm(coef - lasso[None])
    assert np.all(diff <= room), (diff / room).max()
    # reversing the instance order reverses the solution
    S, om = ref.stack(p, 5, 'weighted')
    fwd, _, s1, _ = _twin(S, om, 0.05, 0.1)
    bwd, _, s2, _ = _twin(np.ascontiguousarray(S[::-1]), om[::-1].copy(), 0.05, 0.1)
    assert np.all(s1 == 0) and np.all(s2 == 0) and (fwd != 0).any()
    room = 2 * _room(S, om, fwd, 0.05, 0.1)
    diff = _node_norm(fwd - bwd[::-1])
    assert np.all(diff <= room), (diff / room).max()


@pytest.mark.parametrize("p", (5, 17))
def test_a_large_lambda2_is_the_lasso_on_the_weighted_sum(p):
    K, l1, l2 = 3, 0.05, 10.0
    S, om = ref.stack(p, K, 'weighted')
    B = ref.solve(S, om, ((l1, l2),))[0]
    assert (B != 0).any() and np.all(B == B[:1]), "the comparison value is not constant along k"
    assert float(ref.group_norm(ref.residual(S, om, B, l1, l2)[0]).max()) <= 1e-15
    coef, _, status, _ = _twin(S, om, l1, l2)
    assert np.all(status == 0)
    M = np.einsum('k,kij->ij', om, S)
    M = np.triu(M) + np.triu(M, 1).T
    lasso, lb = _lasso(M, K * l1)
    room = _room(S, om, coef, l1, l2) + np.sqrt(K) * lb
    diff = _node_norm(coef - lasso[None])
    assert np.all(diff <= room), (diff / room).max()


def test_the_order_of_the_instances_matters_to_the_fused_route_only():
    """A permutation that is no reversal: the group route's solution is permuted with the instances (within its bounds), the
    fused route's is not (by far more than its bounds)."""
    from gglasso_amd import utils
    p, K, l1, l2, perm = 17, 3, 0.02, 0.1, [0, 2, 1]
    S, _ = ref.stack(p, K, 'corr')
    Sp = np.ascontiguousarray(S[perm])
    a, _, s1, _ = _twin(S, None, l1, l2)
    b, _, s2, _ = _twin(Sp, None, l1, l2)
    assert np.all(s1 == 0) and np.all(s2 == 0)
    room = _room(S, None, a, l1, l2) + _room(Sp, None, b, l1, l2)
    assert np.max(_node_norm(a[perm] - b) / room) > 10                           # (any factor above 1 proves two different points)
    ga = utils.host_joint_neighborhood_selection(S, [l1], [l2], rule='raw', tol=TOL)[0, 0]
    gb = utils.host_joint_neighborhood_selection(Sp, [l1], [l2], rule='raw', tol=TOL)[0, 0]
    mu = mbj_ref.strong_convexity(S, None)
    groom = (_node_norm(mbj_ref.residual_bound(S, None, ga, l2, TOL)) + _node_norm(mbj_ref.residual_bound(Sp, None, gb, l2, TOL))) / mu
    assert np.all(_node_norm(ga[perm] - gb) <= groom)
    assert np.max(_node_norm(a - ga) / room) > 10                                # and the two routes differ


def test_the_null_model_and_the_screen():
    """max_k |w_k s_ij| <= lambda1: exact zeros, status 0, no sweep, tau^2 = S_jj -- and the exact screen admits nobody where
    the cheap test alone would: a lambda2 that holds back what lambda1 lets through."""
    S, om = ref.stack(17, 3, 'weighted')
    g = np.abs(om[:, None, None] * S)
    g[:, np.arange(17), np.arange(17)] = 0.0
    coef, resvar, status, info = _twin(S, om, float(g.max()), 0.0)
    assert np.all(coef == 0) and np.all(status == 0) and np.all(info['SWEEPS'] == 0)
    assert np.array_equal(resvar, np.diagonal(S, axis1=1, axis2=2))
    assert (_twin(S, om, float(g.max()) * 0.9, 0.0)[0] != 0).any()
    # sum_k g_k / K <= lambda1 < max_k |g_k| with a large lambda2: still the null model, no sweep
    l1 = float(np.abs((om[:, None, None] * S).sum(axis=0) - np.diag((om[:, None] * np.diagonal(S, axis1=1, axis2=2)).sum(axis=0))).max()) / 3
    assert l1 < g.max()
    coef, _, status, info = _twin(S, om, l1 * (1 + 1e-12), 10.0)
    assert np.all(coef == 0) and np.all(status == 0) and np.all(info['SWEEPS'] == 0)


def test_shapes_rules_refit_and_status():
    from gglasso_amd import utils
    S, om = ref.stack(5, 3, 'weighted')
    l1, l2 = (0.05, 0.2, 0.1), (0.1, 0.02)
    raw, info = utils.host_fused_neighborhood_selection(S, l1, l2, rule='raw', instance_weights=om, return_info=True)
    assert raw.shape == (3, 2, 3, 5, 5) and np.array_equal(info['LAMBDA1'], (0.2, 0.1, 0.05)) and np.array_equal(info['LAMBDA2'], l2)
    assert info['RESVAR'].shape == (3, 2, 3, 5) and info['STATUS'].shape == info['SWEEPS'].shape == info['NEWTON'].shape == (3, 2, 5)
    for rule in ('and', 'or'):
        W, inf = utils.host_fused_neighborhood_selection(S, l1, l2, rule=rule, instance_weights=om, refit=True, return_info=True)
        assert np.array_equal(W, mb_ref.and_or(raw, rule)) and np.array_equal(W, np.swapaxes(W, -1, -2))
        rf = utils.host_neighborhood_refit(S, W[1, 1])
        assert np.array_equal(inf['REFIT_COEF'][1, 1], rf['COEF']) and np.array_equal(inf['DEGREE'][1, 1], rf['DEGREE'])
    # a chain's leading part does not depend on what follows, a chain not on the others
    lead = utils.host_fused_neighborhood_selection(S, l1[1:2], l2[1:], rule='raw', instance_weights=om)
    assert np.array_equal(lead[0, 0], raw[0, 1])
    # one sweep is a cap: status 1, finite; an overflowing stack is status 2 with NaN columns and diagonal 0
    _, inf = utils.host_fused_neighborhood_selection(S, [0.01], [0.05], rule='raw', instance_weights=om, max_sweeps=1, return_info=True)
    assert np.any(inf['STATUS'] == 1) and set(np.unique(inf['STATUS'])) <= {0, 1}
    big = np.full((2, 3, 3), 1e200)
    big[:, np.arange(3), np.arange(3)] = 1e-200
    out, inf = utils.host_fused_neighborhood_selection(big, [1e-3], [1e-3], rule='raw', max_sweeps=50, return_info=True)
    assert np.all(inf['STATUS'] == 2) and np.all(np.isnan(out[0, 0][:, ~np.eye(3, dtype=bool)])) and np.all(np.diagonal(out[0, 0], axis1=1, axis2=2) == 0)


def test_search_tables_choice_and_changed_edges():
    from gglasso_amd import model_selection as ms, utils
    S, om = ref.stack(17, 3, 'weighted')
    N = np.array([80, 120, 100])
    l1, l2 = (0.3, 0.15, 0.08, 0.04), (0.2, 0.01)
    W, info = utils.host_fused_neighborhood_selection(S, l1, l2, instance_weights=om, refit=True, return_info=True)
    for method, gamma in (('eBIC', 0.1), ('BIC', 0.3), ('AIC', 0.0)):
        sol, st = ms.fused_neighborhood_search(S, N, l1, l2, method=method, gamma=gamma, instance_weights=om, host=True)
        want = ms.joint_neighborhood_score(info['REFIT_RESVAR'], info['DEGREE'], N.astype(float), 17, method, gamma,
                                           np.zeros((4, 2), dtype=bool))
        assert np.array_equal(st['SCORE'], want) and st['IX'] == tuple(np.unravel_index(np.argmin(want), want.shape))
        i1, i2 = st['IX']
        assert st['BEST'] == {'lambda1': sorted(l1)[::-1][i1], 'lambda2': l2[i2]} and np.all(st['NEWTON'] == 0)
        assert np.array_equal(sol['W'], W[i1, i2]) and np.array_equal(sol['coef'], info['REFIT_COEF'][i1, i2])
        adj = (np.abs(W[i1, i2]) >= 1e-8) & ~np.eye(17, dtype=bool)
        assert np.array_equal(sol['adjacency'], adj)
        want_ce = [int(np.triu(adj[k + 1] != adj[k], 1).sum()) for k in range(2)]
        assert sol['changed_edges'].shape == (2,) and sol['changed_edges'].tolist() == want_ce
    # the group route's search carries no changed_edges: its instances have no order
    assert 'changed_edges' not in ms.joint_neighborhood_search(S, N, l1, l2, host=True)[0]
    # a larger lambda2 changes fewer edges between consecutive graphs (at one lambda1, through the supports alone)
    ce = [ms.fused_neighborhood_search(S, N, [0.08], [b], host=True)[0]['changed_edges'].sum() for b in (0.0, 0.5)]
    assert ce[1] < ce[0]


def test_front_end_and_its_refusals(monkeypatch):
    import problem_helpers
    from gglasso_amd import model_selection as ms
    from gglasso_amd.problem import glasso_problem
    problem_helpers.on_host(monkeypatch)
    S, _ = ref.stack(17, 3, 'corr')
    N = [80, 120, 100]
    l1, l2 = (0.3, 0.15, 0.08), (0.2, 0.05)
    P = glasso_problem(S.copy(), N, reg='FGL')
    P.fused_neighborhood_selection(l1, l2, rule='or', method='eBIC', gamma=0.2)
    sol, st = ms.fused_neighborhood_search(S, N, l1, l2, rule='or', method='eBIC', gamma=0.2, host=True)
    assert np.array_equal(P.solution.precision_, sol['precision']) and np.array_equal(P.solution.adjacency_, sol['adjacency'].astype(int))
    assert P.reg_params['lambda1'] == st['BEST']['lambda1'] and P.reg_params['lambda2'] == st['BEST']['lambda2']
    assert P.modelselect_stats['IX'] == st['IX'] and np.array_equal(P.modelselect_stats['SCORE'], st['SCORE'])
    assert sorted(P.neighborhood_) == sorted(sol) and np.array_equal(P.neighborhood_['changed_edges'], sol['changed_edges'])
    # refused, by name
    with pytest.raises(AssertionError, match="this is a single one"):
        glasso_problem(S[0].copy(), 80, reg=None).fused_neighborhood_selection(l1, l2)
    with pytest.raises(AssertionError, match="latent"):
        glasso_problem(S.copy(), N, reg='FGL', latent=True).fused_neighborhood_selection(l1, l2)
    with pytest.raises(AssertionError, match="lambda1_mask"):
        glasso_problem(S.copy(), N, reg='FGL', reg_params={'lambda1_mask': np.ones((17, 17))}).fused_neighborhood_selection(l1, l2)
    with pytest.raises(AssertionError, match=r"reg='FGL' only, this problem has reg='GGL' \(see joint_neighborhood_selection\)"):
        glasso_problem(S.copy(), N, reg='GGL').fused_neighborhood_selection(l1, l2)
    Q = glasso_problem(S.copy(), N, reg='FGL')
    Q.reg = None
    with pytest.raises(AssertionError, match="reg='FGL' only, this problem has reg=None"):
        Q.fused_neighborhood_selection(l1, l2)
    with pytest.raises(AssertionError, match="rule"):
        P.fused_neighborhood_selection(l1, l2, rule='raw')
    # the group method keeps refusing FGL, and now points here
    with pytest.raises(AssertionError, match=r"reg='FGL'.*fused_neighborhood_selection"):
        P.joint_neighborhood_selection(l1, l2)


def test_arguments_are_refused_on_the_host():
    from gglasso_amd import model_selection as ms, utils
    S, _ = ref.stack(5, 2, 'corr')
    for fn in (utils.host_fused_neighborhood_selection, utils.fused_neighborhood_selection):    # (before the library is looked for)
        with pytest.raises(AssertionError, match="fused_neighborhood_selection needs a .K,p,p"):
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
        with pytest.raises(ValueError, match=r"fused_neighborhood_selection: S of instance 1: the entry \(2, 3\) is not finite"):
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
        ms.fused_neighborhood_search(S, 50, [0.1], [0.1], method='CV', host=True)
    with pytest.raises(AssertionError, match="fused_neighborhood_search: unknown arguments"):
        ms.fused_neighborhood_search(S, 50, [0.1], [0.1], n_folds=3, host=True)
    with pytest.raises(AssertionError, match="N must be"):
        ms.fused_neighborhood_search(S, [50, 60, 70], [0.1], [0.1], host=True)


def test_entry_points_are_wired():
    from gglasso_amd import _lib, build, utils
    from gglasso_amd.problem import glasso_problem
    names = ("ggl_mb_fused_limits", "ggl_neighborhood_fused_path", "ggl_neighborhood_fused_last", "ggl_dev_mb_fused_bench")
    assert all(n in _lib.EXPORTS for n in names)
    assert "neighborhood_fused.hip" in build.SOURCES and callable(glasso_problem.fused_neighborhood_selection)
    assert callable(utils.mb_fused_limits) and not hasattr(utils, "MB_FUSED_MAX_K")       # the limits are the library's alone
