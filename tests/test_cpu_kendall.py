"""Rank correlation, host side (no GPU): the test reference against scipy, dense ranks, and the drivers
(``stars_search(correlation='kendall')``, ``glasso_problem.from_data(correlation='kendall')``) on their host route with the
batch's array work done by the test-only oracle engine."""
import warnings

import numpy as np
import pytest

from kendall_ref import counts_ref, make_data, skeptic_ref, tau_ref

LAM = [0.5, 0.3, 0.15]


def test_reference_tau_is_scipys_tau_b():
    stats = pytest.importorskip("scipy.stats")
    for kind, p, N in (('continuous', 6, 40), ('tied', 6, 40), ('tied', 5, 17)):
        X = make_data(p, N, kind)
        T = tau_ref(counts_ref(X))
        for i in range(p):
            for j in range(p):
                # both divide the same integers: C - D by sqrt((n0 - n1) (n0 - n2))
                assert abs(T[i, j] - stats.kendalltau(X[i], X[j], variant='b').statistic) <= 1e-14, (kind, i, j)


def test_counts_reference_properties():
    X = make_data(7, 33, 'tied')
    G = counts_ref(X)
    assert G.dtype == np.int64 and np.array_equal(G, G.T)
    n0 = 33 * 32 // 2
    for i in range(7):
        _, c = np.unique(X[i], return_counts=True)
        assert G[i, i] == n0 - int(np.sum(c * (c - 1) // 2))
    C = counts_ref(make_data(7, 33, 'constant'))
    assert not C[3].any() and not C[:, 3].any()


def test_dense_ranks_give_the_same_counts():
    from gglasso_amd import utils
    for kind in ('continuous', 'tied', 'constant'):
        X = make_data(9, 50, kind) * 3.7 - 1.0
        R = utils.dense_ranks(X)
        assert R.dtype == np.int32 and R.shape == X.shape and R.min() == 0 and R.max() < 50
        for i in range(9):
            assert R[i].max() == len(np.unique(X[i])) - 1
        assert np.array_equal(counts_ref(R), counts_ref(X)), kind
        assert np.array_equal(utils.dense_ranks(np.exp(X)), R)
    for bad in (np.nan, np.inf, -np.inf):
        Y = X.copy()
        Y[2, 5] = bad
        with pytest.raises(AssertionError, match="finite"):
            utils.dense_ranks(Y)


def test_host_fallback_counts_are_the_reference():
    from gglasso_amd import utils
    X = make_data(8, 40, 'tied')
    assert np.array_equal(utils.host_kendall_counts(X), counts_ref(X))
    assert np.array_equal(utils.host_kendall_counts(X, chunk=100), counts_ref(X))          # several chunks of a-samples
    idx = np.array([np.arange(40)[::-1], np.r_[np.arange(20), np.arange(20)]])             # reversed; every index twice
    G = utils.host_kendall_counts(X, idx)
    for r in range(2):
        assert np.array_equal(G[r], counts_ref(X[:, idx[r]]))
    assert np.array_equal(utils.host_skeptic_correlation(X), skeptic_ref(counts_ref(X)))
    with pytest.raises(AssertionError, match="constant"):
        utils.host_skeptic_correlation(make_data(8, 40, 'constant'))


@pytest.fixture()
def on_host(monkeypatch):
    import problem_helpers
    problem_helpers.on_host(monkeypatch)


def kendall_problem():
    p, N, B = 8, 40, 3
    Th = np.eye(p)
    Th[np.arange(p - 1), np.arange(1, p)] = Th[np.arange(1, p), np.arange(p - 1)] = 0.4
    X = np.linalg.cholesky(np.linalg.inv(Th)) @ np.random.default_rng(11).standard_normal((p, N))
    X = np.exp(X)                                       # not Gaussian any more; the ranks do not notice
    idx = np.stack([np.sort(np.random.default_rng([5, r]).choice(N, 30, replace=False)) for r in range(B)])
    return X, idx


def test_stars_search_kendall_on_the_host_route(on_host):
    from gglasso_amd import model_selection as ms, solver
    X, idx = kendall_problem()
    with warnings.catch_warnings():
        warnings.simplefilter("ignore", RuntimeWarning)
        sol, st = ms.stars_search(X, LAM, indices=idx, beta=0.1, correlation='kendall', store_all=True)
        sol_log, st_log = ms.stars_search(np.log(X), LAM, indices=idx, beta=0.1, correlation='kendall')
        sol_p, st_p = ms.stars_search(X, LAM, indices=idx, beta=0.1, correlation=None, store_all=True)
    p, B = 8, 3
    # the statistics are those of the batch solved on the reference's skeptic matrices
    S = np.stack([skeptic_ref(counts_ref(X[:, idx[r]])) for r in range(B)])
    eye = np.eye(p)
    for l, lam in enumerate(st['LAMBDA']):
        for r in range(B):
            one, _ = solver.ADMM_SGL(S[r], lam, eye, X_0=eye, tol=1e-7, rtol=1e-7, verbose=False)
            assert np.abs(one['Theta'] - st['THETA'][l, r]).max() <= 1e-5, (l, r)
    cnt, num = ms._host_edge_counts(st['THETA'], 1e-8)
    assert st['NUM'] == [int(n) for n in num] and np.array_equal(st['COUNTS'], cnt)
    full, _ = solver.ADMM_SGL(skeptic_ref(counts_ref(X)), st['BEST']['lambda1'], eye, X_0=eye, tol=1e-7, rtol=1e-7, verbose=False)
    assert np.abs(full['Theta'] - sol['Theta']).max() <= 1e-5
    # a monotone transform of the data changes nothing at all
    assert st_log['NUM'] == st['NUM'] and st_log['IX'] == st['IX'] and np.array_equal(sol_log['Theta'], sol['Theta'])
    # None is Pearson, as before (counts of its own batch, final fit on the host covariance); and it is another matrix
    assert st_p['NUM'] == [int(n) for n in ms._host_edge_counts(st_p['THETA'], 1e-8)[1]]
    Sr = ms._host_subset_covariances(X, idx, True, False)
    one, _ = solver.ADMM_SGL(Sr[1], st_p['LAMBDA'][0], eye, X_0=eye, tol=1e-7, rtol=1e-7, verbose=False)
    assert np.abs(one['Theta'] - st_p['THETA'][0, 1]).max() <= 1e-5
    Sp = ms._host_subset_covariances(X, np.arange(40)[None], True, False)[0]
    ref, _ = solver.ADMM_SGL(Sp, st_p['BEST']['lambda1'], eye, X_0=eye, tol=1e-7, rtol=1e-7, verbose=False)
    assert np.array_equal(ref['Theta'], sol_p['Theta'])
    assert not np.array_equal(sol_p['Theta'], sol['Theta'])
    for kw in (dict(center=False), dict(scale=True)):
        with pytest.raises(AssertionError, match="defaults"):
            ms.stars_search(X, LAM, indices=idx, correlation='kendall', **kw)
    with pytest.raises(AssertionError, match="correlation must be"):
        ms.stars_search(X, LAM, indices=idx, correlation='spearman')


def test_from_data_kendall_on_the_host_route(on_host):
    from gglasso_amd import glasso_problem
    X, idx = kendall_problem()
    S = skeptic_ref(counts_ref(X))
    P = glasso_problem.from_data(X, correlation='kendall', reg_params={'lambda1': 0.2})
    assert np.array_equal(P.S, S) and P.N == 40
    P.solve()
    Q = glasso_problem(S, 40, reg_params={'lambda1': 0.2})
    Q.solve()
    assert np.array_equal(P.solution.precision_, Q.solution.precision_)
    # stack and list / dict inputs: one matrix per instance
    X2 = np.stack([X, X[::-1] ** 2])
    P2 = glasso_problem.from_data(X2, correlation='kendall', reg="GGL")
    assert P2.S.shape == (2, 8, 8) and np.array_equal(P2.S[0], S) and np.array_equal(P2.S[1], S[::-1, ::-1])
    ij = np.array([(i, j) for j in range(5) for i in range(j)])               # the pairs of variables 0..4, in both instances
    G = np.stack([np.repeat(ij[:, :1], 2, axis=1), np.repeat(ij[:, 1:], 2, axis=1)]).astype(int)
    P3 = glasso_problem.from_data([X, X[:5, :30]], correlation='kendall', G=G)
    assert np.array_equal(P3.S[0], S) and np.array_equal(P3.S[1], skeptic_ref(counts_ref(X[:5, :30])))
    # None is what it was
    P0 = glasso_problem.from_data(X, correlation=None)
    assert np.abs(P0.S - np.cov(X, bias=True)).max() <= 1e-12 * np.abs(P0.S).max()
    with pytest.raises(AssertionError, match="default"):
        glasso_problem.from_data(X, correlation='kendall', center=False)
    # stability selection passes the choice on
    from gglasso_amd import model_selection as ms
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        P.stability_selection({'lambda1_range': np.array(LAM)}, n_subsamples=3, subsample_size=30, seed=5, beta=0.1)
        sol, st = ms.stars_search(X, LAM, n_subsamples=3, subsample_size=30, seed=5, beta=0.1, correlation='kendall')
    assert P.modelselect_stats['NUM'] == st['NUM'] and np.array_equal(P.solution.precision_, sol['Theta'])


def test_new_entry_points_are_declared():
    import os
    from gglasso_amd import _lib
    header = open(os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "include", "ggl_hip.h")).read()
    for name in ("ggl_kendall_counts", "ggl_kendall_skeptic", "ggl_set_S_from_kendall"):
        assert name in _lib.EXPORTS and f"int {name}(" in header
    assert "#define GGL_VERSION 300" in header and _lib.ABI_VERSION == 300
