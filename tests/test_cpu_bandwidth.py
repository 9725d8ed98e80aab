"""The numpy twins of the bandwidth search (utils.host_cholesky_predict, utils.host_loo_bandwidth_scores) against the
longdouble reference at the bounds derived in tests/chol_ref.py, and the search itself (model_selection.bandwidth_search,
glasso_problem.from_time_series_cv) on the host engine."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import chol_ref as cr  # noqa: E402
import problem_helpers as ph  # noqa: E402

PS = [1, 2, 15, 16, 17, 31, 32, 33, 63, 64, 65, 129]


@pytest.fixture()
def host(monkeypatch):
    ph.on_host(monkeypatch)
    from gglasso_amd import model_selection
    return model_selection


@pytest.fixture(scope="module")
def case_a():
    """seed -> (X, X stationary, (h, stats) of the search on X, (h, stats) on the stationary series), computed once"""
    from gglasso_amd import model_selection, solver
    import problem_helpers
    keep = solver.ENGINE
    solver.ENGINE = problem_helpers.DataOracleEngine
    try:
        out = {}
        for seed in range(4):
            X, Xs = cr.case_a(seed)
            out[seed] = (X, Xs, model_selection.bandwidth_search(X, cr.CASE_A_BANDWIDTHS),
                         model_selection.bandwidth_search(Xs, cr.CASE_A_BANDWIDTHS))
        return out
    finally:
        solver.ENGINE = keep


@pytest.mark.parametrize("p", PS)
def test_twin_against_the_longdouble_reference(p):
    from gglasso_amd import utils
    S, d = cr.spd_stack(3, p, 0)
    res = utils.host_cholesky_predict(S, d)
    assert np.all(res[3] == -1) and res[3].dtype == np.int64
    fr = cr.fractions(res, S, d)
    print(f"twin p={p} fractions of the bounds (log det, q, pivot)", fr)
    assert np.all(fr <= 1.0), fr
    nod = utils.host_cholesky_predict(S)
    assert np.array_equal(nod[0], res[0]) and np.all(nod[1] == 0.0)
    one = utils.host_cholesky_predict(S[1], d[1])
    assert isinstance(one[0], float) and one[0] == res[0][1] and one[1] == res[1][1] and one[3] == -1
    rid = utils.host_cholesky_predict(S, d, ridge=0.25)
    exp = utils.host_cholesky_predict(S + 0.25 * np.eye(p), d)
    assert all(np.array_equal(a, b) for a, b in zip(rid, exp))


def test_twin_failure_rule():
    from gglasso_amd import utils
    S, d = cr.spd_stack(3, 17, 1)
    lam, Q = np.linalg.eigh(S[1])
    lam[0] = -0.1
    bad = S.copy()
    bad[1] = (Q * lam) @ Q.T
    bad[1] = 0.5 * (bad[1] + bad[1].T)
    ld, q, mp, st = utils.host_cholesky_predict(bad, d)
    assert st[0] == -1 and st[2] == -1 and 0 <= st[1] < 17
    assert ld[1] == -np.inf and np.isnan(q[1]) and mp[1] <= 0
    # the first column whose leading block is not positive definite
    first = next(j for j in range(17) if np.linalg.eigvalsh(bad[1][:j + 1, :j + 1])[0] <= 0)
    assert st[1] == first
    good = utils.host_cholesky_predict(S, d)
    assert ld[0] == good[0][0] and q[2] == good[1][2]
    assert np.all(utils.host_cholesky_predict(bad, d, ridge=0.2)[3] == -1)
    nan = S.copy()
    nan[2, 9, 4] = nan[2, 4, 9] = np.nan
    st = utils.host_cholesky_predict(nan, d)[3]
    assert list(st) == [-1, -1, 9]                       # an entry (i, j) of the lower triangle reaches the pivot of column i
    with pytest.raises(AssertionError, match="ridge"):
        utils.host_cholesky_predict(S, d, ridge=-1.0)
    with pytest.raises(AssertionError, match="ridge"):
        utils.host_cholesky_predict(S, d, ridge=np.nan)
    with pytest.raises(AssertionError, match="square"):
        utils.host_cholesky_predict(np.ones((3, 4)))


def test_twin_score_is_the_gaussian_log_density():
    stats = pytest.importorskip("scipy.stats")
    from gglasso_amd import utils
    X, _ = cr.case_a(0)
    ev = np.array([0, 17, 120, 239])
    SCORE, STATUS = utils.host_loo_bandwidth_scores(X, [32.0], eval_index=ev)
    w = utils.loo_weights(np.arange(240.0), ev, 32.0)
    for r, i in enumerate(ev):
        S = utils.host_weighted_covariance(X, w[r])
        m = X @ w[r] / w[r].sum()
        ref = -2.0 * stats.multivariate_normal.logpdf(X[:, i], m, S) - 6 * np.log(2 * np.pi)
        assert abs(SCORE[0, r] - ref) <= 1e-10 * max(1.0, abs(ref)), (i, SCORE[0, r], ref)
    assert np.all(STATUS == -1)


def test_case_a_choices_and_effective_sample_sizes(case_a):
    for seed in range(4):
        _, _, (h, st), (hs, sts) = case_a[seed]
        assert st['NOT_PD'] == [] and sts['NOT_PD'] == []
        assert list(st['BANDWIDTH']) == [200, 64, 32, 16, 8, 4]
        assert [round(float(v), 1) for v in st['N_EFF']] == [229.9, 113.0, 56.3, 27.9, 13.8, 6.7]
        assert h == 32.0 and st['IX'] == 2 and st['BEST'] == {'bandwidth': 32.0}, (seed, st['CV'])
        assert hs == 200.0 and sts['IX'] == 0, (seed, sts['CV'])
        assert st['SCORE'].shape == (6, 240) and np.array_equal(st['EVAL'], np.arange(240))
        assert np.allclose(st['CV'], st['SCORE'].mean(axis=1), rtol=0, atol=0)
        assert np.array_equal(st['SE'], st['SCORE'].std(axis=1, ddof=1) / np.sqrt(240))
    assert [round(float(v), 3) for v in case_a[0][2][1]['CV']] == [5.365, 4.301, 3.886, 4.075, 5.016, 9.077]


def test_twin_scores_against_the_longdouble_formula(case_a):
    from gglasso_amd import utils
    X, _, (_, st), _ = case_a[0]
    worst = 0.0
    for b in (0, 2, 5):
        h = st['BANDWIDTH'][b]
        ev = np.arange(0, 240, 16)
        W = utils.loo_weights(np.arange(240.0), ev, h)
        worst = max(worst, cr.score_fraction(st['SCORE'][b, ev], X, W, ev))
    print("twin: largest fraction of the score bound", worst)
    assert worst <= 1.0


def test_leave_one_out_leaves_out():
    """Another vector in column i leaves the log det of row i as it is, bit for bit: S_-i never saw x_i."""
    from gglasso_amd import utils
    X, _ = cr.case_a(1)
    ev = np.array([5, 100, 239])
    t = np.arange(240.0)
    for h in (64.0, 8.0):
        w = utils.loo_weights(t, ev, h)
        assert np.all(w[np.arange(3), ev] == 0.0)
        for r, i in enumerate(ev):
            Y = X.copy()
            Y[:, i] = 1e3 * np.arange(1.0, 7.0)
            n = np.flatnonzero(w[r])
            a = utils.host_cholesky_predict(utils.host_weighted_covariance(X[:, n], w[r, n]))
            b = utils.host_cholesky_predict(utils.host_weighted_covariance(Y[:, n], w[r, n]))
            assert a[0] == b[0]
            sa = utils.host_loo_bandwidth_scores(X, [h], eval_index=ev[r:r + 1])[0]
            sb = utils.host_loo_bandwidth_scores(Y, [h], eval_index=ev[r:r + 1])[0]
            assert sa[0, 0] != sb[0, 0]                                      # ... while the score of x_i itself moves


def test_eval_index_forms():
    from gglasso_amd import utils
    X, _ = cr.case_a(2)
    full, _ = utils.host_loo_bandwidth_scores(X, [32.0, 64.0])
    assert full.shape == (2, 240)
    X1, h1, t1, ev = utils._loo_setup(X, [32.0, 64.0], None, 40)
    assert ev.size == 40 and ev[0] == 0 and ev[-1] == 239 and np.all(np.diff(ev) > 0) and ev.dtype == np.int32
    some, status = utils.host_loo_bandwidth_scores(X, [32.0, 64.0], eval_index=np.array([7, 3, 200]))
    assert np.array_equal(some, full[:, [7, 3, 200]]) and status.shape == (2, 3)      # an index array is used as given


def test_refusals(monkeypatch):
    from gglasso_amd import utils, _lib
    X, _ = cr.case_a(0)

    def no_device(*a, **k):
        raise AssertionError("a refused search must not reach the device")
    monkeypatch.setattr(_lib, "require_gpu", no_device)
    monkeypatch.setattr(_lib, "load", no_device)
    for fn in (utils.loo_bandwidth_scores, utils.host_loo_bandwidth_scores):
        with pytest.raises(ValueError, match=r"bandwidth 0\.4: the evaluation sample 0 has no neighbour"):
            fn(X, [8.0, 0.4], kernel='epanechnikov')
        with pytest.raises(ValueError, match=r"bandwidth 0\.4: the evaluation sample 17 "):
            fn(X, [0.4], kernel='uniform', eval_index=np.array([17, 30]))
        with pytest.raises(AssertionError, match="kernel must be"):
            fn(X, [8.0], kernel='box')
        with pytest.raises(AssertionError, match="cutoff"):
            fn(X, [8.0], cutoff=1.5)
        with pytest.raises(AssertionError, match="positive and finite"):
            fn(X, [8.0, 0.0])
        with pytest.raises(AssertionError, match="ridge"):
            fn(X, [8.0], ridge=-1e-3)
        with pytest.raises(AssertionError, match="one entry per column"):
            fn(X, [8.0], times=np.arange(239.0))
        with pytest.raises(AssertionError, match=r"eval_index must lie in \[0, 240\)"):
            fn(X, [8.0], eval_index=np.array([0, 240]))
    with pytest.raises(AssertionError, match="chunk"):
        utils.loo_bandwidth_scores(X, [8.0], chunk=-1)


def test_descending_order_and_cv_select(host, monkeypatch):
    from gglasso_amd import utils
    X, _ = cr.case_a(3)
    ev = np.arange(0, 240, 6)
    h, st = host.bandwidth_search(X, [8, 200, 32, 64], eval_index=ev)
    assert list(st['BANDWIDTH']) == [200, 64, 32, 8] and st['rule'] == 'min' and np.array_equal(st['EVAL'], ev)
    SC, _ = utils.host_loo_bandwidth_scores(X, [8, 200, 32, 64], eval_index=ev)
    assert np.array_equal(st['SCORE'], SC[[1, 3, 2, 0]])                   # loo_bandwidth_scores keeps the caller's order
    assert st['IX'] == host.cv_select(st['CV'], st['SE'], 'min') and h == st['BANDWIDTH'][st['IX']]
    h1, st1 = host.bandwidth_search(X, [8, 200, 32, 64], rule='one_se', eval_index=ev)
    assert st1['IX'] == host.cv_select(st['CV'], st['SE'], 'one_se') and h1 >= h and st1['rule'] == 'one_se'
    seen = []
    with monkeypatch.context() as m:                                       # the choice is cv_select's, nothing beside it
        m.setattr(host, "cv_select", lambda CV, SE, rule='min': seen.append((CV.copy(), SE.copy(), rule)) or 1)
        h2, st2 = host.bandwidth_search(X, [8, 200, 32, 64], rule='one_se', eval_index=ev)
    assert h2 == 64.0 and st2['IX'] == 1 and seen[0][2] == 'one_se' and np.array_equal(seen[0][0], st['CV'])
    with pytest.raises(ValueError, match="rule"):
        host.bandwidth_search(X, [8, 32], rule='best')
    # a bandwidth whose covariances are singular has CV = +inf, is listed and is never chosen
    # (variable 3 is exactly 0 over the first half: under h = 4 the first samples see a zero row and column, pivot 3 is 0)
    Y = X.copy()
    Y[3, :120] = 0.0
    h3, st3 = host.bandwidth_search(Y, [4, 200], eval_index=ev[:8])
    assert h3 == 200.0 and np.isinf(st3['CV'][1]) and np.isfinite(st3['CV'][0])
    assert st3['NOT_PD'] == [(1, int(i)) for i in ev[:8]]
    assert np.all(utils.host_loo_bandwidth_scores(Y, [4], eval_index=ev[:8])[1] == 3)
    h4, st4 = host.bandwidth_search(Y, [4, 200], eval_index=ev[:8], ridge=1e-3)
    assert st4['NOT_PD'] == [] and np.isfinite(st4['CV']).all()


def test_from_time_series_cv_on_the_host_engine(host):
    from gglasso_amd import problem
    X, _ = cr.case_a(0)
    ev = np.arange(0, 240, 4)
    P = problem.glasso_problem.from_time_series_cv(X, 5, [64, 32, 16], eval_index=ev, reg_params={'lambda1': 0.1, 'lambda2': 0.05})
    h, st = host.bandwidth_search(X, [64, 32, 16], eval_index=ev)
    assert P.bandwidth_ == h == 32.0 and P.bandwidth_stats['IX'] == st['IX']
    assert np.array_equal(P.bandwidth_stats['SCORE'], st['SCORE'])
    Q = problem.glasso_problem.from_time_series(X, 5, P.bandwidth_, reg_params={'lambda1': 0.1, 'lambda2': 0.05})
    assert np.array_equal(P.S, Q.S) and np.array_equal(P.weights, Q.weights) and P.reg == 'FGL'
    P1 = problem.glasso_problem.from_time_series_cv(X, 5, [64, 32, 16], rule='one_se', eval_index=ev, kernel='epanechnikov')
    assert P1.bandwidth_stats['rule'] == 'one_se' and P1.bandwidth_ >= 16
    with pytest.raises(TypeError):
        problem.glasso_problem.from_time_series_cv(X, 5, [64, 32], 'min')            # keyword-only behind the grid
