"""Nearest-correlation projection, host side (no GPU): the numpy twin ``utils.host_nearest_correlation`` (Higham's example,
the properties of its result on indefinite skeptic matrices, optimality, idempotence, pass-through, covariance input,
refusals), the drivers on their host route (``from_data(project=True)``, ``stars_search(project=True)``) with the batch's
array work done by the test-only oracle engine, and the wiring of the two entry points."""
import functools
import os
import re
import warnings

import numpy as np
import pytest

SHAPES = [(15, 8), (17, 12), (33, 20), (65, 24), (70, 30), (130, 40)]
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@functools.lru_cache(maxsize=None)
def skeptic(p, N):
    """The skeptic matrix of data rounded to one decimal (ties occur); p > N makes it indefinite.  Shared, never changed."""
    from gglasso_amd import utils
    X = np.round(np.random.default_rng([p, N]).standard_normal((p, N)), 1)
    S = utils.host_skeptic_correlation(X)
    S.setflags(write=False)
    return S


def test_highams_example():
    from gglasso_amd import utils
    A = np.array([[1., 1, 0], [1, 1, 1], [0, 1, 1]])
    out, info = utils.host_nearest_correlation(A, eps=0, tol=1e-12, return_info=True)
    assert info['converged'] and info['iterations'] > 1
    assert abs(out[0, 1] - 0.76068985) <= 1e-7 and abs(out[1, 2] - 0.76068985) <= 1e-7 and abs(out[0, 2] - 0.15729811) <= 1e-7
    assert np.array_equal(out, out.T) and np.array_equal(np.diag(out), np.ones(3))


@pytest.mark.parametrize("p,N", SHAPES)
def test_result_is_a_positive_definite_correlation_matrix(p, N):
    from gglasso_amd import utils
    S = skeptic(p, N)
    assert np.linalg.eigvalsh(S).min() < -0.1
    for eps in (0.0, 1e-8, 1e-3, 0.05):
        out, info = utils.host_nearest_correlation(S, eps=eps, return_info=True)
        assert info['converged'] and 1 < info['iterations'] < 500, (eps, info)
        assert np.array_equal(np.diag(out), np.ones(p)) and np.array_equal(out, out.T)
        assert np.linalg.eigvalsh(out).min() >= eps - 1e-12, eps
        assert abs(info['distance'] - np.linalg.norm(out - S)) <= 1e-12 * np.linalg.norm(S)
        assert 0.0 <= info['shrink'] <= 1e-7
    # stopped early: a warning, converged=False, and still positive definite with a unit diagonal
    with pytest.warns(RuntimeWarning, match=r"no convergence within 5 iterations for the matrices \[0\]"):
        out5, info5 = utils.host_nearest_correlation(S, max_iter=5, return_info=True)
    assert not info5['converged'] and info5['iterations'] == 5 and info5['residual'] > 1e-10
    assert np.linalg.eigvalsh(out5).min() >= 1e-8 - 1e-12
    assert np.array_equal(np.diag(out5), np.ones(p)) and np.array_equal(out5, out5.T)
    assert 0.0 < info5['shrink'] < 1.0


@pytest.mark.parametrize("p,N", SHAPES)
def test_result_is_nearer_than_the_linear_shrinkage(p, N):
    from gglasso_amd import utils
    S = skeptic(p, N)
    eps = 1e-8
    _, info = utils.host_nearest_correlation(S, eps=eps, return_info=True)
    lmin = np.linalg.eigvalsh(S).min()
    nu = (eps - lmin) / (1.0 - lmin)                      # the smallest nu with lambda_min((1 - nu) S + nu I) = eps
    assert info['distance'] < nu * np.linalg.norm(S - np.eye(p))


def test_idempotence_and_pass_through():
    from gglasso_amd import utils
    for p, N in SHAPES:
        out = utils.host_nearest_correlation(skeptic(p, N))
        again, info = utils.host_nearest_correlation(out, return_info=True)
        assert np.array_equal(again, out) and info['iterations'] == 1 and info['shrink'] == 0.0 and info['distance'] == 0.0
    C = np.corrcoef(np.random.default_rng(3).standard_normal((12, 200)))
    back, info = utils.host_nearest_correlation(C, return_info=True)
    assert np.array_equal(back, C) and info['iterations'] == 1 and info['converged']
    # a stack: every matrix on its own
    St = np.stack([skeptic(15, 8), np.eye(15), skeptic(15, 8).T])
    outs, infos = utils.host_nearest_correlation(St, return_info=True)
    assert np.array_equal(outs[0], utils.host_nearest_correlation(skeptic(15, 8))) and np.array_equal(outs[0], outs[2])
    assert np.array_equal(outs[1], np.eye(15)) and list(infos['iterations'] == 1) == [False, True, False]
    assert infos['converged'].all() and infos['distance'].shape == (3,)


def test_covariance_input_keeps_its_variances():
    from gglasso_amd import utils
    rng = np.random.default_rng(21)
    p, N = 20, 14
    X = rng.standard_normal((p, N)) * rng.uniform(0.5, 20.0, (p, 1))
    X[rng.random((p, N)) < 0.2] = np.nan
    S, cnt = utils.host_pairwise_covariance(X)
    assert cnt.min() >= 2 and np.linalg.eigvalsh(S).min() < 0
    out, info = utils.host_nearest_correlation(S, return_info=True)
    d = np.diag(S)
    assert np.all(np.abs(np.diag(out) - d) <= 4 * np.spacing(d))
    assert np.array_equal(out, out.T) and info['converged']
    assert np.linalg.eigvalsh(out).min() > 0
    sd = np.sqrt(d)
    assert np.linalg.eigvalsh(out / np.outer(sd, sd)).min() >= 1e-8 - 1e-12


def test_refusals_name_the_offender():
    from gglasso_amd import utils
    S = np.array(skeptic(15, 8))
    bad = np.stack([S, S])
    bad[1, 4, 7] = np.nan
    with pytest.raises(AssertionError, match=r"variable 4 of matrix 1 holds a non-finite entry"):
        utils.host_nearest_correlation(bad)
    bad = S.copy()
    bad[6, 6] = 0.0
    with pytest.raises(AssertionError, match=r"diagonal entry of variable 6 of matrix 0 is 0.0, not positive"):
        utils.host_nearest_correlation(bad)
    bad[6, 6] = -1.0
    with pytest.raises(AssertionError, match=r"variable 6 of matrix 0 is -1.0, not positive"):
        utils.host_nearest_correlation(bad)
    for shape in ((15, 14), (2, 15, 14), (15,), (1, 2, 15, 15)):
        with pytest.raises(AssertionError, match=r"square \(p,p\) matrix or a \(B,p,p\) stack"):
            utils.host_nearest_correlation(np.zeros(shape))
    for kw, what in ((dict(eps=-1e-3), "eps"), (dict(eps=0.6), "eps"), (dict(tol=1e-15), "tol"), (dict(tol=0.1), "tol"),
                     (dict(max_iter=0), "max_iter")):
        with pytest.raises(AssertionError, match=what):
            utils.host_nearest_correlation(S, **kw)


@pytest.fixture()
def on_host(monkeypatch):
    import problem_helpers
    problem_helpers.on_host(monkeypatch)


def small_problem():
    p, N, B, b = 10, 12, 3, 8
    X = np.round(np.random.default_rng(17).standard_normal((p, N)), 1)
    idx = np.stack([np.sort(np.random.default_rng([4, r]).choice(N, b, replace=False)) for r in range(B)])
    return X, idx


def test_from_data_projects_on_the_host_route(on_host):
    from gglasso_amd import glasso_problem, utils
    X, _ = small_problem()
    P0 = glasso_problem.from_data(X, correlation='kendall')
    assert np.array_equal(P0.S, utils.host_skeptic_correlation(X)) and P0.projection is None      # project=False: today's bits
    assert np.array_equal(glasso_problem.from_data(X, correlation='kendall', project=False).S, P0.S)
    assert np.linalg.eigvalsh(P0.S).min() < -0.01               # indefinite, far beyond rounding
    P = glasso_problem.from_data(X, correlation='kendall', project=True)
    ref, info = utils.host_nearest_correlation(P0.S, return_info=True)
    assert np.array_equal(P.S, ref) and P.projection == info and P.projection['iterations'] > 1
    # a stack: every instance; Pearson and pairwise as well
    X2 = np.stack([X[:, :7], X[::-1, :7] * 2.0])                  # 7 observations of 10 variables: singular
    Q0 = glasso_problem.from_data(X2)
    Q = glasso_problem.from_data(X2, project=True)
    assert np.array_equal(Q.S, utils.host_nearest_correlation(Q0.S)) and Q.projection['iterations'].shape == (2,)
    assert np.linalg.eigvalsh(Q0.S).min() < 1e-12 and np.linalg.eigvalsh(Q.S).min() > 0
    Xm = X.copy()
    Xm[2, 3] = Xm[5, 0] = np.nan
    R0 = glasso_problem.from_data(Xm, missing='pairwise')
    R = glasso_problem.from_data(Xm, missing='pairwise', project=True)
    assert np.array_equal(R.S, utils.host_nearest_correlation(R0.S)) and np.array_equal(R.pair_counts, R0.pair_counts)
    # instances of different dimensions: one projection each
    D = glasso_problem.from_data([X, X[:6]], correlation='kendall', project=True,
                                 G=np.stack([np.array([[0, 0], [1, 1]]), np.array([[1, 1], [2, 2]])]).astype(int))
    assert np.array_equal(D.S[1], utils.host_nearest_correlation(utils.host_skeptic_correlation(X[:6])))
    assert sorted(D.projection) == [0, 1] and D.projection[0]['converged']
    with pytest.raises(AssertionError, match=r"correlation must be None \(Pearson\), 'kendall' or 'mixed'"):
        glasso_problem.from_data(X, correlation='spearman', project=True)
    with pytest.raises(AssertionError, match=r"missing must be None \(complete data\) or 'pairwise'"):
        glasso_problem.from_data(X, missing='em', project=True)


def test_stars_search_projects_on_the_host_route(on_host):
    from gglasso_amd import glasso_problem, model_selection as ms, solver, utils
    X, idx = small_problem()
    lam = [0.6, 0.4, 0.25]
    p, B = 10, 3
    S = utils.host_skeptic_correlation(X, idx)
    assert all(np.linalg.eigvalsh(s).min() < -0.1 for s in S)
    Sp = utils.host_nearest_correlation(S)
    with warnings.catch_warnings():
        warnings.simplefilter("ignore", RuntimeWarning)
        sol, st = ms.stars_search(X, lam, indices=idx, beta=0.1, correlation='kendall', project=True, store_all=True)
        sol0, st0 = ms.stars_search(X, lam, indices=idx, beta=0.1, correlation='kendall', store_all=True)
    eye = np.eye(p)
    for l, lm in enumerate(st['LAMBDA']):
        for r in range(B):
            one, _ = solver.ADMM_SGL(Sp[r], lm, eye, X_0=eye, tol=1e-7, rtol=1e-7, verbose=False)
            assert np.abs(one['Theta'] - st['THETA'][l, r]).max() <= 1e-5, (l, r)
    assert not np.array_equal(st['THETA'], st0['THETA']) and 'PROJECTION' not in st0
    full_S, info = utils.host_nearest_correlation(utils.host_skeptic_correlation(X), return_info=True)
    full, _ = solver.ADMM_SGL(full_S, st['BEST']['lambda1'], eye, X_0=eye, tol=1e-7, rtol=1e-7, verbose=False)
    assert np.array_equal(full['Theta'], sol['Theta']) and st['PROJECTION'] == info
    # stability selection passes the choice on
    P = glasso_problem.from_data(X, correlation='kendall', project=True)
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        P.stability_selection({'lambda1_range': np.array(lam)}, n_subsamples=3, subsample_size=8, seed=4, beta=0.1)
        sol_s, st_s = ms.stars_search(X, lam, n_subsamples=3, subsample_size=8, seed=4, beta=0.1, correlation='kendall',
                                      project=True)
    assert P.modelselect_stats['NUM'] == st_s['NUM'] and 'PROJECTION' in P.modelselect_stats
    assert np.array_equal(P.solution.precision_, sol_s['Theta'])


def test_entry_points_are_wired():
    from gglasso_amd import _lib, build
    from gglasso_amd.solver import HipEngine
    assert "ggl_nearest_correlation" in _lib.EXPORTS and "ggl_project_S" in _lib.EXPORTS
    assert "nearcorr.hip" in build.SOURCES and all(os.path.exists(os.path.join(build.CSRC, s)) for s in build.SOURCES)
    assert callable(getattr(HipEngine, "project_S"))
    with open(os.path.join(ROOT, "include", "ggl_hip.h")) as f:
        head = f.read()
    m = re.search(r"^#define GGL_VERSION (\d+)", head, re.M)
    assert m and int(m.group(1)) == 300 == _lib.ABI_VERSION
    front = head[:m.start()]
    assert "ggl_nearest_correlation" in front and "ggl_project_S" in front            # the list of additions
    for name in ("ggl_nearest_correlation", "ggl_project_S"):
        assert re.search(rf"^int {name}\(", head[m.end():], re.M), name
