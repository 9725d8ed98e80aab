"""Latent correlation of mixed binary / continuous data, host side (no GPU): the test reference against scipy's bivariate
normal, the numpy twin ``utils.host_mixed_correlation`` against the reference, and the drivers
(``stars_search(correlation='mixed')``, ``glasso_problem.from_data(correlation='mixed')``) on their host route with the
batch's array work done by the test-only oracle engine."""
import os
import re
import warnings

import numpy as np
import pytest

from bridge_ref import CLIP, F_ref, dF_ref, delta_ref, latent_truth, make_mixed, pair_table, r_ref, types_ref
from kendall_ref import counts_ref

U = 2.0 ** -53
LAM = [0.5, 0.3, 0.15]
ROOT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..")


def test_reference_bridge_is_the_bivariate_normal_form():
    from scipy import stats
    from scipy.special import ndtr
    rng = np.random.default_rng(3)
    worst = 0.0
    for _ in range(40):
        h, k = rng.uniform(-1.5, 1.5, 2)
        r = rng.uniform(-0.95, 0.95)
        phi2 = lambda a, b, c: stats.multivariate_normal.cdf([a, b], mean=[0.0, 0.0], cov=[[1.0, c], [c, 1.0]], abseps=1e-15,
                                                             releps=1e-15, maxpts=10 ** 7)
        bb = 2.0 * (phi2(h, k, r) - ndtr(h) * ndtr(k))
        bc = 4.0 * phi2(h, 0.0, r / np.sqrt(2.0)) - 2.0 * ndtr(h)
        worst = max(worst, abs(F_ref(r, h, k, True) - bb), abs(F_ref(r, h, 0.0, False) - bc))
    print(f"reference bridge against the bivariate normal: {worst:.3e}")
    assert worst <= 1e-12, worst
    # the analytic derivative is the derivative
    for bb in (True, False):
        e = 1e-6
        num = (F_ref(0.3 + e, 0.4, -0.7, bb) - F_ref(0.3 - e, 0.4, -0.7, bb)) / (2 * e)
        assert abs(num - dF_ref(0.3, 0.4, -0.7 if bb else 0.0, bb)) <= 1e-9


def test_variable_types():
    from gglasso_amd import utils
    rng = np.random.default_rng(0)
    X = np.stack([rng.integers(0, 2, 30).astype(float), 2.0 * rng.integers(0, 2, 30) - 1.0, rng.integers(0, 3, 30).astype(float),
                  rng.standard_normal(30), np.full(30, 2.0)])
    X[2, :3] = [0, 1, 2]
    t = utils.variable_types(X)
    assert t.dtype == np.int32 and t.tolist() == [1, 1, 0, 0, 0]
    assert np.array_equal(t[:4], types_ref(X[:4]))


def residuals(X, S, clip=CLIP):
    """(largest |F_ref(S_ij) - tau| over the pairs the reference does not clip, the reference's clipped count)."""
    rows, _, _ = pair_table(X, clip=clip)
    worst = 0.0
    for q in rows:
        if not q['clipped']:
            worst = max(worst, abs(F_ref(S[q['i'], q['j']], q['h'], q['k'], q['bb']) - q['tau']))
    return worst, sum(q['clipped'] for q in rows)


def test_host_twin_solves_the_bridge_equations():
    from gglasso_amd import utils
    worst = 0.0
    for p, N, nb in ((7, 150, 4), (6, 40, 6), (5, 60, 2)):
        X = make_mixed(p, N, nb, 1)
        S, info = utils.host_mixed_correlation(X, return_info=True)
        rows, n0, G = pair_table(X)
        assert np.array_equal(info['types'], types_ref(X))
        assert np.array_equal(info['zero_counts'][info['types'] == 1], n0[info['types'] == 1])
        assert np.array_equal(S, S.T) and np.array_equal(np.diag(S), np.ones(p))
        res, n_clip = residuals(X, S)
        worst = max(worst, res)
        assert info['clipped'] == n_clip
        for q in rows:
            if not q['clipped']:
                bound = 1e-13 / dF_ref(q['r'], q['h'], q['k'], q['bb']) + 4 * U
                assert abs(S[q['i'], q['j']] - q['r']) <= bound, (p, N, q)
        # the thresholds are scipy's
        for i in np.flatnonzero(info['types']):
            assert abs(utils._bridge_delta(n0[i], N) - delta_ref(n0[i], N)) <= 4 * U * max(1.0, abs(delta_ref(n0[i], N)))
    print(f"host twin: largest |F_ref(r) - tau| {worst:.3e}")
    assert worst <= 1e-13, worst
    # subsets: each the matrix of its gathered columns, with the types of the whole data
    X = make_mixed(7, 150, 4, 1)
    idx = np.stack([np.arange(0, 100), np.arange(50, 150)])
    Sb, info = utils.host_mixed_correlation(X, indices=idx, return_info=True)
    for r in range(2):
        assert np.array_equal(Sb[r], utils.host_mixed_correlation(X[:, idx[r]]))
    assert info['zero_counts'].shape == (2, 7) and info['clipped'].shape == (2,)


def test_host_twin_is_invariant_under_increasing_transforms():
    from gglasso_amd import utils
    X = make_mixed(7, 150, 4, 1)
    t = types_ref(X)
    S = utils.host_mixed_correlation(X)
    Y = X.copy()
    Y[t == 0] = np.log(Y[t == 0]) ** 3
    Y[t == 1] = 2.0 * Y[t == 1] - 1.0                       # {0,1} -> {-1,1}
    Y[0] = 4.0 * X[0] + 5.0                                  # {0,1} -> {5,9}
    assert np.array_equal(utils.host_mixed_correlation(Y), S)
    # the other coding of a binary variable flips the sign of its row and column
    Y = X.copy()
    Y[2] = 1.0 - X[2]
    flip = np.ones(7)
    flip[2] = -1.0
    assert np.abs(utils.host_mixed_correlation(Y) - S * np.outer(flip, flip)).max() <= 1e-13


def test_identical_and_complementary_binary_rows_are_clipped():
    """tau = 2 n0 n1 / (n (n - 1)) > 2 pi0 (1 - pi0) = F(1) > F(clip): exactly +clip, and -clip for the complement."""
    from gglasso_amd import utils
    X = make_mixed(6, 80, 3, 2)
    t = types_ref(X)
    b0 = int(np.flatnonzero(t)[0])
    Y = np.concatenate([X, X[b0:b0 + 1], 1.0 - X[b0:b0 + 1]])
    for clip in (0.999, 0.9):
        S, info = utils.host_mixed_correlation(Y, clip=clip, return_info=True)
        assert S[b0, 6] == clip and S[b0, 7] == -clip and S[6, 7] == -clip
        assert info['clipped'] == residuals(Y, S, clip)[1] >= 3
    for bad in (0.0, 1.0, -0.5, np.nan):
        with pytest.raises(AssertionError, match="clip"):
            utils.host_mixed_correlation(Y, clip=bad)
    flat = X.copy()
    flat[1] = 3.0
    with pytest.raises(AssertionError, match="variable 1 is constant"):
        utils.host_mixed_correlation(flat)
    with pytest.raises(AssertionError, match="marked binary"):
        utils.host_mixed_correlation(X, types=np.ones(6, dtype=np.int32))


def test_all_continuous_data_give_the_skeptic_matrix():
    from gglasso_amd import utils
    X = make_mixed(9, 70, 0, 3)
    S, info = utils.host_mixed_correlation(X, return_info=True)
    assert not info['types'].any() and info['clipped'] == 0
    assert np.abs(S - utils.host_skeptic_correlation(X)).max() <= 4 * U


def test_recovery_of_the_latent_correlation():
    """A statistical sanity check, not a rounding bound: p = 6, N = 6000, three variables dichotomised."""
    from gglasso_amd import utils
    X = make_mixed(6, 6000, 3, 1)
    S = utils.host_mixed_correlation(X)
    err = float(np.abs(S - latent_truth(6)).max())
    pearson = float(np.abs(np.corrcoef(X) - latent_truth(6)).max())
    print(f"recovery at (6, 6000): mixed {err:.3f}, Pearson {pearson:.3f}")
    assert err < 0.08 < pearson


@pytest.fixture()
def on_host(monkeypatch):
    import problem_helpers
    problem_helpers.on_host(monkeypatch)


def mixed_problem():
    X = make_mixed(8, 60, 4, 5)
    idx = np.stack([np.sort(np.random.default_rng([5, r]).choice(60, 45, replace=False)) for r in range(3)])
    return X, idx


def test_stars_search_mixed_on_the_host_route(on_host):
    from gglasso_amd import model_selection as ms, solver, utils
    X, idx = mixed_problem()
    p, B = 8, 3
    with warnings.catch_warnings():
        warnings.simplefilter("ignore", RuntimeWarning)
        sol, st = ms.stars_search(X, LAM, indices=idx, beta=0.1, correlation='mixed', store_all=True)
        sol_k, st_k = ms.stars_search(X, LAM, indices=idx, beta=0.1, correlation='kendall', store_all=True)
        sol_p, st_p = ms.stars_search(X, LAM, indices=idx, beta=0.1, correlation=None, store_all=True)
    # the statistics are those of the batch solved on the twin's matrices, types fixed on all observations
    S = utils.host_mixed_correlation(X, utils.variable_types(X), idx)
    eye = np.eye(p)
    for l, lam in enumerate(st['LAMBDA']):
        for r in range(B):
            one, _ = solver.ADMM_SGL(S[r], lam, eye, X_0=eye, tol=1e-7, rtol=1e-7, verbose=False)
            assert np.abs(one['Theta'] - st['THETA'][l, r]).max() <= 1e-5, (l, r)
    cnt, num = ms._host_edge_counts(st['THETA'], 1e-8)
    assert st['NUM'] == [int(n) for n in num] and np.array_equal(st['COUNTS'], cnt)
    full, _ = solver.ADMM_SGL(utils.host_mixed_correlation(X), st['BEST']['lambda1'], eye, X_0=eye, tol=1e-7, rtol=1e-7, verbose=False)
    assert np.array_equal(full['Theta'], sol['Theta'])
    # another matrix than Pearson's and the skeptic's
    assert not np.array_equal(st['THETA'], st_k['THETA']) and not np.array_equal(st['THETA'], st_p['THETA'])
    assert not np.array_equal(sol['Theta'], sol_k['Theta']) and not np.array_equal(sol['Theta'], sol_p['Theta'])
    for kw in (dict(center=False), dict(scale=True)):
        with pytest.raises(AssertionError, match="defaults"):
            ms.stars_search(X, LAM, indices=idx, correlation='mixed', **kw)
    with pytest.raises(AssertionError, match=r"correlation must be None \(Pearson\), 'kendall' or 'mixed'"):
        ms.stars_search(X, LAM, indices=idx, correlation='spearman')
    with pytest.raises(ValueError, match="missing='pairwise' with correlation='mixed'"):
        ms.stars_search(X, LAM, indices=idx, correlation='mixed', missing='pairwise')
    with pytest.raises(ValueError, match="missing='pairwise' with correlation='kendall'"):
        ms.stars_search(X, LAM, indices=idx, correlation='kendall', missing='pairwise')


def test_from_data_mixed_on_the_host_route(on_host):
    from gglasso_amd import glasso_problem, model_selection as ms, utils
    X, idx = mixed_problem()
    S = utils.host_mixed_correlation(X)
    P = glasso_problem.from_data(X, correlation='mixed', reg_params={'lambda1': 0.2})
    assert np.array_equal(P.S, S) and P.N == 60
    P.solve()
    Q = glasso_problem(S, 60, reg_params={'lambda1': 0.2})
    Q.solve()
    assert np.array_equal(P.solution.precision_, Q.solution.precision_)
    Pk = glasso_problem.from_data(X, correlation='kendall')
    P0 = glasso_problem.from_data(X, correlation=None)
    assert not np.array_equal(P.S, Pk.S) and not np.array_equal(P.S, P0.S)
    assert np.abs(P0.S - np.cov(X, bias=True)).max() <= 1e-12 * np.abs(P0.S).max()
    # a stack: one matrix per instance
    X2 = np.stack([X, X[::-1]])
    P2 = glasso_problem.from_data(X2, correlation='mixed', reg="GGL")
    assert P2.S.shape == (2, 8, 8) and np.array_equal(P2.S[0], S) and np.abs(P2.S[1] - S[::-1, ::-1]).max() <= 1e-13
    with pytest.raises(AssertionError, match="default"):
        glasso_problem.from_data(X, correlation='mixed', center=False)
    with pytest.raises(AssertionError, match=r"correlation must be None \(Pearson\), 'kendall' or 'mixed'"):
        glasso_problem.from_data(X, correlation='spearman')
    with pytest.raises(ValueError, match="missing='pairwise' with correlation='mixed'"):
        glasso_problem.from_data(X, correlation='mixed', missing='pairwise')
    # stability selection passes the choice on
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        P.stability_selection({'lambda1_range': np.array(LAM)}, n_subsamples=3, subsample_size=45, seed=5, beta=0.1)
        sol, st = ms.stars_search(X, LAM, n_subsamples=3, subsample_size=45, seed=5, beta=0.1, correlation='mixed')
    assert P.modelselect_stats['NUM'] == st['NUM'] and np.array_equal(P.solution.precision_, sol['Theta'])


def test_new_entry_points_are_declared():
    from gglasso_amd import _lib, build, utils
    from gglasso_amd.solver import HipEngine
    header = open(os.path.join(ROOT, "include", "ggl_hip.h")).read()
    for name in ("ggl_mixed_correlation", "ggl_set_S_from_mixed"):
        assert name in _lib.EXPORTS and f"int {name}(" in header
        assert header.index(name) < header.index("#define GGL_VERSION")         # in the list of additions
    assert "#define GGL_VERSION 300" in header and _lib.ABI_VERSION == 300
    assert "bridge.hip" in build.SOURCES
    assert hasattr(HipEngine, "set_mixed_subsets")
    # the kernel's quadrature table is the twin's
    src = open(os.path.join(ROOT, "gglasso_amd", "csrc", "bridge.hip")).read()
    for name, table in (("BR_U", utils._GL64_U), ("BR_V", utils._GL64_V)):
        body = re.search(name + r"\[64\] = \{(.*?)\};", src, re.S).group(1)
        assert np.array_equal(np.array([float(v) for v in body.replace("\n", " ").split(",")]), table)
    x, w = np.polynomial.legendre.leggauss(64)
    assert np.abs(utils._GL64_U - (1 + x) / 2).max() <= 2 * U and np.abs(utils._GL64_V - w / 2).max() <= 1e-14
    assert abs(utils._GL64_V.sum() - 1.0) <= 4 * U
