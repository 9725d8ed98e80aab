"""Inference on a fitted precision matrix, host side (no GPU): the numpy twin ``utils.host_debiased_precision`` against the
longdouble reference (tests/debias_ref.py, where the bounds are derived), ``utils.edge_tests`` / ``adjust_pvalues`` /
``differential_tests`` against their definitions, the scale of the statistic on data drawn from a known precision matrix,
and ``glasso_problem.edge_inference(host=True)``."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import debias_ref as dr  # noqa: E402
import problem_helpers as ph  # noqa: E402


@pytest.fixture()
def host(monkeypatch):
    ph.on_host(monkeypatch)
    from gglasso_amd import problem
    return problem


@pytest.mark.parametrize("kind", ["cov", "inv"])
@pytest.mark.parametrize("p", [1, 2, 17, 64])
def test_twin_against_the_longdouble_reference(p, kind):
    """``|T - T_ref|_ij <= (2p + 8) u (|Theta||S||Theta|)_ij + 4u |Theta_ij|`` and SE relatively within 6u: both derived in
    tests/debias_ref.py (the standard bound of a product of three matrices, which holds for any summation order -- numpy's
    BLAS included -- plus the one subtraction; five rounded operations for SE)."""
    from gglasso_amd import utils
    Th, Sm = dr.inputs(p, kind, 3)
    n = dr.n_of(3)
    T, SE = utils.host_debiased_precision(Th, Sm, n)
    assert T.shape == SE.shape == (3, p, p)
    assert np.array_equal(T, np.swapaxes(T, 1, 2)) and np.array_equal(SE, np.swapaxes(SE, 1, 2))
    dr.check_against_reference(T, SE, Th, Sm, dr.reference(Th, Sm, n), f"twin p={p} {kind}")
    # a single matrix with a scalar N is instance 0 of the stack
    T0, SE0 = utils.host_debiased_precision(Th[0], Sm[0], float(n[0]))
    assert np.array_equal(T0, T[0]) and np.array_equal(SE0, SE[0])
    if kind == "inv" and p > 1:
        assert np.abs(T - Th).max() <= 1e-10 * np.abs(Th).max()       # 2 Theta - Theta Theta^-1 Theta = Theta


def test_twin_refusals():
    from gglasso_amd import utils
    Th, Sm = (a.copy() for a in dr.inputs(5, "cov", 3))
    n = dr.n_of(3)
    bad = Th.copy(); bad[1, 2, 3] = np.nan
    with pytest.raises(AssertionError, match=r"Theta of instance 1, variable 2 holds a non-finite"):
        utils.host_debiased_precision(bad, Sm, n)
    bad = Sm.copy(); bad[2, 4, 0] = np.inf
    with pytest.raises(AssertionError, match=r"S of instance 2, variable 4 holds a non-finite"):
        utils.host_debiased_precision(Th, bad, n)
    bad = Th.copy(); bad[0, 3, 3] = 0.0
    with pytest.raises(AssertionError, match=r"Theta of instance 0, variable 3: the diagonal entry is 0.0"):
        utils.host_debiased_precision(bad, Sm, n)
    with pytest.raises(AssertionError, match=r"N of instance 1 is 0.0"):
        utils.host_debiased_precision(Th, Sm, [10, 0, 10])
    with pytest.raises(AssertionError, match=r"N must be one number or an array of length K = 3"):
        utils.host_debiased_precision(Th, Sm, [10, 10])
    with pytest.raises(AssertionError, match=r"they must match"):
        utils.host_debiased_precision(Th, Sm[:2], n)


# ---------------------------------------------------------------------------------------------------------------------
# multiplicity adjustment and edge_tests
# ---------------------------------------------------------------------------------------------------------------------
def bh_by_definition(pv, alpha):
    """Reject the k smallest p-values for the largest k with p_(k) <= k alpha / m."""
    m = len(pv)
    order = np.argsort(pv, kind="stable")
    k = 0
    for j in range(m, 0, -1):
        if pv[order[j - 1]] <= j * alpha / m:
            k = j
            break
    rej = np.zeros(m, dtype=bool)
    rej[order[:k]] = True
    return rej


def bh_adjusted_by_definition(pv):
    m = len(pv)
    ps = np.sort(pv)
    return np.array([min(min(1.0, m * ps[j] / (j + 1)) for j in range(m) if ps[j] >= x) for x in pv])


HAND = np.array([0.01, 0.04, 0.03, 0.005, 0.03, 0.5, 0.03, 0.9, 0.04, 1.0])      # ties at 0.03 (three) and 0.04 (two)


def test_bh_against_the_definition():
    from gglasso_amd import utils
    # the hand-made vector: m = 10, alpha = 0.06; sorted .005 .01 .03 .03 .03 .04 .04 .5 .9 1 against .006 .012 ... .06:
    # p_(7) = .04 <= .042 is the last one that passes, so the seven smallest are rejected, the tied ones together
    adj, rej = utils.adjust_pvalues(HAND, alpha=0.06, method="bh")
    assert rej.tolist() == [True, True, True, True, True, False, True, False, True, False]
    assert np.array_equal(rej, bh_by_definition(HAND, 0.06))
    # at alpha = 0.05 p_(5) = .03 <= .025 fails, p_(2) = .01 <= .01 passes: two rejections
    adj5, rej5 = utils.adjust_pvalues(HAND, alpha=0.05, method="bh")
    assert np.array_equal(rej5, bh_by_definition(HAND, 0.05)) and rej5.sum() == 2
    assert np.array_equal(adj, adj5) and np.allclose(adj, bh_adjusted_by_definition(HAND), rtol=1e-15, atol=0)
    assert adj[2] == adj[4] == adj[6]                                          # ties share their adjusted value
    rng = np.random.default_rng(5)
    for m in (1, 2, 7, 45, 300):
        for frac in (0.0, 0.3, 1.0):
            pv = rng.random(m)
            small = rng.random(m) < frac
            pv[small] *= 1e-3
            pv = np.round(pv, 3) if m == 45 else pv                            # ties
            for alpha in (0.01, 0.05, 0.2):
                adj, rej = utils.adjust_pvalues(pv, alpha=alpha, method="bh")
                assert np.array_equal(rej, bh_by_definition(pv, alpha)), (m, frac, alpha)
                assert np.allclose(adj, bh_adjusted_by_definition(pv), rtol=1e-15, atol=0)
                o = np.argsort(pv, kind="stable")
                assert np.all(np.diff(adj[o]) >= 0) and np.all(adj >= pv * (1 - 4 * dr.U)) and np.all(adj <= 1)      # monotone
                # the adjusted values say the same up to the rounding of m p / k against k alpha / m
                clear = np.abs(adj - alpha) > 1e-12
                assert np.array_equal((adj <= alpha)[clear], rej[clear])


def test_bonferroni_and_none():
    from gglasso_amd import utils
    adj, rej = utils.adjust_pvalues(HAND, alpha=0.05, method="bonferroni")
    assert np.array_equal(adj, np.minimum(1.0, 10 * HAND)) and np.array_equal(rej, adj <= 0.05) and rej.sum() == 1
    adj, rej = utils.adjust_pvalues(HAND, alpha=0.05, method="none")
    assert np.array_equal(adj, HAND) and rej.sum() == 7
    with pytest.raises(AssertionError, match="method must be one of"):
        utils.adjust_pvalues(HAND, method="holm")
    with pytest.raises(AssertionError, match="a level lies in"):
        utils.adjust_pvalues(HAND, alpha=1.5)


@pytest.mark.parametrize("method", ["bh", "bonferroni", "none"])
def test_edge_tests(method):
    from scipy.special import erfc, ndtri
    from gglasso_amd import utils
    Th, Sm = dr.inputs(17, "cov", 3)
    T, SE = utils.host_debiased_precision(Th, Sm, dr.n_of(3))
    alpha = 0.1
    r = utils.edge_tests(T, SE, alpha=alpha, method=method)
    assert set(r) == {"z", "pvalue", "pvalue_adj", "reject", "ci_low", "ci_high"}
    p, iu, di = 17, np.triu_indices(17, 1), np.arange(17)
    assert np.array_equal(r["z"], T / SE)
    assert np.array_equal(r["pvalue"], erfc(np.abs(T / SE) / np.sqrt(2.0)))
    assert r["reject"].dtype == bool and not r["reject"][:, di, di].any()       # the diagonal is never rejected
    assert np.isnan(r["pvalue_adj"][:, di, di]).all()
    for key in r:                                                                # symmetric
        assert np.array_equal(r[key], np.swapaxes(r[key], 1, 2), equal_nan=True), key
    for k in range(3):                                                           # the family: the pairs of ONE instance
        adj, rej = utils.adjust_pvalues(r["pvalue"][k][iu], alpha, method)
        assert np.array_equal(r["pvalue_adj"][k][iu], adj) and np.array_equal(r["reject"][k][iu], rej)
        if method == "bonferroni":
            assert np.array_equal(adj, np.minimum(1.0, (p * (p - 1) // 2) * r["pvalue"][k][iu]))
    assert 0 < r["reject"].sum() < r["reject"].size
    # intervals: contain T, half-width ndtri(1 - alpha / 2) SE
    assert np.all(r["ci_low"] < T) and np.all(T < r["ci_high"])
    q = ndtri(1 - alpha / 2)
    assert abs(q - 1.6448536269514722) < 1e-12
    assert np.allclose((r["ci_high"] - r["ci_low"]) / 2, q * SE, rtol=1e-12, atol=0)
    # without adjustment an edge is rejected exactly when its interval excludes the null
    if method == "none":
        out = (r["ci_low"] > 0) | (r["ci_high"] < 0)
        clear = np.abs(np.abs(r["z"]) - q) > 1e-9
        off = ~np.eye(p, dtype=bool)[None]
        assert np.array_equal((out & off)[clear], r["reject"][clear])
    # a single matrix is instance 0; a null other than zero shifts z
    r0 = utils.edge_tests(T[0], SE[0], alpha=alpha, method=method)
    for key in r:
        assert r0[key].shape == (p, p) and np.array_equal(r0[key], r[key][0], equal_nan=True), key
    rn = utils.edge_tests(T[0], SE[0], alpha=alpha, method=method, null=Th[0])
    assert np.array_equal(rn["z"], (T[0] - Th[0]) / SE[0])
    # p = 1: no pairs, nothing to adjust
    r1 = utils.edge_tests(np.array([[2.0]]), np.array([[0.5]]), method=method)
    assert r1["z"][0, 0] == 4.0 and not r1["reject"].any()


def precision_40():
    """p = 40: unit diagonal, 0.4 on the first off-diagonals, -0.2 at distance 5 on every third row."""
    p = 40
    Th = np.eye(p)
    i = np.arange(p - 1)
    Th[i, i + 1] = Th[i + 1, i] = 0.4
    i = np.arange(0, p - 5, 3)
    Th[i, i + 5] = Th[i + 5, i] = -0.2
    return Th


@pytest.mark.parametrize("seed", [0, 1, 2, 3])
def test_scale_of_the_statistic(seed):
    """With the truth plugged in for the estimate (no solver), the 820 pivots (T - Theta0) / SE of the upper triangle are
    close to standard normal: standard deviation in [0.9, 1.1], |mean| <= 0.15, 95 % coverage in [0.92, 0.98] at N = 4000.
    A missing sqrt(n), or n in its place, is off by a factor 63."""
    from scipy.special import ndtri
    from gglasso_amd import utils
    Th0, N = precision_40(), 4000
    assert np.linalg.eigvalsh(Th0).min() > 0
    rng = np.random.default_rng(seed)
    X = np.linalg.cholesky(np.linalg.inv(Th0)) @ rng.standard_normal((40, N))
    T, SE = utils.host_debiased_precision(Th0, np.cov(X, bias=True), N)
    iu = np.triu_indices(40)
    piv = ((T - Th0) / SE)[iu]
    assert piv.size == 820
    cover = np.mean(np.abs(piv) <= ndtri(0.975))
    print(f"seed {seed}: sd {piv.std():.3f}, mean {piv.mean():+.3f}, coverage {cover:.3f}")
    assert 0.9 <= piv.std() <= 1.1
    assert abs(piv.mean()) <= 0.15
    assert 0.92 <= cover <= 0.98
    ci = utils.edge_tests(T, SE, alpha=0.05)
    assert np.mean((ci["ci_low"][iu] <= Th0[iu]) & (Th0[iu] <= ci["ci_high"][iu])) == cover


def test_differential_tests():
    from scipy.special import erfc
    from gglasso_amd import utils
    # by hand: T_a - T_b = 0.6, SE_a = 0.3, SE_b = 0.4 -> z = 0.6 / 0.5 = 1.2
    T = np.array([[[2.0, 0.9], [0.9, 2.0]], [[2.0, 0.3], [0.3, 1.0]]])
    SE = np.array([[[0.3, 0.3], [0.3, 0.3]], [[0.4, 0.4], [0.4, 0.4]]])
    (d,) = utils.differential_tests(T, SE)
    assert d["pair"] == (0, 1)
    assert abs(d["z"][0, 1] - 1.2) < 1e-15 and d["z"][0, 0] == 0.0 and abs(d["z"][1, 1] - 2.0) < 1e-15
    assert abs(d["pvalue"][0, 1] - erfc(1.2 / np.sqrt(2))) < 1e-16
    assert d["pvalue_adj"][0, 1] == d["pvalue"][0, 1] and not d["reject"].any()      # one pair in the family
    Th, Sm = dr.inputs(17, "cov", 3)
    T, SE = utils.host_debiased_precision(Th, Sm, dr.n_of(3))
    cons = utils.differential_tests(T, SE, alpha=0.1)
    assert [c["pair"] for c in cons] == [(0, 1), (1, 2)]
    ab, ba = utils.differential_tests(T, SE, pairs=[(0, 2), (2, 0)], alpha=0.1)
    assert np.array_equal(ab["z"], -ba["z"]) and np.array_equal(ab["pvalue"], ba["pvalue"])      # antisymmetric in the pair
    assert np.array_equal(ab["reject"], ba["reject"]) and ab["reject"].any()
    iu = np.triu_indices(17, 1)
    adj, rej = utils.adjust_pvalues(ab["pvalue"][iu], 0.1, "bh")
    assert np.array_equal(ab["pvalue_adj"][iu], adj) and np.array_equal(ab["reject"][iu], rej)
    for key in ("z", "pvalue", "pvalue_adj", "reject"):
        assert np.array_equal(ab[key], ab[key].T, equal_nan=True)
    # identical instances: zero everywhere, nothing rejected
    (same,) = utils.differential_tests(np.stack([T[0], T[0]]), np.stack([SE[0], SE[1]]))
    assert not same["z"].any() and np.all(same["pvalue"] == 1.0) and not same["reject"].any()
    with pytest.raises(AssertionError, match="a pair names two different instances"):
        utils.differential_tests(T, SE, pairs=[(0, 3)])
    with pytest.raises(AssertionError, match="compare the instances"):
        utils.differential_tests(T[0], SE[0])


# ---------------------------------------------------------------------------------------------------------------------
# glasso_problem.edge_inference(host=True)
# ---------------------------------------------------------------------------------------------------------------------
ATTRS = ("debiased_precision_", "standard_error_", "zscore_", "pvalue_", "pvalue_adj_", "significant_")


def fitted(problem, K=None, p=12, N=300, **kw):
    """A problem with a solution set by hand: S the covariance of data, Theta a thresholded inverse (any SPD matrix does)."""
    rng = np.random.default_rng(11)
    Ss, Ths = [], []
    for _ in range(K or 1):
        X = rng.standard_normal((p, N)) * rng.uniform(0.5, 3.0, (p, 1))
        X[1:] += 0.5 * X[:-1]
        S = np.cov(X, bias=True)
        Th = np.linalg.inv(S + 0.1 * np.diag(np.diag(S)))
        Th[np.abs(Th) < 0.02 * np.sqrt(np.outer(np.diag(Th), np.diag(Th)))] = 0.0
        Ss.append(S)
        Ths.append(Th)
    S, Th = (Ss[0], Ths[0]) if K is None else (np.stack(Ss), np.stack(Ths))
    P = problem.glasso_problem(S, N if K is None else N * np.ones(K), **kw)
    return P, S, Th


@pytest.mark.parametrize("K", [None, 3])
def test_edge_inference_sets_the_attributes(host, K):
    from gglasso_amd import utils
    P, S, Th = fitted(host, K)
    with pytest.raises(AssertionError, match="needs a solution"):
        P.edge_inference(host=True)
    P.solution._set_solution(Theta=Th)
    P.edge_inference(alpha=0.1, method="bonferroni", host=True, differential="all" if K else None)
    sol = P.solution
    shape = Th.shape
    for name in ATTRS:
        a = getattr(sol, name)
        assert a.shape == shape, name
        assert np.array_equal(a, np.swapaxes(a, -1, -2), equal_nan=True), name
    lo, hi = sol.confidence_interval_
    assert lo.shape == hi.shape == shape and np.all(lo < sol.debiased_precision_) and np.all(sol.debiased_precision_ < hi)
    T, SE = utils.host_debiased_precision(Th, S, 300)
    ref = utils.edge_tests(T, SE, alpha=0.1, method="bonferroni")
    assert np.array_equal(sol.debiased_precision_, T) and np.array_equal(sol.standard_error_, SE)
    assert np.array_equal(sol.zscore_, ref["z"]) and np.array_equal(sol.significant_, ref["reject"].astype(int))
    assert sol.significant_.dtype == sol.adjacency_.dtype and 0 < sol.significant_.sum() < sol.significant_.size
    assert not sol.significant_[..., np.arange(12), np.arange(12)].any()
    if K:
        assert [d["pair"] for d in sol.differential_] == [(0, 1), (0, 2), (1, 2)]
        assert all(d["z"].shape == (12, 12) for d in sol.differential_)
        P.edge_inference(host=True, differential="consecutive")
        assert [d["pair"] for d in sol.differential_] == [(0, 1), (1, 2)]
        P.edge_inference(host=True, differential=[(2, 0)])
        assert [d["pair"] for d in sol.differential_] == [(2, 0)]
        P.edge_inference(host=True)
        assert sol.differential_ is None
    else:
        with pytest.raises(ValueError, match="this is a single one"):
            P.edge_inference(host=True, differential="consecutive")


@pytest.mark.parametrize("K", [None, 3])
def test_zscores_do_not_depend_on_do_scaling(host, K):
    """Theta' = D Theta D against S' = D^-1 S D^-1 gives T' = D T D and SE' = d_i d_j SE: the same z.  The scaled problem is
    handed what its solver would return (the estimate on the correlations' scale) through ``_keep``."""
    import warnings
    P, S, Th = fitted(host, K)
    P.solution._set_solution(Theta=Th)
    P.edge_inference(host=True)
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        Q, _, _ = fitted(host, K, do_scaling=True)
    sd = np.sqrt(np.diagonal(S, axis1=-2, axis2=-1))
    Q._keep({"Theta": Th * sd[..., :, None] * sd[..., None, :]})
    Q.edge_inference(host=True)
    z, zq = P.solution.zscore_, Q.solution.zscore_
    assert np.abs(zq - z).max() <= 1e-12 * np.abs(z).max()
    assert np.all(np.abs(zq - z) <= 1e-12 * np.abs(z) + 1e-13)
    assert np.array_equal(P.solution.significant_, Q.solution.significant_)
    if K is None:        # a single problem's solution goes back to the covariances' scale
        assert np.allclose(Q.solution.debiased_precision_, P.solution.debiased_precision_, rtol=1e-10, atol=1e-12)
    else:                # a stack's stays on the correlations' scale (class docstring): T' = D T D
        assert np.allclose(Q.solution.debiased_precision_,
                           P.solution.debiased_precision_ * sd[..., :, None] * sd[..., None, :], rtol=1e-10, atol=1e-12)


def test_edge_inference_refusals(host):
    rng = np.random.default_rng(3)
    X = rng.standard_normal((6, 80))
    Th = np.eye(6)
    P, _, Th12 = fitted(host, None, latent=True)
    P.solution._set_solution(Theta=Th12, L=np.zeros_like(Th12))
    with pytest.raises(ValueError, match="latent variables: Theta is then not the precision matrix"):
        P.edge_inference(host=True)
    S2 = {0: np.eye(3), 1: np.eye(4)}
    G = np.array([[[0, 0]], [[1, 1]]])
    P = host.glasso_problem(S2, 50, G=G)
    P.solution._set_solution(Theta=S2)
    with pytest.raises(ValueError, match="different dimension"):
        P.edge_inference(host=True)
    for kw, text in ((dict(correlation="kendall"), r"correlation='kendall'"), (dict(correlation="mixed"), r"correlation='mixed'"),
                     (dict(missing="pairwise"), r"missing='pairwise'"), (dict(project=True), r"project=True")):
        Xk = np.where(X > 0, 1.0, 0.0) if kw.get("correlation") == "mixed" else X
        P = host.glasso_problem.from_data(Xk, **kw)
        P.solution._set_solution(Theta=Th)
        with pytest.raises(ValueError, match=text + r".*Gaussian sample covariance"):
            P.edge_inference(host=True)
    P = host.glasso_problem.from_data(X)
    P.solution._set_solution(Theta=Th)
    with pytest.raises(ValueError, match="differential must be None"):
        P.multiple = True
        P.edge_inference(host=True, differential="every")
    P.multiple = False
    P.edge_inference(host=True)                   # the plain problem from data is served
    assert P.solution.zscore_.shape == (6, 6)
