"""StARS stability selection, host side (no GPU): the subsample rule, the choice on an instability curve, and
``stars_search`` on its host route (numpy covariances, numpy counts) with the batch's array work done by the test-only
oracle engine.  The end-to-end problem is the one of tests/test_gpu_stars.py: a chain graph with one extra edge, p = 16,
N = 400, B = 12 subsamples of 200, whose integer sums at tol = rtol = 1e-8 are NUM below (cuts: 432 for beta = 0.05,
864 for beta = 0.1; the last value is smaller than the one before it, which is why the running maximum matters)."""
import warnings

import numpy as np
import pytest

NUM = [154, 274, 593, 1154, 1931, 2626, 2929, 2202]
LAM = [0.5, 0.35, 0.25, 0.18, 0.12, 0.08, 0.05, 0.02]


def stars_problem():
    p, N, B = 16, 400, 12
    Th = np.eye(p)
    Th[np.arange(p - 1), np.arange(1, p)] = Th[np.arange(1, p), np.arange(p - 1)] = 0.4
    Th[0, 5] = Th[5, 0] = 0.3
    X = np.linalg.cholesky(np.linalg.inv(Th)) @ np.random.default_rng(7).standard_normal((p, N))
    indices = np.stack([np.sort(np.random.default_rng([3, r]).choice(N, 200, replace=False)) for r in range(B)])
    return X, indices


def numpy_counts(THETA, t):
    """(counts (L,p,p), num (L,)) of the specification, straight from the definition."""
    L, B, p, _ = THETA.shape
    iu = np.triu_indices(p, 1)
    counts = np.zeros((L, p, p), dtype=np.int64)
    for l in range(L):
        c = np.zeros((p, p), dtype=np.int64)
        for r in range(B):
            c[iu] += (np.abs(THETA[l, r]) >= t)[iu]
        counts[l] = c + c.T
    num = np.array([int(np.sum(counts[l][iu] * (B - counts[l][iu]))) for l in range(L)])
    return counts, num


@pytest.fixture()
def oracle_engine(monkeypatch):
    from gglasso_amd import solver
    from oracle_engine import OracleEngine
    monkeypatch.setattr(solver, "ENGINE", OracleEngine)
    return OracleEngine


def test_stars_subsamples_rule():
    from gglasso_amd.model_selection import stars_subsamples
    for N, b in ((100, 80), (144, 115), (145, 120), (400, 200)):
        idx = stars_subsamples(N, 5)
        assert idx.shape == (5, b) and idx.dtype == np.int32, (N, idx.shape)
        assert np.all(np.diff(idx, axis=1) > 0)                        # sorted, no duplicates
        assert idx.min() >= 0 and idx.max() < N
    idx = stars_subsamples(400, 4, seed=3)
    for r in range(4):
        assert np.array_equal(idx[r], np.sort(np.random.default_rng([3, r]).choice(400, 200, replace=False)))
    assert np.array_equal(idx, stars_subsamples(400, 4, seed=3))
    assert not np.array_equal(idx, stars_subsamples(400, 4, seed=4))
    assert not np.array_equal(idx[0], idx[1])
    assert stars_subsamples(400, 2, subsample_size=7).shape == (2, 7)
    assert stars_subsamples(1, 3).shape == (3, 1)                      # int(0.8) = 0: at least one observation
    with pytest.raises(AssertionError):
        stars_subsamples(10, 2, subsample_size=11)


def test_stars_select_on_hand_made_curves():
    from gglasso_amd.model_selection import stars_select
    p, B = 16, 12
    D = np.array([2 * n / (B * B * (p * (p - 1) // 2)) for n in NUM])
    with warnings.catch_warnings():
        warnings.simplefilter("error")
        ix, Dbar = stars_select(D, 0.05)
        assert ix == 1 and np.array_equal(Dbar, np.maximum.accumulate(D))
        assert Dbar[-1] == D[-2] > D[-1]
        assert stars_select(D, 0.1)[0] == 2
        assert stars_select(D, 1.0)[0] == len(D) - 1
        # a dip below beta behind a point above it is not chosen: the running maximum decides
        assert stars_select([0.01, 0.2, 0.02, 0.03], 0.05)[0] == 0
        assert stars_select([0.01, 0.02, 0.05], 0.05)[0] == 2          # <= beta
        # a NaN is never chosen and does not enter the running maximum
        ix, Dbar = stars_select([0.01, 0.02, np.nan, 0.03, 0.2], 0.05)
        assert ix == 3 and np.array_equal(Dbar, [0.01, 0.02, 0.02, 0.03, 0.2])
        assert stars_select([0.01, 0.02, np.nan, 0.2], 0.05)[0] == 1
        assert stars_select([np.nan, 0.02, 0.2], 0.05)[0] == 1
    with pytest.warns(RuntimeWarning, match="no lambda1"):
        ix, Dbar = stars_select([0.3, 0.4, 0.2], 0.05)
    assert ix == 0 and np.array_equal(Dbar, [0.3, 0.4, 0.4])


@pytest.fixture(scope="module")
def host_run():
    """One host-route run shared by the tests below (array work: the test-only oracle engine)."""
    from gglasso_amd import solver, model_selection as ms
    from oracle_engine import OracleEngine
    X, indices = stars_problem()
    keep, solver.ENGINE = solver.ENGINE, OracleEngine
    try:
        sol, stats = ms.stars_search(X, LAM[::-1], beta=0.05, indices=indices, tol=1e-8, rtol=1e-8, store_all=True)
    finally:
        solver.ENGINE = keep
    return X, indices, sol, stats


def test_stars_search_host_route(host_run):
    from gglasso_amd import model_selection as ms
    X, indices, sol, stats = host_run
    p, B = 16, 12
    assert np.array_equal(stats['LAMBDA'], LAM)                         # sorted in descending order
    assert stats['NUM'] == NUM and all(isinstance(n, int) for n in stats['NUM'])
    assert stats['IX'] == 1 and stats['BEST'] == {'lambda1': 0.35}
    assert ms.stars_select(stats['INSTABILITY'], 0.1)[0] == 2
    counts, num = numpy_counts(stats['THETA'], 1e-8)
    assert np.array_equal(stats['COUNTS'], counts) and list(num) == NUM
    assert stats['COUNTS'].shape == (8, p, p) and stats['THETA'].shape == (8, B, p, p)
    D = np.array([2 * n / (B * B * (p * (p - 1) // 2)) for n in NUM])
    assert np.array_equal(stats['INSTABILITY'], D)
    assert np.array_equal(stats['INSTABILITY_MONOTONE'], np.maximum.accumulate(D))
    assert np.array_equal(stats['INDICES'], indices) and stats['subsample_size'] == 200 and stats['n_subsamples'] == B
    assert stats['FAILED'] == []
    # every point is the single solve on the subsample's numpy covariance
    from oracle import ggl_oracle as orc
    S3 = np.cov(X[:, indices[3]], bias=True)
    ref, _ = orc.ADMM_SGL(S3, LAM[2], np.eye(p), X_0=np.eye(p), tol=1e-8, rtol=1e-8)
    assert np.abs(stats['THETA'][2, 3] - ref['Theta']).max() <= 1e-10
    ref, _ = orc.ADMM_SGL(np.cov(X, bias=True), 0.35, np.eye(p), X_0=np.eye(p), tol=1e-8, rtol=1e-8)
    assert sorted(sol) == ['Omega', 'Theta', 'X'] and np.abs(sol['Theta'] - ref['Theta']).max() <= 1e-10


def test_stars_search_chunks_and_plain_stats(oracle_engine, host_run):
    from gglasso_amd import model_selection as ms
    X, indices, sol, stats = host_run
    sol2, st2 = ms.stars_search(X, LAM, beta=0.1, indices=indices, tol=1e-8, rtol=1e-8, lambdas_per_batch=3)
    assert st2['NUM'] == NUM and st2['IX'] == 2
    assert 'THETA' not in st2 and 'COUNTS' not in st2


def test_stars_search_failed_point(oracle_engine, monkeypatch, host_run):
    """A point of lambda index 4 that ends as 'solver error': that lambda has no instability, is named and not chosen."""
    from gglasso_amd import solver, model_selection as ms
    X, indices, sol, stats = host_run
    B = 12

    class Failing(oracle_engine):
        def sgl_batch_step(self, rho, lambda1, latent, mu1):
            out = super().sgl_batch_step(rho, lambda1, latent, mu1)
            out[4 * B + 5] = np.nan
            return out

    monkeypatch.setattr(solver, "ENGINE", Failing)
    with pytest.warns(RuntimeWarning) as rec:
        sol2, st2 = ms.stars_search(X, LAM, beta=0.05, indices=indices, tol=1e-8, rtol=1e-8)
    assert any("StARS: a subsample failed at lambda1 = [0.12]" in str(w.message) for w in rec)
    assert st2['FAILED'] == [4] and np.isnan(st2['INSTABILITY'][4])
    keep = [l for l in range(8) if l != 4]
    assert np.array_equal(st2['INSTABILITY'][keep], stats['INSTABILITY'][keep])
    assert st2['INSTABILITY_MONOTONE'][4] == st2['INSTABILITY'][3]
    assert st2['IX'] == 1 and st2['BEST'] == {'lambda1': 0.35}
    assert np.array_equal(sol2['Theta'], sol['Theta'])


def test_binding_has_the_stars_entry_points():
    from gglasso_amd import _lib
    for name in ("ggl_covariance_subsets", "ggl_set_S_from_subsets", "ggl_edge_stability"):
        assert name in _lib.EXPORTS
    assert _lib.ABI_VERSION == 300


def test_stability_selection_refusals_need_no_device():
    """The assertions of glasso_problem.stability_selection come before any work (problems built from covariances)."""
    from gglasso_amd.problem import glasso_problem
    S = np.eye(4)
    grid = {'lambda1_range': np.array([0.5, 0.1])}
    with pytest.raises(AssertionError, match="from_data"):
        glasso_problem(S, 50).stability_selection(grid)
    with pytest.raises(AssertionError, match="from_data"):
        glasso_problem(np.stack([S, S]), 50).stability_selection(grid)


def test_device_route_hands_the_engine_one_placeholder_matrix(oracle_engine, monkeypatch, host_run):
    """The driver's device route on an engine that has the two methods (numpy behind them here): the S the engine is built
    with is a stride-0 view of ONE matrix -- nothing of size K p p exists on the host or is uploaded -- the real S arrives
    through set_data_subsets, and the statistics are those of the host route."""
    from gglasso_amd import solver, model_selection as ms
    X, indices, sol, stats = host_run
    seen = []

    class WithStars(oracle_engine):
        def __init__(self, S, *a, **k):
            seen.append((np.shape(S), np.asarray(S).strides[0]))
            super().__init__(S, *a, **k)

        def set_data_subsets(self, X_, idx, center=True, scale=False):
            S = ms._host_subset_covariances(np.asarray(X_), np.asarray(idx), center, scale)
            self.S = np.tile(S, (self.K // len(S), 1, 1))

        def edge_stability(self, B, t=1e-8, counts=False):
            cnt, num = ms._host_edge_counts(self._snapT.reshape(self.K // B, B, self.p, self.p), t)
            return (num, cnt) if counts else num

    from gglasso_amd import utils
    monkeypatch.setattr(solver, "ENGINE", WithStars)
    # (the covariance of all observations for the final solve is the device operator's on this route: numpy stands in)
    monkeypatch.setattr(utils, "sample_covariance", lambda X_, center=True, scale=False:
                        ms._host_subset_covariances(X_, np.arange(X_.shape[1])[None], center, scale)[0])
    sol2, st2 = ms.stars_search(X, LAM, beta=0.05, indices=indices, tol=1e-8, rtol=1e-8, store_all=True)
    assert seen[0] == ((96, 16, 16), 0), seen[0]                      # the batch's engine: a broadcast view
    assert st2['NUM'] == NUM and st2['IX'] == 1
    assert np.array_equal(st2['COUNTS'], stats['COUNTS']) and np.array_equal(st2['THETA'], stats['THETA'])
    assert np.array_equal(sol2['Theta'], sol['Theta'])
    sol3, st3 = ms.stars_search(X, LAM, beta=0.05, indices=indices, tol=1e-8, rtol=1e-8)
    assert st3['NUM'] == NUM and 'THETA' not in st3
