"""Meinshausen-Buhlmann neighbourhood selection without a GPU: the numpy twin (``utils.host_neighborhood_selection``) against
the longdouble comparison value and the derived bounds of tests/mb_ref.py (sizes up to 65), the edges of the method, the
graph rule, ``stars_search(method='mb')`` on its host route and -- numpy behind a stub engine -- on its device route, and the
bookkeeping of the new entry points."""
import os
import re
import warnings

import numpy as np
import pytest

import mb_ref
from conftest import ROOT

TOL = 1e-7
SIZES = tuple(p for p in mb_ref.SIZES if p <= 65)


@pytest.fixture(scope="module")
def twin():
    from gglasso_amd import utils
    cache = {}

    def run(p):
        if p not in cache:
            cache[p] = utils.host_neighborhood_selection(mb_ref.stack(p), mb_ref.GRID, 'and', tol=TOL, return_info=True)
        return cache[p]
    return run


@pytest.mark.parametrize("p", SIZES)
def test_twin_against_the_comparison_value(twin, p):
    """Checks 1-5: optimality residual, distance to the solution, supports and graphs, the symmetrised matrix, the residual
    variance, for the three seeds as one stack."""
    from gglasso_amd import utils
    W, info = twin(p)
    assert W.shape == (3, 4, p, p) and np.array_equal(info['LAMBDA'], mb_ref.GRID)
    Wor = utils.host_neighborhood_selection(mb_ref.stack(p), mb_ref.GRID, 'or', tol=TOL)
    for seed in range(3):
        _, ok = mb_ref.check_case(p, seed, info['COEF'][seed], info['RESVAR'][seed], info['STATUS'][seed], TOL, "twin")
        for rule, Wr in (('and', W[seed]), ('or', Wor[seed])):
            mb_ref.check_graphs(p, seed, Wr, rule, ok)
            assert np.array_equal(Wr, Wr.transpose(0, 2, 1)) and np.all(np.diagonal(Wr, axis1=1, axis2=2) == 0)
            assert np.array_equal(Wr, mb_ref.and_or(info['COEF'][seed], rule))


def test_twin_bits(twin):
    """Check 6 on the twin: two calls, one matrix of a stack alone, the leading part of a grid."""
    from gglasso_amd import utils
    p = 17
    W, info = twin(p)
    W2, info2 = utils.host_neighborhood_selection(mb_ref.stack(p), mb_ref.GRID, 'and', tol=TOL, return_info=True)
    assert np.array_equal(W, W2) and all(np.array_equal(info[k], info2[k]) for k in info)
    W1, info1 = utils.host_neighborhood_selection(mb_ref.stack(p)[1], mb_ref.GRID, 'and', tol=TOL, return_info=True)
    assert W1.shape == (4, p, p) and np.array_equal(W1, W[1]) and all(np.array_equal(info1[k], info[k][1]) for k in info if k != 'LAMBDA')
    Wh, infoh = utils.host_neighborhood_selection(mb_ref.stack(p), mb_ref.GRID[:2], 'and', tol=TOL, return_info=True)
    assert np.array_equal(Wh, W[:, :2]) and np.array_equal(infoh['COEF'], info['COEF'][:, :2])
    assert np.array_equal(infoh['SWEEPS'], info['SWEEPS'][:, :2])
    # the grid is used in descending order whatever order it is given in
    Wr = utils.host_neighborhood_selection(mb_ref.stack(p), mb_ref.GRID[::-1], 'and', tol=TOL)
    assert np.array_equal(Wr, W)


def test_twin_edges_of_the_method():
    """Check 7 on the twin."""
    from gglasso_amd import utils
    S = mb_ref.stack(17)[0]
    top = float(np.abs(S - np.diag(np.diag(S))).max())
    W, info = utils.host_neighborhood_selection(S, (top * 1.01, 0.1), 'or', tol=TOL, return_info=True)
    assert not W[0].any() and not info['COEF'][0].any() and not info['SWEEPS'][0].any() and not info['STATUS'].any()
    assert np.array_equal(info['RESVAR'][0], np.diag(S)) and W[1].any()
    # p = 1
    W, info = utils.host_neighborhood_selection(np.array([[2.0]]), mb_ref.GRID, 'and', return_info=True)
    assert W.shape == (4, 1, 1) and not W.any() and not info['STATUS'].any() and np.all(info['RESVAR'] == 2.0)
    # an uncorrelated variable stays isolated
    S = mb_ref.stack(17)[1].copy()
    S[4, :] = S[:, 4] = 0.0
    S[4, 4] = 1.0
    W, info = utils.host_neighborhood_selection(S, mb_ref.GRID, 'or', tol=TOL, return_info=True)
    assert not W[:, 4, :].any() and not W[:, :, 4].any() and not info['COEF'][:, 4, :].any() and not info['STATUS'].any()
    # two identical variables: S singular
    S5 = mb_ref.stack(5)[0].copy()
    S5[1, :], S5[:, 1] = S5[0, :], S5[:, 0]
    S5[1, 1] = S5[0, 1] = S5[1, 0] = S5[0, 0]
    W, info = utils.host_neighborhood_selection(S5, mb_ref.GRID, 'and', tol=TOL, return_info=True)
    assert np.all(info['STATUS'] <= 1) and np.all(np.isfinite(info['COEF']))
    mb_ref.check_residual_where_converged(S5, mb_ref.GRID, info['COEF'], info['STATUS'], TOL)
    # one sweep is not enough at the smallest lambda
    W, info = utils.host_neighborhood_selection(mb_ref.stack(17)[0], mb_ref.GRID[-1:], 'and', tol=TOL, max_sweeps=1, return_info=True)
    assert np.all(info['STATUS'] == 1) and np.all(info['SWEEPS'] == 1) and np.all(np.isfinite(info['COEF']))
    assert np.all(np.isfinite(info['RESVAR'])) and np.all(np.isfinite(W))


def test_twin_non_finite_matrix():
    """A NaN in S: status 2 for every node it reaches, NaN coefficients from there on, nobody else touched."""
    from gglasso_amd import utils
    S = mb_ref.stack(5).copy()
    S[1, 2, 3] = S[1, 3, 2] = np.nan
    W, info = utils.host_neighborhood_selection(S, mb_ref.GRID, 'and', tol=TOL, return_info=True)
    clean = utils.host_neighborhood_selection(mb_ref.stack(5), mb_ref.GRID, 'and', tol=TOL, return_info=True)[1]
    assert np.array_equal(info['COEF'][[0, 2]], clean['COEF'][[0, 2]]) and not info['STATUS'][[0, 2]].any()
    assert np.all(info['STATUS'][1][:, [2, 3]] == 2)                       # their own column s_j holds the NaN
    bad = info['STATUS'][1] == 2
    assert np.all(np.isnan(info['RESVAR'][1][bad]))
    for l, j in np.argwhere(bad):
        col = info['COEF'][1, l, :, j]
        assert col[j] == 0 and np.all(np.isnan(np.delete(col, j)))
        assert np.all(info['STATUS'][1, l:, j] == 2)


def test_arguments_are_refused_on_the_host():
    from gglasso_amd import utils
    S = mb_ref.stack(5)[0]
    for kw in (dict(lambda_range=(0.1, -0.2)), dict(lambda_range=(0.1, np.inf)), dict(lambda_range=(0.1, 0.1)),
               dict(lambda_range=()), dict(rule='xor'), dict(tol=-1.0), dict(tol=np.nan), dict(max_sweeps=0)):
        args = dict(lambda_range=mb_ref.GRID)
        args.update(kw)
        with pytest.raises(AssertionError):
            utils.host_neighborhood_selection(S, **args)
    with pytest.raises(AssertionError):
        utils.host_neighborhood_selection(np.zeros((3, 4)), mb_ref.GRID)


def test_graph_rule_ties_and_signs():
    from gglasso_amd import utils
    raw = np.array([[0.0, 0.5, -0.2, 0.0], [-0.5, 0.0, 0.3, 0.0], [0.1, -0.3, 0.0, 0.7], [0.0, 0.0, 0.0, 0.0]])
    for rule in ('and', 'or'):
        W = utils.neighborhood_graph(raw, rule)
        assert np.array_equal(W, mb_ref.and_or(raw, rule)) and np.array_equal(W, W.T)
    assert utils.neighborhood_graph(raw, 'and')[0, 1] == 0.5 and utils.neighborhood_graph(raw, 'or')[1, 2] == 0.3   # ties: a
    assert utils.neighborhood_graph(raw, 'and')[2, 3] == 0.0 and utils.neighborhood_graph(raw, 'or')[2, 3] == 0.7


class _NoDeviceRoute:
    """An engine without ``set_data_subsets``: ``stars_search`` takes its host route and never builds one."""


def _stars_inputs():
    from gglasso_amd import model_selection as ms
    X = mb_ref.stars_data()
    idx = ms.stars_subsamples(X.shape[1], 6, None, seed=5)
    return X, idx


@pytest.mark.parametrize("rule", ("and", "or"))
def test_stars_host_route(monkeypatch, rule):
    """Check 10 through the twin."""
    from gglasso_amd import model_selection as ms, solver, utils
    monkeypatch.setattr(solver, "ENGINE", _NoDeviceRoute)
    X, idx = _stars_inputs()
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        sol, stats = ms.stars_search(X, mb_ref.GRID, n_subsamples=6, seed=5, beta=0.1, scale=True, tol=TOL, store_all=True,
                                     method='mb', rule=rule)
        _, per1 = ms.stars_search(X, mb_ref.GRID, n_subsamples=6, seed=5, beta=0.1, scale=True, tol=TOL, store_all=True,
                                  method='mb', rule=rule, lambdas_per_batch=1)
    assert np.array_equal(stats['INDICES'], idx) and stats['FAILED'] == []
    S_sub = ms._host_subset_covariances(X, idx, True, True)
    mb_ref.check_stars(stats, S_sub, mb_ref.GRID, rule, 1e-8, 0.1)
    mb_ref.check_stars(per1, S_sub, mb_ref.GRID, rule, 1e-8, 0.1)
    ix = stats['IX']
    S_full = ms._host_subset_covariances(X, np.arange(X.shape[1])[None], True, True)[0]
    W, info = utils.host_neighborhood_selection(S_full, mb_ref.GRID[:ix + 1], rule, tol=TOL, return_info=True)
    assert sorted(sol) == ['adjacency', 'coef', 'lambda1', 'resvar'] and sol['lambda1'] == mb_ref.GRID[ix]
    assert np.array_equal(sol['coef'], info['COEF'][ix]) and np.array_equal(sol['resvar'], info['RESVAR'][ix])
    assert np.array_equal(sol['adjacency'], W[ix] != 0) and sol['adjacency'].dtype == bool


def test_stars_kendall_host_route(monkeypatch):
    from gglasso_amd import model_selection as ms, solver, utils
    monkeypatch.setattr(solver, "ENGINE", _NoDeviceRoute)
    X, idx = _stars_inputs()
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        _, stats = ms.stars_search(np.exp(X), mb_ref.GRID, n_subsamples=6, seed=5, beta=0.1, tol=TOL, store_all=True,
                                   method='mb', correlation='kendall')
    mb_ref.check_stars(stats, utils.host_skeptic_correlation(np.exp(X), idx), mb_ref.GRID, 'and', 1e-8, 0.1)


def test_stars_device_route_with_numpy_behind_the_engine(monkeypatch):
    """The driver's device route: a ctx of B instances shaped by one placeholder matrix, the subsample matrices written by
    ``set_data_subsets``, one ``neighborhood_stability`` per batch of lambdas; statuses 2 and 1 become FAILED and a warning."""
    from gglasso_amd import model_selection as ms, solver, utils
    X, idx = _stars_inputs()
    seen = []

    class Stub:
        def __init__(self, S, Omega_0, Theta_0, X_0):
            assert S.shape == (6, 17, 17) and S.strides[0] == 0
            self.K, self.p = 6, 17
            seen.append('ctx')

        def set_data_subsets(self, X_, indices, center=True, scale=False):
            self.S = ms._host_subset_covariances(X_, indices, center, scale)

        def edge_stability(self, *a, **k):
            raise AssertionError("the glasso reduction is not part of the mb route")

        def neighborhood_stability(self, lam, rule, tol, t, counts, stack, max_sweeps=10000):
            W, info = utils.host_neighborhood_selection(self.S, lam, rule, tol=tol, max_sweeps=max_sweeps, return_info=True)
            Th = np.ascontiguousarray(np.swapaxes(W, 0, 1))
            cnt, num = ms._host_edge_counts(Th, t)
            status = np.swapaxes(info['STATUS'], 0, 1).copy()
            if len(seen) == 3:                                          # the second batch: lambda 3
                status[0, 1, 3] = 2
                status[0, 2, 5] = 1
            return {'num': num, 'counts': cnt, 'stack': Th, 'status': status, 'sweeps': np.swapaxes(info['SWEEPS'], 0, 1)}

        def close(self):
            seen.append('closed')

    monkeypatch.setattr(solver, "ENGINE", Stub)
    monkeypatch.setattr(utils, "neighborhood_selection", lambda S, lam, rule, tol, return_info, **k:
                        utils.host_neighborhood_selection(S, lam, rule, tol=tol, return_info=return_info))
    monkeypatch.setattr(utils, "sample_covariance", lambda X_, center=True, scale=False:
                        ms._host_subset_covariances(X_, np.arange(X_.shape[1])[None], center, scale))
    with pytest.warns(RuntimeWarning) as rec:
        sol, stats = ms.stars_search(X, mb_ref.GRID, n_subsamples=6, seed=5, beta=0.1, scale=True, tol=TOL, store_all=True,
                                     method='mb', lambdas_per_batch=3)
    assert seen == ['ctx', 'closed', 'ctx', 'closed']
    assert stats['FAILED'] == [3] and np.isnan(stats['INSTABILITY'][3]) and stats['IX'] < 3
    assert any("1 (subsample, lambda1, node) units reached a cap" in str(w.message) for w in rec)
    monkeypatch.setattr(solver, "ENGINE", _NoDeviceRoute)
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        _, host = ms.stars_search(X, mb_ref.GRID, n_subsamples=6, seed=5, beta=0.1, scale=True, tol=TOL, store_all=True,
                                  method='mb', lambdas_per_batch=3)
    assert stats['NUM'] == host['NUM'] and np.array_equal(stats['THETA'], host['THETA'])
    assert np.array_equal(stats['COUNTS'], host['COUNTS'])


def test_glasso_route_is_untouched(monkeypatch):
    """``method='glasso'`` and no ``method`` at all: the same bits."""
    from gglasso_amd import model_selection as ms, solver
    from oracle_engine import OracleEngine
    monkeypatch.setattr(solver, "ENGINE", OracleEngine)
    X = mb_ref.stars_data(p=6, N=60)
    kw = dict(n_subsamples=3, seed=2, beta=0.2, store_all=True, tol=1e-6, rtol=1e-6)
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        sol_a, st_a = ms.stars_search(X, (0.4, 0.2), **kw)
        sol_b, st_b = ms.stars_search(X, (0.4, 0.2), method='glasso', rule='or', **kw)
    assert sorted(st_a) == sorted(st_b) and sorted(sol_a) == sorted(sol_b)
    for k in ('LAMBDA', 'INSTABILITY', 'INSTABILITY_MONOTONE', 'INDICES', 'COUNTS', 'THETA'):
        assert np.array_equal(st_a[k], st_b[k], equal_nan=True), k
    for k in ('NUM', 'IX', 'BEST', 'FAILED', 'subsample_size', 'n_subsamples'):
        assert st_a[k] == st_b[k], k
    for k in sol_a:
        assert np.array_equal(sol_a[k], sol_b[k]), k
    with pytest.raises(AssertionError, match="method"):
        ms.stars_search(X, (0.4, 0.2), method='tiger')
    with pytest.raises(AssertionError, match="rule"):
        ms.stars_search(X, (0.4, 0.2), method='mb', rule='raw')


def test_entry_points_are_wired():
    from gglasso_amd import _lib, build, utils
    from gglasso_amd.solver import HipEngine
    names = ("ggl_neighborhood_path", "ggl_neighborhood_stability")
    assert all(n in _lib.EXPORTS for n in names)
    assert "neighborhood.hip" in build.SOURCES and "capi_neighborhood.hip" in build.SOURCES
    assert all(os.path.exists(os.path.join(build.CSRC, s)) for s in build.SOURCES)
    assert callable(getattr(HipEngine, "neighborhood_stability")) and callable(utils.neighborhood_selection)
    with open(os.path.join(ROOT, "include", "ggl_hip.h")) as f:
        head = f.read()
    m = re.search(r"^#define GGL_VERSION (\d+)", head, re.M)
    assert m and int(m.group(1)) == 300 == _lib.ABI_VERSION
    for name in names:
        assert name in head[:m.start()]                                     # the list of additions
        assert re.search(rf"^int {name}\(", head[m.end():], re.M), name
    with open(os.path.join(build.CSRC, "capi_internal.hpp")) as f:
        assert "capi_neighborhood.hip" in f.read()
    with open(os.path.join(build.CSRC, "kernels.hpp")) as f:
        assert re.search(r"MB_MAX_P = 2048", f.read())
