"""Meinshausen-Buhlmann neighbourhood selection on the device (csrc/neighborhood.hip behind ``ggl_neighborhood_path`` and
``ggl_neighborhood_stability``): the checks of tests/mb_ref.py against the longdouble comparison value at every size at which
the kernel takes another path or a lane falls off an edge, the bits, the edges of the method, non-finite data, the refusals of
the C ABI, and ``stars_search(method='mb')`` end to end."""
import warnings

import numpy as np
import pytest

import mb_ref

pytestmark = pytest.mark.gpu

TOL = 1e-7


@pytest.fixture(scope="module")
def device():
    from gglasso_amd import utils
    cache = {}

    def run(p):
        if p not in cache:
            cache[p] = utils.neighborhood_selection(mb_ref.stack(p), mb_ref.GRID, 'and', tol=TOL, return_info=True)
        return cache[p]
    return run


@pytest.mark.parametrize("p", mb_ref.SIZES)
def test_device_against_the_comparison_value(device, p):
    """Checks 1-5 for the stack of three seeds: optimality residual, distance to the solution, supports and graphs, the
    symmetrised matrix bit for bit, the residual variance."""
    from gglasso_amd import utils
    W, info = device(p)
    assert W.shape == (3, 4, p, p) and np.array_equal(info['LAMBDA'], mb_ref.GRID)
    Wor = utils.neighborhood_selection(mb_ref.stack(p), mb_ref.GRID, 'or', tol=TOL)
    for seed in range(3):
        _, ok = mb_ref.check_case(p, seed, info['COEF'][seed], info['RESVAR'][seed], info['STATUS'][seed], TOL, "device")
        for rule, Wr in (('and', W[seed]), ('or', Wor[seed])):
            mb_ref.check_graphs(p, seed, Wr, rule, ok)
            assert np.array_equal(Wr, Wr.transpose(0, 2, 1)) and np.all(np.diagonal(Wr, axis1=1, axis2=2) == 0)
            assert np.array_equal(Wr, utils.neighborhood_graph(info['COEF'][seed], rule))
    if p <= 65:
        assert np.array_equal(W[1], mb_ref.and_or(info['COEF'][1], 'and'))      # the definition, entry by entry


@pytest.mark.parametrize("p", (17, 65, 257, 300))
def test_device_bits(device, p):
    """Check 6: two calls, one matrix of a stack alone, the leading part of a grid."""
    from gglasso_amd import utils
    W, info = device(p)
    W2, info2 = utils.neighborhood_selection(mb_ref.stack(p), mb_ref.GRID, 'and', tol=TOL, return_info=True)
    assert np.array_equal(W, W2) and all(np.array_equal(info[k], info2[k]) for k in info)
    W1, info1 = utils.neighborhood_selection(mb_ref.stack(p)[1], mb_ref.GRID, 'and', tol=TOL, return_info=True)
    assert np.array_equal(W1, W[1]) and all(np.array_equal(info1[k], info[k][1]) for k in info if k != 'LAMBDA')
    Wh, infoh = utils.neighborhood_selection(mb_ref.stack(p), mb_ref.GRID[:2], 'and', tol=TOL, return_info=True)
    assert np.array_equal(Wh, W[:, :2]) and all(np.array_equal(infoh[k], info[k][:, :2]) for k in info if k != 'LAMBDA')


@pytest.mark.parametrize("p", (513, 1025))
def test_device_wide_variants(p):
    """The kernel's instantiations with 16 and 32 values per lane (p > 512, p > 1024), which no size of the list above
    reaches: every node converges, and check 1 -- the only one that needs no comparison value -- holds on a two-lambda grid;
    the symmetrised matrix is the host rule's."""
    from gglasso_amd import utils
    S, lam = mb_ref.case(p, 0), (0.2, 0.1)
    W, info = utils.neighborhood_selection(S, lam, 'and', tol=TOL, return_info=True)
    assert not info['STATUS'].any() and W[1].any()
    mb_ref.check_residual_where_converged(S, lam, info['COEF'], info['STATUS'], TOL)
    assert np.array_equal(W, utils.neighborhood_graph(info['COEF'], 'and'))


def test_device_edges_of_the_method():
    """Check 7."""
    from gglasso_amd import utils
    S = mb_ref.stack(17)[0]
    top = float(np.abs(S - np.diag(np.diag(S))).max())
    W, info = utils.neighborhood_selection(S, (top * 1.01, 0.1), 'or', tol=TOL, return_info=True)
    assert not W[0].any() and not info['COEF'][0].any() and not info['SWEEPS'][0].any() and not info['STATUS'].any()
    assert np.array_equal(info['RESVAR'][0], np.diag(S)) and W[1].any()
    W, info = utils.neighborhood_selection(np.array([[2.0]]), mb_ref.GRID, 'and', return_info=True)
    assert W.shape == (4, 1, 1) and not W.any() and not info['STATUS'].any() and np.all(info['RESVAR'] == 2.0)
    S = mb_ref.stack(65)[1].copy()
    S[64, :] = S[:, 64] = 0.0
    S[64, 64] = 1.0
    W, info = utils.neighborhood_selection(S, mb_ref.GRID, 'or', tol=TOL, return_info=True)
    assert not W[:, 64, :].any() and not W[:, :, 64].any() and not info['COEF'][:, 64, :].any() and not info['STATUS'].any()
    S5 = mb_ref.stack(5)[0].copy()
    S5[1, :], S5[:, 1] = S5[0, :], S5[:, 0]
    S5[1, 1] = S5[0, 1] = S5[1, 0] = S5[0, 0]
    W, info = utils.neighborhood_selection(S5, mb_ref.GRID, 'and', tol=TOL, return_info=True)
    assert np.all(info['STATUS'] <= 1) and np.all(np.isfinite(info['COEF']))
    mb_ref.check_residual_where_converged(S5, mb_ref.GRID, info['COEF'], info['STATUS'], TOL)
    W, info = utils.neighborhood_selection(mb_ref.stack(17)[0], mb_ref.GRID[-1:], 'and', tol=TOL, max_sweeps=1, return_info=True)
    assert np.all(info['STATUS'] == 1) and np.all(info['SWEEPS'] == 1) and np.all(np.isfinite(info['COEF']))
    assert np.all(np.isfinite(info['RESVAR'])) and np.all(np.isfinite(W))


def _path_call(S, lam, rule=1, tol=TOL, max_sweeps=100, M=None, p=None, L=None, coef=True, info=True, s_null=False,
               lam_null=False):
    """One raw ``ggl_neighborhood_path`` call with sentinel-filled outputs: (rc, message, coef, resvar, info)."""
    from gglasso_amd import _lib
    lib = _lib.load()
    S = np.ascontiguousarray(S, dtype=np.float64)
    lam = np.ascontiguousarray(lam, dtype=np.float64)
    M = S.shape[0] if M is None else M
    p = S.shape[-1] if p is None else p
    L = lam.size if L is None else L
    n = max(1, S.shape[0]) * max(1, lam.size) * S.shape[-1]
    C, R = np.full(n * S.shape[-1], -7.5), np.full(n, -7.5)
    I = np.full(n * 2, -7, dtype=np.int32)
    rc = lib.ggl_neighborhood_path(0, M, p, None if s_null else _lib.ptr(S), L, None if lam_null else _lib.ptr(lam), rule,
                                   tol, max_sweeps, _lib.ptr(C) if coef else None, _lib.ptr(R),
                                   I.ctypes.data_as(_lib._ip) if info else None)
    return rc, _lib.last_error(), C, R, I


def test_refusals_write_nothing():
    """Check 9 and the second half of check 8: GGL_E_ARG before any device work, the outputs keep their sentinel."""
    from gglasso_amd import _lib
    S = mb_ref.stack(5).copy()
    lam = np.array(mb_ref.GRID)
    bad_S, neg_d = S.copy(), S.copy()
    bad_S[1, 2, 3] = np.nan
    neg_d[2, 4, 4] = 0.0
    cases = {
        "M": dict(M=0), "L": dict(L=0), "p": dict(p=0), "p max": dict(p=2049), "S NULL": dict(s_null=True),
        "lam NULL": dict(lam_null=True), "coef NULL": dict(coef=False), "info NULL": dict(info=False),
        "lambda 0": dict(lam=[0.4, 0.0]), "lambda < 0": dict(lam=[0.4, -0.1]), "lambda inf": dict(lam=[np.inf, 0.1]),
        "lambda nan": dict(lam=[0.4, np.nan]), "ascending": dict(lam=[0.1, 0.4]), "equal": dict(lam=[0.4, 0.4]),
        "tol < 0": dict(tol=-1e-9), "tol nan": dict(tol=np.nan), "tol inf": dict(tol=np.inf), "sweeps": dict(max_sweeps=0),
        "rule": dict(rule=3), "rule < 0": dict(rule=-1), "S nan": dict(S=bad_S), "diagonal": dict(S=neg_d),
    }
    for name, kw in cases.items():
        args = dict(S=S, lam=lam)
        args.update(kw)
        rc, msg, C, R, I = _path_call(**args)
        assert rc == _lib.E_ARG, (name, rc, msg)
        assert np.all(C == -7.5) and np.all(R == -7.5) and np.all(I == -7), name
        if name == "S nan":
            assert "matrix 1" in msg and "(2, 3)" in msg, msg
        if name == "diagonal":
            assert "matrix 2" in msg and "variable 4" in msg, msg
    rc, msg, C, R, I = _path_call(S, lam)
    assert rc == 0 and not np.any(C == -7.5) and not np.any(I == -7)


def test_ctx_call_and_its_refusals():
    """``ggl_neighborhood_stability`` on a ctx that holds three matrices: the stack of the stateless call, the counts of the
    host definition; what it refuses raises."""
    from gglasso_amd import _lib, solver
    p, B = 5, 3
    eye = np.broadcast_to(np.eye(p), (B, p, p))
    eng = solver.HipEngine(mb_ref.stack(p), eye, eye, np.zeros((B, p, p)))
    try:
        lam = np.array(mb_ref.GRID)
        for kw in (dict(rule='raw'), dict(t=-1.0), dict(t=np.inf), dict(tol=-1.0), dict(max_sweeps=0),
                   dict(lambda_range=lam[::-1]), dict(lambda_range=[0.1, np.nan])):
            args = dict(lambda_range=lam)
            args.update(kw)
            with pytest.raises(AssertionError):
                eng.neighborhood_stability(**args)
        out = eng.neighborhood_stability(lam, 'and', tol=TOL, counts=True, stack=True)
    finally:
        eng.close()
    from gglasso_amd import model_selection as ms, utils
    W = utils.neighborhood_selection(mb_ref.stack(p), lam, 'and', tol=TOL)             # (B,L,p,p)
    assert np.array_equal(out['stack'], np.swapaxes(W, 0, 1)) and not out['status'].any()
    cnt, num = ms._host_edge_counts(out['stack'], 1e-8)
    assert np.array_equal(out['counts'], cnt) and np.array_equal(out['num'], num)


def _stars_inputs():
    from gglasso_amd import model_selection as ms
    X = mb_ref.stars_data()
    return X, ms.stars_subsamples(X.shape[1], 6, None, seed=5)


@pytest.mark.parametrize("rule,kw", [("and", {}), ("or", {}), ("and", {"lambdas_per_batch": 1})])
def test_stars_on_the_device(rule, kw):
    """Check 10: NUM, COUNTS, IX and THETA against the host route assembled from the comparison value."""
    from gglasso_amd import model_selection as ms, utils
    X, idx = _stars_inputs()
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        sol, stats = ms.stars_search(X, mb_ref.GRID, n_subsamples=6, seed=5, beta=0.1, scale=True, tol=TOL, store_all=True,
                                     method='mb', rule=rule, **kw)
    assert stats['FAILED'] == []
    mb_ref.check_stars(stats, ms._host_subset_covariances(X, idx, True, True), mb_ref.GRID, rule, 1e-8, 0.1)
    ix = stats['IX']
    S_full = utils.sample_covariance(X, center=True, scale=True)[0]
    W, info = utils.neighborhood_selection(S_full, mb_ref.GRID[:ix + 1], rule, tol=TOL, return_info=True)
    assert sorted(sol) == ['adjacency', 'coef', 'lambda1', 'resvar'] and sol['lambda1'] == mb_ref.GRID[ix]
    assert np.array_equal(sol['coef'], info['COEF'][ix]) and np.array_equal(sol['adjacency'], W[ix] != 0)


def test_stars_kendall_on_the_device():
    from gglasso_amd import model_selection as ms, utils
    X, idx = _stars_inputs()
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        _, stats = ms.stars_search(np.exp(X), mb_ref.GRID, n_subsamples=6, seed=5, beta=0.1, tol=TOL, store_all=True,
                                   method='mb', correlation='kendall')
    mb_ref.check_stars(stats, utils.host_skeptic_correlation(np.exp(X), idx), mb_ref.GRID, 'and', 1e-8, 0.1)


def test_stars_nan_in_one_subsample():
    """Check 8: a NaN in a column of X that only subsample 2 draws -- status 2 there, every lambda FAILED, and the other
    subsamples' matrices and counts those of the run without it."""
    from gglasso_amd import model_selection as ms
    X = mb_ref.stars_data()
    rng = np.random.default_rng(3)
    idx = np.stack([np.sort(rng.choice(119, 60, replace=False)) for _ in range(4)]).astype(np.int32)
    idx[2, -1] = 119                                                        # column 119: subsample 2 alone
    Xn = X.copy()
    Xn[3, 119] = np.nan
    kw = dict(indices=idx, beta=0.1, tol=TOL, store_all=True, method='mb')
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        _, clean = ms.stars_search(X, mb_ref.GRID, **kw)
    with pytest.warns(RuntimeWarning, match="failed"):
        _, stats = ms.stars_search(Xn, mb_ref.GRID, **kw)
    assert stats['FAILED'] == [0, 1, 2, 3] and np.all(np.isnan(stats['INSTABILITY'])) and clean['FAILED'] == []
    others = [0, 1, 3]
    assert np.array_equal(stats['THETA'][:, others], clean['THETA'][:, others])
    off = ~np.eye(17, dtype=bool)
    assert np.all(np.isnan(stats['THETA'][:, 2][:, off]))
    cnt, num = ms._host_edge_counts(np.ascontiguousarray(clean['THETA'][:, others]), 1e-8)
    assert np.array_equal(stats['COUNTS'], cnt)


def test_glasso_route_is_untouched():
    """``method='glasso'`` and no ``method``: identical ``stats`` and ``sol`` bits."""
    from gglasso_amd import model_selection as ms
    X = mb_ref.stars_data(p=6, N=60)
    kw = dict(n_subsamples=3, seed=2, beta=0.2, store_all=True, tol=1e-6, rtol=1e-6)
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        sol_a, st_a = ms.stars_search(X, (0.4, 0.2), **kw)
        sol_b, st_b = ms.stars_search(X, (0.4, 0.2), method='glasso', **kw)
    assert sorted(st_a) == sorted(st_b) and sorted(sol_a) == sorted(sol_b)
    for k in ('LAMBDA', 'INSTABILITY', 'INSTABILITY_MONOTONE', 'INDICES', 'COUNTS', 'THETA'):
        assert np.array_equal(st_a[k], st_b[k], equal_nan=True), k
    for k in ('NUM', 'IX', 'BEST', 'FAILED', 'subsample_size', 'n_subsamples'):
        assert st_a[k] == st_b[k], k
    for k in sol_a:
        assert np.array_equal(sol_a[k], sol_b[k]), k
