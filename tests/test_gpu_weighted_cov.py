"""Weighted covariance of one data array under K weight rows on the device (covariance_weighted.hip behind
ggl_covariance_weighted / ggl_set_S_from_weighted), utils.weighted_covariance / kernel_covariance, HipEngine.set_data_weighted
and glasso_problem.from_time_series.

Data as in test_gpu_covariance (row means up to +-1e3: a wrong or unweighted mean is ~1e6 against a bound of ~1e-13);
comparison value and the derived elementwise bound: weighted_ref.py.  The range rule -- instance k loops over its support
only -- is checked bitwise against GGL_COV_FULL_RANGE.
"""
import contextlib
import io
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import weighted_ref as wr  # noqa: E402

pytestmark = pytest.mark.gpu

U = wr.U
TILES = (4, 8, 0)                                   # GGL_COV_TILE32, GGL_COV_TILE64, the library's choice
CENTER, SCALE, FULL = 1, 2, 16
SHAPES = sorted({(p, N) for p in (1, 2, 17, 33, 65, 130) for N in (5, 33)} |
                {(p, N) for p in (17, 65) for N in (1, 3, 4, 5, 31, 32, 33, 64, 65, 257)})


def wcov(X, w, flags):
    from gglasso_amd import utils
    return utils._covariance_weighted_call(np.ascontiguousarray(X, dtype=np.float64), np.ascontiguousarray(w, dtype=np.float64), flags)


def random_weights(K, N, seed):
    return np.random.default_rng([77, K, N, seed]).uniform(0.1, 2.0, (K, N))


def support_rows(N=257):
    """Twelve rows whose supports start at, before and behind slab (16, 32) and lane (64) boundaries, of lengths 1 .. 33, with
    zeros inside the longer ones."""
    los = (0, 1, 15, 16, 17, 31, 32, 33, 63, 64, 65, 200)
    lens = (1, 3, 4, 5, 33, 33, 5, 4, 3, 1, 33, 33)
    rng = np.random.default_rng(5)
    w = np.zeros((len(los), N))
    for k, (lo, ln) in enumerate(zip(los, lens)):
        w[k, lo:lo + ln] = rng.uniform(0.1, 2.0, ln)
        if ln >= 3:
            w[k, lo + 1:lo + ln - 1:2] = 0.0                           # zeros inside the support; both ends stay positive
        assert wr.support(w[k]) == (lo, lo + ln)
    return w


@pytest.mark.parametrize("p,N", SHAPES)
def test_weighted_covariance_within_derived_bound(p, N):
    X = wr.make_data(p, N, 0)
    worst = 0.0
    for K in (1, 3, 9):                                              # nine: more than one round over the eight XCDs
        w = random_weights(K, N, p)
        refs = {(k, c): wr.reference(X, w[k], c) for k in range(K) for c in (True, False)}
        for tile in TILES:
            S, _, W = wcov(X, w, CENTER | tile)
            R, _, _ = wcov(X, w, tile)
            assert np.all(np.abs(W - w.sum(axis=1)) <= 2 * (N - 1) * U * w.sum(axis=1))   # two sums of N terms, any order
            for k in range(K):
                worst = max(worst, wr.check(S[k], X, w[k], True, (p, N, K, k, tile, "centred"), refs[k, True]))
                worst = max(worst, wr.check(R[k], X, w[k], False, (p, N, K, k, tile, "raw"), refs[k, False]))
    print("shape", (p, N), "max err/bound", worst)


@pytest.mark.parametrize("tile", (4, 8))
def test_supports_across_slab_and_lane_boundaries(tile):
    p, N = 33, 257
    X = wr.make_data(p, N, 1)
    w = support_rows(N)
    for center in (CENTER, 0):
        S, _, W = wcov(X, w, center | tile)
        F, _, WF = wcov(X, w, center | tile | FULL)
        assert np.array_equal(S, F) and np.array_equal(W, WF), "the range rule changed bits"
        for k in range(w.shape[0]):
            wr.check(S[k], X, w[k], bool(center), ("support", k, tile, center))
    # kernel weights, as the front end makes them: supports of 8.6 h in the middle, cut off at both ends
    from gglasso_amd import utils
    wk = utils.kernel_weights(np.arange(float(N)), np.linspace(0, N - 1, 9), 6.0)
    S, _, _ = wcov(X, wk, CENTER | tile)
    assert np.array_equal(S, wcov(X, wk, CENTER | tile | FULL)[0])
    for k in range(9):
        wr.check(S[k], X, wk[k], True, ("gaussian", k, tile))


@pytest.mark.parametrize("tile", (4, 8))
def test_bitwise_invariants(tile):
    p, N = 33, 257
    X = wr.make_data(p, N, 2)
    w = np.concatenate([random_weights(3, N, 0), support_rows(N)[[2, 8, 11]]])
    S, _, W = wcov(X, w, CENTER | tile)
    S2, _, W2 = wcov(X, w, CENTER | tile)
    assert np.array_equal(S, S2) and np.array_equal(W, W2)                       # fixed reduction orders
    for k in range(w.shape[0]):                                                   # no cross-instance leakage
        alone, _, Wa = wcov(X, w[k:k + 1], CENTER | tile)
        assert np.array_equal(alone[0], S[k]) and Wa[0] == W[k], k
    S4, _, W4 = wcov(X, 4.0 * w, CENTER | tile)                                   # sqrt and / commute with an even power of two
    assert np.array_equal(S4, S) and np.array_equal(W4, 4.0 * W)
    # leading and trailing samples outside every support do not exist for the result
    ws = np.zeros((4, N))
    rng = np.random.default_rng(9)
    for k, (lo, hi) in enumerate(((64, 65), (65, 130), (100, 200), (127, 193))):
        ws[k, lo:hi] = rng.uniform(0.1, 2.0, hi - lo)
    for center in (CENTER, 0):
        full, _, Wf = wcov(X, ws, center | tile)
        for a, b in ((64, N), (0, 200), (0, 201), (64, 200)):
            part, _, Wp = wcov(X[:, a:b], ws[:, a:b], center | tile)
            assert np.array_equal(part, full) and np.array_equal(Wp, Wf), (a, b, center)


@pytest.mark.parametrize("p,N,K", [(33, 70, 3), (65, 17, 1)])
def test_unit_weights_give_the_bits_of_the_plain_covariance(p, N, K):
    """Every weight exactly 1.0: sqrt(1) = 1 and 1 (x - m) is exact, the weighted mean sums in the lane order of k_row_means
    from sample 0, and W = N is exact -- the weighted kernel is the plain one under the one tile body (gram_nt_tile.hpp)."""
    from gglasso_amd import utils
    X = np.ascontiguousarray(wr.make_data(p, N, 3))
    for center in (CENTER, 0):
        for tile in TILES:
            plain, _ = utils._covariance_call([X], center | tile)
            S, _, W = wcov(X, np.ones((K, N)), center | tile)
            assert np.array_equal(W, np.full(K, float(N))), (center, tile)
            for k in range(K):
                assert np.array_equal(S[k], plain[0]), (center, tile, k)


def test_special_weights():
    from gglasso_amd import utils
    from test_gpu_covariance import reference as cov_reference
    p, N = 33, 70
    X = wr.make_data(p, N, 3)
    e = np.zeros((2, N))
    e[0, 41], e[1, 0] = 1.0, 1.0
    S = utils.weighted_covariance(X, e)
    assert S.shape == (2, p, p) and not S.any()                                   # x - m = 0 exactly
    # all weights equal: the sample covariance
    Sw = utils.weighted_covariance(X, np.full(N, 0.75))
    Sc = utils.sample_covariance(X)
    _, bw = wr.reference(X, np.full(N, 0.75))
    _, bc = cov_reference(X)
    assert Sw.shape == (p, p) and np.all(np.abs(Sw - Sc) <= bw + bc)
    # 0/1 weights: the covariance of the selected columns
    rng = np.random.default_rng(4)
    idx = np.stack([np.sort(rng.choice(N, 30, replace=False)) for _ in range(3)])
    w01 = np.zeros((3, N))
    for r in range(3):
        w01[r, idx[r]] = 1.0
    Sw = utils.weighted_covariance(X, w01)
    Ss = utils.sample_covariance_subsets(X, idx)
    for r in range(3):
        _, bw = wr.reference(X, w01[r])
        _, bc = cov_reference(X[:, idx[r]])
        assert np.all(np.abs(Sw[r] - Ss[r]) <= bw + bc), r


def test_scale_and_python_kinds():
    from gglasso_amd import utils
    p, N = 17, 120
    X = wr.make_data(p, N, 4)
    w = random_weights(3, N, 1)
    S, W = utils.weighted_covariance(X, w, return_wsum=True)
    C, var = utils.weighted_covariance(X, w, scale=True)
    assert np.array_equal(var, np.stack([np.diag(s) for s in S]))
    assert np.allclose(np.diagonal(C, axis1=1, axis2=2), 1.0, rtol=0, atol=4 * U)
    want = S / (np.sqrt(var)[:, :, None] * np.sqrt(var)[:, None, :])
    assert np.all(np.abs(C - want) <= 8 * U * np.abs(want)) and np.array_equal(C, C.transpose(0, 2, 1))
    one, v1, W1 = utils.weighted_covariance(X, w[1], scale=True, return_wsum=True)
    assert one.shape == (p, p) and np.array_equal(one, C[1]) and np.array_equal(v1, var[1]) and W1 == W[1]
    assert np.array_equal(utils.weighted_covariance(X, w, center=False), wcov(X, w, 0)[0])
    # the kernel-smoothed stack
    Sk, n_eff, vk = utils.kernel_covariance(X, at=4, bandwidth=10.0, scale=True)
    wk = utils.kernel_weights(np.arange(float(N)), np.linspace(0, N - 1, 4), 10.0)
    Ck, vk2 = utils.weighted_covariance(X, wk, scale=True)
    assert np.array_equal(Sk, Ck) and np.array_equal(vk, vk2) and np.array_equal(n_eff, utils.effective_sample_size(wk))
    host = utils.host_weighted_covariance(X, wk)
    Sd, _ = utils.kernel_covariance(X, at=4, bandwidth=10.0)
    for k in range(4):
        _, bound = wr.reference(X, wk[k])
        assert np.all(np.abs(Sd[k] - host[k]) <= 2 * bound)                       # both within the bound of the same value


def test_refusals_name_the_offender_and_write_nothing():
    from gglasso_amd import _lib
    lib = _lib.load()
    p, N, K = 5, 64, 3
    X = np.ascontiguousarray(wr.make_data(p, N, 5))
    w = random_weights(K, N, 2)
    S, sc, W = np.full((K, p, p), -7.5), np.full((K, p), -7.5), np.full(K, -7.5)

    def call(X=X, w=w, p=p, N=N, K=K, flags=CENTER, S=S, sc=sc, W=W):
        return lib.ggl_covariance_weighted(0, p, N, _lib.ptr(X), K, _lib.ptr(None if w is None else np.ascontiguousarray(w)),
                                           flags, _lib.ptr(S), _lib.ptr(sc), _lib.ptr(W))

    def refused(match=None, **kw):
        assert call(**kw) == _lib.E_ARG
        msg = _lib.last_error()
        assert msg and (match is None or match in msg), msg
        assert np.all(S == -7.5) and np.all(sc == -7.5) and np.all(W == -7.5), "a refused call wrote to an output"

    refused(p=0), refused(N=0), refused(K=0), refused(X=None), refused(w=None), refused(S=None)
    refused("unknown bits", flags=CENTER | 32), refused("exclude each other", flags=CENTER | 4 | 8)
    refused("scale_out", flags=CENTER | SCALE, sc=None)
    for bad in (-1e-300, -1.0, np.nan, np.inf, -np.inf):
        wb = w.copy()
        wb[1, 3] = bad
        wb[2, 1] = bad                                                # the smallest k * N + n is named
        refused("instance 1, sample 3", w=wb)
    wz = w.copy()
    wz[2] = 0.0
    refused("instance 2", w=wz)
    wo = w.copy()
    wo[0, :2] = 1.5e308                                               # finite weights, a sum that is not
    refused("instance 0", w=wo)
    flat = X.copy()
    flat[3] = 7.0                                                     # constant: the weighted mean of equal weights is exact
    ones = np.stack([np.ones(N), 2.0 * np.ones(N), np.ones(N)])
    refused("instance 0, variable 3", X=flat, w=ones, flags=CENTER | SCALE)
    assert call() == 0 and not np.any(S == -7.5) and not np.any(W == -7.5) and np.all(sc == -7.5)
    assert lib.ggl_set_S_from_weighted(None, _lib.ptr(X), N, _lib.ptr(w), CENTER) == _lib.E_ARG


def quiet(fn, *a, **k):
    with contextlib.redirect_stdout(io.StringIO()):
        return fn(*a, **k)


def test_ctx_route():
    from gglasso_amd import solver, utils
    from gglasso_amd.solver import HipEngine
    K, p, N = 3, 17, 120
    X = wr.make_data(p, N, 6) / 50.0
    w = utils.kernel_weights(np.arange(float(N)), np.linspace(0, N - 1, K), 15.0)
    S = utils.weighted_covariance(X, w)
    C, var = utils.weighted_covariance(X, w, scale=True)
    eye = np.stack([np.eye(p)] * K)
    a = HipEngine(eye, eye, eye, 0 * eye)
    b = HipEngine(eye, eye, eye, 0 * eye)
    try:
        for eng in (a, b):
            eng.set_data_weighted(X, w)
        assert np.array_equal(a.get_S(), S)
        # refused calls leave S, and the next step, as they were
        wneg = w.copy()
        wneg[1, 60] = -0.5
        with pytest.raises(AssertionError, match="instance 1, sample 60"):
            b.set_data_weighted(X, wneg)
        flat = X.copy()
        flat[4] = 0.25
        with pytest.raises(AssertionError, match=r"instance 0, variable 4"):
            b.set_data_weighted(flat, np.ones((K, N)), scale=True)
        with pytest.raises(AssertionError, match="weights must be"):
            b.set_data_weighted(X, w[:2])
        assert np.array_equal(b.get_S(), S)
        for eng in (a, b):
            for _ in range(3):
                eng.step(1.0, 0.1, 0.05, 'FGL', False, None, np.ones(K))
        sa, sb = a.state(), b.state()
        for nm in ("Omega", "Theta", "X"):
            assert np.array_equal(sa[nm], sb[nm]), nm
        # with scaling the variances are kept, also across a refused call
        b.set_data_weighted(X, w, scale=True)
        with pytest.raises(AssertionError, match="instance 1, sample 60"):
            b.set_data_weighted(X, wneg, scale=True)
        Cb, vb = b.get_S()
        assert np.array_equal(Cb, C) and np.array_equal(vb, var)
        # one short solve on the ctx-set S against the solve on the uploaded stack
        ref, rinfo = quiet(solver.ADMM_MGL, S, 0.1, 0.05, 'FGL', eye, tol=1e-7, rtol=1e-7, max_iter=40)
        c = HipEngine(eye, eye, eye, 0 * eye)
        try:
            c.set_data_weighted(X, w)
            info, _ = quiet(solver._run_admm, c, 'FGL', K, p, 0.1, 0.05, False, None, np.ones(K), 1.0, 1e-7, 1e-7, 'boyd', True,
                            40, False, False, "Multiple", want_objective=True)
            sc = c.state()
        finally:
            c.close()
        assert info['status'] == rinfo['status']
        for nm in ("Omega", "Theta", "X"):
            assert np.array_equal(sc[nm], ref[nm]), nm
    finally:
        a.close()
        b.close()


def test_from_time_series_front_end():
    from gglasso_amd import glasso_problem, solver, utils
    p, N, K = 17, 120, 4
    X = wr.make_data(p, N, 7) / 50.0
    P = glasso_problem.from_time_series(X, K, 12.0, reg_params={'lambda1': 0.1, 'lambda2': 0.05})
    S, n_eff = utils.kernel_covariance(X, at=K, bandwidth=12.0)
    assert P.reg == 'FGL' and P.K == K and np.array_equal(P.S, S)
    assert np.array_equal(P.N, n_eff) and np.array_equal(P.N, utils.effective_sample_size(P.weights))
    assert np.array_equal(P.eval_times, np.linspace(0, N - 1, K))
    P.solve(tol=1e-7, rtol=1e-7)
    assert P.solver_info['status'] == 'optimal'
    ref, _ = quiet(solver.ADMM_MGL, S, 0.1, 0.05, 'FGL', np.stack([np.eye(p)] * K), tol=1e-7, rtol=1e-7)
    assert np.array_equal(P.solution.precision_, ref['Theta'])
    with pytest.raises(AssertionError, match="from_data"):
        P.stability_selection()
