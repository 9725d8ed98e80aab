"""Nearest-correlation projection on the device (``ggl_nearest_correlation``, ``ggl_project_S``; csrc/nearcorr.hip around the
L-step's rank_step) against the numpy twin ``utils.host_nearest_correlation``, and what is built on it
(``HipEngine.project_S``, ``stars_search(project=True)``).

Shapes: p = 1 .. 8 take the Jacobi route (8 its edge), 9 is the first Newton-Schulz size, 65 / 70 and 130 are two and three
64-tiles (and three to five of the update kernel's 32-tiles); odd and even p take the 8- and the 16-byte loads.  N is about
p / 3 (at least 5), so the skeptic matrices are indefinite.  A correlation matrix of p <= 2 cannot be indefinite: p = 2 runs on the
symmetric, unit-diagonal [[1, 1.3], [1.3, 1]] (eigenvalue -0.3) and on two more of its kind, p = 1 on positive numbers."""
import ctypes
import functools
import warnings

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

PS = [1, 2, 5, 8, 9, 17, 33, 65, 70, 130]
TOL = 1e-11
# max |device - twin| at tol = 1e-11 over the shapes below, measured on an MI355X: MEASURED; the bound is 4 x that,
# and has to stay at or below the project's bar for Theta
MEASURED = 5.218e-15
BOUND = 4 * MEASURED
THETA_BAR = 1e-8


@functools.lru_cache(maxsize=None)
def inputs(p):
    """(3,p,p) indefinite inputs of dimension p (see the module's docstring).  Shared, never changed."""
    from gglasso_amd import utils
    if p == 1:
        S = np.array([[[1.0]], [[2.5]], [[0.3]]])
    elif p == 2:
        S = np.array([[[1, 1.3], [1.3, 1]], [[1, -1.7], [-1.7, 1]], [[1, 1.05], [1.05, 1]]], dtype=np.float64)
    else:
        N = max(5, p // 3)
        S = np.stack([utils.host_skeptic_correlation(np.round(np.random.default_rng([p, r]).standard_normal((p, N)), 1))
                      for r in range(3)])
    S.setflags(write=False)
    return S


@functools.lru_cache(maxsize=None)
def twin(p):
    from gglasso_amd import utils
    out, info = utils.host_nearest_correlation(inputs(p), tol=TOL, return_info=True)
    out.setflags(write=False)
    return out, info


@pytest.mark.parametrize("B", [1, 3])
@pytest.mark.parametrize("p", PS)
def test_device_against_the_twin_and_on_its_own(p, B):
    from gglasso_amd import utils
    S = inputs(p)[:B]
    if p >= 2:
        assert all(np.linalg.eigvalsh(s).min() < -0.01 for s in S)
    ref, rinfo = twin(p)
    out, info = utils.nearest_correlation(S, tol=TOL, return_info=True)
    dev = np.abs(out - ref[:B]).max()
    rel = np.abs(info['distance'] - rinfo['distance'][:B]) / np.maximum(rinfo['distance'][:B], 1e-300)
    print(f"nearcorr p={p} B={B}: max|device - twin| = {dev:.3e}, distance rel = {rel.max():.3e}, iterations "
          f"{info['iterations'].tolist()} (twin {rinfo['iterations'][:B].tolist()}), fallbacks {info['fallbacks']}")
    assert info['converged'].all()
    assert BOUND <= THETA_BAR
    assert dev <= BOUND
    if p >= 2:
        assert np.all(rel <= 1e-9)
    # independent of the twin
    d = np.diagonal(S, axis1=1, axis2=2)
    assert np.array_equal(np.diagonal(out, axis1=1, axis2=2), d) and np.array_equal(out, out.transpose(0, 2, 1))
    for b in range(B):
        sd = np.sqrt(d[b])
        assert np.linalg.eigvalsh(out[b] / np.outer(sd, sd)).min() >= 0.5e-8, b
    again, info2 = utils.nearest_correlation(S, tol=TOL, return_info=True)
    assert np.array_equal(again, out) and np.array_equal(info2['residual'], info['residual'])
    assert np.array_equal(info2['distance'], info['distance'])
    # one matrix alone, as a (p,p) array: its matrix of the stack, to the bound (a batch of another size)
    if B == 3:
        one = utils.nearest_correlation(S[1], tol=TOL)
        assert one.shape == (p, p) and np.abs(one - out[1]).max() <= BOUND


@pytest.mark.parametrize("p", [5, 8, 17, 70, 130])
def test_pass_through_and_idempotence(p):
    from gglasso_amd import utils
    out = utils.nearest_correlation(inputs(p))
    again, info = utils.nearest_correlation(out, return_info=True)
    assert np.array_equal(again, out) and np.all(info['iterations'] == 1) and np.all(info['shrink'] == 0.0)
    assert np.all(info['distance'] == 0.0)
    C = np.corrcoef(np.random.default_rng(p).standard_normal((p, 20 * p)))
    V = np.cov(np.random.default_rng(p + 1).standard_normal((p, 20 * p)) * np.arange(1, p + 1)[:, None])
    for A in (C, V):
        back, info = utils.nearest_correlation(A, return_info=True)
        assert np.array_equal(back, A) and info['iterations'] == 1 and info['converged']
    # in a stack with a matrix that needs the projection: the one that does not is frozen and comes back bit for bit
    St = np.stack([inputs(p)[0], C, inputs(p)[1]])
    outs, infos = utils.nearest_correlation(St, return_info=True)
    assert np.array_equal(outs[1], C) and infos['iterations'][1] == 1 and infos['iterations'][0] > 1
    # (the other two ran in another batch: the L-step's schedule is common to a batch, so they agree to the bound, not bitwise)
    dev = max(np.abs(outs[0] - out[0]).max(), np.abs(outs[2] - out[1]).max())
    print(f"nearcorr p={p}: the same matrices in another stack differ by {dev:.3e}")
    assert dev <= BOUND


def test_eigenvalues_at_the_threshold_take_the_fallback_and_keep_the_guarantee():
    """p = 130 (beyond the Jacobi kernel: the L-step's fallback is rocSOLVER, which uses the ctx's small scratch), eps = 0, a
    block-diagonal covariance: an indefinite skeptic block that needs the iteration beside a singular Pearson block (20
    observations of 65 variables) whose 46 zero eigenvalues sit at the threshold in every iteration, where the sign iteration
    cannot decide.  The bound against the twin is the project's bar for Theta on the correlation scale: both routes converge
    to the same point through different eigen routines, so it cannot be derived (as for the shapes above); the figure is
    printed.  lambda_min: the floor is 0, and numpy's eigvalsh of a 130 x 130 matrix of norm < 40 is good to ~1e-13."""
    from gglasso_amd import utils
    p = 130
    C = np.zeros((p, p))
    C[:65, :65] = inputs(65)[0]
    C[65:, 65:] = np.corrcoef(np.random.default_rng(8).standard_normal((65, 20)))
    i = np.arange(p)
    C[i, i] = 1.0
    d = np.random.default_rng(9).uniform(0.5, 9.0, p)
    sc = np.sqrt(np.outer(d, d))
    A = C * sc
    A[i, i] = d
    assert np.linalg.eigvalsh(C[:65, :65]).min() < -0.1 and abs(np.linalg.eigvalsh(C[65:, 65:])[:46]).max() < 1e-13
    out, info = utils.nearest_correlation(A, eps=0.0, return_info=True)
    ref, rinfo = utils.host_nearest_correlation(A, eps=0.0, return_info=True)
    corr = out / sc
    lmin = np.linalg.eigvalsh(corr).min()
    dev = np.abs(corr - ref / sc).max()
    print(f"nearcorr fallback route: fallbacks {info['fallbacks']}, iterations {info['iterations']} (twin {rinfo['iterations']}), "
          f"lambda_min {lmin:.3e}, max|device - twin| on the correlation scale {dev:.3e}")
    assert info['fallbacks'] > 0, "the input did not reach the L-step's eigendecomposition fallback"
    assert info['converged'] and info['iterations'] > 1
    assert np.array_equal(np.diag(out), d) and np.array_equal(out, out.T)
    assert np.abs(corr).max() <= 1.0 + 1e-12 and lmin >= -1e-12
    assert dev <= THETA_BAR
    assert abs(info['distance'] - rinfo['distance']) <= 1e-9 * rinfo['distance']


def test_highams_example():
    from gglasso_amd import utils
    A = np.array([[1., 1, 0], [1, 1, 1], [0, 1, 1]])
    out, info = utils.nearest_correlation(A, eps=0, tol=1e-12, return_info=True)
    assert info['converged']
    assert abs(out[0, 1] - 0.76068985) <= 1e-7 and abs(out[1, 2] - 0.76068985) <= 1e-7 and abs(out[0, 2] - 0.15729811) <= 1e-7
    assert np.array_equal(out, out.T) and np.array_equal(np.diag(out), np.ones(3))


def test_covariance_input_and_truncated_run():
    from gglasso_amd import utils
    rng = np.random.default_rng(21)
    p, N = 20, 14
    X = rng.standard_normal((p, N)) * rng.uniform(0.5, 20.0, (p, 1))
    X[rng.random((p, N)) < 0.2] = np.nan
    S, _ = utils.host_pairwise_covariance(X)
    assert np.linalg.eigvalsh(S).min() < 0
    out, info = utils.nearest_correlation(S, return_info=True)
    d = np.diag(S)
    assert np.array_equal(np.diag(out), d) and np.array_equal(out, out.T) and info['converged']
    sd = np.sqrt(d)
    assert np.linalg.eigvalsh(out / np.outer(sd, sd)).min() >= 0.5e-8
    with pytest.warns(RuntimeWarning, match=r"no convergence within 5 iterations for the matrices \[0, 2\]"):
        St = np.stack([inputs(33)[0], np.eye(33), inputs(33)[1]])
        out5, info5 = utils.nearest_correlation(St, max_iter=5, return_info=True)
    assert info5['converged'].tolist() == [False, True, False] and info5['iterations'].tolist() == [5, 1, 5]
    for b in (0, 2):
        assert np.linalg.eigvalsh(out5[b]).min() >= 0.5e-8 and np.array_equal(np.diag(out5[b]), np.ones(33))
        assert 0.0 < info5['shrink'][b] < 1.0


def kendall_data(p=17, N=9, B=3, b=6):
    X = np.round(np.random.default_rng(31).standard_normal((p, N)), 1)
    idx = np.stack([np.sort(np.random.default_rng([6, r]).choice(N, b, replace=False)) for r in range(B)]).astype(np.int32)
    return X, idx


def test_project_S_in_a_ctx():
    from gglasso_amd import utils
    from gglasso_amd.solver import HipEngine
    p, K, B = 17, 6, 3
    X, idx = kendall_data()
    S3 = utils.skeptic_correlation(X, idx)
    assert all(np.linalg.eigvalsh(s).min() < -0.01 for s in S3)
    ref = utils.nearest_correlation(S3)
    eye = np.broadcast_to(np.eye(p), (K, p, p))
    lam = np.full(K, 0.2)
    eng = HipEngine(eye, eye, eye, 0 * eye)
    try:
        eng.set_kendall_subsets(X, idx)
        info = eng.project_S(period=B)
        S = eng.get_S()
        assert np.array_equal(S[:B], ref) and np.array_equal(S[B:], S[:B])
        assert info['converged'].all() and info['iterations'].shape == (B,) and np.all(info['iterations'] > 1)
        # all K on their own agree to the measured bound (another batch size, another schedule of the products)
        eng.set_kendall_subsets(X, idx)
        info0 = eng.project_S()
        S0 = eng.get_S()
        assert info0['iterations'].shape == (K,) and np.abs(S0 - S).max() <= BOUND
        # the solver runs on the projected S
        eng.set_kendall_subsets(X, idx)
        eng.project_S(period=B)
        n1 = eng.sgl_batch_step(np.ones(K), lam, False, None).copy()
        st1 = {k: np.copy(v) for k, v in eng.state().items()}
        other = HipEngine(S, eye, eye, 0 * eye)
        try:
            n2 = other.sgl_batch_step(np.ones(K), lam, False, None)
            st2 = other.state()
            assert np.array_equal(n1, n2) and all(np.array_equal(st1[k], st2[k]) for k in ('Omega', 'Theta', 'X'))
        finally:
            other.close()
        raw = HipEngine(np.tile(S3, (2, 1, 1)), eye, eye, 0 * eye)
        try:
            assert not np.array_equal(raw.sgl_batch_step(np.ones(K), lam, False, None), n1)
        finally:
            raw.close()
        with pytest.raises(AssertionError, match="period"):
            eng.project_S(period=4)
    finally:
        eng.close()
    # a refused call leaves S bit for bit
    bad = np.tile(S3, (2, 1, 1))
    bad[4, 3, 11] = np.nan
    eng = HipEngine(bad, eye, eye, 0 * eye)
    try:
        with pytest.raises(AssertionError, match=r"S of instance 4, variable 3"):
            eng.project_S()
        assert np.array_equal(eng.get_S(), bad, equal_nan=True)
    finally:
        eng.close()


def test_project_S_refuses_a_nan_among_the_projected():
    from gglasso_amd.solver import HipEngine
    p, K = 9, 4
    S = np.tile(np.array(inputs(9)[:2]), (2, 1, 1))
    S[1, 8, 8] = -0.5
    S[0, 2, 7] = np.inf
    eye = np.broadcast_to(np.eye(p), (K, p, p))
    eng = HipEngine(S, eye, eye, 0 * eye)
    try:
        with pytest.raises(AssertionError, match=r"S of instance 0, variable 2"):
            eng.project_S(period=2)
        assert np.array_equal(eng.get_S(), S)
    finally:
        eng.close()


def test_stars_search_projected_device_and_host_routes_agree(monkeypatch):
    from gglasso_amd import model_selection as ms, solver
    p, N, B, b = 12, 14, 4, 9
    X = np.round(np.random.default_rng(13).standard_normal((p, N)), 1)
    idx = np.stack([np.sort(np.random.default_rng([2, r]).choice(N, b, replace=False)) for r in range(B)])
    lam = [0.5, 0.3, 0.15]
    with warnings.catch_warnings():
        warnings.simplefilter("ignore", RuntimeWarning)
        sol, st = ms.stars_search(X, lam, indices=idx, beta=0.1, correlation='kendall', project=True, tol=1e-8, rtol=1e-8)
        _, st0 = ms.stars_search(X, lam, indices=idx, beta=0.1, correlation='kendall', tol=1e-8, rtol=1e-8)
        for name in ("project_S", "set_kendall_subsets", "set_mixed_subsets", "set_data_subsets"):
            monkeypatch.delattr(solver.HipEngine, name)              # an engine without the routes: the numpy twins
        assert not hasattr(solver.ENGINE, "project_S")
        sol_h, st_h = ms.stars_search(X, lam, indices=idx, beta=0.1, correlation='kendall', project=True, tol=1e-8, rtol=1e-8)
    assert st['NUM'] == st_h['NUM'] and st['IX'] == st_h['IX'] and st['BEST'] == st_h['BEST']
    assert np.abs(sol['Theta'] - sol_h['Theta']).max() <= 1e-6
    assert st['PROJECTION']['converged'] and st['PROJECTION']['iterations'] > 1 and 'PROJECTION' not in st0


def test_abi_misuse_is_refused_and_writes_nothing():
    from gglasso_amd import _lib
    from gglasso_amd.solver import HipEngine
    lib = _lib.load()
    B, p = 2, 9
    A = np.array(inputs(9)[:B])
    out = np.full((B, p, p), -7.0)
    iters = np.full(B, -7, dtype=np.int32)
    info = np.full((B, 4), -7.0)
    ip, dp = iters.ctypes.data_as(_lib._ip), _lib.ptr
    ok = (B, p, dp(A), dp(out), 1e-8, 1e-10, 500, ip, dp(info))

    def call(**kw):
        names = ("B", "p", "A", "out", "eps", "tol", "max_iter", "iters", "info")
        args = [kw.get(n, v) for n, v in zip(names, ok)]
        return lib.ggl_nearest_correlation(*args)

    nan = float("nan")
    for kw, word in ((dict(eps=-1e-9), "eps"), (dict(eps=0.51), "eps"), (dict(eps=nan), "eps"), (dict(tol=9e-15), "tol"),
                     (dict(tol=0.011), "tol"), (dict(tol=nan), "tol"), (dict(max_iter=0), "max_iter"), (dict(max_iter=-3), "max_iter"),
                     (dict(A=None), "A"), (dict(out=None), "out"), (dict(iters=None), "iters"), (dict(info=None), "info"),
                     (dict(B=0), "B"), (dict(p=0), "p"), (dict(B=65536), "65535")):
        assert call(**kw) == _lib.E_ARG, kw
        assert word in _lib.last_error(), (kw, _lib.last_error())
        assert np.all(out == -7.0) and np.all(iters == -7) and np.all(info == -7.0), kw
    for plant, where in (((1, 4, 6), "instance 1, variable 4"), ((0, 6, 2), "instance 0, variable 6")):
        Abad = A.copy()
        Abad[plant] = nan
        assert call(A=dp(Abad)) == _lib.E_ARG and where in _lib.last_error()
        assert np.all(out == -7.0) and np.all(iters == -7) and np.all(info == -7.0)
    Abad = A.copy()
    Abad[1, 5, 5] = 0.0
    assert call(A=dp(Abad)) == _lib.E_ARG and "instance 1, variable 5" in _lib.last_error()
    assert np.all(out == -7.0)
    # the ctx route: a bad period, null pointers, the scalar arguments
    eye = np.broadcast_to(np.eye(p), (4, p, p))
    eng = HipEngine(np.tile(A, (2, 1, 1)), eye, eye, 0 * eye)
    try:
        S0 = eng.get_S()
        it4 = np.full(4, -7, dtype=np.int32)
        in4 = np.full((4, 4), -7.0)
        i4 = it4.ctypes.data_as(_lib._ip)
        assert lib.ggl_project_S(None, 0, 1e-8, 1e-10, 500, i4, dp(in4)) == _lib.E_ARG
        for period in (-1, 3, 5, 8):
            assert lib.ggl_project_S(eng.h, period, 1e-8, 1e-10, 500, i4, dp(in4)) == _lib.E_ARG, period
            assert "period" in _lib.last_error()
        assert lib.ggl_project_S(eng.h, 2, 0.7, 1e-10, 500, i4, dp(in4)) == _lib.E_ARG and "eps" in _lib.last_error()
        assert lib.ggl_project_S(eng.h, 2, 1e-8, 1.0, 500, i4, dp(in4)) == _lib.E_ARG and "tol" in _lib.last_error()
        assert lib.ggl_project_S(eng.h, 2, 1e-8, 1e-10, 0, i4, dp(in4)) == _lib.E_ARG and "max_iter" in _lib.last_error()
        assert lib.ggl_project_S(eng.h, 2, 1e-8, 1e-10, 500, None, dp(in4)) == _lib.E_ARG
        assert lib.ggl_project_S(eng.h, 2, 1e-8, 1e-10, 500, i4, None) == _lib.E_ARG
        assert np.all(it4 == -7) and np.all(in4 == -7.0) and np.array_equal(eng.get_S(), S0)
        # and a valid call follows
        assert lib.ggl_project_S(eng.h, 2, 1e-8, 1e-10, 500, i4, dp(in4)) == 0
        assert np.all(it4[:2] > 1) and np.all(it4[2:] == -7) and call() == 0 and np.array_equal(eng.get_S()[:2], out)
    finally:
        eng.close()
