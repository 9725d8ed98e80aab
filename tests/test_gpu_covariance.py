"""Sample covariance from data and scaling by a diagonal on the device (covariance.hip behind ggl_covariance,
ggl_scale_by_diagonal, ggl_set_S_from_data, ggl_get_S).

Inputs: fixed seed, mean + std * z with per-row means in [-1e3, 1e3] and std in [0.1, 10], so a wrong centring (or a padded
column that contributes m_i m_j) is ~1e6 against a bound of ~1e-13.  Comparison value: the two-pass formula in
numpy.longdouble.  Bound (derived, u = 2^-53, xc = x - m, A_ij = (1/N) sum_n |xc_in| |xc_jn|, M_i = mean_n |x_in|):

    |S_dev - S_ref|_ij <= (N + 8) u A_ij + (N u)^2 M_i M_j

first term: rounding of an N-term inner product in any order, of x - m, of the division by N and of the comparison
value; second term: the rounded mean, N (m^_i - m_i)(m^_j - m_j) -- second order because sum_n xc_in = 0.
"""
import ctypes

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

U = 2.0 ** -53
P_ALL = (1, 2, 15, 16, 17, 33, 64, 65, 130)
N_ALL = (1, 3, 4, 5, 31, 32, 33, 257)
SHAPES = sorted({(p, N) for p in P_ALL for N in (5, 33)} | {(p, N) for p in (17, 65) for N in N_ALL})


def make_data(p, N, seed):
    rng = np.random.default_rng([20241018, p, N, seed])
    mean = rng.uniform(-1e3, 1e3, (p, 1))
    std = rng.uniform(0.1, 10.0, (p, 1))
    return mean + std * rng.standard_normal((p, N))


def reference(X, center=True):
    """(S in longdouble, elementwise bound)."""
    Xl = X.astype(np.longdouble)
    N = X.shape[1]
    m = Xl.sum(axis=1, keepdims=True) / N if center else np.zeros((X.shape[0], 1), dtype=np.longdouble)
    Xc = Xl - m
    S = (Xc @ Xc.T) / N
    A = (np.abs(Xc) @ np.abs(Xc).T) / N
    bound = (N + 8) * U * A
    if center:
        M = np.abs(Xl).sum(axis=1) / N
        bound = bound + (N * U) ** 2 * np.outer(M, M)
    return S, bound


def cov(Xs, flags):
    from gglasso_amd import utils
    return utils._covariance_call([np.ascontiguousarray(x) for x in Xs], flags)


def check(S, X, center, what):
    ref, bound = reference(X, center)
    err = np.abs(S.astype(np.longdouble) - ref)
    worst = float((err - bound).max())
    print(what, "max err", float(err.max()), "max bound", float(bound.max()), "max ratio", float((err / np.maximum(bound, 1e-300)).max()))
    assert np.all(err <= bound), (what, worst)
    assert np.array_equal(S, S.T), what


@pytest.mark.parametrize("p,N", SHAPES)
def test_covariance_within_derived_bound(p, N):
    from gglasso_amd import _lib
    X = make_data(p, N, 0)
    for tile in (_lib.COV_TILE32, _lib.COV_TILE64, 0):
        S, _ = cov([X], _lib.COV_CENTER | tile)
        check(S[0], X, True, (p, N, tile, "centred"))
        S2, _ = cov([X], _lib.COV_CENTER | tile)
        assert np.array_equal(S, S2)                                  # fixed reduction order: bitwise reproducible
        R, _ = cov([X], tile)
        check(R[0], X, False, (p, N, tile, "raw"))
        if N == 1:
            assert not S.any()                                        # x - mean(x) = 0 exactly


@pytest.mark.parametrize("tile", (4, 8))
def test_ragged_batch_equals_single_instances(tile):
    from gglasso_amd import _lib
    p, Ns = 65, (5, 32, 257)
    Xs = [make_data(p, N, 1 + k) for k, N in enumerate(Ns)]
    S, _ = cov(Xs, _lib.COV_CENTER | tile)
    for k, X in enumerate(Xs):
        check(S[k], X, True, (p, Ns, k))
        alone, _ = cov([X], _lib.COV_CENTER | tile)
        assert np.array_equal(S[k], alone[0]), k                      # no cross-instance leakage
    # eight and more instances take the other branch of the tile decoding
    Xs9 = [make_data(17, 5 + k, 10 + k) for k in range(9)]
    S9, _ = cov(Xs9, _lib.COV_CENTER | tile)
    for k, X in enumerate(Xs9):
        check(S9[k], X, True, (17, "K=9", k))


def test_sample_covariance_kinds_and_scale():
    from gglasso_amd import utils
    X = np.stack([make_data(16, 40, k) for k in range(3)])
    S3 = utils.sample_covariance(X)
    assert S3.shape == (3, 16, 16) and np.array_equal(utils.sample_covariance(X[1]), S3[1])
    ragged = [make_data(8, 20, 0), make_data(12, 31, 1), make_data(8, 7, 2)]
    Sd = utils.sample_covariance(ragged)
    assert sorted(Sd) == [0, 1, 2] and [Sd[k].shape[0] for k in range(3)] == [8, 12, 8]
    for k in range(3):
        check(Sd[k], ragged[k], True, ("dict", k))
    C, var = utils.sample_covariance(X, scale=True)
    d = np.stack([np.diag(S3[k]) for k in range(3)])
    assert np.array_equal(var, d)
    want = S3 / (np.sqrt(d)[:, :, None] * np.sqrt(d)[:, None, :])
    assert np.all(np.abs(C - want) <= 8 * U * np.abs(want))
    assert np.allclose(np.diagonal(C, axis1=1, axis2=2), 1.0, rtol=0, atol=4 * U)


@pytest.mark.parametrize("p", (1, 2, 17, 64, 65))
def test_scale_by_diagonal(p):
    from gglasso_amd import ops
    rng = np.random.default_rng(p)
    B = rng.standard_normal((3, p, p + 3))
    S = B @ B.transpose(0, 2, 1) * rng.uniform(0.1, 50.0, (3, p, 1)) * rng.uniform(0.1, 50.0, (3, 1, p))
    Y, d = ops._scale_by_diagonal(S)
    assert np.array_equal(d, np.stack([np.diag(s) for s in S]))
    want = S / (np.sqrt(d)[:, :, None] * np.sqrt(d)[:, None, :])
    assert np.all(np.abs(Y - want) <= 8 * U * np.abs(want))
    # round trip: the returned d on a Theta (the rescaling of a solution), single matrix and stack
    Th = rng.standard_normal((3, p, p))
    back = ops.scale_array_by_diagonal(Th, d)
    want = Th / (np.sqrt(d)[:, :, None] * np.sqrt(d)[:, None, :])
    assert np.all(np.abs(back - want) <= 8 * U * np.abs(want))
    one = ops.scale_array_by_diagonal(Th[1], d[1])
    assert one.shape == (p, p) and np.array_equal(one, back[1])


def test_zero_variance_is_refused_with_instance_and_variable():
    from gglasso_amd import ops, utils
    S = np.stack([np.eye(6)] * 3)
    S[2, 4, 4] = 0.0
    with pytest.raises(AssertionError, match=r"instance 2, variable 4"):
        ops.scale_array_by_diagonal(S)
    d = np.ones((3, 6))
    d[1, 3] = np.inf
    with pytest.raises(AssertionError, match=r"instance 1, variable 3"):
        ops.scale_array_by_diagonal(S, d)
    X = make_data(5, 9, 0)
    X[3] = 7.0                                                        # a constant variable
    with pytest.raises(AssertionError, match=r"instance 0, variable 3"):
        utils.sample_covariance(X, scale=True)


def test_misuse_of_the_four_entry_points():
    from gglasso_amd import _lib
    lib = _lib.load()
    X = np.ascontiguousarray(make_data(4, 6, 0))
    Xp = (_lib._dp * 1)(_lib.ptr(X))
    N = (ctypes.c_int * 1)(6)
    S, sc = np.empty((1, 4, 4)), np.empty((1, 4))
    good = (0, 1, 4, N, Xp, 1, _lib.ptr(S), _lib.ptr(sc))

    def bad(i, v, fn=lib.ggl_covariance, args=good):
        a = list(args)
        a[i] = v
        assert fn(*a) == _lib.E_ARG and _lib.last_error()
    assert lib.ggl_covariance(*good) == 0
    bad(1, 0), bad(2, 0), bad(3, None), bad(4, None), bad(5, 16), bad(5, 4 | 8), bad(6, None)
    bad(3, (ctypes.c_int * 1)(0))
    bad(4, (_lib._dp * 1)(None))
    a = list(good)
    a[5], a[7] = 3, None                                              # GGL_COV_SCALE without scale_out
    assert lib.ggl_covariance(*a) == _lib.E_ARG
    Y = np.empty((1, 4, 4))
    sgood = (0, 1, 4, _lib.ptr(np.eye(4)[None].copy()), None, _lib.ptr(Y), None)
    assert lib.ggl_scale_by_diagonal(*sgood) == 0
    for i, v in ((1, 0), (2, 0), (3, None), (5, None)):
        bad(i, v, lib.ggl_scale_by_diagonal, sgood)
    assert lib.ggl_set_S_from_data(None, Xp, N, 1) == _lib.E_ARG
    assert lib.ggl_get_S(None, _lib.ptr(S), None) == _lib.E_ARG
    from gglasso_amd.solver import HipEngine
    eye = np.eye(4)[None]
    eng = HipEngine(eye, eye, eye, 0 * eye)
    try:
        assert lib.ggl_set_S_from_data(eng.h, None, N, 1) == _lib.E_ARG
        assert lib.ggl_set_S_from_data(eng.h, Xp, None, 1) == _lib.E_ARG
        assert lib.ggl_set_S_from_data(eng.h, Xp, N, 32) == _lib.E_ARG
        assert lib.ggl_get_S(eng.h, None, None) == _lib.E_ARG
        assert lib.ggl_get_S(eng.h, _lib.ptr(S), _lib.ptr(sc)) == _lib.E_ARG      # no variances: S was uploaded
        eng.set_instance_dims(np.array([3]))
        assert lib.ggl_set_S_from_data(eng.h, Xp, N, 1) == _lib.E_ARG
        eng.set_instance_dims(None)
        assert lib.ggl_set_S_from_data(eng.h, Xp, N, 1) == 0 and lib.ggl_get_S(eng.h, _lib.ptr(S), None) == 0
    finally:
        eng.close()


def test_ctx_route_equals_the_operator_and_the_uploaded_solve():
    from gglasso_amd import _lib
    from gglasso_amd.solver import HipEngine
    p, N = 33, 70
    X = make_data(p, N, 3) / 50.0
    S, _ = cov([X], _lib.COV_CENTER)
    eye = np.eye(p)[None]
    a = HipEngine(S, eye, eye, 0 * eye)
    b = HipEngine(eye, eye, eye, 0 * eye)
    try:
        b.set_data(X[None], N)
        assert np.array_equal(b.get_S(), S)
        for eng in (a, b):
            for _ in range(5):
                eng.step(1.0, 0.1, 0.0, 'SGL', False, None, np.ones(1))
        sa, sb = a.state(), b.state()
        for nm in ("Omega", "Theta", "X"):
            assert np.array_equal(sa[nm], sb[nm]), nm
        # with scaling: correlations on the device, variances beside them
        b.set_data([X], [N], scale=True)
        C, var = b.get_S()
        C2, var2 = cov([X], _lib.COV_CENTER | _lib.COV_SCALE)
        assert np.array_equal(C, C2) and np.array_equal(var, var2) and np.array_equal(var[0], np.diag(S[0]))
    finally:
        a.close()
        b.close()


def test_ctx_route_failed_call_leaves_nothing_of_the_old_S():
    """A set_data that is refused after the Gram kernel ran (a constant variable under scale=True) has overwritten S: the
    ctx must hold nothing built for the old S (variances, the fused next-W of the Theta-step)."""
    from gglasso_amd import _lib
    from gglasso_amd.solver import HipEngine
    p, N = 33, 64                                                     # 64: the mean of a constant row is exact
    X = make_data(p, N, 4) / 50.0
    bad = X.copy()
    bad[7] = 0.25                                                     # a constant variable
    Sbad, _ = cov([bad], _lib.COV_CENTER)
    assert Sbad[0, 7, 7] == 0.0
    eye = np.eye(p)[None]
    b = HipEngine(eye, eye, eye, 0 * eye)
    a = HipEngine(Sbad, eye, eye, 0 * eye)
    try:
        b.set_data([X], scale=True)
        for _ in range(2):
            b.step(1.0, 0.1, 0.0, 'SGL', False, None, np.ones(1))
        with pytest.raises(AssertionError, match=r"instance 0, variable 7"):
            b.set_data([bad], scale=True)
        got = b.get_S()                                               # no variances any more: an array, not a pair
        assert isinstance(got, np.ndarray) and np.array_equal(got, Sbad)
        b.set_state(eye, eye, 0 * eye)
        for eng in (a, b):
            for _ in range(3):
                eng.step(1.0, 0.1, 0.0, 'SGL', False, None, np.ones(1))
        sa, sb = a.state(), b.state()
        for nm in ("Omega", "Theta", "X"):
            assert np.array_equal(sa[nm], sb[nm]), nm
    finally:
        a.close()
        b.close()
