"""Weighted covariance and the kernel-smoothed front end without a GPU: the numpy route against numpy.cov within the derived
bound (weighted_ref.py), the weight generators, the ABI's bookkeeping, and glasso_problem.from_time_series over the test-only
oracle engine."""
import os
import re
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import problem_helpers as ph  # noqa: E402
import weighted_ref as wr  # noqa: E402
from conftest import ROOT  # noqa: E402
from oracle import ggl_oracle as orc  # noqa: E402


def test_host_weighted_covariance_against_numpy_cov():
    from gglasso_amd import utils
    rng = np.random.default_rng(7)
    for p, N, K in ((1, 5, 1), (17, 33, 3), (33, 257, 4)):
        X = wr.make_data(p, N, 0)
        w = rng.uniform(0.1, 2.0, (K, N))
        w[0, : N // 3] = 0.0                                             # a support that starts late, zeros not counted
        S = utils.host_weighted_covariance(X, w)
        R = utils.host_weighted_covariance(X, w, center=False)
        assert S.shape == R.shape == (K, p, p)
        for k in range(K):
            # (the device's result is bitwise symmetric; a BLAS product on the host need not be)
            assert wr.ratio(S[k], X, w[k], True) <= 1.0 and wr.ratio(R[k], X, w[k], False) <= 1.0, (p, N, k)
            _, bound = wr.reference(X, w[k])
            ref = np.atleast_2d(np.cov(X, aweights=w[k], bias=True))
            assert np.all(np.abs(S[k] - ref) <= bound), (p, N, k)
        one = utils.host_weighted_covariance(X, w[0])
        assert one.shape == (p, p) and np.array_equal(one, S[0])
    with pytest.raises(AssertionError, match=r"weights must be \(N,\) or \(K,N\)"):
        utils.host_weighted_covariance(wr.make_data(3, 8, 0), np.ones(7))


def test_kernel_weights():
    from gglasso_amd import utils
    t = np.arange(50.0)
    at = np.array([0.0, 10.0, 24.5, 49.0])
    for kernel, fn in (('gaussian', lambda u: np.exp(-0.5 * u * u)), ('epanechnikov', lambda u: np.maximum(0.0, 1.0 - u * u)),
                       ('uniform', lambda u: (np.abs(u) <= 1.0).astype(float))):
        w = utils.kernel_weights(t, at, 4.0, kernel, cutoff=0.0)
        assert w.shape == (4, 50) and np.array_equal(w, fn((t[None] - at[:, None]) / 4.0))
        assert w[1, 10] == 1.0 == w[1].max() and w[0, 0] == 1.0 and w[3, 49] == 1.0     # the row maximum where times = at
    # per-point bandwidths
    h = np.array([1.0, 2.0, 4.0, 8.0])
    w = utils.kernel_weights(t, at, h, 'gaussian', cutoff=0.0)
    for k in range(4):
        assert np.array_equal(w[k], np.exp(-0.5 * ((t - at[k]) / h[k]) ** 2))
    # the cutoff turns the Gaussian's tail into exact zeros: support |u| <= sqrt(2 ln 2^53) = 8.57
    w = utils.kernel_weights(np.arange(400.0), [200.0], 10.0)
    nz = np.flatnonzero(w[0])
    assert nz[0] == 200 - 85 and nz[-1] == 200 + 85 and w[0, nz].min() >= 2.0 ** -53 and (w[0] >= 0).all()
    assert np.count_nonzero(w[0, nz[0]:nz[-1] + 1] == 0) == 0
    assert np.count_nonzero(utils.kernel_weights(np.arange(400.0), [200.0], 10.0, cutoff=1e-3)) < nz.size
    # unsorted times: the same weights, permuted
    perm = np.random.default_rng(0).permutation(50)
    assert np.array_equal(utils.kernel_weights(t[perm], at, 4.0), utils.kernel_weights(t, at, 4.0)[:, perm])
    assert utils.kernel_weights(t, 3.0, 2.0).shape == (1, 50)            # a scalar evaluation point
    for bad in (dict(bandwidth=0.0), dict(bandwidth=-1.0), dict(bandwidth=np.inf), dict(kernel='box'), dict(cutoff=1.0)):
        with pytest.raises(AssertionError):
            utils.kernel_weights(t, at, **{'bandwidth': 4.0, **bad})


def test_effective_sample_size():
    from gglasso_amd import utils
    assert utils.effective_sample_size(np.full(37, 0.25)) == 37.0
    e = np.zeros(20)
    e[11] = 3.5
    assert utils.effective_sample_size(e) == 1.0
    n = utils.effective_sample_size(np.stack([np.ones(20), e, np.r_[np.ones(10), np.zeros(10)]]))
    assert n.dtype == np.float64 and np.array_equal(n, [20.0, 1.0, 10.0])
    w = np.random.default_rng(1).uniform(0, 1, 30)
    assert 1.0 < utils.effective_sample_size(w) < 30.0


def test_header_and_exports_carry_the_two_names():
    from gglasso_amd import _lib
    header = open(os.path.join(ROOT, "include", "ggl_hip.h")).read()
    for name in ("ggl_covariance_weighted", "ggl_set_S_from_weighted"):
        assert name in _lib.EXPORTS and f"int {name}(" in header
        assert name in header[:header.index("#define GGL_VERSION")]       # the list of additions that leave the version alone
    assert re.search(r"#define\s+GGL_VERSION\s+300\b", header) and _lib.ABI_VERSION == 300
    assert int(re.search(r"#define\s+GGL_COV_FULL_RANGE\s+(\d+)", header).group(1)) == _lib.COV_FULL_RANGE == 16
    src = open(os.path.join(ROOT, "gglasso_amd", "build.py")).read()
    assert '"covariance_weighted.hip"' in src


def test_kernel_covariance_argument_handling(monkeypatch):
    from gglasso_amd import utils
    calls = []

    def stub(X, w, flags, device=0):
        calls.append((X.shape, w.shape, flags))
        assert X.flags['C_CONTIGUOUS'] and w.flags['C_CONTIGUOUS'] and X.dtype == w.dtype == np.float64
        S = utils.host_weighted_covariance(X, w, bool(flags & 1))
        var = None
        if flags & 2:
            var = np.stack([np.diag(s).copy() for s in S])
            S = ph.scale_by_diagonal_numpy(S, var)[0]
        return S, var, w.sum(axis=1)
    monkeypatch.setattr(utils, "_covariance_weighted_call", stub)
    X = wr.make_data(5, 60, 1)
    S, n_eff = utils.kernel_covariance(np.asfortranarray(X), at=4, bandwidth=6.0)
    w = utils.kernel_weights(np.arange(60.0), np.linspace(0, 59, 4), 6.0)
    assert calls == [((5, 60), (4, 60), 1)] and S.shape == (4, 5, 5)
    assert np.array_equal(S, utils.host_weighted_covariance(X, w)) and np.array_equal(n_eff, utils.effective_sample_size(w))
    times = np.linspace(2.0, 3.0, 60)
    C, n2, var = utils.kernel_covariance(X, at=[2.5], bandwidth=0.1, times=times, kernel='epanechnikov', scale=True, center=False)
    assert calls[-1] == ((5, 60), (1, 60), 2) and C.shape == (1, 5, 5) and var.shape == (1, 5) and n2.shape == (1,)
    assert np.allclose(np.diagonal(C, axis1=1, axis2=2), 1.0)
    S1, W1 = utils.weighted_covariance(X, w[2], return_wsum=True)
    assert S1.shape == (5, 5) and np.array_equal(S1, S[2]) and W1 == w[2].sum()
    with pytest.raises(AssertionError, match="bandwidth"):
        utils.kernel_covariance(X, at=4)
    with pytest.raises(AssertionError, match="evaluation points"):
        utils.kernel_covariance(X, bandwidth=2.0)
    with pytest.raises(AssertionError, match="one entry per column"):
        utils.kernel_covariance(X, at=4, bandwidth=2.0, times=np.arange(59.0))


@pytest.fixture()
def host(monkeypatch):
    ph.on_host(monkeypatch)
    from gglasso_amd import problem
    return problem


def test_from_time_series_over_the_oracle_engine(host):
    from gglasso_amd import utils
    rng = np.random.default_rng(3)
    p, N, K = 6, 90, 3
    X = rng.standard_normal((p, N)) * rng.uniform(0.5, 2.0, (p, 1)) + rng.uniform(-5, 5, (p, 1))
    P = host.glasso_problem.from_time_series(X, K, 12.0, reg_params={'lambda1': 0.1, 'lambda2': 0.05})
    w = utils.kernel_weights(np.arange(float(N)), np.linspace(0, N - 1, K), 12.0)
    S = utils.host_weighted_covariance(X, w)
    assert P.multiple and P.reg == 'FGL' and P.K == K and P.p == p
    assert np.array_equal(P.S, S) and np.array_equal(P.N, utils.effective_sample_size(w))
    assert np.array_equal(P.weights, w) and np.array_equal(P.eval_times, np.linspace(0, N - 1, K))
    P.solve(tol=1e-9, rtol=1e-9)
    eye = np.stack([np.eye(p)] * K)
    ref, info = orc.ADMM_MGL(S, 0.1, 0.05, 'FGL', eye, tol=1e-9, rtol=1e-9)
    assert P.solver_info['status'] == 'optimal' == info['status']
    assert np.abs(P.solution.precision_ - ref['Theta']).max() <= 1e-10      # as the host-loop tests of test_cpu_boundary.py
    with pytest.raises(AssertionError, match="from_data"):
        P.stability_selection()
    # other evaluation points, kernel and time stamps; K = 1 is a single problem
    times = np.sort(rng.uniform(0, 10, N))
    P2 = host.glasso_problem.from_time_series(X, [2.0, 7.5], [1.0, 2.0], times=times, kernel='epanechnikov', reg='GGL', center=False)
    w2 = utils.kernel_weights(times, [2.0, 7.5], [1.0, 2.0], 'epanechnikov')
    assert P2.reg == 'GGL' and np.array_equal(P2.S, utils.host_weighted_covariance(X, w2, center=False))
    P1 = host.glasso_problem.from_time_series(X, 1, 20.0)
    assert not P1.multiple and isinstance(P1.N, float) and P1.S.shape == (p, p)
    with pytest.raises(TypeError):
        host.glasso_problem.from_time_series(X, 3, 12.0, None)            # keyword-only behind the bandwidth
