"""The case list, the bounds and the NumPy twin of tests/eig_ref.py, checked on the CPU: the cases have the spectra they
claim, LAPACK alone meets every bound (so the bounds are attainable), the twin meets them with the committed ratios
reproduced, the twin is scale-free, and no new bound is looser than what test_gpu_ops.py asserts at its own inputs."""
import numpy as np
import pytest

import eig_ref as er
from conftest import load_golden
from eig_ref import EPS, EPS_LD, JACOBI, LD, ROCSOLVER

SMALL_P = (1, 2, 3, 7, 33)


@pytest.mark.parametrize("p", SMALL_P + (65, 129))
def test_cases_have_the_spectrum_they_claim(p):
    names = [c.name for c in er.cases(p)]
    assert len(set(names)) == len(names) == 15
    for c in er.cases(p):
        assert np.array_equal(c.A, c.A.T)
        if c.Q is None:
            assert c.name == "wilkinson"
            continue
        A, n = c.A.astype(LD), LD(c.norm)
        assert float(np.abs(c.Q.T @ c.Q - np.eye(p)).max()) <= 64 * EPS_LD, c.name
        R = A @ c.Q - c.Q * c.d_q
        res = float(np.sqrt((R * R).sum(axis=0)).max())
        assert res <= 64 * EPS_LD * n + c.slack, (c.name, res, c.slack)
        assert np.all(np.diff(c.d) >= 0)
        # the slack is rounding to float64 and nothing else; the cases written down directly are exact
        assert c.slack <= p * EPS * c.norm
        if c.name in ("zero", "identity", "ones", "diag_1e-8_1e8", "blocks_2x2", "toeplitz_-1_2_-1"):
            assert c.slack <= 64 * EPS_LD * p * c.norm, (c.name, c.slack)
    by = {c.name: c for c in er.cases(p)}
    assert np.all(by["cluster_pm1"].d * by["cluster_pm1"].d == 1)
    assert np.count_nonzero(by["rank_third"].d) == p // 3 and np.count_nonzero(by["rank1"].d) == 1
    if p >= 4:
        st = by["straddle"]
        assert np.sum(np.abs(np.abs(st.d - LD(st.mu)) - LD(1e-9)) < 1e-15) == 4


@pytest.mark.parametrize("p", SMALL_P + (65, 129))
def test_lapack_alone_meets_every_bound(p):
    for c in er.cases(p):
        D, Q, outs = er.lapack_outputs(c)
        er.check(c, ROCSOLVER, D, Q, outs)
        er.check(c, JACOBI, D, Q, outs)


@pytest.mark.parametrize("p", SMALL_P)
def test_twin_meets_every_bound_and_reproduces_the_committed_ratios(p):
    worst, sweeps = {}, 0
    for c, sw_committed in zip(er.cases(p), er.TWIN_SWEEPS[p]):
        D, Q, sw, outs = er.twin_outputs(c)
        assert 0 < sw <= 40 and sw == sw_committed, (c.name, sw)
        sweeps = max(sweeps, sw)
        assert np.all(np.diff(D) >= 0)
        for o in outs.values():
            assert np.array_equal(o, o.T)
        er.check(c, JACOBI, D, Q, outs, worst)
    print(p, sweeps, {k: round(float(v), 3) for k, v in worst.items()})
    if p in er.TWIN_RATIO_BY_P:
        assert sweeps == er.TWIN_SWEEPS_BY_P[p]
        for k, v in er.TWIN_RATIO_BY_P[p].items():
            assert abs(worst[k] - v) <= 6e-4, (k, worst[k], v)


def test_twin_graded_p128():
    c = {c.name: c for c in er.cases(128)}["graded"]
    D, Q, sw, outs = er.twin_outputs(c)
    assert sw == er.TWIN_SWEEPS_BY_P[128] == 22                  # the slowest case of the list
    assert er.TWIN_SWEEPS[128][[c.name for c in er.cases(128)].index("graded")] == 22
    assert all(len(v) == 15 and 0 < min(v) and max(v) <= 22 for v in er.TWIN_SWEEPS.values())
    r = er.check(c, JACOBI, D, Q, outs)
    assert all(r[k] <= er.TWIN_RATIO_BY_P[128][k] + 6e-4 for k in r)


def test_constants_are_four_times_the_measured_ratios():
    for k in er.KEYS:
        assert er.CONST[JACOBI][k] == 4.0 * max(r[k] for r in er.TWIN_RATIO_BY_P.values())
        assert er.CONST[ROCSOLVER][k] == 4.0 * max(r[k] for r in er.LAPACK_RATIO_BY_P.values())
    assert tuple(er.TWIN_RATIO_BY_P) == tuple(er.LAPACK_RATIO_BY_P) == er.MEASURE_P
    # what the device was seen to give is recorded beside them, and below the bounds
    for m in (JACOBI, ROCSOLVER):
        assert all(0 < er.DEVICE_RATIO[m][k] <= er.CONST[m][k] for k in er.KEYS)


def _gaussian33():
    return {c.name: c for c in er.cases(33)}["gaussian"]


def test_unscaled_kernel_had_two_scale_defects():
    """The kernel before the power-of-two scaling (prescale=False), for the record: at 2^300 the rotation test's product of
    squared norms is infinite, no rotation is applied and the first sweep counts as converged with wrong eigenvalues; at
    2^-320 the product is zero, the test fires on rounding noise and the sweeps run out."""
    c = _gaussian33()
    big, small = c.scaled(300), c.scaled(-320)
    D, Q, sw, _ = er.jacobi_twin(big.A, prescale=False)
    assert sw == 1
    r = er.ratios(big, *er.sorted_pair(D, Q))
    assert r["val"] > 1e10 and r["val"] > er.CONST[JACOBI]["val"]
    assert er.jacobi_twin(small.A, prescale=False)[2] == -1


@pytest.mark.parametrize("k", [-480, -320, 300, 480])
def test_twin_extreme_scales(k):
    """With the scaling the same matrices are ordinary: same sweeps, same bits up to the exact factor, every bound met."""
    c = _gaussian33()
    D0, Q0, sw0, _ = er.jacobi_twin(c.A)
    s = c.scaled(k)
    D, Q, sw, _ = er.jacobi_twin(s.A)
    assert sw == sw0 and np.array_equal(D, np.ldexp(D0, k)) and np.array_equal(Q, Q0)
    er.check(s, JACOBI, *er.sorted_pair(D, Q))


@pytest.mark.parametrize("prescale", [True, False])
@pytest.mark.parametrize("name", ["gaussian", "cluster_1_2_spread", "graded"])
def test_twin_is_bitwise_scale_equivariant(name, prescale):
    c = {c.name: c for c in er.cases(33)}[name]
    D0, Q0, sw0, o0 = er.jacobi_twin(c.A, prescale=prescale, want_out=("rank", c.mu))
    for k in (-200, -100, 100, 200):
        D, Q, sw, o = er.jacobi_twin(np.ldexp(c.A, k), prescale=prescale, want_out=("rank", float(np.ldexp(c.mu, k))))
        assert sw == sw0 and np.array_equal(D, np.ldexp(D0, k)) and np.array_equal(Q, Q0), (name, k)
        assert np.array_equal(o, np.ldexp(o0, k))
    # ... and the scaling changes no bit at scale 1: what the kernel computed before, it computes now
    D1, Q1, sw1, o1 = er.jacobi_twin(c.A, prescale=not prescale, want_out=("rank", c.mu))
    assert sw1 == sw0 and np.array_equal(D1, D0) and np.array_equal(Q1, Q0) and np.array_equal(o1, o0)


def test_twin_reads_the_lower_triangle_and_handles_nonfinite():
    c = _gaussian33()
    P = c.A.copy()
    P[np.triu_indices(33, 1)] = 1e300
    a, b = er.jacobi_twin(c.A), er.jacobi_twin(P)
    assert np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1]) and a[2] == b[2]
    for bad in (np.nan, np.inf):
        P = c.A.copy()
        P[5, 2] = bad
        D, Q, sw, _ = er.jacobi_twin(P)            # bounded by the sweep cap
        assert not np.all(np.isfinite(D))


def _sym(rng, K, p, scale=1.0):
    A = rng.standard_normal((K, p, p)) * scale
    return 0.5 * (A + A.transpose(0, 2, 1))


def test_bounds_are_not_looser_than_the_operator_tests():
    """At the inputs of test_gpu_ops.py the new bounds are below the tolerances asserted there."""
    g = load_golden("g1_g2_eigen_prox")
    for n in range(int(g["count"])):
        W = g[f"W_{n}"]
        p = W.shape[0]
        Wl = np.tril(W) + np.tril(W, -1).T
        scale, nrm = max(1.0, np.abs(W).max()), er.norm_inf(Wl)
        for m in (JACOBI, ROCSOLVER):
            if m == JACOBI and p > er.JMAXP:
                continue
            C = er.CONST[m]
            assert C["val"] * p * EPS * nrm <= 1e-12 * scale * p                       # test_eigh_golden_matrices
            assert C["orth"] * np.sqrt(p) * EPS <= 1e-12
            for which in ("phiplus", "rank"):                                          # test_g1_g2_phiplus_rank_from_matrix
                fn = er.norm_inf(g[f"{which}_{n}"])
                assert C["out"] * p * EPS * max(nrm, fn) <= 1e-12 * scale * p, (n, which)
    from oracle import ggl_oracle as orc
    for m, seed0, shapes in ((JACOBI, 100, [(1, 1), (2, 2), (3, 7), (5, 50), (4, 64), (3, 65), (2, 127), (2, 128)]),
                             (ROCSOLVER, 200, [(3, 7), (2, 64), (3, 100), (2, 129), (2, 200)])):
        for K, p in shapes:                        # test_phiplus_stack_jacobi_sizes / _rocsolver_mfma_sizes
            rng = np.random.default_rng(seed0 + p)
            W = _sym(rng, K, p, 2.0)
            beta = rng.uniform(0.3, 2.0, K)
            ref, _ = orc.phiplus_stack(W, beta)
            for k in range(K):
                ours = er.CONST[m]["out"] * p * EPS * max(er.norm_inf(W[k]), er.norm_inf(ref[k]))
                assert ours <= 1e-11 * max(1.0, np.abs(ref).max()), (m, K, p)
