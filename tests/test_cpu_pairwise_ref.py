"""The reference of the pairwise-complete covariance (tests/pairwise_ref.py) against pandas and numpy, and the numpy route
``utils.host_pairwise_covariance`` (the four products of the kernel) against the reference within the derived bound.  No GPU."""
import numpy as np
import pytest

import pairwise_ref as pr

SHAPES = ((17, 33), (65, 257), (33, 130), (17, 2000), (8, 5), (16, 64))


def cases():
    for p, N in SHAPES:
        for pattern in pr.PATTERNS:
            X = pr.make_case(p, N, pattern)
            if X is not None:
                yield (p, N, pattern), X


def test_reference_equals_pandas_up_to_the_normalisation():
    pd = pytest.importorskip("pandas")
    for what, X in cases():
        S, n, _ = pr.reference(X, True)
        C = pd.DataFrame(X.T).cov().to_numpy()                        # 1 / (n_ij - 1); NaN where n_ij < 2
        ok = n >= 2
        want = C[ok] * (n[ok] - 1) / n[ok]
        got = S[ok].astype(np.float64)
        # relative to the matrix (pandas works in fp64: with row means of 1e3 and a std of 0.1 its own rounding is about
        # 1e3 / 0.1 u = 1e-12 of a single small entry, so entry by entry there is nothing to compare at 1e-12)
        rel = np.abs(got - want).max() / np.abs(want).max()
        assert rel <= 1e-12, (what, rel)


def test_reference_equals_numpy_on_complete_data():
    for p, N in SHAPES:
        X = pr.make_data(p, N, 1)
        S, n, D = pr.reference(X, True)
        assert np.all(n == N)
        want = np.atleast_2d(np.cov(X, bias=True))
        assert np.all(np.abs(S.astype(np.float64) - want) <= 1e-12 * np.sqrt(np.outer(np.diag(want), np.diag(want))))
        R, _, _ = pr.reference(X, False)
        assert np.all(np.abs(R.astype(np.float64) - X @ X.T / N) <= 1e-12 * np.abs(X) @ np.abs(X).T / N)


def test_reference_of_a_hand_computed_case():
    nan = np.nan
    X = np.array([[1.0, 2.0, 3.0, nan],
                  [2.0, nan, 6.0, 1.0],
                  [nan, nan, nan, 5.0]])
    S, n, _ = pr.reference(X, True)
    assert np.array_equal(n, [[3, 2, 0], [2, 3, 1], [0, 1, 1]])
    assert S[0, 0] == np.longdouble(2) / 3                             # var of 1, 2, 3
    assert S[0, 1] == S[1, 0] == 2                                     # samples 0 and 2: (-1)(-2) and (1)(2), over 2
    assert S[1, 2] == 0 and S[2, 2] == 0 and np.isnan(S[0, 2])
    R, _, _ = pr.reference(X, False)
    assert R[0, 1] == 10 and R[1, 2] == 5 and R[2, 2] == 25


def test_host_route_within_the_bound_of_the_reference():
    from gglasso_amd import utils
    worst = 0.0
    for what, X in cases():
        for center in (True, False):
            ref = pr.reference(X, center)
            S, cnt = utils.host_pairwise_covariance(X, center)
            assert cnt.dtype == np.int32 and np.array_equal(cnt, ref[1]), what
            r = pr.ratio(S, ref)
            worst = max(worst, r)
            assert r <= 1.0, (what, center, r)
    print("host route: largest |S - S_ref| / bound =", worst)


def test_host_route_subsets_are_the_gathered_columns():
    from gglasso_amd import utils
    X = pr.make_case(9, 40, "r30")
    idx = np.stack([np.sort(np.random.default_rng(r).choice(40, 25, replace=False)) for r in range(3)])
    idx[2, 5] = idx[2, 6]                                              # a duplicate: a bootstrap draw
    S, cnt = utils.host_pairwise_covariance(X, True, idx)
    assert S.shape == cnt.shape == (3, 9, 9)
    for r in range(3):
        Sr, cr = utils.host_pairwise_covariance(X[:, idx[r]], True)
        assert np.array_equal(S[r], Sr, equal_nan=True) and np.array_equal(cnt[r], cr)


def test_arguments_are_checked_before_any_device_work():
    """What the Python layer refuses itself: no GPU is needed to get these."""
    from gglasso_amd import model_selection as ms, utils
    from gglasso_amd.problem import glasso_problem
    X = pr.make_case(6, 30, "r30")
    with pytest.raises(AssertionError, match="missing must be"):
        utils.sample_covariance(X, missing="listwise")
    with pytest.raises(AssertionError, match="return_counts needs"):
        utils.sample_covariance(X, return_counts=True)
    with pytest.raises(AssertionError, match="missing must be"):
        utils.sample_covariance_subsets(X, np.arange(10)[None], missing="em")
    with pytest.raises(ValueError, match="kendall"):
        ms.stars_search(X, [0.1], missing="pairwise", correlation="kendall")
    with pytest.raises(ValueError, match="kendall"):
        glasso_problem.from_data(X, missing="pairwise", correlation="kendall")


def test_header_and_binding_declare_the_entry_points():
    import os
    from conftest import ROOT
    from gglasso_amd import _lib
    header = open(os.path.join(ROOT, "include", "ggl_hip.h")).read()
    for name in ("ggl_covariance_pairwise", "ggl_covariance_pairwise_subsets", "ggl_set_S_from_data_pairwise",
                 "ggl_set_S_from_subsets_pairwise"):
        assert name in _lib.EXPORTS and f"int {name}(" in header
