"""The debiased graphical lasso on the device (``ggl_debias``: launch_gemm_right, then k_debias of csrc/debias.hip) against
the longdouble reference at the bounds derived in tests/debias_ref.py, its bitwise guarantees and refusals, and what is
built on it (``utils.debiased_precision``, ``glasso_problem.edge_inference``).

Shapes: p = 15 / 16 / 17, 31 / 33 and 63 / 64 / 65 lie on both sides of the edges of the 16-wide matrix-core block and of the
32- and 64-tiles, odd p rows are not 16-byte aligned, p = 129 has three 64-tiles (five 32-tiles), so a tile pair that is not
adjacent to the diagonal; K = 9 crosses the XCD decode (one full round of eight and a remainder of one)."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import debias_ref as dr  # noqa: E402

pytestmark = pytest.mark.gpu

PS = [1, 2, 15, 16, 17, 31, 33, 63, 64, 65, 129]
KS = [1, 3, 9]
TILES = (4, 8, 0)                                   # GGL_DEBIAS_TILE32, GGL_DEBIAS_TILE64, the library's choice
SENTINEL = -12345.678


def call(Th, Sm, n, flags=0):
    from gglasso_amd import utils
    return utils._debias_call(np.ascontiguousarray(Th), np.ascontiguousarray(Sm), np.ascontiguousarray(n, dtype=np.float64), flags)


@pytest.mark.parametrize("kind", ["cov", "inv"])
@pytest.mark.parametrize("p", PS)
def test_device_against_the_longdouble_reference(p, kind):
    """Every K and every tile choice at ``|T - T_ref|_ij <= (2p + 8) u (|Theta||S||Theta|)_ij + 4u |Theta_ij|`` and SE
    relatively within 6u (tests/debias_ref.py), with both stacks bitwise symmetric.  kind 'inv': S = inv(Theta), T ~ Theta."""
    Th, Sm = dr.inputs(p, kind)
    ref = dr.reference_of(p, kind)
    n = dr.n_of(9)
    assert n[1] != int(n[1]) and len(set(n)) == 9
    if p >= 15:
        off = ~np.eye(p, dtype=bool)
        assert 0.6 <= np.mean(Th[0][off] == 0.0) <= 0.8
    for K in KS:
        for flags in TILES:
            T, SE = call(Th[:K], Sm[:K], n[:K], flags)
            assert np.array_equal(T, np.swapaxes(T, 1, 2)) and np.array_equal(SE, np.swapaxes(SE, 1, 2)), (K, flags)
            dr.check_against_reference(T, SE, Th[:K], Sm[:K], (ref[0][:K], ref[1][:K]), f"device p={p} {kind} K={K} flags={flags}")
    if kind == "inv" and p > 1:
        assert np.abs(T - Th).max() <= 1e-10 * np.abs(Th).max()


@pytest.mark.parametrize("p", [17, 65, 129])
def test_bitwise_properties(p):
    Th, Sm = dr.inputs(p, "cov")
    n = dr.n_of(9)
    for flags in TILES:
        T, SE = call(Th, Sm, n, flags)
        T2, SE2 = call(Th, Sm, n, flags)
        assert np.array_equal(T, T2) and np.array_equal(SE, SE2), flags                     # two calls, the same bits
        assert np.array_equal(T, np.swapaxes(T, 1, 2)) and np.array_equal(SE, np.swapaxes(SE, 1, 2))
        for k in (0, 4, 8):                                                                 # instance k alone
            Tk, SEk = call(Th[k:k + 1], Sm[k:k + 1], n[k:k + 1], flags)
            assert np.array_equal(Tk[0], T[k]) and np.array_equal(SEk[0], SE[k]), (flags, k)


def refused(Th, Sm, n, flags, K=None, p=None):
    """(return code, message, T_out, SE_out) of a raw call whose outputs were pre-filled with the sentinel."""
    from gglasso_amd import _lib
    Th, Sm, n = (np.ascontiguousarray(a, dtype=np.float64) for a in (Th, Sm, n))
    T, SE = np.full(Th.shape, SENTINEL), np.full(Th.shape, SENTINEL)
    rc = _lib.load().ggl_debias(0, Th.shape[0] if K is None else K, Th.shape[1] if p is None else p, _lib.ptr(Th), _lib.ptr(Sm),
                                _lib.ptr(n), flags, _lib.ptr(T), _lib.ptr(SE))
    return rc, _lib.last_error(), T, SE


def test_refusals():
    from gglasso_amd import _lib
    Th0, Sm0 = dr.inputs(17, "cov")
    n0 = dr.n_of(3)
    cases = []
    Th = Th0[:3].copy(); Th[1, 4, 9] = np.nan
    cases.append((Th, Sm0[:3], n0, 0, r"Theta of instance 1, variable 4"))
    Sm = Sm0[:3].copy(); Sm[2, 16, 0] = np.nan
    cases.append((Th0[:3], Sm, n0, 0, r"S of instance 2, variable 16"))
    Sm = Sm0[:3].copy(); Sm[0, 3, 3] = np.inf
    cases.append((Th0[:3], Sm, n0, 0, r"S of instance 0, variable 3"))
    Th = Th0[:3].copy(); Th[2, 5, 5] = 0.0
    cases.append((Th, Sm0[:3], n0, 0, r"Theta of instance 2, variable 5: the diagonal entry is 0"))
    Th = Th0[:3].copy(); Th[0, 0, 0] = -1.0
    cases.append((Th, Sm0[:3], n0, 0, r"Theta of instance 0, variable 0: the diagonal entry is -1"))
    n = n0.copy(); n[1] = 0.0
    cases.append((Th0[:3], Sm0[:3], n, 0, r"n of instance 1 is 0"))
    n = n0.copy(); n[2] = np.nan
    cases.append((Th0[:3], Sm0[:3], n, 0, r"n of instance 2 is nan"))
    n = n0.copy(); n[0] = np.inf
    cases.append((Th0[:3], Sm0[:3], n, 0, r"n of instance 0 is inf"))
    cases.append((Th0[:3], Sm0[:3], n0, 1, r"flags: unknown bits"))
    cases.append((Th0[:3], Sm0[:3], n0, 16, r"flags: unknown bits"))
    cases.append((Th0[:3], Sm0[:3], n0, 12, r"exclude each other"))
    import re
    for Th, Sm, n, flags, text in cases:
        rc, msg, T, SE = refused(Th, Sm, n, flags)
        assert rc == _lib.E_ARG and re.search(text, msg), (text, rc, msg)
        assert np.all(T == SENTINEL) and np.all(SE == SENTINEL), text                      # nothing was written
    rc, msg, T, SE = refused(Th0[:3], Sm0[:3], n0, 0, K=0)
    assert rc == _lib.E_ARG and np.all(T == SENTINEL)
    # ... and the same inputs, untouched, are served
    rc, msg, T, SE = refused(Th0[:3], Sm0[:3], n0, 0)
    assert rc == 0 and not np.any(T == SENTINEL) and not np.any(SE == SENTINEL)
    # the Python wrapper turns the code into the AssertionError of a bad argument
    from gglasso_amd import utils
    Th = Th0[0].copy(); Th[2, 2] = 0.0
    with pytest.raises(AssertionError, match=r"Theta of instance 0, variable 2"):
        utils.debiased_precision(Th, Sm0[0], 100)


@pytest.mark.parametrize("p", [1, 17, 65, 129])
def test_wrapper_against_the_twin(p):
    """Device and twin each lie within the bounds of the reference, so within twice the bounds of each other."""
    from gglasso_amd import utils
    Th, Sm = dr.inputs(p, "cov")
    n = dr.n_of(3)
    T, SE = utils.debiased_precision(Th[:3], Sm[:3], n)
    Tt, SEt = utils.host_debiased_precision(Th[:3], Sm[:3], n)
    assert T.shape == SE.shape == (3, p, p)
    assert np.all(np.abs(T - Tt) <= 2 * dr.t_bound(Th[:3], Sm[:3]))
    assert np.all(np.abs(SE - SEt) <= 12 * dr.U * SEt)
    # a single matrix with a scalar N; return_se=False
    T0, SE0 = utils.debiased_precision(Th[0], Sm[0], float(n[0]))
    assert T0.shape == (p, p) and np.array_equal(T0, T[0]) and np.array_equal(SE0, SE[0])
    assert np.array_equal(utils.debiased_precision(Th[0], Sm[0], float(n[0]), return_se=False), T[0])


def test_edge_inference_device_against_host():
    """from_data -> solve -> edge_inference at p = 30, N = 600: the device route and ``host=True`` give the same
    ``significant_`` and z-scores within what the bounds on T (twice, device against twin) and SE (12u) allow for z = T / SE:
    ``|dz| <= 2 bound_T / SE + 16u |z|``."""
    from gglasso_amd import glasso_problem
    rng = np.random.default_rng(2)
    p, N = 30, 600
    Th0 = np.eye(p)
    i = np.arange(p - 1)
    Th0[i, i + 1] = Th0[i + 1, i] = 0.4
    X = np.linalg.cholesky(np.linalg.inv(Th0)) @ rng.standard_normal((p, N))
    P = glasso_problem.from_data(X, reg_params={"lambda1": 0.08})
    P.solve()
    P.edge_inference()
    sol = P.solution
    dev = {a: np.copy(getattr(sol, a)) for a in ("debiased_precision_", "standard_error_", "zscore_", "pvalue_adj_", "significant_")}
    P.edge_inference(host=True)
    assert np.array_equal(dev["significant_"], sol.significant_)
    bound = 2 * dr.t_bound(sol.precision_, sol.sample_covariance_) / sol.standard_error_ + 16 * dr.U * np.abs(sol.zscore_)
    assert np.all(np.abs(dev["zscore_"] - sol.zscore_) <= bound)
    assert np.array_equal(dev["debiased_precision_"], dev["debiased_precision_"].T)
    # the true edges (the first off-diagonals) are found, and few others at the 5 % false discovery rate
    sig = dev["significant_"]
    assert sig[i, i + 1].all()
    assert sig.sum() // 2 - (p - 1) <= 5
