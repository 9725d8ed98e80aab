"""The two symmetric eigensolver routes on hard spectra: the LDS Jacobi kernel (method 1) and rocSOLVER's syevd with the
matrix-core reconstruction (method 2), through ops.eigh / ops.phiplus_matrix / ops.rank_matrix, against the longdouble
references and the derived bounds of tests/eig_ref.py.  Needs a real MI355X.

Each test prints the largest observed ratio error / unit before it asserts; eig_ref.DEVICE_RATIO records them."""
import numpy as np
import pytest

import eig_ref as er
from eig_ref import EPS, JACOBI, ROCSOLVER

pytestmark = pytest.mark.gpu

ROCSOLVER_P = (7, 64, 65, 128, 129, 200)
SIZES = [(JACOBI, p) for p in er.JACOBI_P] + [(ROCSOLVER, p) for p in ROCSOLVER_P]
WORST = {JACOBI: {}, ROCSOLVER: {}}

# Found by these tests on an MI355X (ROCm 7, rocsolver_dsyevd_strided_batched returns info = 0 in both cases).
#  1. Not fixed here, a strict expected-failure test below so that a rocSOLVER that mends it is noticed: ones((200, 200)), one
#     eigenvalue 200 and 199 zeros, inside the K = 15 stack: the returned vectors are not orthogonal, max |Q^T Q - I| = 1.9e-2
#     (6.1e12 sqrt(p) eps; the bound is 8.75), and the fused phiplus output is off by 8.7e8 p eps |A|; eigenvalues (0.0085)
#     and residual (0.12) are fine.  p = 128, 129 and every other case at 200 pass.
#  2. Fixed by scaling the input of syevd by a power of two (csrc/recon_gemm.hip: k_eig_prescale): given any matrix scaled by
#     2^-100 or less (entries of 1e-30) rocSOLVER returns eigenvalue errors of 1e11 .. 3e13 p eps |A|, that is 0.1 % to 10 % of
#     |A|, the same figures at 2^-100, 2^-200 and 2^-320, at every p in 7 .. 200 (p = 65: gaussian 1.0e12, graded 1.3e11,
#     clustered 7.1e12, Toeplitz 1.0e13; p = 129: 6.5e11, 7.8e11, 3.4e12, 5.8e12); at 2^-480 orthogonality goes as well
#     (clustered, p = 65: 2.8e6 sqrt(p) eps).  Scaled up (2^100 .. 2^480) everything but item 1 passed before the fix too.
ROCSOLVER_KNOWN = {(ROCSOLVER, 200): ("ones",)}


@pytest.fixture(scope="module")
def ops():
    from gglasso_amd import ops as o
    yield o
    for m, w in WORST.items():
        print(f"\nmethod {m}: largest observed ratios " + " ".join(f"{k} {v:.3f}" for k, v in sorted(w.items())))


def _stack(cs):
    return np.ascontiguousarray(np.stack([c.A for c in cs]))


def _refusal(fn, *a, **kw):
    """The call's result, or None when the library refused it with GGL_E_SOLVER."""
    from gglasso_amd import _lib
    try:
        return fn(*a, **kw)
    except RuntimeError as e:
        assert f"error {_lib.E_SOLVER}:" in str(e), e
        return None


def _poisoned(A):
    P = A.copy()
    iu = np.triu_indices(A.shape[-1], 1)
    P[:, iu[0], iu[1]] = 1e300
    return P


@pytest.mark.parametrize("method,p", SIZES)
def test_case_list(ops, method, p):
    """Every case of the list at one p as one stack (K = 15): eigenvalues, residual, orthogonality, both fused outputs
    against F_ref, their bitwise symmetry, and only the lower triangle read.  A case that ended in GGL_E_SOLVER would
    raise here."""
    cs = er.cases(p)
    A = _stack(cs)
    beta, mu = np.array([c.beta for c in cs]), np.array([c.mu for c in cs])
    D, Q = ops.eigh(A, method=method)
    ph = ops.phiplus_matrix(A, beta, method=method)
    rk = ops.rank_matrix(A, mu, method=method)
    worst = {}
    for k, c in enumerate(cs):
        if c.name in ROCSOLVER_KNOWN.get((method, p), ()):
            continue
        r = er.ratios(c, D[k], Q[k], {"phiplus": ph[k], "rank": rk[k]})
        for key, v in r.items():
            worst[key] = max(worst.get(key, 0.0), v)
            WORST[method][key] = max(WORST[method].get(key, 0.0), v)
    print(f"method {method} p {p}: " + " ".join(f"{k} {v:.3f}" for k, v in sorted(worst.items())))
    for k, c in enumerate(cs):
        assert np.all(np.diff(D[k]) >= 0), c.name
        if c.name not in ROCSOLVER_KNOWN.get((method, p), ()):           # (asserted by the expected-failure test below)
            er.check(c, method, D[k], Q[k], {"phiplus": ph[k], "rank": rk[k]})
    assert np.array_equal(ph, ph.transpose(0, 2, 1)) and np.array_equal(rk, rk.transpose(0, 2, 1))
    P = _poisoned(A)
    D2, Q2 = ops.eigh(P, method=method)
    assert np.array_equal(D2, D) and np.array_equal(Q2, Q)
    assert np.array_equal(ops.phiplus_matrix(P, beta, method=method), ph)
    assert np.array_equal(ops.rank_matrix(P, mu, method=method), rk)


@pytest.mark.xfail(strict=True, reason="rocSOLVER syevd on ones((200, 200)) inside a stack: max |Q^T Q - I| = 1.9e-2")
def test_rocsolver_ones_p200(ops):
    """Item 1 of the list above: the case test_case_list[2-200] leaves out, in the same stack."""
    cs = er.cases(200)
    A = _stack(cs)
    D, Q = ops.eigh(A, method=ROCSOLVER)
    ph = ops.phiplus_matrix(A, np.array([c.beta for c in cs]), method=ROCSOLVER)
    k = [c.name for c in cs].index("ones")
    print("rocSOLVER ones p 200:", er.ratios(cs[k], D[k], Q[k], {"phiplus": ph[k]}))
    er.check(cs[k], ROCSOLVER, D[k], Q[k], {"phiplus": ph[k]})


@pytest.mark.parametrize("lo", [1, 33, 65, 97])
def test_every_p(ops, lo):
    """Every p from 1 to 128 on the Jacobi kernel, one clustered and one generic matrix each: the switch from 32 to 16
    lanes per row pair at 64 / 65, the dummy row of every odd p, every p mod 16 tail of the per-lane row slices."""
    worst = {}
    for p in range(lo, lo + 32):
        cs = er.sweep_cases(p)
        D, Q = ops.eigh(_stack(cs), method=JACOBI)
        for k, c in enumerate(cs):
            r = er.ratios(c, D[k], Q[k])
            for key, v in r.items():
                if v >= worst.get(key, (-1.0, 0))[0]:
                    worst[key] = (v, p)
                WORST[JACOBI][key] = max(WORST[JACOBI].get(key, 0.0), v)
    print(f"p {lo} .. {lo + 31}: " + " ".join(f"{k} {v[0]:.3f} (p = {v[1]})" for k, v in sorted(worst.items())))
    for key, (v, p) in worst.items():
        assert v <= er.CONST[JACOBI][key], (key, v, p)


@pytest.mark.parametrize("p", er.JACOBI_P)
def test_sweep_budget(p):
    """The same stacks through a ctx created with eig = 1: S = 0, X = 0, Theta = the case, so that W of the Omega-step is
    the case.  Every instance converges (a step that did not would raise), in at most twice the sweeps the NumPy twin
    needs, 40 at the most: headroom below the kernel's cap of 48, and no near-stall passes."""
    from gglasso_amd.solver import HipEngine
    cs = er.cases(p)
    A = _stack(cs)
    Z = np.zeros_like(A)
    eng = HipEngine(Z, Z, A, Z, eig=JACOBI)
    try:
        eng.step(1.0, 0.1, 0.1, "GGL", False, None, np.array([c.beta for c in cs]))
        sweeps = eng.eig_info().copy()
    finally:
        eng.close()
    twin = np.array(er.TWIN_SWEEPS[p])
    print(f"p {p}: device sweeps {sweeps.tolist()}  twin {twin.tolist()}")
    assert np.all(sweeps > 0)
    assert np.all(sweeps <= np.minimum(2 * twin, 40)), [(c.name, int(s), int(t)) for c, s, t in zip(cs, sweeps, twin)]


def _many(K, p, seed):
    """K different matrices: Gaussian ones at scales 2^-3 .. 2^3, every third with a +-1 cluster instead."""
    rng = np.random.default_rng(seed)
    A = rng.standard_normal((K, p, p)) * (2.0 ** rng.integers(-3, 4, K))[:, None, None]
    A = 0.5 * (A + A.transpose(0, 2, 1))
    for k in range(0, K, 3):
        Qk, _ = np.linalg.qr(rng.standard_normal((p, p)))
        d = np.where(np.arange(p) < p // 2, -1.0, 1.0) * (1.0 + k)
        A[k] = (Qk * d) @ Qk.T
        A[k] = 0.5 * (A[k] + A[k].T)
    return A


@pytest.mark.parametrize("K,p", [(600, 5), (300, 33)])
def test_more_matrices_than_compute_units(ops, K, p):
    """One workgroup per matrix and more matrices than the card has CUs: instance k of the stack is bitwise what a K = 1
    call returns for it."""
    A = _many(K, p, 40 + p)
    beta = np.linspace(0.3, 2.0, K)
    D, Q = ops.eigh(A, method=JACOBI)
    ph = ops.phiplus_matrix(A, beta, method=JACOBI)
    assert np.all(np.isfinite(D)) and np.all(np.isfinite(Q)) and np.all(np.isfinite(ph))
    # against LAPACK, at the sum of the two routes' eigenvalue bounds
    unit = p * EPS * np.abs(A).sum(axis=2).max(axis=1)
    err = np.abs(D - np.linalg.eigvalsh(A)).max(axis=1)
    assert np.all(err <= (er.CONST[JACOBI]["val"] + er.CONST[ROCSOLVER]["val"]) * unit), (err / unit).max()
    for k in sorted({0, K - 1} | set(np.random.default_rng(3).choice(K, 14, replace=False).tolist())):
        D1, Q1 = ops.eigh(A[k], method=JACOBI)
        assert np.array_equal(D1, D[k]) and np.array_equal(Q1, Q[k]), k
        assert np.array_equal(ops.phiplus_matrix(A[k], beta[k], method=JACOBI), ph[k]), k


SCALED = ("gaussian", "cluster_1_2_spread", "graded", "toeplitz_-1_2_-1")


def _scale_params(sizes, ks):
    return [(m, p, k) for m, p in sizes for k in ks]


@pytest.mark.parametrize("method,p,k", _scale_params([(JACOBI, 33), (JACOBI, 65), (JACOBI, 128), (ROCSOLVER, 7), (ROCSOLVER, 65),
                                                      (ROCSOLVER, 129)], (-200, -100, 100, 200)))
def test_power_of_two_scaling(ops, method, p, k):
    """eigh(2^k A): on the Jacobi kernel exactly 2^k D and the same bits of Q; on rocSOLVER the same bounds relative to
    |2^k A|_inf."""
    cs = [c for c in er.cases(p) if c.name in SCALED]
    sc = [c.scaled(k) for c in cs]
    D, Q = ops.eigh(_stack(sc), method=method)
    if method == JACOBI:
        D0, Q0 = ops.eigh(_stack(cs), method=method)
        assert np.array_equal(D, np.ldexp(D0, k)) and np.array_equal(Q, Q0)
    for i, c in enumerate(sc):
        er.check(c, method, D[i], Q[i])


@pytest.mark.parametrize("method,p", [(JACOBI, 33), (JACOBI, 65), (ROCSOLVER, 65), (ROCSOLVER, 129)])
def test_ctx_omega_step_at_a_small_scale(method, p):
    """The Omega-step of a ctx (eig_recon: the route the solvers take) on W = 2^-100 A with beta = 2^-200 beta_0: phiplus is
    homogeneous, so Omega must be 2^-100 F_ref(beta_0) to the bound of the unscaled case."""
    from gglasso_amd.solver import HipEngine
    cs = [c for c in er.cases(p) if c.name in SCALED]
    A = np.ldexp(_stack(cs), -100)
    Z = np.zeros_like(A)
    eng = HipEngine(Z, Z, A, Z, eig=method)
    try:
        eng.step_omega(1.0, False, np.ldexp(np.array([c.beta for c in cs]), -200))
        Om = np.ldexp(eng.state()["Omega"], 100)
    finally:
        eng.close()
    for k, c in enumerate(cs):
        err, scale = er.out_error(c, "phiplus", Om[k])
        assert err <= er.CONST[method]["out"] * p * EPS * scale, (c.name, err / (p * EPS * scale))
    assert np.array_equal(Om, Om.transpose(0, 2, 1))


@pytest.mark.parametrize("method,p,k", _scale_params([(JACOBI, 33), (JACOBI, 128), (ROCSOLVER, 65), (ROCSOLVER, 129)],
                                                     (-480, -320, 300, 480)))
def test_extreme_scales(ops, method, p, k):
    """2^k A far outside the range in which sigma^4 is finite and normal: the call meets the same relative bounds or
    refuses with GGL_E_SOLVER; GGL_OK with a result outside the bounds is the one thing it may not do.  (Before the
    kernel scaled its input, k = 300 and 480 returned |row| - sigma of the unrotated matrix with info = 1, and k = -320,
    -480 ran out of sweeps.  Now the Jacobi kernel answers all four, with the bits of the unscaled matrix.)"""
    sc = [c.scaled(k) for c in er.cases(p) if c.name in SCALED]
    got = _refusal(ops.eigh, _stack(sc), method=method)
    print(f"method {method} p {p} k {k}: " + ("refused" if got is None else "answered"))
    if got is not None:
        for i, c in enumerate(sc):
            er.check(c, method, got[0][i], got[1][i])
        if method == JACOBI:
            D0, Q0 = ops.eigh(_stack([c for c in er.cases(p) if c.name in SCALED]), method=method)
            assert np.array_equal(got[0], np.ldexp(D0, k)) and np.array_equal(got[1], Q0)


@pytest.mark.parametrize("bad", [np.nan, np.inf])
@pytest.mark.parametrize("method,p", [(JACOBI, 33), (JACOBI, 65)])
def test_nonfinite_input(ops, method, p, bad):
    """One NaN / Inf in the lower triangle of instance 2 of four: the call refuses, or that instance's outputs say so and
    the other three are bitwise those of the clean stack.  On the Jacobi kernel only, whose loops are bounded by the sweep
    cap whatever the data; the iteration limits of rocSOLVER's syevd cannot be read from this repository."""
    cs = [c for c in er.cases(p) if c.name in SCALED]
    A = _stack(cs)
    beta = np.array([c.beta for c in cs])
    B = A.copy()
    B[2, p // 2, 1] = bad
    D0, Q0 = ops.eigh(A, method=method)
    ph0 = ops.phiplus_matrix(A, beta, method=method)
    got, ph = _refusal(ops.eigh, B, method=method), _refusal(ops.phiplus_matrix, B, beta, method=method)
    print(f"method {method} p {p} {bad}: eigh " + ("refused" if got is None else "answered")
          + ", phiplus " + ("refused" if ph is None else "answered"))
    keep = [0, 1, 3]
    if got is not None:
        assert not np.all(np.isfinite(got[0][2]))
        assert np.array_equal(got[0][keep], D0[keep]) and np.array_equal(got[1][keep], Q0[keep])
    if ph is not None:
        assert not np.all(np.isfinite(ph[2]))
        assert np.array_equal(ph[keep], ph0[keep])
