"""Hard spectra, residual-based references and derived bounds for the two symmetric eigensolver routes of the library -- the
LDS Jacobi kernel (csrc/eig_jacobi.hip, p <= 128) and rocsolver_dsyevd followed by the matrix-core reconstruction
(csrc/recon_gemm.hip) -- shared by test_cpu_eig_ref.py and test_gpu_eig_spectra.py.  No GPU import.

Notation: eps = 2^-52, |A| = |A|_inf (largest absolute row sum, >= |A|_2 for symmetric A), p the dimension.

Cases.  `cases(p)` returns named matrices with their exact spectrum in numpy.longdouble.  Every case (but the Wilkinson
matrix) is known as A_ld = Q_ld diag(d) Q_ld^T with Q_ld orthogonal to longdouble rounding: for the constructed cases Q_ld
is a product of p Householder reflectors formed in longdouble and A the symmetrised rounding of A_ld to float64; for the
cases written down directly (zero, identity, ones, diagonal, 2x2 blocks, Toeplitz) A is exact and (d, Q_ld) is the analytic
eigendecomposition evaluated in longdouble.  Either way slack = |A - A_ld|_F, evaluated in longdouble, bounds the distance
of A's true eigenvalues from d (Weyl: |lambda_i(A) - d_i| <= |A - A_ld|_2 <= slack).  It is added to every bound that
compares with d and never folded into a constant.  For a map f with Lipschitz constant 1 on the reals (phiplus:
f' = (1 + d / sqrt(d^2 + 4 beta)) / 2 in (0, 1); max(d - mu, 0)) the matrix function is Lipschitz in the Frobenius norm
with the same constant, so F_ref = Q_ld f(d) Q_ld^T is within slack of f(A), whatever the multiplicities.

The bounds, and where their form comes from.  The Jacobi kernel works on G = (A + sigma I) / 2^e, sigma = 2 |A|: the
eigenvalues of A + sigma I lie in [sigma / 2, 3 sigma / 2], so |G|_2 <= 1.5 sigma <= 3 |A| and cond(G) <= 3.  One-sided
Jacobi applies plane rotations to the rows of G; each rotation is orthogonal to a few eps, a row takes part in p - 1
rotations a sweep, and the stopping rule |g_a . g_b| <= sqrt(p) eps |g_a||g_b| leaves the rows orthogonal to that relative
level.  With cond(G) <= 3 the singular values |g_i| are then those of G to a relative c p eps (Demmel & Veselic 1992 for
the one-sided method; the growth with p is the rotations a row sees, sweeps is a constant here), i.e. absolutely
c p eps 3 |A|; subtracting sigma is one more rounding of size eps 3 |A|.  Hence

    eigenvalues    |D_i - d_i|                    <= C_VAL p eps |A| + slack
    residual       max_i |A q_i - D_i q_i|_2      <= C_RES p eps |A|
    orthogonality  max |Q^T Q - I|                <= C_ORTH sqrt(p) eps
    fused output   max |out - F_ref|              <= C_OUT p eps max(|A|, |f(A)|_inf) + slack

(residual: a row of the rotated G is G q_i to c p eps |G|_2, and q_i is it, normalised; orthogonality: the stopping rule's
own sqrt(p) eps plus the normalisation; fused output: out = sum_m f_m q_m q_m^T is a sum of p terms of size |f|, each
carrying the eigenpair's error, against |f(A)|_inf; the eigenvalue error enters through Lip(f) = 1, hence the max with
|A|.)  The same forms hold for a backward-stable tridiagonalisation + divide and conquer (LAPACK dsyevd, rocSOLVER's
dsyevd) with the usual p eps |A|_2 backward error, and for a float64 reconstruction.

The constants are measured, not chosen: the worst ratio over the whole case list at p in MEASURE_P of the float64 NumPy twin
of the kernel below (`jacobi_twin`) for the Jacobi route, and of numpy.linalg.eigh with a longdouble reconstruction for the
rocSOLVER route; the bound is 4 x that ratio (the margin of diag_ref.EIG_CONST), so that another summation order passes and
a lost digit does not.  `measure_constants()` reproduces the ratios (python tests/eig_ref.py prints them);
test_cpu_eig_ref.py asserts that they are reproduced.  The device's observed ratios are recorded beside them.
"""
import functools

import numpy as np

LD = np.longdouble
EPS = 2.0 ** -52
EPS_LD = float(np.finfo(LD).eps)
PI_LD = 4 * np.arctan(LD(1))
JMAXP, JMAXC, JMAXSWEEP = 128, 8, 48          # csrc/eig_jacobi.hip
MEASURE_P = (7, 33, 64, 65, 128)
JACOBI, ROCSOLVER = 1, 2                     # GGL_EIG_JACOBI, GGL_EIG_ROCSOLVER

# Worst ratio over cases(p) at every p of MEASURE_P (measure_constants(); python tests/eig_ref.py prints them): eigenvalues,
# residual, orthogonality, fused output.  The twin's are reproduced to the digit by test_cpu_eig_ref.py (its arithmetic is
# elementwise float64 in a fixed order); LAPACK's are those of the NumPy build they were measured with.
TWIN_RATIO_BY_P = {
    7: {"val": 1.299, "res": 1.422, "orth": 0.927, "out": 1.158},
    33: {"val": 1.746, "res": 2.320, "orth": 0.976, "out": 1.725},
    64: {"val": 2.533, "res": 2.558, "orth": 1.001, "out": 2.084},
    65: {"val": 2.037, "res": 2.048, "orth": 1.008, "out": 1.807},
    128: {"val": 2.020, "res": 2.034, "orth": 1.006, "out": 1.588},
}
LAPACK_RATIO_BY_P = {
    7: {"val": 0.431, "res": 0.511, "orth": 2.188, "out": 0.560},
    33: {"val": 0.117, "res": 0.148, "orth": 1.897, "out": 0.229},
    64: {"val": 0.031, "res": 0.074, "orth": 1.474, "out": 0.072},
    65: {"val": 0.030, "res": 0.082, "orth": 1.550, "out": 0.111},
    128: {"val": 0.013, "res": 0.054, "orth": 1.223, "out": 0.032},
}
TWIN_SWEEPS_BY_P = {7: 7, 33: 14, 64: 19, 65: 17, 128: 22}      # largest sweep count of the twin (the cap is 48)
# The twin's sweep count for every case of cases(p), in the list's order, at the sizes the device's sweep-budget test runs
# (twin_sweep_table() recomputes it; test_cpu_eig_ref.py checks the rows up to p = 33 and the slowest case of p = 128).
JACOBI_P = (1, 2, 3, 7, 33, 63, 64, 65, 66, 127, 128)
TWIN_SWEEPS = {
    1: (1, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1),
    2: (2, 2, 2, 2, 1, 2, 2, 2, 1, 1, 2, 1, 2, 2, 2),
    3: (3, 2, 3, 2, 2, 3, 2, 4, 1, 1, 2, 1, 2, 5, 5),
    7: (5, 7, 6, 2, 5, 6, 6, 6, 1, 1, 2, 1, 2, 7, 6),
    33: (11, 14, 8, 2, 8, 13, 10, 8, 1, 1, 2, 1, 2, 8, 7),
    63: (14, 16, 8, 3, 9, 18, 9, 9, 1, 1, 2, 1, 2, 9, 7),
    64: (15, 18, 8, 3, 9, 19, 10, 9, 1, 1, 2, 1, 2, 9, 7),
    65: (13, 15, 8, 2, 9, 17, 10, 9, 1, 1, 2, 1, 2, 9, 7),
    66: (12, 14, 8, 2, 10, 20, 11, 9, 1, 1, 2, 1, 2, 9, 7),
    127: (17, 20, 9, 2, 9, 21, 11, 10, 1, 1, 2, 1, 2, 10, 7),
    128: (15, 17, 9, 3, 10, 22, 11, 10, 1, 1, 2, 1, 2, 10, 7),
}
KEYS = ("val", "res", "orth", "out")
TWIN_RATIO = {k: max(r[k] for r in TWIN_RATIO_BY_P.values()) for k in KEYS}          # jacobi_twin
LAPACK_RATIO = {k: max(r[k] for r in LAPACK_RATIO_BY_P.values()) for k in KEYS}      # numpy.linalg.eigh, longdouble reconstruction
# ... and the worst ratios an MI355X gave (test_gpu_eig_spectra.py prints them).  Jacobi, every case at JACOBI_P and two
# cases at every p from 1 to 128: eigenvalues and residual at p = 66, orthogonality at p = 2, fused output at p = 127.
# rocSOLVER + reconstruction, every case at p = 7 .. 200 (all four at p = 7) but the one the test module lists as found and
# not fixed (ones((200, 200)): orthogonality 6.1e12).  Before its input was scaled the route also gave eigenvalue ratios of up
# to 3e13 for every case scaled by 2^-100 or less.
DEVICE_RATIO = {JACOBI: {"val": 3.574, "res": 3.583, "orth": 1.065, "out": 2.094},
                ROCSOLVER: {"val": 0.419, "res": 0.483, "orth": 2.871, "out": 1.037}}
MARGIN = 4.0
CONST = {JACOBI: {k: MARGIN * v for k, v in TWIN_RATIO.items()},
         ROCSOLVER: {k: MARGIN * v for k, v in LAPACK_RATIO.items()}}


def norm_inf(A):
    return float(np.abs(np.asarray(A, dtype=np.float64)).sum(axis=-1).max()) if np.size(A) else 0.0


# ---- eigenvalue maps (longdouble) -------------------------------------------------------------------------------------------

def phiplus_ld(d, beta):
    d = np.asarray(d, dtype=LD)
    return (np.sqrt(d * d + 4 * LD(beta)) + d) / 2


def rank_ld(d, mu):
    return np.maximum(np.asarray(d, dtype=LD) - LD(mu), LD(0))


# ---- the case list ----------------------------------------------------------------------------------------------------------

class Case:
    """A (p,p) float64; d (p,) longdouble, ascending, or None (Wilkinson); Q_ld (p,p) longdouble with A_ld = Q_ld diag(d_q)
    Q_ld^T (d_q: d in the order of Q_ld's columns); slack = |A - A_ld|_F; beta, mu: the parameters of the two fused maps."""

    def __init__(self, name, A, d_q=None, Q=None, mu=None):
        self.name, self.A, self.p = name, np.ascontiguousarray(A, dtype=np.float64), A.shape[0]
        assert np.array_equal(self.A, self.A.T)
        self.Q, self.d_q = Q, (None if d_q is None else np.asarray(d_q, dtype=LD))
        self.d = None if d_q is None else np.sort(self.d_q)
        self.norm = norm_inf(self.A)
        if Q is not None:
            A_ld = (Q * self.d_q) @ Q.T
            self.slack = float(np.sqrt(((self.A.astype(LD) - A_ld) ** 2).sum()))
        else:
            self.slack = None
        dmax = self.norm if self.d is None else float(np.abs(self.d).max())
        # phiplus without cancellation to speak of: beta >= 0.05 at |d| <= 100, growing with d^2 beyond
        self.beta = max(0.05, 5e-6 * dmax * dmax)
        self.mu = (0.25 * dmax if dmax > 0 else 0.5) if mu is None else mu

    def scaled(self, k):
        """The case 2^k A with spectrum 2^k d: exact in float64 while nothing leaves the normal range (the entries of the
        constructed cases are of order 1), and the slack is evaluated anew."""
        s = LD(2) ** k
        return Case(f"{self.name}*2^{k}", np.ldexp(self.A, k), None if self.d_q is None else self.d_q * s, self.Q)

    def f_ref(self, which):
        """(F_ref longdouble (p,p), |f(A)|_inf) of 'phiplus' (beta) or 'rank' (mu); None for a case without (d, Q_ld)."""
        if self.Q is None:
            return None
        f = phiplus_ld(self.d_q, self.beta) if which == "phiplus" else rank_ld(self.d_q, self.mu)
        F = (self.Q * f) @ self.Q.T
        return F, float(np.abs(F).sum(axis=1).max())


@functools.lru_cache(maxsize=None)
def householder_q(p, seed=0):
    """Product of p Householder reflectors I - 2 v v^T / (v^T v), Gaussian v, accumulated in longdouble."""
    rng = np.random.default_rng(1000 * p + seed)
    Q = np.eye(p, dtype=LD)
    for _ in range(p):
        v = rng.standard_normal(p).astype(LD)
        Q = Q - np.outer(Q @ v, (2 / (v @ v)) * v)
    return Q


def _constructed(name, d, p, mu=None, seed=0):
    Q = householder_q(p, seed)
    d = np.asarray(d, dtype=LD)
    A_ld = (Q * d) @ Q.T
    A = A_ld.astype(np.float64)
    A = np.tril(A) + np.tril(A, -1).T
    return Case(name, A, d, Q, mu)


def spectra(p, rng):
    """name -> (d, mu or None) of the constructed cases."""
    h = p // 2
    goe = rng.standard_normal((p, p))
    mu = 0.7
    straddle = rng.uniform(-2.0, 2.0, p)
    straddle[: min(p, 4)] = (mu + 1e-9, mu - 1e-9, mu + 1e-9, mu - 1e-9)[: min(p, 4)]
    lowrank = np.zeros(p)
    lowrank[: p // 3] = rng.uniform(0.5, 3.0, p // 3) * rng.choice([-1.0, 1.0], p // 3)
    one = np.zeros(p)
    one[0] = 3.0
    return {
        "cluster_pm1": (np.r_[np.ones(p - h), -np.ones(h)], 0.5),
        "cluster_1_2_spread": (np.r_[1 + 1e-13 * rng.uniform(-1, 1, p - h), 2 + 1e-13 * rng.uniform(-1, 1, h)], 1.5),
        "identity_plus_goe": (1 + 1e-10 * np.linalg.eigvalsh((goe + goe.T) / np.sqrt(2.0)), 0.5),
        "rank1": (one, None),
        "rank_third": (lowrank, None),
        "graded": (10.0 ** np.linspace(-12, 2, p), 1e-3),
        "straddle": (straddle, mu),
        "gaussian": (np.linalg.eigvalsh((goe + goe.T) / 2), None),
    }


def _direct(p, rng):
    I = np.eye(p, dtype=LD)
    out = [Case("zero", np.zeros((p, p)), np.zeros(p), I), Case("identity", np.eye(p), np.ones(p), I)]
    # ones = p v v^T, v = 1 / sqrt(p): the reflector that maps e_1 to v diagonalises it
    v = np.full(p, 1 / np.sqrt(LD(p)))
    w = -v.copy()
    w[0] += 1
    H = I - np.outer(w, (2 / (w @ w)) * w) if p > 1 else I
    out.append(Case("ones", np.ones((p, p)), np.r_[LD(p), np.zeros(p - 1, dtype=LD)], H))
    dg = 10.0 ** np.linspace(-8, 8, p)
    out.append(Case("diag_1e-8_1e8", np.diag(dg), dg, I))
    # 2x2 blocks [[a, b], [b, a]] (a 1x1 block [a] closes an odd p): a +- b, vectors (e_i +- e_{i+1}) / sqrt 2
    a, b = rng.uniform(-2, 2, (p + 1) // 2), rng.uniform(-2, 2, (p + 1) // 2)
    A, Q, d = np.zeros((p, p)), np.zeros((p, p), dtype=LD), np.zeros(p, dtype=LD)
    r = 1 / np.sqrt(LD(2))
    for m in range((p + 1) // 2):
        i = 2 * m
        if i + 1 < p:
            A[i, i] = A[i + 1, i + 1] = a[m]
            A[i, i + 1] = A[i + 1, i] = b[m]
            Q[i, i], Q[i + 1, i], Q[i, i + 1], Q[i + 1, i + 1] = r, r, r, -r
            d[i], d[i + 1] = LD(a[m]) + LD(b[m]), LD(a[m]) - LD(b[m])
        else:
            A[i, i], Q[i, i], d[i] = a[m], 1, a[m]
    out.append(Case("blocks_2x2", A, d, Q))
    # tridiagonal Toeplitz (-1, 2, -1): 2 - 2 cos(k pi / (p + 1)), vectors sqrt(2 / (p + 1)) sin(j k pi / (p + 1))
    T = 2 * np.eye(p) - np.eye(p, k=1) - np.eye(p, k=-1)
    k = np.arange(1, p + 1, dtype=LD)
    Qt = np.sqrt(LD(2) / (p + 1)) * np.sin(np.outer(k, k) * (PI_LD / (p + 1)))
    out.append(Case("toeplitz_-1_2_-1", T, 2 - 2 * np.cos(k * (PI_LD / (p + 1))), Qt))
    # Wilkinson W_p^+: diagonal |i - (p - 1) / 2|, off-diagonals 1; pairs of eigenvalues that agree to working precision.
    # No closed form: checked by residual and orthogonality only.
    out.append(Case("wilkinson", np.diag(np.abs(np.arange(p) - (p - 1) / 2)) + np.eye(p, k=1) + np.eye(p, k=-1)))
    return out


@functools.lru_cache(maxsize=None)
def cases(p):
    """The case list at dimension p (a tuple of Case; built once per p, read-only)."""
    rng = np.random.default_rng(7000 + p)
    out = [_constructed(name, d, p, mu) for name, (d, mu) in spectra(p, rng).items()] + _direct(p, rng)
    for c in out:
        c.A.setflags(write=False)
    return tuple(out)


@functools.lru_cache(maxsize=None)
def sweep_cases(p):
    """One clustered and one generic case for the sweep over every p (a second Q_ld, so not the matrices of cases(p))."""
    rng = np.random.default_rng(9000 + p)
    sp = spectra(p, rng)
    return tuple(_constructed(n, sp[n][0], p, sp[n][1], seed=1) for n in ("cluster_pm1", "gaussian"))


# ---- residual-based checks (longdouble) -------------------------------------------------------------------------------------

def errors(case, D, Q):
    """{'val', 'res', 'orth'}: max |sort(D) - d| less the slack (None without a spectrum), max_i |A q_i - D_i q_i|_2,
    max |Q^T Q - I|, all in longdouble.  A non-finite entry gives inf."""
    if not (np.all(np.isfinite(D)) and np.all(np.isfinite(Q))):
        return {"val": np.inf, "res": np.inf, "orth": np.inf}
    A, Dl, Ql = case.A.astype(LD), np.asarray(D, dtype=LD), np.asarray(Q, dtype=LD)
    R = A @ Ql - Ql * Dl
    out = {"res": float(np.sqrt((R * R).sum(axis=0)).max()), "orth": float(np.abs(Ql.T @ Ql - np.eye(case.p)).max())}
    out["val"] = None if case.d is None else max(float(np.abs(np.sort(Dl) - case.d).max()) - case.slack, 0.0)
    return out


def out_error(case, which, out):
    """(max |out - F_ref| less the slack, the scale max(|A|, |f(A)|_inf)); None for a case without F_ref."""
    ref = case.f_ref(which)
    if ref is None:
        return None
    F, fn = ref
    if not np.all(np.isfinite(out)):
        return np.inf, max(case.norm, fn)
    return max(float(np.abs(np.asarray(out, dtype=LD) - F).max()) - case.slack, 0.0), max(case.norm, fn)


def units(case):
    """The bounds' units without their constants: {'val', 'res'}: p eps |A|, 'orth': sqrt(p) eps."""
    u = case.p * EPS * case.norm
    return {"val": u, "res": u, "orth": np.sqrt(case.p) * EPS}


def ratios(case, D, Q, outs=None):
    """Observed error / unit for every quantity that applies: {'val', 'res', 'orth', 'out'}.  A zero unit (the zero matrix)
    demands a zero error: ratio 0 then, inf otherwise.  outs: {'phiplus': out, 'rank': out} or None."""
    e, u = errors(case, D, Q), units(case)
    r = {}
    for k in ("val", "res", "orth"):
        if e[k] is not None:
            r[k] = (0.0 if e[k] == 0 else np.inf) if u[k] == 0 else e[k] / u[k]
    for which, o in (outs or {}).items():
        oe = out_error(case, which, o)
        if oe is not None:
            v = ((0.0 if oe[0] == 0 else np.inf) if oe[1] == 0 else oe[0] / (case.p * EPS * oe[1]))
            r["out"] = max(r.get("out", 0.0), v)
    return r


def check(case, method, D, Q, outs=None, worst=None):
    """Asserts every bound of `method` on (D, Q[, outs]); folds the ratios into `worst` (a dict) when given."""
    r = ratios(case, D, Q, outs)
    for k, v in r.items():
        if worst is not None:
            worst[k] = max(worst.get(k, 0.0), v)
        assert v <= CONST[method][k], f"{case.name} p={case.p} method={method}: {k} ratio {v:.3g} > {CONST[method][k]:.3g}"
    return r


# ---- the float64 NumPy twin of k_jacobi -------------------------------------------------------------------------------------

def _lane_sum(X, LG):
    """Row sums of X (..., JMAXC * LG) in the kernel's order: each of the LG lanes adds its JMAXC elements in turn, then an
    xor butterfly over the lanes (every lane ends with the same bits; lane 0 is returned)."""
    s = np.zeros(X.shape[:-1] + (LG,))
    for u in range(X.shape[-1] // LG):
        s = s + X[..., u * LG:(u + 1) * LG]
    lanes = np.arange(LG)
    off = LG // 2
    while off:
        s = s + s[..., lanes ^ off]
        off >>= 1
    return s[..., 0]


def jacobi_twin(A, prescale=True, want_q=True, want_out=None):
    """k_jacobi in float64 NumPy: the same shift sigma = 2 |A|_inf (1 for the zero matrix), the same power-of-two scaling
    by 2^-ilogb(sigma) (prescale=False: the kernel as it was before the scaling, for the record of its two scale defects),
    the same round-robin pairing, rotation formulas, stopping rule and sweep cap, the same |row| - sigma eigenvalues.  The
    pairs of one step are disjoint and rotate at once, as on the device; the inner products are summed lane by lane as the
    kernel's shuffles do, but without its fused multiply-adds.  The lower triangle is read.
    Returns (D, Q or None, sweeps (-1: not converged), out or None); D as the kernel leaves it (unsorted), Q's columns the
    eigenvectors in that order; want_out = ('phiplus', beta) or ('rank', mu)."""
    A = np.asarray(A, dtype=np.float64)
    p = A.shape[0]
    assert 1 <= p <= JMAXP
    LG = 32 if (p + 1) // 2 <= 32 else 16
    W = JMAXC * LG
    G = np.zeros((p, W))
    G[:, :p] = np.tril(A) + np.tril(A, -1).T
    with np.errstate(all="ignore"):
        rows = np.zeros(p)
        for j in range(p):
            rows = rows + np.abs(G[:, j])
        sigma = 0.0
        for i in range(p):
            sigma = np.fmax(sigma, rows[i])
        sigma = 2.0 * sigma if sigma > 0.0 else 1.0
        e = int(np.frexp(sigma)[1]) - 1 if (prescale and np.isfinite(sigma)) else 0        # ilogb
        if e != 0:
            s1, s2 = np.ldexp(1.0, -(int(e / 2))), np.ldexp(1.0, -(e - int(e / 2)))
            G = (G * s1) * s2
            sigma = (sigma * s1) * s2
        G[np.arange(p), np.arange(p)] += sigma
        n = p + (p & 1)
        g = np.arange(1, n // 2)
        tol = np.sqrt(float(p)) * 2.220446049250313e-16
        sweeps = -1
        for sweep in range(JMAXSWEEP):
            rotated = False
            for s in range(n - 1):
                ra = np.r_[n - 1, (s + g) % (n - 1)]
                rb = np.r_[s, (s - g + (n - 1)) % (n - 1)]
                ok = (ra < p) & (rb < p)
                ra, rb = ra[ok], rb[ok]
                va, vb = G[ra], G[rb]
                al, be, ga = _lane_sum(va * va, LG), _lane_sum(vb * vb, LG), _lane_sum(va * vb, LG)
                rot = np.abs(ga) > tol * np.sqrt(al * be)
                if not rot.any():
                    continue
                rotated = True
                ra, rb, va, vb, al, be, ga = ra[rot], rb[rot], va[rot], vb[rot], al[rot], be[rot], ga[rot]
                zeta = (be - al) / (2.0 * ga)
                t = np.copysign(1.0, zeta) / (np.abs(zeta) + np.sqrt(1.0 + zeta * zeta))
                c = 1.0 / np.sqrt(1.0 + t * t)
                sn = c * t
                G[ra] = c[:, None] * va - sn[:, None] * vb
                G[rb] = sn[:, None] * va + c[:, None] * vb
            if not rotated:
                sweeps = sweep + 1
                break
        nu = np.sqrt(_lane_sum(G * G, LG))       # the final norms run c = li, li + LG, ...: the same lane order
        Gn = G[:, :p] * (1.0 / nu)[:, None]
        D = np.ldexp(nu - sigma, e)
        out = None
        if want_out is not None:
            f = (0.5 * (np.sqrt(D * D + 4.0 * want_out[1]) + D)) if want_out[0] == "phiplus" else np.fmax(D - want_out[1], 0.0)
            out = np.zeros((p, p))                # the kernel's order: m in turn, g_i g_j first (bitwise symmetric)
            for m in range(p):
                out = out + f[m] * (Gn[m][:, None] * Gn[m][None, :])
    return D, (Gn.T.copy() if want_q else None), sweeps, out


def sorted_pair(D, Q):
    """(D ascending, Q's columns in that order): the NumPy convention the C ABI returns."""
    idx = np.argsort(D, kind="stable")
    return D[idx], Q[:, idx]


def twin_outputs(case):
    """(D sorted, Q, sweeps, {'phiplus': out, 'rank': out}) of the twin on one case."""
    D, Q, sweeps, o1 = jacobi_twin(case.A, want_out=("phiplus", case.beta))
    o2 = jacobi_twin(case.A, want_q=False, want_out=("rank", case.mu))[3]
    Ds, Qs = sorted_pair(D, Q)
    return Ds, Qs, sweeps, {"phiplus": o1, "rank": o2}


def lapack_outputs(case):
    """numpy.linalg.eigh and the two fused outputs reconstructed from it in longdouble."""
    D, Q = np.linalg.eigh(case.A)
    Ql = Q.astype(LD)
    outs = {"phiplus": (Ql * phiplus_ld(D, case.beta)) @ Ql.T, "rank": (Ql * rank_ld(D, case.mu)) @ Ql.T}
    return D, Q, outs


def twin_sweep_table(ps=JACOBI_P):
    return {p: tuple(jacobi_twin(c.A, want_q=False)[2] for c in cases(p)) for p in ps}


def measure_constants(ps=MEASURE_P, verbose=False):
    """({p: worst twin ratios}, {p: worst LAPACK ratios}, {p: largest twin sweep count}) over cases(p), p in ps."""
    tw, la, sw = {}, {}, {}
    for p in ps:
        tw[p], la[p], sw[p] = {}, {}, 0
        for c in cases(p):
            D, Q, sweeps, outs = twin_outputs(c)
            assert sweeps > 0, (c.name, p)
            sw[p] = max(sw[p], sweeps)
            rt = ratios(c, D, Q, outs)
            Dl, Ql, ol = lapack_outputs(c)
            rl = ratios(c, Dl, Ql, ol)
            for k in rt:
                tw[p][k], la[p][k] = max(tw[p].get(k, 0.0), rt[k]), max(la[p].get(k, 0.0), rl[k])
            if verbose:
                print(f"p={p:4d} {c.name:22s} sweeps {sweeps:2d}  twin " + " ".join(f"{k} {v:6.3f}" for k, v in rt.items())
                      + "   lapack " + " ".join(f"{k} {v:6.3f}" for k, v in rl.items()))
    return tw, la, sw


if __name__ == "__main__":
    tw, la, sw = measure_constants(verbose=True)
    for name, t in (("twin", tw), ("lapack", la)):
        for p in t:
            print(name, p, {k: round(float(v), 3) for k, v in t[p].items()})
    print("twin sweeps", sw)
