"""Term-by-term reference of the KKT residual (ggl_kkt_terms / ggl_kkt_residual) and of the three parts of the objective
(ggl_objective), and the table of cases tests/test_cpu_diag_ref.py and tests/test_gpu_diagnostics.py share.

The reference is evaluated on the state it is GIVEN (in the GPU tests: what the device holds, read back with ``state()``), so
every comparison isolates the diagnostic's own arithmetic.  X is the SCALED dual the ctx holds; the reference's functions take
rho X (admm_solver.py:262).

  term1 = |Theta - prox(Theta + rho X)| / (1 + |Theta|)        prox_p (GGL / FGL), prox_od_1norm per instance (SGL)
  term2 = |Theta - Omega - L| / (1 + |Theta|)
  term3 = |Omega - phiplus(eigh(Omega - nk S - rho X), nk)| / (1 + |Omega|)
  term4 = |L - prox_rank(eigh(L - rho X), mu1)| / (1 + |L|)     latent, else 0               admm_solver.py:343-371
  obj   = { -sum_k log det Omega_k, <Omega, S>, P_val(Theta) }                               ggl_helper.py:266-270, 162-176

The prox operators and the eigendecompositions are the oracle's (float64); differences, squares and sums are numpy.longdouble.

States are NOT ADMM iterates (on an iterate term 1 and term 4 vanish by construction and the maximum hides them): a few oracle
iterations from the identity ('generic') or a converged oracle solve ('near' a fixed point), then independent symmetric
Gaussian noise on each of Omega, Theta, L, X -- standard deviation 0.03 (generic: every applicable term is 1e-2 .. 1) or 1e-6
(near: every term is about 1e-6, which asks whether it survives the cancellation in Theta - prox(.) and Omega - phiplus(.)).

Bounds (u = 2^-53, N = K p^2 elements of a stack)
  terms 1, 2 (derived)   The device's prox input and output differ from the reference's by at most e = 8 n u max(1, max|V|) per
      element (n the reduction length behind one element: 1 for SGL and for term 2, K for GGL / FGL; V = Theta + rho X for
      term 1, |Theta| + |Omega| + |L| for term 2; the prox is non-expansive, so this holds at its kinks: theta_step_ref.py), so
      |dD|_F <= e sqrt(N); a float64 sum of N squares errs by at most (N + 8) u relative, which -- not halved by the square
      root -- also covers the sum behind the denominator.  bound = (e sqrt(N) + (N + 8) u |D|_F) / (1 + |Theta|).
  terms 3, 4 (measured constant)   An eigendecomposition stands on both sides; unit = p u max_k |W_k|_2 / (1 + |.|), W the
      stack decomposed.  The reference's own uncertainty is of that order, so the constant cannot go below about 1.  Measured
      on an MI355X over CASES: largest deviation / unit = EIG_RATIO_MEASURED = 20.4 (LDS Jacobi, p = 64 .. 128; 0.14 at most on
      rocSOLVER); the bound is EIG_CONST = 82 = 4 x that, so that another eigensolver build passes and a lost digit does not.
  <Omega, S>     (N + 8) u sum |Omega_ij S_ij|   (the sum can cancel)
  P_val          (N_pairs + K + 8) u relative    (all terms non-negative; N_pairs = p (p - 1) / 2, FSGL: p^2 entries)
  -log det       unit = K p u kappa_max, kappa from the reference's eigenvalues of Omega; measured LOGDET_RATIO_MEASURED = 1.73
      (at p = 1; 0.21 at most above), the bound is LOGDET_CONST = 7 = 4 x that, the same on the three routes (eigenvalues of W,
      Cholesky factor, eigenvalues of Omega)."""
import numpy as np

from oracle import ggl_oracle as orc
import fsgl_fixtures as fx
from theta_step_ref import sym

U = 2.0 ** -53
NOISE_GENERIC, NOISE_NEAR = 0.03, 1e-6
FLOOR = 1e-3                    # every applicable term of a generic case is at least this (the CPU twin asserts it)

# measured on an MI355X over CASES / OBJ_CASES (largest deviation / unit), and the constants derived from them
EIG_RATIO_MEASURED = 20.4        # term 4 on the LDS Jacobi eigensolver at p = 64, 65, 128 (rocSOLVER: 0.14 at most)
EIG_CONST = 82.0
LOGDET_RATIO_MEASURED = 1.73     # p = 1 (two roundings of one logarithm); 0.21 at most for p >= 2
LOGDET_CONST = 7.0

EIG_AUTO, EIG_JACOBI, EIG_ROCSOLVER = 0, 1, 2
ld = np.longdouble


def fro(A):
    """Frobenius norm of a whole stack, squares summed in longdouble"""
    A = np.asarray(A).astype(ld)
    return np.sqrt((A * A).sum())


# ---- the reference ---------------------------------------------------------------------------------------------------------
def sgl_thresholds(K, p, lambda1, mask):
    """(K,p,p) thresholds of prox_od_1norm: lambda1, the shared (p,p) array or the (K,p,p) per-instance arrays"""
    if mask is None:
        return np.full((K, p, p), float(lambda1))
    return np.broadcast_to(np.asarray(mask, dtype=np.float64), (K, p, p)).copy()


def prox_theta(reg, V, lambda1, lambda2, mask=None):
    if reg == "SGL":
        thr = sgl_thresholds(V.shape[0], V.shape[-1], lambda1, mask)
        return np.stack([orc.prox_od_1norm(V[k], thr[k]) for k in range(V.shape[0])])
    return orc.prox_p(V, lambda1, lambda2, reg)


class KktRef:
    """terms (4,) longdouble; bounds (4,) float64 for terms 1, 2 (derived) and the UNITS of terms 3, 4 (times EIG_CONST: the bound);
    D: |D|_F of the four numerators."""

    def __init__(self, **kw):
        self.__dict__.update(kw)


def kkt_ref(reg, Omega, Theta, L, X, S, rho, lambda1, lambda2, nk, latent, mu1, mask=None):
    K, p = Omega.shape[0], Omega.shape[-1]
    N = K * p * p
    nk = np.ones(K) if nk is None else np.asarray(nk, dtype=np.float64)
    Xu = rho * X
    nT, nO, nL = fro(Theta), fro(Omega), fro(L)
    n_red = 1 if reg == "SGL" else K
    # term 1
    V = Theta + Xu
    D1 = Theta.astype(ld) - prox_theta(reg, V, lambda1, lambda2, mask).astype(ld)
    e1 = 8 * n_red * U * max(1.0, float(np.abs(V).max()))
    # term 2
    D2 = Theta.astype(ld) - Omega.astype(ld) - L.astype(ld)
    e2 = 8 * U * max(1.0, float((np.abs(Theta) + np.abs(Omega) + np.abs(L)).max()))
    # term 3
    W3 = Omega - nk[:, None, None] * S - Xu
    D3 = Omega.astype(ld) - orc.phiplus_stack(W3, nk)[0].astype(ld)
    w3 = float(np.abs(np.linalg.eigvalsh(W3)).max())
    terms = [fro(D1) / (1 + nT), fro(D2) / (1 + nT), fro(D3) / (1 + nO), ld(0)]
    Dn = [float(fro(D1)), float(fro(D2)), float(fro(D3)), 0.0]
    bounds = [(e1 * np.sqrt(N) + (N + 8) * U * Dn[0]) / float(1 + nT), (e2 * np.sqrt(N) + (N + 8) * U * Dn[1]) / float(1 + nT),
              p * U * w3 / float(1 + nO), 0.0]
    if latent:
        W4 = L - Xu
        D4 = L.astype(ld) - orc.rank_stack(W4, np.asarray(mu1, dtype=np.float64)).astype(ld)
        terms[3] = fro(D4) / (1 + nL)
        Dn[3] = float(fro(D4))
        bounds[3] = p * U * float(np.abs(np.linalg.eigvalsh(W4)).max()) / float(1 + nL)
    return KktRef(terms=np.array(terms, dtype=ld), bounds=np.array(bounds), D=np.array(Dn))


def oracle_kkt(reg, Omega, Theta, L, X, S, rho, lambda1, lambda2, nk, latent, mu1, mask=None):
    """The oracle's own residual (the maximum) for the same state.  K single problems (SGL) are one block-diagonal single
    problem: eigh, the soft threshold (zero stays zero) and the Frobenius norms all act block by block."""
    K, p = Omega.shape[0], Omega.shape[-1]
    if reg != "SGL":
        nk3 = (np.ones(K) if nk is None else np.asarray(nk, dtype=np.float64)).reshape(K, 1, 1)
        return orc.kkt_stopping_criterion_mgl(Omega, Theta, L, rho * X, S, lambda1, lambda2, nk3, reg, latent,
                                              None if mu1 is None else np.asarray(mu1, dtype=np.float64))
    from scipy.linalg import block_diag
    bd = lambda A: block_diag(*list(A))
    thr = bd(sgl_thresholds(K, p, lambda1, mask))
    if latent:
        assert np.ptp(mu1) == 0.0, "one mu1 for the block-diagonal single problem"
    return orc.kkt_stopping_criterion_sgl(bd(Omega), bd(Theta), bd(L), rho * bd(X), bd(S), thr, latent,
                                          None if mu1 is None else float(np.asarray(mu1).ravel()[0]))


class ObjRef:
    """parts (3,) longdouble {-sum log det Omega, <Omega,S>, P_val}; bounds (3,): the UNIT of part 0 (times LOGDET_CONST: the
    bound), the absolute bounds of parts 1 and 2."""

    def __init__(self, **kw):
        self.__dict__.update(kw)


def p_val(reg, Theta, lambda1, lambda2, M=None):
    """(value in longdouble, number of terms of the outer sum).  The upper triangle decides, as in ggl_helper.py:162-176; FSGL:
    lambda1 sum_{I != J} |Theta_IJ|_F over all off-diagonal blocks (functional_sgl_admm.py:36)."""
    K, p = Theta.shape[0], Theta.shape[-1]
    if reg == "FSGL":
        s = ld(0)
        for k in range(K):
            bn = fx.block_norms(Theta[k], M).astype(ld)
            s += bn.sum() - np.trace(bn)
        return lambda1 * s, p * p
    iu = np.triu_indices(p, 1)
    V = Theta[:, iu[0], iu[1]].astype(ld)
    res = lambda1 * np.abs(V).sum()
    if reg == "GGL":
        res += lambda2 * np.sqrt((V * V).sum(axis=0)).sum()
    else:
        res += lambda2 * np.abs(V[1:] - V[:-1]).sum()
    return 2 * res, p * (p - 1) // 2


def obj_ref(reg, Omega, Theta, S, lambda1, lambda2, M=None):
    K, p = Omega.shape[0], Omega.shape[-1]
    N = K * p * p
    R = np.linalg.cholesky(Omega)
    logdet = 2 * np.log(np.diagonal(R, axis1=-2, axis2=-1).astype(ld)).sum()
    ev = np.linalg.eigvalsh(Omega)
    kappa = float((ev[:, -1] / ev[:, 0]).max())
    OS = Omega.astype(ld) * S.astype(ld)
    pv, n_pairs = p_val(reg, Theta, lambda1, lambda2, M)
    parts = np.array([-logdet, OS.sum(), pv], dtype=ld)
    bounds = np.array([K * p * U * kappa, (N + 8) * U * float(np.abs(OS).sum()), (n_pairs + K + 8) * U * float(pv)])
    return ObjRef(parts=parts, bounds=bounds, kappa=kappa)


# ---- the cases ---------------------------------------------------------------------------------------------------------------
class Case:
    """One state.  mask: None | 'shared' ((p,p) array) | 'zero' ((p,p) zeros) | 'k' (per-instance arrays); eig: ctx selector;
    noise: NOISE_GENERIC | NOISE_NEAR; M: FSGL block size (objective cases only)."""

    def __init__(self, reg, K, p, latent=False, rho=1.0, noise=NOISE_GENERIC, eig=EIG_AUTO, mask=None, M=None, tag=""):
        self.reg, self.K, self.p, self.latent, self.rho, self.noise, self.eig, self.mask, self.M = reg, K, p, latent, rho, noise, eig, mask, M
        self.name = (f"{reg.lower()}-K{K}-p{p}" + ("-latent" if latent else "") + (f"-rho{rho:g}" if rho != 1.0 else "")
                     + ("-near" if noise == NOISE_NEAR else "") + ({0: "", 1: "-jacobi", 2: "-rocsolver"}[eig])
                     + (f"-mask{mask}" if mask else "") + (f"-M{M}" if M else "") + tag)

    @property
    def seed(self):
        return 7000 + 131 * self.K + self.p + (17 if self.latent else 0) + {"SGL": 0, "GGL": 1, "FGL": 2, "FSGL": 3}[self.reg]

    @property
    def generic(self):
        return self.noise == NOISE_GENERIC


def _noise(rng, K, p, sd):
    return sd * sym(rng.standard_normal((K, p, p))) * np.sqrt(2.0)     # symmetric, every entry of standard deviation sd


def build_case(c):
    """Everything a case needs, host side: S, nk and mu1 (unequal per instance), lambda1 / lambda2, the mask array, rho and the
    state {Omega, Theta, L, X} (X the scaled dual; L = 0 and None-able where not latent)."""
    from gglasso_amd import synth
    K, p, rho = c.K, c.p, c.rho
    rng = np.random.default_rng(c.seed)
    single = c.reg in ("SGL", "FSGL")
    S, _ = synth.make_problem("SGL" if single else c.reg, K, p, seed=c.seed)
    eye = np.repeat(np.eye(p)[None], K, axis=0)
    lambda1, lambda2 = 0.05, (0.0 if single else 0.02)
    nk = None if single else 1.0 + 0.25 * np.arange(K)
    # (the block-diagonal twin of K single problems has ONE mu1; the multiple-graph problems take one per instance)
    mu1 = None if not c.latent else (np.full(K, 0.15) if single else 0.1 + 0.05 * np.arange(K))
    mask = None
    if c.mask == "shared":
        mask = lambda1 * sym(rng.uniform(0.5, 1.5, (p, p)))
    elif c.mask == "zero":
        mask = np.zeros((p, p))
    elif c.mask == "k":
        # instance k's thresholds are scaled apart so that a call that took the scalar, or instance 0's array, is far off
        mask = lambda1 * sym(rng.uniform(0.5, 1.5, (K, p, p))) * np.array([1.0, 2.5, 0.4, 1.7, 0.8])[:K, None, None]
    # generic: three iterations; near: a converged solve (its dual rescaled to the case's rho: the fixed point's rho X is one)
    it = dict(max_iter=3, tol=1e-20, rtol=1e-20, update_rho=False, rho=rho) if c.generic else dict(max_iter=3000, tol=1e-11, rtol=1e-11)
    if single:
        sols = []
        for k in range(K):
            mk = None if mask is None else (mask[k] if mask.ndim == 3 else mask) / lambda1
            if c.reg == "FSGL":
                mk = None
            sol, info = orc.ADMM_SGL(S[k], lambda1, np.eye(p), latent=c.latent, mu1=None if mu1 is None else float(mu1[k]),
                                     lambda1_mask=mk, **it)
            sol["X"] = sol["X"] * (info["rho"] / rho)
            sols.append(sol)
        st = {nm: np.stack([s[nm] if nm in s else np.zeros((p, p)) for s in sols]) for nm in ("Omega", "Theta", "L", "X")}
    else:
        st, info = orc.ADMM_MGL(S, lambda1, lambda2, c.reg, eye, n_samples=nk, latent=c.latent, mu1=mu1, **it)
        st["X"] = st["X"] * (info["rho"] / rho)
    state = {nm: sym(st[nm]) + _noise(rng, K, p, c.noise) for nm in ("Omega", "Theta", "X")}
    state["L"] = sym(st["L"]) + _noise(rng, K, p, c.noise) if c.latent else np.zeros((K, p, p))
    return dict(S=S, nk=nk, mu1=mu1, lambda1=lambda1, lambda2=lambda2, mask=mask, rho=rho, state=state)


def kkt_ref_of(c, b, st=None):
    st = b["state"] if st is None else st
    return kkt_ref(c.reg, st["Omega"], st["Theta"], st["L"], st["X"], b["S"], b["rho"], b["lambda1"], b["lambda2"], b["nk"],
                   c.latent, b["mu1"], b["mask"])


def _cases():
    C = Case
    out = []
    # GGL / FGL: every p at which a piece changes behaviour (Jacobi for everything <= 8, k_pval's 32-tile, the 1024-element
    # chunk, the LDS Omega-step's 64, Jacobi / rocSOLVER at 128 / 129), K in {1, 2, 3, 5}, latent and rho != 1 alternating
    shapes = ((1, 1), (2, 2), (1, 8), (3, 9), (5, 31), (2, 32), (2, 33), (3, 64), (3, 65), (2, 128), (2, 129), (2, 200))
    for i, (K, p) in enumerate(shapes):
        for j, reg in enumerate(("GGL", "FGL")):
            out.append(C(reg, K, p, latent=(i + j) % 2 == 1, rho=(1.0, 1.7, 0.6)[(i + 2 * j) % 3]))
    out += [C("GGL", 5, 8, latent=True, rho=1.7), C("FGL", 5, 9), C("GGL", 1, 33, latent=True), C("FGL", 1, 65, rho=0.6),
            C("GGL", 3, 129, latent=True, rho=1.7), C("FGL", 3, 128, latent=True)]
    # near a fixed point
    out += [C(reg, K, p, latent=lat, rho=rho, noise=NOISE_NEAR)
            for reg, K, p, lat, rho in (("GGL", 1, 8, False, 1.0), ("FGL", 3, 9, True, 1.7), ("GGL", 2, 33, True, 0.6),
                                        ("FGL", 3, 65, False, 1.0), ("GGL", 2, 129, True, 1.7), ("SGL", 1, 33, False, 1.7))]
    # forced eigensolvers at p = 33
    out += [C("GGL", 3, 33, latent=True, rho=1.7, eig=EIG_JACOBI), C("FGL", 3, 33, latent=True, eig=EIG_ROCSOLVER)]
    # SGL: scalar lambda1, a (p,p) mask, a zero mask (K = 1); per-instance masks (K = 3); latent
    out += [C("SGL", 1, 9), C("SGL", 1, 65, rho=1.7), C("SGL", 1, 33, mask="shared", rho=1.7), C("SGL", 1, 33, mask="zero"),
            C("SGL", 3, 33, mask="k", rho=0.6), C("SGL", 3, 9, mask="k"), C("SGL", 3, 65, mask="shared"),
            C("SGL", 1, 33, latent=True, rho=1.7), C("SGL", 2, 129, latent=True)]
    return out


def _obj_cases():
    """Objective: evaluated after ONE step from the generic start (the eigenvalue-of-W route needs an Omega-step to have run)."""
    C = Case
    out = []
    for i, (K, p) in enumerate(((1, 1), (2, 2), (1, 8), (5, 8), (3, 9), (5, 31), (2, 32), (2, 33), (3, 64), (3, 65), (2, 128),
                                (2, 129), (2, 200))):
        for j, reg in enumerate(("GGL", "FGL")):
            out.append(C(reg, K, p, latent=(i + j) % 2 == 0 and p > 1, rho=(1.0, 1.7, 0.6)[(i + j) % 3]))
    out += [C("GGL", 3, 33, rho=1.7, eig=EIG_JACOBI), C("FGL", 3, 33, latent=True, eig=EIG_ROCSOLVER),
            C("FSGL", 2, 36, M=4, rho=1.7), C("FSGL", 2, 80, M=40)]
    return out


CASES = _cases()
OBJ_CASES = _obj_cases()
