"""Comparison values and derived error bounds of the least-squares refit of neighbourhood selection (csrc/mb_refit.hip,
utils.neighborhood_refit, utils.host_neighborhood_refit, utils.neighborhood_precision), shared by test_cpu_mbrefit.py and
test_gpu_mbrefit.py.

The problem of node j in a graph: A = {i != j : |W[j,i]| >= t}, d = |A|, beta* = S_AA^-1 s_A with s_A = S[A, j],
q(M; b) = M_jj - 2 m_A' b + b' M_AA b, tau^2 = q(S; beta), r = q(T; beta).  The graph is an INPUT: there is no support to
compare and no case is left out.

Comparison value (``solve_node``): a Cholesky factorisation, the two substitutions and the quadratic forms written out in
numpy.longdouble.  It is never the twin and never the device.

Notation: u = 2^-53, gamma_n = n u / (1 - n u); beta^ the returned coefficients.

1. The normal-equation residual rho = s_A - S_AA beta^ (formed in longdouble), componentwise (``residual_bound``):
       |rho_i| <= gamma_{3d+4} (1 - gamma_{d+2})^-1 sqrt(S_ii) sum_k sqrt(S_kk) |beta^_k|.
   Higham, Accuracy and Stability, 2nd ed., Thm 10.4: the solution computed from a Cholesky factor R^ and two substitutions
   satisfies (S_AA + dA) beta^ = s_A with |dA| <= gamma_{3d+1} |R^'||R^|.  The constant is the sum of three:  gamma_{d+1} for
   the factor (Thm 10.3) and gamma_d for each substitution (Thm 8.5), each from Lemma 8.4: y = (c - sum_{i<k} a_i b_i) / b_k
   evaluated in ANY order satisfies b_k y (1 + theta_k) = c - sum a_i b_i (1 + theta_i), |theta| <= gamma_k, counting one
   rounding per product, per subtraction and for the division.  The factorisation the kernel runs is that recurrence column
   by column (a_i = S_ik - sum_{q<k} L_iq L_kq with q ascending, L_kk = sqrt(a_k), L_ik = a_i / L_kk); its multiply-adds are
   fused, which only removes roundings.  What is NOT assumed is that the device's square root and division are correctly
   rounded: each is allowed 2u, one u more per stage, hence gamma_{d+2} + 2 gamma_{d+1} <= gamma_{3d+4}.  The twin
   (numpy.linalg.cholesky: LAPACK's blocked order; substitutions by numpy dot products) is covered by "any order".
   (|R^'||R^|)_ik <= ||r^_i||_2 ||r^_k||_2 (Cauchy-Schwarz on columns) and ||r^_i||^2 = (R^'R^)_ii <= S_ii + gamma_{d+2}
   ||r^_i||^2, so ||r^_i||^2 <= S_ii / (1 - gamma_{d+2}).  rho = dA beta^ gives the line above.

2. The distance to the solution: S_AA (beta^ - beta*) = -rho, so ||beta^ - beta*||_2 <= ||rho||_2 / lambda_min(S_AA), with
   ||rho||_2 bounded by the norm of step 1's bound (not by the observed residual); the comparison value's own observed
   residual is added in the same way (``distance_bound``).  lambda_min comes from numpy.linalg.eigvalsh in float64, whose
   error (a few u ||S_AA||) is six orders below the smallest lambda_min met here (1 / 22 of the largest diagonal entry).

3. tau^2 and r are compared AT THE RETURNED beta^ with q in longdouble (``quad``), against the rounding bound of their own
   sums of magnitudes (``quad_bound``):
       |d q| <= gamma_{2d+3} ( |M_jj| + sum_i |beta_i| (2 |m_i| + sum_k |M_ik| |beta_k|) ).
   The arrangement is q = M_jj + sum_i beta_i x_i, x_i = w_i - 2 m_i, w_i = sum_k M_ik beta_k.  w_i: d products and d - 1
   additions, in any order gamma_d of sum_k |M_ik||beta_k| (Higham (3.4)); x_i one more rounding (2 m_i is exact); the outer
   sum d products, d additions with M_jj: gamma_{d+1}.  Together at most 2d + 2 roundings on any term, one spare.  Fused
   multiply-adds (the device) only remove roundings.

4. The precision matrix of a COMPLETE graph is inv(S): column j of inv(S) is (1, -beta*) / tau*^2.  q(S; .) is minimised at
   beta* with Hessian 2 S_AA, so q(S; beta^) - tau*^2 = (beta^ - beta*)' S_AA (beta^ - beta*) exactly, and with D_j step 2's
   bound and e_j step 3's:  |tau^^2 - tau*^2| <= dt_j = e_j + lambda_max(S_AA) D_j^2.  Then, with lo_j = tau^^2 - dt_j > 0,
       |1 / tau^^2 - 1 / tau*^2| <= dd_j = dt_j / (tau^^2 lo_j),
       |beta^_i / tau^^2 - beta*_i / tau*^2| <= D_j / lo_j + |beta^_i| dd_j,
   plus 2u of the entry for the division and the comparison value's own rounding (``precision_bound``).  An off-diagonal
   entry of the symmetrised matrix is one of its two estimates (rule 'min'): the larger of their two bounds.
"""
import numpy as np

import mb_ref

U = 2.0 ** -53
LD = np.longdouble


def gamma(n):
    return n * U / (1.0 - n * U)


def neighbours(w_row, j, t):
    with np.errstate(invalid='ignore'):
        e = np.abs(np.asarray(w_row, dtype=np.float64)) >= t
    e[j] = False
    return np.flatnonzero(e)


def solve_node(S, j, A):
    """beta* (d,) in longdouble: S_AA = L L' column by column, L y = s_A, L' beta = y."""
    d = A.size
    SAA = np.asarray(S)[np.ix_(A, A)].astype(LD)
    y = np.asarray(S)[A, j].astype(LD)
    Lf = np.zeros((d, d), dtype=LD)
    for k in range(d):
        a = SAA[k:, k] - Lf[k:, :k] @ Lf[k, :k]
        assert a[0] > 0, "the comparison value needs a positive definite S_AA"
        Lf[k, k] = np.sqrt(a[0])
        Lf[k + 1:, k] = a[1:] / Lf[k, k]
    y = y.copy()
    for k in range(d):
        y[k] = (y[k] - Lf[k, :k] @ y[:k]) / Lf[k, k]
    b = np.zeros(d, dtype=LD)
    for k in range(d - 1, -1, -1):
        b[k] = (y[k] - Lf[k + 1:, k] @ b[k + 1:]) / Lf[k, k]
    return b


def quad(Mat, j, A, beta):
    """q(M; beta) in longdouble."""
    Ml = np.asarray(Mat)[np.ix_(A, A)].astype(LD)
    m = np.asarray(Mat)[A, j].astype(LD)
    b = np.asarray(beta).astype(LD)
    return LD(np.asarray(Mat)[j, j]) - 2 * (m @ b) + b @ (Ml @ b)


def quad_bound(Mat, j, A, beta):
    """Step 3."""
    Ma = np.abs(np.asarray(Mat, dtype=np.float64))
    b = np.abs(np.asarray(beta, dtype=np.float64))
    d = A.size
    return gamma(2 * d + 3) * (Ma[j, j] + float(b @ (2 * Ma[A, j] + Ma[np.ix_(A, A)] @ b)))


def residual(S, j, A, beta):
    """rho = s_A - S_AA beta in longdouble."""
    return np.asarray(S)[A, j].astype(LD) - np.asarray(S)[np.ix_(A, A)].astype(LD) @ np.asarray(beta).astype(LD)


def residual_bound(S, A, beta):
    """Step 1, a vector over A."""
    d = A.size
    sd = np.sqrt(np.diagonal(np.asarray(S, dtype=np.float64))[A])
    return gamma(3 * d + 4) / (1.0 - gamma(d + 2)) * sd * float(sd @ np.abs(np.asarray(beta, dtype=np.float64)))


def distance_bound(S, j, A, beta, beta_ref):
    """Step 2: (the bound of ||beta - beta_ref||_2, lambda_min, lambda_max of S_AA)."""
    if A.size == 0:
        return 0.0, 1.0, 1.0
    ev = np.linalg.eigvalsh(np.asarray(S, dtype=np.float64)[np.ix_(A, A)])
    own = float(np.sqrt((residual(S, j, A, beta_ref) ** 2).sum()))
    return (float(np.linalg.norm(residual_bound(S, A, beta))) + own) / ev[0], float(ev[0]), float(ev[-1])


def check_node(S, T, w_row, j, t, coef_col, tau, r, degree, status, what=""):
    """Everything about one solved node: the list, steps 1-3.  Returns the observed fractions (residual, distance, tau^2, r)
    of their bounds."""
    A = neighbours(w_row, j, t)
    assert degree == A.size and status == 0, f"{what} node {j}: degree {degree} (expected {A.size}), status {status}"
    off = np.ones(len(coef_col), dtype=bool)
    off[A] = False
    assert np.all(coef_col[off] == 0), f"{what} node {j}: a coefficient outside the neighbourhood"
    b = coef_col[A]
    assert np.all(np.isfinite(b)) and np.isfinite(tau)
    fr = fd = 0.0
    if A.size:
        rb = residual_bound(S, A, b)
        fr = float(np.max(np.abs(residual(S, j, A, b)).astype(np.float64) / rb))
        bref = solve_node(S, j, A)
        db, _, _ = distance_bound(S, j, A, b, bref)
        fd = float(np.sqrt(((b.astype(LD) - bref) ** 2).sum())) / db
    ft = float(abs(LD(tau) - quad(S, j, A, b))) / quad_bound(S, j, A, b)
    fh = 0.0
    if T is not None:
        fh = float(abs(LD(r) - quad(T, j, A, b))) / quad_bound(T, j, A, b)
    assert fr <= 1.0 and fd <= 1.0 and ft <= 1.0 and fh <= 1.0, f"{what} node {j} (d = {A.size}): fractions {(fr, fd, ft, fh)}"
    return fr, fd, ft, fh


def check_stack(S, T, W, t, out, what=""):
    """``check_node`` over a whole result ``out`` of (host_)neighborhood_refit for S (M,p,p), T (M,p,p) or None, W (M,G,p,p);
    prints and returns the largest fractions."""
    S, W = np.asarray(S), np.asarray(W)
    M, G, p = W.shape[0], W.shape[1], W.shape[2]
    worst = np.zeros(4)
    for m in range(M):
        for g in range(G):
            for j in range(p):
                f = check_node(S[m], None if T is None else T[m], W[m, g, j], j, t, out['COEF'][m, g][:, j], out['RESVAR'][m, g, j],
                               None if T is None else out['HELDOUT'][m, g, j], int(out['DEGREE'][m, g, j]),
                               int(out['STATUS'][m, g, j]), f"{what} m={m} g={g}")
                worst = np.maximum(worst, f)
    print(f"{what} p={p}: residual {worst[0]:.3f}, distance {worst[1]:.3f}, resvar {worst[2]:.3f}, heldout {worst[3]:.3f} "
          f"of their bounds")
    return worst


def precision_reference(S):
    """inv(S) in longdouble, column by column from the comparison value on the complete graph."""
    p = S.shape[0]
    Th = np.zeros((p, p), dtype=LD)
    for j in range(p):
        A = np.delete(np.arange(p), j)
        b = solve_node(S, j, A)
        tau = quad(S, j, A, b)
        Th[A, j] = -b / tau
        Th[j, j] = 1 / tau
    return Th


def precision_bound(S, coef, resvar):
    """Step 4: (p,p) entrywise bound for ``neighborhood_precision(coef, resvar, 'min')`` of a complete-graph refit."""
    p = S.shape[0]
    E = np.zeros((p, p))
    for j in range(p):
        A = np.delete(np.arange(p), j)
        b, tau = coef[A, j], float(resvar[j])
        D, _, lmax = distance_bound(S, j, A, b, solve_node(S, j, A))
        dt = quad_bound(S, j, A, b) + lmax * D * D
        lo = tau - dt
        assert lo > 0
        dd = dt / (tau * lo)
        E[A, j] = D / lo + np.abs(b) * dd + 2 * U * np.abs(b) / tau
        E[j, j] = dd + 2 * U / tau
    off = np.maximum(E, E.T)
    off[np.arange(p), np.arange(p)] = np.diagonal(E)
    return off


def graphs(p, t=1e-8):
    """The graphs of the ``mb_ref.stack(p)`` matrices: W (3, 3 * L, p, p) -- per matrix the AND stack, the OR stack and the raw
    supports (transposed: row j = node j's support) of ``host_neighborhood_selection`` along ``mb_ref.GRID``."""
    from gglasso_amd import utils
    S = mb_ref.stack(p)
    Wa, inf = utils.host_neighborhood_selection(S, mb_ref.GRID, 'and', return_info=True)
    Wo = utils.neighborhood_graph(inf['COEF'], 'or')
    raw = np.swapaxes(inf['COEF'], -1, -2)
    return np.ascontiguousarray(np.concatenate([Wa, Wo, raw], axis=1))


def heldout_stack(p):
    """T (3,p,p): ``mb_ref.case`` of other seeds."""
    return np.stack([mb_ref.case(p, seed) for seed in (7, 8, 9)])


def star(p, hub, deg):
    """A (p,p) pattern: ``hub`` adjacent to the ``deg`` variables after it (cyclically), symmetric."""
    W = np.zeros((p, p))
    nb = (hub + 1 + np.arange(deg)) % p
    W[hub, nb] = W[nb, hub] = 1.0
    return W

