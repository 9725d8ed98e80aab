"""Comparison values and derived error bounds of the batched Cholesky (csrc/cholesky.hip, utils.cholesky_predict,
utils.host_cholesky_predict) and of the leave-one-out bandwidth scores built on it (utils.loo_bandwidth_scores), shared by
test_cpu_bandwidth.py and test_gpu_bandwidth.py.

Comparison value: the column Cholesky A = L L^T with the right-hand side d as a border row (y = L^-1 d), in numpy.longdouble,

    log det = 2 sum_j log l_jj,    q = y^T y = d^T A^-1 d,    smallest pivot = min_j l_jj^2.

Notation: u = 2^-53, gamma_n = n u / (1 - n u), kappa = kappa_2(A) = lambda_max / lambda_min, p the dimension.

1. The factor (Higham, Accuracy and Stability, 2nd ed., Theorem 10.3).  The computed factor satisfies L^ L^^T = A + dA with
   |dA| <= gamma_{p+1} |L^||L^^T| for ANY order of the inner products (the blocked kernel sums them four at a time on the
   matrix cores, the twin through BLAS), and (10.7) || |L^||L^^T| ||_2 <= p (1 - p gamma_{p+1})^-1 ||A||_2.  So
   ||dA||_2 <= e1 ||A||_2 with e1 = p gamma_{p+1} / (1 - p gamma_{p+1}).

2. log det.  det(A + dA) = det(A) prod_i (1 + mu_i), mu_i the eigenvalues of A^-1/2 dA A^-1/2, |mu_i| <= ||A^-1||_2 ||dA||_2
   <= e1 kappa.  |log(1 + mu)| <= |mu| / (1 - |mu|), so the exact 2 sum log l^_jj is within p e1 kappa / (1 - e1 kappa) of
   log det A: to first order p^2 gamma_{p+1} kappa.  The p logarithms are then rounded (a correctly rounded log would be u
   relative; 9 u is allowed for the device's and the C library's) and summed in order (gamma_{p-1} relative to the sum of the
   absolute terms), and the doubling is exact: 2 (p + 8) u sum_j |log l_jj|.  Together

       |d log det| <= p^2 gamma_{p+1} kappa / (1 - p gamma_{p+1} (1 + kappa)) + 2 (p + 8) u sum_j |log l_jj|

   -- the expected first-order form with the denominators of steps 1 and 2 kept.

3. The quadratic form (Theorem 10.4 is this argument for a full solve).  The border row is a forward substitution:
   (L^ + dL) y^ = d with |dL| <= gamma_p |L^| (Theorem 8.5).  So y^^T y^ = d^T (A + dA')^-1 d with
   A + dA' = (L^ + dL)(L^ + dL)^T, |dA'| <= (gamma_{p+1} + 2 gamma_p + gamma_p^2) |L^||L^^T| <= gamma_{3p+1} |L^||L^^T|, and
   ||dA'||_2 <= e3 ||A||_2 with e3 = p gamma_{3p+1} / (1 - p gamma_{p+1}).  With z = A^-1/2 d (z^T z = q) and
   F = A^-1/2 dA' A^-1/2, ||F||_2 <= e3 kappa: d^T (A + dA')^-1 d = z^T (I + F)^-1 z, which is within
   e3 kappa / (1 - e3 kappa) q of q.  The final dot product of p non-negative terms adds gamma_p q.  Because kappa >= 1,
   gamma_p <= p gamma_{3p+1} kappa, so

       |dq| <= 2 p gamma_{3p+1} kappa q / (1 - p gamma_{3p+1} (1 + kappa))

   -- again the expected form, 2 p gamma_{3p+1} kappa q, with its denominator.

4. The smallest pivot.  l_jj^2 = 1 / (e_j^T A_j^-1 e_j) with A_j the leading j x j block: step 3's argument with d = e_j and
   dA of step 1 (no substitution) gives a relative perturbation of at most e1 kappa_2(A_j) / (1 - ...) and
   kappa_2(A_j) <= kappa_2(A) (interlacing); the minimum over j of quantities within r relative of each other is within r.
   So |d min pivot| <= p gamma_{p+1} kappa / (1 - p gamma_{p+1} (1 + kappa)) min pivot.

5. The leave-one-out score log det S + d^T S^-1 d of a weighted covariance (tests/weighted_ref.py, DESIGN 19, has its
   bound: |S^ - S|_ij <= B_ij elementwise).  The kernel factors S^ = S + E, ||E||_2 <= ||B||_F, and a right-hand side
   d^ = fl(x - m^) = d + dd with |dd_i| <= (2 n + 2) u M_i + u |d_i| (the mean's bound there, one subtraction).  With
   eta = ||B||_F / lambda_min(S) and rho = ||dd||_2 / sqrt(lambda_min(S)):

       |log det S^ - log det S| <= p eta / (1 - eta)                                   (step 2's argument)
       |d^^T S^^-1 d^ - q|      <= eta / (1 - eta) qq + 2 sqrt(q) rho + rho^2,   qq = q + 2 sqrt(q) rho + rho^2

   and the factorisation of S^ adds the bounds of steps 2 and 3 with kappa_2(S^) <= kappa (1 + eta) / (1 - eta) and q^ <= the
   bound just given.  kappa and lambda_min are taken from the comparison value's own matrix.  A ridge is added to S exactly on
   both sides (one rounding of the diagonal, u |s_ii|, goes into B).

The bounds are loose (worst-case constants, 2-norm estimates); the tests print the largest observed fraction.
"""
import numpy as np

U = 2.0 ** -53
LD = np.longdouble


def gamma(n):
    return n * U / (1.0 - n * U)


def chol_reference(A, d=None):
    """(log det, q, smallest pivot, sum |log l_jj|) of one symmetric positive definite A (p,p) in longdouble, d (p,) or None
    (q = 0): the column Cholesky, the right-hand side as a border row."""
    A = np.asarray(A)
    p = A.shape[0]
    M = np.tril(A).astype(LD) if d is None else np.vstack([np.tril(A).astype(LD), np.asarray(d, dtype=LD)[None]])
    L = np.zeros_like(M)
    for j in range(p):
        piv = M[j, j] - L[j, :j] @ L[j, :j]
        assert piv > 0, "the comparison value needs a positive definite matrix"
        L[j, j] = np.sqrt(piv)
        L[j + 1:, j] = (M[j + 1:, j] - L[j + 1:, :j] @ L[j, :j]) / L[j, j]
    dg = np.diagonal(L[:p])
    logs = np.log(dg)
    q = L[p] @ L[p] if d is not None else LD(0)
    return 2 * logs.sum(), q, (dg * dg).min(), float(np.abs(logs).sum())


def logdet_bound(p, kappa, abslog):
    return p * p * gamma(p + 1) * kappa / (1.0 - p * gamma(p + 1) * (1.0 + kappa)) + 2 * (p + 8) * U * abslog


def quad_bound(p, kappa, q):
    return 2 * p * gamma(3 * p + 1) * kappa * q / (1.0 - p * gamma(3 * p + 1) * (1.0 + kappa))


def pivot_bound(p, kappa, piv):
    return p * gamma(p + 1) * kappa * piv / (1.0 - p * gamma(p + 1) * (1.0 + kappa))


def spd_stack(K, p, seed, kappa=100.0):
    """S (K,p,p) = Q diag(lambda) Q^T with lambda log-spaced over [1, kappa] (kappa_2 known), symmetrised exactly, and d (K,p)."""
    rng = np.random.default_rng([20250301, K, p, seed])
    S = np.empty((K, p, p))
    lam = np.logspace(0.0, np.log10(kappa), p) if p > 1 else np.array([kappa])
    for k in range(K):
        Q, _ = np.linalg.qr(rng.standard_normal((p, p)))
        A = (Q * lam) @ Q.T
        S[k] = 0.5 * (A + A.T)
    return S, rng.standard_normal((K, p))


def fractions(res, S, d, kappa=100.0):
    """Largest observed fractions (log det, q, smallest pivot) of the bounds of steps 2-4 over a stack; res as
    ``cholesky_predict`` returns it for a stack.  d None: q must be exactly 0 (fraction 0) -- anything else counts as inf."""
    logdet, quad, minpiv, status = res
    fr = np.zeros(3)
    for k in range(S.shape[0]):
        ld, q, mp, al = chol_reference(S[k], None if d is None else d[k])
        p = S.shape[1]
        fr[0] = max(fr[0], float(abs(LD(logdet[k]) - ld)) / logdet_bound(p, kappa, al))
        if d is None:
            fr[1] = max(fr[1], 0.0 if quad[k] == 0.0 else np.inf)
        else:
            fr[1] = max(fr[1], float(abs(LD(quad[k]) - q)) / quad_bound(p, kappa, float(q)))
        fr[2] = max(fr[2], float(abs(LD(minpiv[k]) - mp)) / pivot_bound(p, kappa, float(mp)))
    return fr


def score_reference(X, w, target, center=True, ridge=0.0):
    """(score in longdouble as a float pair (value, bound)) of one weight row w (N,) scoring column ``target`` of X (p,N): the
    comparison value log det S + d^T S^-1 d of step 5 and its bound."""
    import weighted_ref
    p = X.shape[0]
    S, B = weighted_ref.reference(X, w, center)
    lo, hi = weighted_ref.support(w)
    n = hi - lo
    Xl, wl = X.astype(LD), np.asarray(w).astype(LD)
    wt = wl / wl.sum()
    if center:
        m = (Xl * wt).sum(axis=1)
        Mabs = (np.abs(Xl) * wt).sum(axis=1)
    else:
        m, Mabs = np.zeros(p, dtype=LD), np.zeros(p, dtype=LD)
    d = Xl[:, target] - m
    S = S + ridge * np.eye(p, dtype=LD)
    B = B + U * np.diag(np.abs(np.diagonal(S)))
    ld, q, _, al = chol_reference(S, d)
    ev = np.linalg.eigvalsh(S.astype(np.float64))
    lmin, kappa = float(ev[0]), float(ev[-1] / ev[0])
    assert lmin > 0
    dd = ((2 * n + 2) * U * Mabs if center else 0.0) + U * np.abs(d)
    eta = float(np.sqrt((B * B).sum())) / lmin
    rho = float(np.sqrt((dd * dd).sum())) / np.sqrt(lmin)
    assert eta < 0.5
    q = float(q)
    qq = q + 2 * np.sqrt(q) * rho + rho * rho
    bound = p * eta / (1 - eta) + eta / (1 - eta) * qq + (qq - q)
    kap = kappa * (1 + eta) / (1 - eta)
    bound += logdet_bound(p, kap, al + p * eta / (1 - eta)) + quad_bound(p, kap, qq * (1 + eta / (1 - eta)))
    return float(ld + LD(q)), float(bound)


def score_fraction(SCORE, X, W, targets, center=True, ridge=0.0):
    """Largest |SCORE[r] - reference| / bound over the rows of one bandwidth: W (M,N) its weights, targets (M,)."""
    fr = 0.0
    for r in range(W.shape[0]):
        ref, bound = score_reference(X, W[r], int(targets[r]), center, ridge)
        fr = max(fr, abs(SCORE[r] - ref) / bound)
    return fr


def case_a(seed):
    """(X (6,240) with the correlation of neighbours swinging 0.8 -> -0.8 over the series, X (6,240) stationary, drawn next
    from the same generator): the generator of the search tests."""
    rng = np.random.default_rng(seed)
    i = np.arange(6)
    X = np.empty((6, 240))
    for n in range(240):
        rho = 0.8 * np.cos(np.pi * n / 239)
        X[:, n] = np.linalg.cholesky(rho ** np.abs(i[:, None] - i[None, :])) @ rng.standard_normal(6)
    Xs = np.linalg.cholesky(0.5 ** np.abs(i[:, None] - i[None, :])) @ rng.standard_normal((6, 240))
    return X, Xs


CASE_A_BANDWIDTHS = [200, 64, 32, 16, 8, 4]


def case_b(seed=0):
    """(X (33,150), times (150,) unsorted and non-integer, eval_index (25,)): correlated variables of unit scale."""
    rng = np.random.default_rng([20250302, seed])
    p, N = 33, 150
    A = np.eye(p) + 0.3 * rng.standard_normal((p, p)) / np.sqrt(p)
    X = A @ rng.standard_normal((p, N))
    times = rng.permutation(2.0 * (np.arange(N) + rng.uniform(-0.3, 0.3, N)))      # mean spacing 2
    ev = np.sort(rng.choice(N, 25, replace=False)).astype(np.int32)
    return X, times, ev
