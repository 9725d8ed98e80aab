"""TEST-ONLY reference of the debiased graphical lasso (``ggl_debias``, ``utils.host_debiased_precision``): the same
expressions in ``numpy.longdouble``, the error bounds the implementations are held to, and the inputs the tests share.

Bounds (u = 2^-53; the products in any summation order, fused or not):

* ``T = 2 Theta - (Theta S) Theta``.  For a computed product of (p x p) matrices ``|fl(AB) - AB| <= g_p |A||B|`` with
  ``g_p = p u / (1 - p u)`` (Higham, Accuracy and Stability, (3.13)), whatever the order of the sums.  With M^ = fl(Theta S),
  ``|M^| <= (1 + g_p)|Theta||S|``, so ``|fl(M^ Theta) - Theta S Theta| <= (2 g_p + g_p^2)|Theta||S||Theta|``, below
  ``(2 p + 1) u |Theta||S||Theta|`` for the sizes here.  2 Theta_ij is exact and the subtraction adds one rounding,
  ``u |t| <= u (2 |Theta_ij| + (1 + 3 p u)(|Theta||S||Theta|)_ij)``.  The longdouble reference (unit roundoff 2^-64) and its
  rounding when compared add less than ``2^-10`` of that.  Together: ``|T - T_ref|_ij <= (2 p + 8) u (|Theta||S||Theta|)_ij +
  4 u |Theta_ij|``, with room to spare.
* ``SE = sqrt((Theta_ii Theta_jj + Theta_ij^2) / n)``: two products, a sum of two non-negative terms (no cancellation), a
  quotient, a root: five roundings, or four with the sum and the second product fused.  The root halves the relative error
  it is handed (at most 4 u) and adds its own: about 3 u.  The bound is ``6 u`` relative."""
import functools

import numpy as np

U = 2.0 ** -53
LD = np.longdouble


def reference(Theta, S, n):
    """(T, SE) in longdouble, the upper triangle deciding and the lower one mirroring it, as the implementations do."""
    Theta, S = np.asarray(Theta), np.asarray(S)
    single = Theta.ndim == 2
    Th, Sm = (Theta[None], S[None]) if single else (Theta, S)
    nn = np.broadcast_to(np.asarray(n, dtype=np.float64), (Th.shape[0],))
    T, SE = np.empty(Th.shape, dtype=LD), np.empty(Th.shape, dtype=LD)
    for k in range(Th.shape[0]):
        A, B = Th[k].astype(LD), Sm[k].astype(LD)
        Uk = np.triu(A)
        d = np.diagonal(A)
        t = np.triu(2 * Uk - (A @ B) @ A.T)
        se = np.triu(np.sqrt((d[:, None] * d[None, :] + Uk * Uk) / LD(nn[k])))
        T[k] = t + np.triu(t, 1).T
        SE[k] = se + np.triu(se, 1).T
    return (T[0], SE[0]) if single else (T, SE)


def t_bound(Theta, S):
    """(2p + 8) u |Theta||S||Theta| + 4u |Theta|, per entry (of a matrix or a stack)."""
    Theta, S = np.asarray(Theta, dtype=np.float64), np.asarray(S, dtype=np.float64)
    p = Theta.shape[-1]
    A = np.abs(Theta)
    return (2 * p + 8) * U * (A @ np.abs(S) @ np.swapaxes(A, -1, -2)) + 4 * U * A


def check_against_reference(T, SE, Theta, S, ref, what, factor=1):
    """Asserts the two bounds (times ``factor``) and returns the worst ratios (T error / bound, SE relative error / u)."""
    Tr, SEr = ref
    et = np.abs(np.asarray(T).astype(LD) - Tr).astype(np.float64)
    bt = t_bound(Theta, S)
    rt = float(np.divide(et, bt, out=np.zeros_like(et), where=bt > 0).max())      # (a zero bound: the assert below decides)
    rs = float((np.abs(np.asarray(SE).astype(LD) - SEr) / SEr).max() / U)
    print(f"{what}: max |T - T_ref| / bound = {rt:.3e}, max rel SE error = {rs:.2f} u")
    assert np.all(et <= factor * bt), (what, rt)
    assert rs <= 6 * factor, (what, rs)
    return rt, rs


def n_of(K):
    """Per-instance numbers of observations that differ, every second one not an integer."""
    return 50.0 + 37.5 * np.arange(K)


@functools.lru_cache(maxsize=None)
def inputs(p, kind, K=9):
    """(Theta, S) (K,p,p): Theta random, symmetric, diagonally dominant (so positive definite) with about 70 % exact zeros off
    the diagonal; S the covariance of random data (kind 'cov') or inv(Theta), symmetrised (kind 'inv': T ~ Theta, the two terms
    cancel).  Shared, never changed."""
    rng = np.random.default_rng([p, 7])
    Th, Sm = np.empty((K, p, p)), np.empty((K, p, p))
    for k in range(K):
        A = np.triu(rng.uniform(-1, 1, (p, p)) * (rng.random((p, p)) < 0.3), 1)
        A = A + A.T
        Th[k] = A + np.diag(np.abs(A).sum(axis=1) + rng.uniform(0.5, 1.5, p))
        if kind == 'cov':
            X = rng.standard_normal((p, 3 * p + 5)) * rng.uniform(0.5, 2.0, (p, 1))
            Sm[k] = np.cov(X, bias=True).reshape(p, p)
        else:
            Si = np.linalg.inv(Th[k])
            Sm[k] = (Si + Si.T) / 2
    Th.setflags(write=False)
    Sm.setflags(write=False)
    return Th, Sm


@functools.lru_cache(maxsize=None)
def reference_of(p, kind, K=9):
    Th, Sm = inputs(p, kind, K)
    T, SE = reference(Th, Sm, n_of(K))
    T.setflags(write=False)
    SE.setflags(write=False)
    return T, SE
