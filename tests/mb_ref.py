"""Inputs, comparison values and derived error bounds of Meinshausen-Buhlmann neighbourhood selection (csrc/neighborhood.hip,
utils.neighborhood_selection, utils.host_neighborhood_selection), shared by test_cpu_neighborhood.py and
test_gpu_neighborhood.py.

The problem of node j at penalty lambda, on a symmetric S with positive diagonal (s_j its column j):

    beta = argmin over beta with beta_j = 0 of  1/2 beta' S beta - s_j' beta + lambda sum_{k != j} |beta_k|,      g = s_j - S beta
    optimal  <=>  g_k = lambda sign(beta_k) where beta_k != 0,  |g_k| <= lambda where beta_k = 0            (k != j)

Comparison value (``solve``): the cyclic coordinate loop z = g_k + S_kk beta_k, beta_k <- soft(z, lambda) / S_kk in
numpy.longdouble with tol = 0 -- sweeps until one changes nothing or a limit is reached, a screen of all variables from a
gradient recomputed from beta, again until the screen finds nothing.  All nodes of a stack advance together (step i of a sweep
updates the i-th active coordinate, ascending, of every node), which is the same loop per node and takes Python out of the
per-node cost; the limit and the restart that keeps it short are described at ``solve``.  It is never the twin and never the
device, and its own optimality residual is asserted <= 1e-15 before anything is compared with it.

Notation: u = 2^-53, nnz the size of the support of the returned beta, A_k = |s_jk| + sum_l |S_kl| |beta_l|.

1. The optimality residual r_k (``residual``) of a returned beta, with g formed from it in longdouble, against
       |r_k| <= tol sum_{l in supp, l != k} |S_kl| / S_ll  +  C_ROUND (nnz + 2) u A_k.                       (``residual_bound``)
   First term.  The solver ends in a state where the last sweep changed every beta_l by at most tol / S_ll.  Coordinate k's own
   update leaves g_k = lambda sign(beta_k) (or |g_k| <= lambda with beta_k = 0) up to rounding; the updates of the coordinates
   l behind it in that sweep move g_k by S_kl d_l, |d_l| <= tol / S_ll.
   Second term, C_ROUND = 3.  The g the last sweep starts from is recomputed in a fixed order, g = s - sum_l beta_l S_l over the
   support: nnz rounded products and nnz subtractions (one rounding each with a fused multiply-add, two without), so
   |g^_k - g_k| <= gamma_{nnz+1} A_k (Higham, Accuracy and Stability, 2nd ed., (3.4)).  The updates of the sweep in front of
   coordinate k's are at most nnz more operations g <- g - d_l S_kl on a value bounded by A_k: nnz u A_k (the rounding of the
   product, u |d_l S_kl| <= u tol |S_kl| / S_ll, is of second order and dropped).  So the g_k that k's update reads is within
   e = (2 nnz + 1) u A_k of the true one.  The update itself: z = fl(g_k + fl(S_kk beta_k)), two roundings, |z| <= 2 A_k:
   3 u A_k; b = fl(fl(|z| - lambda) / S_kk) is stored as beta_k, so S_kk b = (|z| - lambda)(1 + 2u'): 2 u S_kk |b| <= 2 u A_k.
   With the true g, beta_k = b leaves g_k - lambda sign = (z_true - z) + (z - lambda sign - S_kk b): at most e + 5 u A_k
   = (2 nnz + 6) u A_k <= 3 (nnz + 2) u A_k.  For a k outside the support the final screen saw |g^_k| <= lambda with the same
   e.  The slack nnz u A_k is what is left for the second-order terms.

2. The distance to the solution: the objective is lambda_min(S)-strongly convex and r is a subgradient of it at the returned
   beta, so ||beta - beta*||_2 <= ||r||_2 / lambda_min(S); the comparison value's own residual is added in the same way.

3. The residual variance tau^2 = S_jj - sum_k beta_k (s_jk + g_k) over the support, against its longdouble value at the
   returned beta (``resvar_reference``): the g_k used is within (2 nnz + 1) u A_k of the true one (step 1, all of the last
   sweep's updates included), every term takes two roundings and the sum of nnz terms, in any order, gamma_{nnz-1} of the
   sum of their magnitudes; the last subtraction one more:
       |d tau^2| <= sum_k |beta_k| (2 nnz + 1) u A_k + (nnz + 3) u (S_jj + sum_k |beta_k| (|s_jk| + |g_k|)).
"""
import functools

import numpy as np

U = 2.0 ** -53
LD = np.longdouble
C_ROUND = 3
GRID = (0.4, 0.2, 0.1, 0.05)
SIZES = (1, 2, 3, 5, 17, 63, 64, 65, 130, 255, 256, 257, 300)
MARGIN = 1e-5


def case(p, seed):
    """S (p,p): the correlation matrix of X = chol(Sigma) Z, Sigma_ik = 0.6^|i-k|, Z (p, 4p + 40) standard normal."""
    i = np.arange(p)
    Sigma = 0.6 ** np.abs(i[:, None] - i[None, :])
    X = np.linalg.cholesky(Sigma) @ np.random.default_rng([seed, p]).standard_normal((p, 4 * p + 40))
    S = np.atleast_2d(np.corrcoef(X))
    S = 0.5 * (S + S.T)
    S[i, i] = 1.0
    return S


@functools.lru_cache(maxsize=None)
def stack(p):
    """The (3,p,p) stack of seeds 0, 1, 2 (shared, read-only)."""
    S = np.stack([case(p, seed) for seed in range(3)])
    S.setflags(write=False)
    return S


def gradient_stack(Sl, coef):
    """G (K,p,p) in longdouble, G[k,:,j] = s_j - S_k coef[k,:,j] for longdouble stacks Sl, coef (K,p,p), through the supports
    (a column of coef has few non-zeros)."""
    K, p, _ = coef.shape
    G = Sl.copy()
    cols = np.arange(p)
    for k in range(K):
        nz = coef[k] != 0
        amax = int(nz.sum(axis=0).max())
        order = np.argsort(~nz, axis=0, kind='stable')[:amax]          # (amax,p): a column's non-zero rows first, ascending
        for a in range(amax):                                           # (a row behind a column's support holds a zero)
            G[k] -= Sl[k][:, order[a]] * coef[k][order[a], cols]
    return G


def gradient(S, coef):
    """G (L,p,p) in longdouble, G[l,:,j] = s_j - S coef[l,:,j], for one matrix S and a stack of coefficient matrices."""
    coef = np.asarray(coef).astype(LD)
    return gradient_stack(np.broadcast_to(np.asarray(S).astype(LD), coef.shape), coef)


def _polish(SA, rhs, live):
    """x (node, position) with SA x = rhs on the positions marked live and x = 0 elsewhere: Gauss-Jordan elimination without
    pivoting (the blocks are principal minors of a positive definite matrix), all nodes at once."""
    n, a, _ = SA.shape
    both = live[:, :, None] & live[:, None, :]
    M = np.where(both, SA, 0) + np.where(live, 0, 1)[:, :, None] * np.eye(a, dtype=LD)[None]
    x = np.where(live, rhs, 0)
    for i in range(a):
        f = M[:, :, i] / M[:, i, i][:, None]
        f[:, i] = 0
        x = x - f * x[:, i][:, None]
        M = M - f[:, :, None] * M[:, i, :][:, None, :]
    return x / np.diagonal(M, axis1=1, axis2=2)


def solve(S, lam, sweep_limit=2000, round_limit=100, polish_at=1e-4, sweeps_after=4):
    """The comparison value: B ([M,]L,p,p) longdouble, column j = beta^(j), along the descending grid with warm starts; S (p,p)
    or a (M,p,p) stack, whose nodes all advance together.  Once a sweep moves nothing by more than ``polish_at`` the loop is
    restarted from the solution of the linear system the current support and signs define (``_polish``), which spares the
    hundreds of sweeps of a linearly convergent tail.  The sweep limit: ``sweep_limit`` up to that restart and ``sweeps_after``
    behind it -- from there the loop only moves last bits of a longdouble and, measured, wanders among them for thousands of
    sweeps without ever repeating a state exactly.  What the result is worth is decided by its residual (``reference``)."""
    S = np.asarray(S)
    single = S.ndim == 2
    Sl = (S[None] if single else S).astype(LD)
    M, p, _ = Sl.shape
    n = M * p
    mi, ji = np.repeat(np.arange(M), p), np.tile(np.arange(p), M)      # node -> (matrix, variable)
    dg = np.diagonal(Sl, axis1=1, axis2=2)
    B = np.zeros((M, p, p), dtype=LD)
    member = np.zeros((n, p), dtype=bool)                               # [node, k]
    rows = np.arange(n)[:, None]
    out = np.zeros((M, len(lam), p, p), dtype=LD)
    for l, lv in enumerate(lam):
        lv = LD(lv)
        for rnd in range(round_limit):
            G = gradient_stack(Sl, B)                                   # (M,p,p), column j of matrix m: node (m, j)
            Gn, Bn = G.transpose(0, 2, 1).reshape(n, p), B.transpose(0, 2, 1).reshape(n, p)
            viol = (np.abs(Gn) > lv) & ~member
            viol[rows[:, 0], ji] = False
            if rnd > 0 and not viol.any():
                break
            member |= viol
            amax = int(member.sum(axis=1).max())
            if amax == 0:
                break
            order = np.argsort(~member, axis=1, kind='stable')[:, :amax]         # (node, position): ascending active set
            valid = member[rows, order]
            Bt, Gr, Sd = Bn[rows, order], Gn[rows, order], dg[mi[:, None], order]
            SA = Sl[mi[:, None, None], order[:, :, None], order[:, None, :]]     # (node, position, position)
            sA = Sl[mi[:, None], order, ji[:, None]]
            polished, left = False, sweep_limit
            while left > 0:
                left -= 1
                dmax = 0.0
                for i in range(amax):
                    z = Gr[:, i] + Sd[:, i] * Bt[:, i]
                    b = np.where(valid[:, i], np.sign(z) * np.maximum(np.abs(z) - lv, 0) / Sd[:, i], 0)
                    d = b - Bt[:, i]
                    if d.any():
                        Gr -= d[:, None] * SA[:, i, :]
                        Bt[:, i] = b
                        dmax = max(dmax, float(np.abs(d).max()))
                if dmax == 0.0:
                    break
                if not polished and dmax <= polish_at:
                    polished, left = True, sweeps_after
                    Bt = _polish(SA, sA - lv * np.sign(Bt), Bt != 0)
                    Gr = sA - np.einsum('nab,nb->na', SA, Bt)
            Bn[rows, order] = Bt
            B = Bn.reshape(M, p, p).transpose(0, 2, 1).copy()
        out[:, l] = B
    return out[0] if single else out


def residual(S, coef, lam):
    """r (L,p,p) longdouble, r[l,k,j] of node j: g_k - lambda sign(beta_k) on the support, max(|g_k| - lambda, 0) off it; 0 at
    k = j.  Also returns g."""
    G = gradient(S, coef)
    lv = np.asarray(lam, dtype=LD)[:, None, None]
    C = np.asarray(coef).astype(LD)
    R = np.where(C != 0, G - lv * np.sign(C), np.maximum(np.abs(G) - lv, 0))
    i = np.arange(C.shape[1])
    R[:, i, i] = 0
    return R, G


def residual_bound(S, coef, tol):
    """(L,p,p): step 1's bound for r[l,k,j]."""
    S = np.asarray(S, dtype=np.float64)
    aS = np.abs(S)
    C = np.abs(np.asarray(coef, dtype=np.float64))
    Z = (C != 0).astype(np.float64)
    nnz = Z.sum(axis=1, keepdims=True)
    W1 = aS / np.diagonal(S)[None, :]
    T1 = W1 @ Z - Z                                                     # W1_kk = 1: the term l = k leaves
    A = aS[None] + aS @ C
    return tol * T1 + C_ROUND * (nnz + 2) * U * A


def resvar_reference(S, coef, G):
    """(tau^2 (L,p) in longdouble at the given coefficients, step 3's bound)."""
    Sl = np.asarray(S).astype(LD)
    C = np.asarray(coef).astype(LD)
    tau = np.diagonal(Sl)[None, :] - (C * (Sl[None] + G)).sum(axis=1)
    S64, C64, G64 = np.abs(np.asarray(S, dtype=np.float64)), np.abs(np.asarray(coef, dtype=np.float64)), np.abs(G.astype(np.float64))
    nnz = (C64 != 0).sum(axis=1)
    A = S64[None] + S64 @ C64
    bound = (C64 * A).sum(axis=1) * (2 * nnz + 1) * U + (nnz + 3) * U * (np.diagonal(S64)[None, :] + (C64 * (S64[None] + G64)).sum(axis=1))
    return tau, bound


@functools.lru_cache(maxsize=None)
def _reference_stack(p, grid):
    lam = np.asarray(grid, dtype=np.float64)
    Bs = solve(stack(p), lam)
    out = []
    for seed in range(3):
        S, B = stack(p)[seed], Bs[seed]
        R, G = residual(S, B, lam)
        assert float(np.abs(R).max()) <= 1e-15, f"the comparison value is not optimal: residual {float(np.abs(R).max()):.3g}"
        off = ~np.eye(p, dtype=bool)[None]
        lv = lam[:, None, None]
        slack = np.where((B == 0) & off, lv - np.abs(G), np.inf).min(axis=1, initial=np.inf)
        small = np.where(B != 0, np.abs(B), np.inf).min(axis=1, initial=np.inf)
        margin = np.minimum(slack, small).astype(np.float64)
        for a in (B, R, margin):
            a.setflags(write=False)
        out.append((B, R, margin, float(np.linalg.eigvalsh(S)[0])))
    return out


def reference(p, seed, grid=GRID):
    """(B (L,p,p) longdouble, r (L,p,p) its residual, margin (L,p), lambda_min(S)) of ``case(p, seed)``, computed once for the
    three seeds together.  The margin of (lambda, node): the smaller of lambda - |g_k| over the zeros and |beta_k| over the
    non-zeros."""
    return _reference_stack(p, tuple(grid))[seed]


def and_or(raw, rule):
    """The symmetrised matrix from raw columns, entry by entry from the definition (the tests' own, not the package's)."""
    raw = np.asarray(raw)
    W = np.zeros_like(raw)
    p = raw.shape[-1]
    for i in range(p):
        for j in range(i + 1, p):
            a, b = raw[..., i, j], raw[..., j, i]                       # beta^(j)_i, beta^(i)_j
            with np.errstate(invalid='ignore'):
                tb = np.abs(b) < np.abs(a) if rule == 'and' else np.abs(b) > np.abs(a)
            W[..., i, j] = W[..., j, i] = np.where(tb, b, a)
    return W


def check_case(p, seed, coef, resvar, status, tol, what=""):
    """Checks 1, 2, 3 and 5 of one matrix: coef (L,p,p) raw columns, resvar (L,p), status (L,p) of the twin or the device on
    ``case(p, seed)`` along GRID.  Returns the largest observed fractions (residual, distance, resvar) of their bounds and the
    boolean (L,p) mask of the (lambda, node) whose supports were compared; asserts everything."""
    S = stack(p)[seed]
    lam = np.asarray(GRID)
    B, Rref, margin, lmin = reference(p, seed)
    assert np.all(status == 0), f"{what}: a node did not converge (status {np.unique(status)})"
    assert np.all(np.isfinite(coef)) and np.all(np.diagonal(coef, axis1=1, axis2=2) == 0)
    R, G = residual(S, coef, lam)
    bound = residual_bound(S, coef, tol)
    off = ~np.eye(p, dtype=bool)[None]
    fr = float((np.abs(R) / bound)[np.broadcast_to(off, R.shape)].max()) if p > 1 else 0.0
    # 2: strong convexity
    dist = np.sqrt(((np.asarray(coef).astype(LD) - B) ** 2).sum(axis=1)).astype(np.float64)
    dbound = (np.sqrt((R * R).sum(axis=1)) + np.sqrt((Rref * Rref).sum(axis=1))).astype(np.float64) / lmin
    fd = float(np.max(np.where(dbound > 0, dist / np.where(dbound > 0, dbound, 1.0), np.where(dist > 0, np.inf, 0.0))))
    # 5: residual variance
    tau, tb = resvar_reference(S, coef, G)
    ft = float(np.max(np.abs(np.asarray(resvar).astype(LD) - tau).astype(np.float64) / tb))
    print(f"{what} p={p} seed={seed}: residual {fr:.3f}, distance {fd:.3f}, resvar {ft:.3f} of their bounds")
    assert fr <= 1.0 and fd <= 1.0 and ft <= 1.0, (fr, fd, ft)
    # 3: supports where the comparison value's margin allows
    ok = margin >= MARGIN
    assert (~ok).sum() <= 0.01 * ok.size, f"{what}: {(~ok).sum()} of {ok.size} (lambda, node) left out"
    same = ((np.asarray(coef) != 0) == (B != 0)).all(axis=1)
    assert np.all(same[ok]), f"{what}: supports differ at (lambda, node) {np.argwhere(~same & ok)[:5]}"
    return (fr, fd, ft), ok


def check_graphs(p, seed, W, rule, ok):
    """The AND / OR graph of a symmetrised stack W (L,p,p) against the comparison value's, on the pairs whose two nodes both
    passed the margin rule."""
    B = reference(p, seed)[0]
    nz = B != 0
    want = (nz & nz.transpose(0, 2, 1)) if rule == 'and' else (nz | nz.transpose(0, 2, 1))
    both = ok[:, :, None] & ok[:, None, :]
    assert np.array_equal((np.asarray(W) != 0) & both, want & both)


def stars_data(seed=11, p=17, N=120):
    """X (p,N) of the StARS checks: the covariance of ``case``, variables in rows."""
    i = np.arange(p)
    return np.linalg.cholesky(0.6 ** np.abs(i[:, None] - i[None, :])) @ np.random.default_rng([seed, p, N]).standard_normal((p, N))


def stars_expected(S_sub, lam, rule, t):
    """What ``stars_search(method='mb')`` must return for the subsample matrices S_sub (B,p,p), assembled from the comparison
    value: (NUM (L,), COUNTS (L,p,p), THETA (L,B,p,p) float64, ok (L,B,p) the margin mask)."""
    from gglasso_amd import model_selection as ms
    lam = np.asarray(lam, dtype=np.float64)
    Bs = solve(S_sub, lam)                                                  # (B,L,p,p)
    ok = np.zeros(Bs.shape[:3], dtype=bool)
    p = S_sub.shape[-1]
    off = ~np.eye(p, dtype=bool)[None]
    for r in range(S_sub.shape[0]):
        R, G = residual(S_sub[r], Bs[r], lam)
        assert float(np.abs(R).max()) <= 1e-15
        slack = np.where((Bs[r] == 0) & off, lam[:, None, None] - np.abs(G), np.inf).min(axis=1, initial=np.inf)
        small = np.where(Bs[r] != 0, np.abs(Bs[r]), np.inf).min(axis=1, initial=np.inf)
        ok[r] = np.minimum(slack, small) >= MARGIN
    THETA = np.ascontiguousarray(np.swapaxes(and_or(Bs, rule), 0, 1)).astype(np.float64)
    COUNTS, NUM = ms._host_edge_counts(THETA, t)
    return NUM, COUNTS, THETA, np.swapaxes(ok, 0, 1)


def check_stars(stats, S_sub, lam, rule, t, beta):
    """Check 10 of one ``stars_search(method='mb', store_all=True)`` result against ``stars_expected``."""
    from gglasso_amd import model_selection as ms
    NUM, COUNTS, THETA, ok = stars_expected(S_sub, lam, rule, t)
    assert ok.mean() >= 0.99, f"{(~ok).sum()} of {ok.size} (lambda, subsample, node) fall under the margin"
    L, B, p, _ = THETA.shape
    both = ok[:, :, :, None] & ok[:, :, None, :]
    assert np.array_equal((stats['THETA'] != 0) & both, (THETA != 0) & both)
    assert np.array_equal(stats['THETA'], np.swapaxes(stats['THETA'], -1, -2))
    if ok.all():
        assert stats['NUM'] == [int(v) for v in NUM] and np.array_equal(stats['COUNTS'], COUNTS)
        D = np.array([2 * int(v) / (B * B * (p * (p - 1) // 2)) for v in NUM])
        assert stats['IX'] == ms.stars_select(D, beta)[0]
    cnt, num = ms._host_edge_counts(stats['THETA'], t)                     # the counts are those of the stack returned
    assert np.array_equal(stats['COUNTS'], cnt) and stats['NUM'] == [int(v) for v in num]
    return bool(ok.all())


def check_residual_where_converged(S, lam, coef, status, tol):
    """Check 1 alone, for the nodes that ended with status 0, on any matrix (a singular one included)."""
    R, _ = residual(S, coef, lam)
    bound = residual_bound(S, coef, tol)
    conv = np.broadcast_to((np.asarray(status) == 0)[:, None, :], R.shape)
    fr = float(np.max(np.where(conv, np.abs(R).astype(np.float64) / bound, 0.0)))
    print(f"residual {fr:.3f} of its bound over {int((np.asarray(status) == 0).sum())} converged (lambda, node)")
    assert fr <= 1.0
