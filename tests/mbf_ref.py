"""Inputs, comparison values and derived error bounds of fused joint neighbourhood selection (csrc/neighborhood_fused.hip,
utils.fused_neighborhood_selection, utils.host_fused_neighborhood_selection), shared by test_cpu_neighborhood_fused.py and
test_gpu_neighborhood_fused.py, after the pattern of mbj_ref.py (whose stacks, gradient and magnitudes are used as they are).

The problem of node j at the pair (l1, l2), on a stack S (K,p,p) in the instances' given order, weights w_k > 0, beta^(k)_j = 0:

    min_B  sum_k w_k [ 1/2 beta^(k)' S^(k) beta^(k) - s_j^(k)' beta^(k) ] + l1 sum_k sum_i |beta^(k)_i|
           + l2 sum_i sum_{k<K} |beta^(k+1)_i - beta^(k)_i|
    g^(k) = w_k (s_j^(k) - S^(k) beta^(k)),   a_i = max_k w_k S^(k)_ii,   P_i(v) = soft(tv(v, l2 / a_i), l1 / a_i)
    B solves it  <=>  for every i != j:  b = P_i(b + g_i / a_i),  b = beta^(.)_i     (fixed point of the metric-a_i prox step)

0. The prox.  ``condat`` is Condat's direct scan (the decisions and the order of condat_inplace) in longdouble, for many
   K-vectors at once: every vector walks its own scan, the trips are taken together.  It is validated WITHOUT a second
   algorithm by the optimality certificate of x = tv(v, lam) (``certificate``): stationarity of 1/2 ||x - v||^2 +
   lam sum_k |x_{k+1} - x_k| reads v_m - x_m = lam (s_{m-1} - s_m) with s_k in the subdifferential of |.| at x_{k+1} - x_k,
   s_0 = s_K = 0.  Summed over m <= k:  t_k = sum_{m<=k} (v_m - x_m) = -lam s_k, hence
       |t_k| <= lam,   t_K = 0,   t_k = -lam sign(x_{k+1} - x_k) where x jumps.
   A difference within 64 eps (max |v| + lam) is the rounding of two equal segment values and no jump.
   (With the partial sums of x - v the last sign is +; it is the sign convention of t only.)  The certificate's largest
   violation is asserted <= 64 eps_longdouble (|v| + lam) K for every prox the comparison value's LAST sweep took, and the scan
   asserts k0 <= kminus, kplus at every close (the invariant behind the device scan's trip cap).

Comparison value (``solve``): the block loop in numpy.longdouble with tol = 0 -- v = b + g_i / a_i, b = P_i(v), g updated --
over ALL variables in ascending order (no active set; a block that is zero and has max_k |g_k| <= l1 stays zero and is
skipped, a prox output lying within the range of its input), all nodes of a stack and all penalty pairs advancing together.
mbj_ref's stopping rules: a sweep changes nothing, the largest change falls to 1e-18 or has not decreased for 5 sweeps, or a
sweep limit.  It is never the twin and never the device; its own residual (1.) is asserted <= 1e-15.

Notation: u = 2^-53; A_ki = w_k (|s^(k)_ji| + sum_m |S^(k)_im| |beta^(k)_m|) bounds g^(k)_i and every partial sum of it
(mbj_ref); Y_ki = A_ki + a_i |beta^(k)_i| bounds a_i |v_k|; Ymax_i = max_k Y_ki; ngrp the number of non-zero groups.

1. The optimality residual (``residual``), formed in longdouble from the returned B alone:
       R_i = a_i (b - P_i(b + g_i / a_i)),   a K-vector per (node, variable);  R = 0 exactly at the solution.
   P_i is a prox, hence nonexpansive in the 2-norm.  The solver's last update of block i computed b = fl P_i(y), y = fl(b_old +
   g^_i / a_i), from its own g^ and the b_old of the sweep before, so
       ||R_i|| <= a_i ||fl P_i(y) - P_i(y)|| + a_i ||y - (b + g_i / a_i)||
              <= || (SCAN_i + SOFT_ki + YR_ki + OWN + T_ki + E_ki)_k ||_2                                    (``residual_bound``)
   OWN = tol: the last sweep moved b_k by at most tol / a_i (the stopping rule a_i max_k |d_k| <= tol): a_i |b_old - b|.
   T_ki = tol sum_{m in a non-zero group, m != i} w_k |S^(k)_im| / a_m: the blocks behind i in that sweep move g^(k)_i by
     w_k S^(k)_im d^(k)_m, |d^(k)_m| <= tol / a_m.  (mbj_ref's first term with the block's one curvature.)
   E_ki = C_ROUND (ngrp + 4) u A_ki, C_ROUND = 4: the rounding of the g the update read -- recomputed in a fixed order and
     updated by the sweep in front of block i -- mbj_ref's derivation, unchanged: (4 ngrp + 1) u A_ki for g, the rest spare.
   YR_ki = 2 u Y_ki: y = fl(b_old + fl(g / a)), two roundings, of |g| / a <= A / a and of |y| <= Y / a; times a.
   SCAN_i = 8 K u (Ymax_i + 2 l2): the scan returns, per segment, the mean of y over the segment -+ lam' / len, built as a
     running sum: a segment of n <= K elements takes n extensions, each with two roundings of the running sum u_min (or
     u_max; |.| <= n (2 M), M = max |y| + 2 lam' bounding every y - v_min) and two of the bound v_min += (u_min - lam') / n,
     which divides the sum's error by n again: 4 roundings of size 2 M u per extension, 8 n u M <= 8 K u M per element, and
     a M <= Ymax + 2 l2.  lam' = fl(l2 / a) has relative error u, moving x by at most lam' u: inside the 2 l2.
   SOFT_ki = 2 u (Y_ki + l1): soft(x, fl(l1 / a)): the threshold's rounding and the subtraction's, |x| <= max |y|.
   A zero block outside the active list: the last screen found the dual of the prox feasible at 0 in floating point, walking
     lo <- fl(fl(lo + g_k) - l1), hi <- fl(fl(hi + g_k) + l1) cut to [-l2, l2]: two roundings per step on values bounded by
     l2 + |g_k| + l1.  The computed interval lies within the exact one of the thresholds l1 + WALK_k, WALK_k = 2 u (l1 + l2 +
     A_ki), so P(g'_i) = 0 for a g' within WALK of the screen's g^, and ||P(g_i / a) a|| <= ||g - g'|| by nonexpansiveness:
     || (WALK + T + E)_k ||.  ``residual_bound`` adds WALK to the sum above for every block rather than telling the two apart.
   None of the constants is fitted; the largest observed fraction of the bound is printed by every check.

2. The distance to the solution.  With D = diag(a_i) and B+ = P(B + D^-1 g(B)) block by block, R = D (B - B+), the prox's
   optimality reads R + g(B) in dh(B+) (h the penalty), so R + g(B) - g(B+) is a subgradient of the objective at B+; g(B) -
   g(B+) = w S (B+ - B) has norm <= Lip ||B - B+||, Lip = max_k w_k lambda_max(S^(k)), and ||B - B+|| <= ||R|| / min_i a_i.
   The smooth part is mu-strongly convex, mu = min_k w_k lambda_min(S^(k)):  ||B+ - B*|| <= (1 + Lip / min a) ||R|| / mu, and
       ||B - B*||_F <= ||R|| / min_i a_i + (1 + Lip / min_i a_i) ||R|| / mu        per node;
   the comparison value's own residual is added in the same way.  Beyond p = 17 the comparison value, and so this check, covers
   the nodes ``nodes_of(p)``; checks 1 and 3 cover every node at every p.

3. The residual variance: mbj_ref's step 3 (``mbj_ref.resvar_reference``), the formula and the g being the same.
"""
import functools

import numpy as np

import mbj_ref

U = 2.0 ** -53
LD = np.longdouble
EPS_LD = float(np.finfo(LD).eps)
C_ROUND = mbj_ref.C_ROUND
MARGIN = 1e-5
PAIRS = ((0.05, 0.2), (0.1, 0.05), (0.0, 0.15), (0.1, 0.0))
KINDS = ('corr', 'weighted')


def stack(p, K, kind):
    """(S (K,p,p), omega or None): mbj_ref's stacks -- 'corr' (equal diagonals, all weights 1: the exact block step) and
    'weighted' (unequal diagonals, weights 0.5, 0.75, ...: the majorised step)."""
    assert kind in KINDS
    return mbj_ref.stack(p, K, kind)


def _soft(z, l):
    return np.sign(z) * np.maximum(np.abs(z) - l, 0)


def _condat_row(y, lam):
    """tv(y, lam) of one longdouble vector (N >= 2): the scan as condat_inplace writes it."""
    N, x = len(y), y.copy()
    k = k0 = kp = km = 0
    vmin, vmax, umin, umax = y[0] - lam, y[0] + lam, lam, -lam
    for _ in range(N * (N + 1) // 2):
        if k == N - 1:
            if umin < 0:
                assert k0 <= km, "a close with k0 beyond the touching point"
                x[k0:km + 1] = vmin
                km += 1
                k = k0 = km
                umin, vmin = lam, y[k]
                umax = vmin + lam - vmax
            elif umax > 0:
                assert k0 <= kp, "a close with k0 beyond the touching point"
                x[k0:kp + 1] = vmax
                kp += 1
                k = k0 = kp
                umax, vmax = -lam, y[k]
                umin = vmax - lam - vmin
            else:
                x[k0:] = vmin + umin / LD(k - k0 + 1)
                return x
            if k == N - 1:
                x[k] = vmin + umin
                return x
        else:
            yn = y[k + 1]
            if yn + umin - vmin < -lam:
                assert k0 <= km, "a close with k0 beyond the touching point"
                x[k0:km + 1] = vmin
                km += 1
                k = kp = k0 = km
                vmin = y[k]
                vmax, umin, umax = vmin + 2 * lam, lam, -lam
            elif yn + umax - vmax > lam:
                assert k0 <= kp, "a close with k0 beyond the touching point"
                x[k0:kp + 1] = vmax
                kp += 1
                k = km = k0 = kp
                vmax = y[k]
                vmin, umin, umax = vmax - 2 * lam, lam, -lam
            else:
                k += 1
                umin, umax = umin + yn - vmin, umax + yn - vmax
                if umin >= lam:
                    vmin, umin, km = vmin + (umin - lam) / LD(k - k0 + 1), lam, k
                if umax <= -lam:
                    vmax, umax, kp = vmax + (umax + lam) / LD(k - k0 + 1), -lam, k
    raise AssertionError("the scan did not end within N (N + 1) / 2 trips")


def condat(V, lam):
    """tv(V[n, :], lam[n]) for every row n, longdouble: Condat's direct scan, each row walking its own decisions -- row by row
    for a few rows, all rows trip by trip (the same decisions and arithmetic, under masks) for many."""
    V = np.asarray(V, dtype=LD)
    n, N = V.shape
    lam = np.broadcast_to(np.asarray(lam, dtype=LD).reshape(-1), (n,)).copy()
    X = V.copy()
    if N == 1 or n == 0:
        return X
    if n <= 64:
        for r in range(n):
            X[r] = _condat_row(V[r], lam[r])
        return X
    rows, col = np.arange(n), np.arange(N)[None, :]
    at = lambda k: V[rows, np.minimum(k, N - 1)]
    k, k0, kp, km = (np.zeros(n, dtype=np.int64) for _ in range(4))
    vmin, vmax, umin, umax = V[:, 0] - lam, V[:, 0] + lam, lam.copy(), -lam
    done = np.zeros(n, dtype=bool)

    def fill(mask, a, b, val):
        r = np.flatnonzero(mask)
        if r.size:
            assert np.all(a[r] <= b[r]), "a close with k0 beyond the touching point"
            X[r] = np.where((col >= a[r, None]) & (col <= b[r, None]), val[r, None], X[r])

    for _ in range(N * (N + 1) // 2):
        if done.all():
            break
        last = (k == N - 1) & ~done
        e_neg, e_pos = last & (umin < 0), last & ~(umin < 0) & (umax > 0)
        e_fin = last & ~e_neg & ~e_pos
        yn = at(k + 1)
        mid = ~last & ~done
        m_neg = mid & (yn + umin - vmin < -lam)
        m_pos = mid & ~m_neg & (yn + umax - vmax > lam)
        m_ext = mid & ~m_neg & ~m_pos
        # closes at the lower bound (end of signal / negative jump) and at the upper bound
        neg, pos = e_neg | m_neg, e_pos | m_pos
        fill(neg, k0, km, vmin)
        fill(pos, k0, kp, vmax)
        fill(e_fin, k0, np.full(n, N - 1), vmin + umin / (k - k0 + 1).astype(LD))
        done |= e_fin
        km = np.where(neg, km + 1, km)
        kp = np.where(pos, kp + 1, kp)
        nk = np.where(neg, km, np.where(pos, kp, k))
        k0 = np.where(neg | pos, nk, k0)
        kp, km = np.where(m_neg, nk, kp), np.where(m_pos, nk, km)
        ynk = at(nk)
        # end of signal
        umax = np.where(e_neg, ynk + lam - vmax, umax)
        umin = np.where(e_pos, ynk - lam - vmin, umin)
        vmin, umin = np.where(e_neg, ynk, vmin), np.where(e_neg, lam, umin)
        vmax, umax = np.where(e_pos, ynk, vmax), np.where(e_pos, -lam, umax)
        one = (e_neg | e_pos) & (nk == N - 1)
        fill(one, nk, nk, vmin + umin)
        done |= one
        # jumps inside the signal
        vmin = np.where(m_neg, ynk, np.where(m_pos, ynk - 2 * lam, vmin))
        vmax = np.where(m_neg, ynk + 2 * lam, np.where(m_pos, ynk, vmax))
        umin, umax = np.where(m_neg | m_pos, lam, umin), np.where(m_neg | m_pos, -lam, umax)
        k = nk
        # extension
        k = np.where(m_ext, k + 1, k)
        umin, umax = np.where(m_ext, umin + yn - vmin, umin), np.where(m_ext, umax + yn - vmax, umax)
        ln = (k - k0 + 1).astype(LD)
        lo, hi = m_ext & (umin >= lam), m_ext & (umax <= -lam)
        vmin, umin, km = np.where(lo, vmin + (umin - lam) / ln, vmin), np.where(lo, lam, umin), np.where(lo, k, km)
        vmax, umax, kp = np.where(hi, vmax + (umax + lam) / ln, vmax), np.where(hi, -lam, umax), np.where(hi, k, kp)
    assert done.all(), "the scan did not end within N (N + 1) / 2 trips"
    return X


def certificate(V, X, lam):
    """The largest violation, per row, of step 0's three conditions for X = tv(V, lam)."""
    V, X = np.asarray(V, dtype=LD), np.asarray(X, dtype=LD)
    lam = np.broadcast_to(np.asarray(lam, dtype=LD).reshape(-1), (V.shape[0],))[:, None]
    t = np.cumsum(V - X, axis=1)
    e = np.maximum(np.abs(t[:, :-1]) - lam, 0).max(axis=1, initial=0)
    e = np.maximum(e, np.abs(t[:, -1]))
    dx = X[:, 1:] - X[:, :-1]
    jump = np.where(np.abs(dx) > 64 * EPS_LD * (np.abs(V).max(axis=1, keepdims=True) + lam), np.sign(dx), 0)
    return np.maximum(e, np.where(jump != 0, np.abs(t[:, :-1] + lam * jump), 0).max(axis=1, initial=0))


def prox(V, a, l1, l2, check=False):
    """P(V[n, :]) = soft(tv(V, l2 / a), l1 / a) per row; a, l1, l2 per row.  ``check``: assert the certificate of the tv."""
    a = np.asarray(a, dtype=LD).reshape(-1)
    lam = np.asarray(l2, dtype=LD).reshape(-1) / a
    X = condat(V, lam)
    if check and len(X):
        c = certificate(V, X, lam)
        lim = 64 * EPS_LD * (np.abs(np.asarray(V, dtype=LD)).max(axis=1) + lam) * V.shape[1]
        assert np.all(c <= lim), f"the scan's output misses its certificate by {float((c / np.where(lim > 0, lim, 1)).max()):.3g} of the limit"
    return _soft(X, (np.asarray(l1, dtype=LD).reshape(-1) / a)[:, None])


def curvature(S, om):
    """a (p,) longdouble: a_i = max_k w_k S^(k)_ii."""
    Sl = np.asarray(S).astype(LD)
    w = np.ones(len(Sl), dtype=LD) if om is None else np.asarray(om).astype(LD)
    return (w[:, None] * np.diagonal(Sl, axis1=1, axis2=2)).max(axis=0)


def nodes_of(p):
    """The nodes the comparison value is computed for: all up to p = 17; the first two and the last two beyond (at p = 63, 64,
    65 they straddle the lane boundary) -- the loop's cost is its sweeps times p Python-level block updates per unit, and the
    residual, which needs no comparison value, is checked for every node."""
    return np.arange(p) if p <= 17 else np.array([0, 1, p - 2, p - 1])


def solve(S, om, pairs, nodes=None, sweep_limit=20000):
    """The comparison value: B (P,K,p,len(nodes)) longdouble for the P pairs (each on its own, from zero), column c = beta of
    node nodes[c] (default: all)."""
    Sl = np.asarray(S).astype(LD)
    K, p, _ = Sl.shape
    nodes = np.arange(p) if nodes is None else np.asarray(nodes)
    q = len(nodes)
    w = np.ones(K, dtype=LD) if om is None else np.asarray(om).astype(LD)
    P = len(pairs)
    l1 = np.repeat(np.array([a for a, _ in pairs], dtype=LD), q)                   # unit (pair, node)
    l2 = np.repeat(np.array([b for _, b in pairs], dtype=LD), q)
    node = np.tile(nodes, P)
    wS = w[:, None, None] * Sl
    am = curvature(S, om)
    B = np.zeros((P * q, K, p), dtype=LD)
    G = np.ascontiguousarray(np.tile(np.swapaxes(wS, 0, 1)[nodes], (P, 1, 1)))     # G[unit,k,:] = w_k S^(k)[j,:]
    best, stall = np.inf, 0

    def sweep(check):
        dmax = 0.0
        for i in range(p):
            bo, gi = B[:, :, i], G[:, :, i]
            live = np.flatnonzero(((np.abs(gi).max(axis=1) > l1) | (bo != 0).any(axis=1)) & (node != i))
            if live.size == 0:
                continue
            a = np.full(live.size, am[i], dtype=LD)
            b = prox(bo[live] + gi[live] / am[i], a, l1[live], l2[live], check)
            d = b - bo[live]
            if d.any():
                G[live] -= d[:, :, None] * wS[None, :, i, :]
                B[live, :, i] = b
                dmax = max(dmax, float(np.abs(d).max()))
        return dmax

    for _ in range(sweep_limit):
        dmax = sweep(False)
        if dmax == 0.0 or dmax <= 1e-18:
            break
        if dmax < best:
            best, stall = dmax, 0
        else:
            stall += 1
            if stall >= 5:
                break
    sweep(True)                                                                  # one more, every prox certified
    return np.ascontiguousarray(B.reshape(P, q, K, p).transpose(0, 2, 3, 1))


def residual(S, om, coef, l1, l2, nodes=None):
    """(R (K,p,q) longdouble with R[:,i,c] = a_i (b - P_i(b + g_i / a_i)) of node nodes[c] (default: all) and variable i, 0 at
    i = node; G).  A zero block with max_k |g_k| <= l1 has R = 0 without a scan: a prox output lies within the range of its
    input."""
    C = np.asarray(coef).astype(LD)
    K, p, q = C.shape
    nodes = np.arange(p) if nodes is None else np.asarray(nodes)
    Sl = np.asarray(S).astype(LD)
    w = np.ones(K, dtype=LD) if om is None else np.asarray(om).astype(LD)
    G = Sl[:, :, nodes].copy()                                                   # through the supports, as mb_ref.gradient_stack
    cols = np.arange(q)
    for k in range(K):
        nz = C[k] != 0
        order = np.argsort(~nz, axis=0, kind='stable')[:int(nz.sum(axis=0).max())]
        for r in order:                                                          # (a row behind a column's support holds a zero)
            G[k] -= Sl[k][:, r] * C[k][r, cols]
    G *= w[:, None, None]
    a = np.repeat(curvature(S, om), q)                                           # row (i, c) -> a_i
    Bv, Gv = C.reshape(K, p * q).T, G.reshape(K, p * q).T
    need = np.flatnonzero((Bv != 0).any(axis=1) | (np.abs(Gv).max(axis=1) > LD(l1)))
    Rv = np.zeros((p * q, K), dtype=LD)
    if need.size:
        Pv = prox(Bv[need] + Gv[need] / a[need, None], a[need], np.full(need.size, LD(l1)), np.full(need.size, LD(l2)))
        Rv[need] = a[need, None] * (Bv[need] - Pv)
    R = np.ascontiguousarray(Rv.T).reshape(K, p, q)
    R[:, nodes, np.arange(q)] = 0
    return R, G


def group_norm(R):
    return np.sqrt((R * R).sum(axis=0))


def residual_bound(S, om, coef, l1, l2, tol):
    """(p,p): step 1's bound for ||R[:,i,j]||_2."""
    S = np.asarray(S, dtype=np.float64)
    K = S.shape[0]
    w = np.ones(K) if om is None else np.asarray(om, dtype=np.float64)
    a = curvature(S, om).astype(np.float64)
    A, ngrp, Z = mbj_ref._magnitudes(S, om, coef)
    Y = A + a[None, :, None] * np.abs(np.asarray(coef, dtype=np.float64))
    W1 = w[:, None, None] * np.abs(S) / a[None, None, :]                          # w_k |S_im| / a_m
    d = np.arange(S.shape[1])
    W1[:, d, d] = 0                                                              # the term m = i is OWN
    T = tol * (W1 @ Z)
    E = C_ROUND * (ngrp[None] + 4) * U * A
    H = tol + T + E + U * (8 * K * (Y.max(axis=0, keepdims=True) + 2 * l2) + 2 * Y + 2 * (Y + l1) + 2 * (l1 + l2 + A))
    return np.sqrt((H ** 2).sum(axis=0))


def constants(S, om):
    """(mu, Lip, min_i a_i) of step 2."""
    w = np.ones(len(S)) if om is None else np.asarray(om, dtype=np.float64)
    ev = [np.linalg.eigvalsh(np.asarray(S[k], dtype=np.float64)) for k in range(len(S))]
    return float(min(w[k] * ev[k][0] for k in range(len(S)))), float(max(w[k] * ev[k][-1] for k in range(len(S)))), \
        float(curvature(S, om).min())


def distance_bound(rn, mu, lip, amin):
    """step 2 per node, from the norms rn (p,p) of the residual's K-vectors."""
    r = np.sqrt((rn * rn).sum(axis=0)).astype(np.float64)
    return r / amin + (1 + lip / amin) * r / mu


@functools.lru_cache(maxsize=None)
def _reference(p, K, kind):
    S, om = stack(p, K, kind)
    nodes = nodes_of(p)
    Bs = solve(S, om, PAIRS, nodes)
    out = []
    for (l1, l2), B in zip(PAIRS, Bs):
        R, _ = residual(S, om, B, l1, l2, nodes)
        rn = group_norm(R)
        assert float(rn.max()) <= 1e-15, f"the comparison value is not optimal: residual {float(rn.max()):.3g} (p={p}, K={K}, {kind})"
        for x in (B, rn):
            x.setflags(write=False)
        out.append((B, rn))
    return out


def reference(p, K, kind, ip):
    """(B (K,p,q) longdouble, the norms (p,q) of its residual) of ``stack(p, K, kind)`` at ``PAIRS[ip]`` for the q nodes
    ``nodes_of(p)``, computed once for the four pairs together and left unchanged."""
    return _reference(p, K, kind)[ip]


def check_case(p, K, kind, ip, coef, resvar, status, tol, what=""):
    """Checks 1, 2, 3 of one stack at one pair: coef (K,p,p) raw columns, resvar (K,p), status (p,) of the twin or the device.
    Returns the largest observed fractions (residual, distance, resvar) of their bounds; asserts everything."""
    S, om = stack(p, K, kind)
    l1, l2 = PAIRS[ip]
    B, rn_ref = reference(p, K, kind, ip)
    assert np.all(np.asarray(status) == 0), f"{what}: a node did not converge (status {np.unique(status)})"
    coef = np.asarray(coef)
    assert coef.shape == (K, p, p) and np.all(np.isfinite(coef)) and np.all(np.diagonal(coef, axis1=1, axis2=2) == 0)
    R, G = residual(S, om, coef, l1, l2)
    rn = group_norm(R)
    fr = float((rn / residual_bound(S, om, coef, l1, l2, tol)).max())
    mu, lip, amin = constants(S, om)
    nodes = nodes_of(p)
    dist = np.sqrt(((coef[:, :, nodes].astype(LD) - B) ** 2).sum(axis=(0, 1))).astype(np.float64)
    dbound = distance_bound(rn[:, nodes], mu, lip, amin) + distance_bound(rn_ref, mu, lip, amin)
    fd = float(np.max(np.where(dbound > 0, dist / np.where(dbound > 0, dbound, 1.0), np.where(dist > 0, np.inf, 0.0))))
    tau, tb = mbj_ref.resvar_reference(S, om, coef, G)                           # (G: all nodes here)
    ft = float(np.max(np.abs(np.asarray(resvar).astype(LD) - tau).astype(np.float64) / tb))
    print(f"{what} p={p} K={K} {kind} pair={PAIRS[ip]}: residual {fr:.3f}, distance {fd:.3f}, resvar {ft:.3f} of their bounds")
    assert fr <= 1.0 and fd <= 1.0 and ft <= 1.0, (fr, fd, ft)
    return fr, fd, ft


def spread_nodes(p, n=32):
    """At most n + 2 nodes of p: evenly spread, so that every slot of 64 and many lane positions occur, and both ends."""
    return np.unique(np.concatenate([np.linspace(0, p - 1, min(n, p)).astype(int), [0, p - 1]]))


def check_residual(S, om, coef, status, l1, l2, tol, what="", nodes=None):
    """Check 1 alone on any stack, over the nodes (default: all) with status 0 (no longdouble solve).  Returns the largest
    fraction."""
    nodes = np.arange(S.shape[1]) if nodes is None else np.asarray(nodes)
    R, _ = residual(S, om, np.asarray(coef)[:, :, nodes], l1, l2, nodes)
    rn = group_norm(R)
    conv = (np.asarray(status)[nodes] == 0)[None, :]
    fr = float(np.max(np.where(conv, (rn / residual_bound(S, om, coef, l1, l2, tol)[:, nodes]).astype(np.float64), 0.0)))
    print(f"{what}: residual {fr:.3f} of its bound over {int(conv.sum())} converged nodes")
    assert fr <= 1.0, fr
    return fr
