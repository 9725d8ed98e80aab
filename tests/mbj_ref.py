"""Inputs, comparison values and derived error bounds of joint neighbourhood selection (csrc/neighborhood_joint.hip,
utils.joint_neighborhood_selection, utils.host_joint_neighborhood_selection), shared by test_cpu_neighborhood_joint.py and
test_gpu_neighborhood_joint.py, after the pattern of mb_ref.py.

The problem of node j at the pair (l1, l2), on a stack S (K,p,p) of bitwise symmetric matrices with positive diagonals and
instance weights w_k > 0, with B = (beta^(1), ..., beta^(K)), beta^(k)_j = 0:

    min_B  sum_k w_k [ 1/2 beta^(k)' S^(k) beta^(k) - s_j^(k)' beta^(k) ] + l1 sum_k sum_i |beta^(k)_i| + l2 sum_i ||beta^(.)_i||_2
    g^(k) = w_k (s_j^(k) - S^(k) beta^(k));  with b = beta^(.)_i, for every i != j:
      b = 0            <=>  ||soft(g^(.)_i, l1)||_2 <= l2
      b != 0, b_k != 0  =>  g^(k)_i = l1 sign(b_k) + l2 b_k / ||b||
      b != 0, b_k = 0   =>  |g^(k)_i| <= l1

Comparison value (``solve``): the block loop of DESIGN 30 in numpy.longdouble with tol = 0 -- a_k = w_k S^(k)_ii,
z = g_i + a b, u = soft(z, l1); b = 0 if ||u|| <= l2, u / a if l2 = 0, else u nu / (a nu + l2) with nu the root of
phi(nu) = sum_k u_k^2 / (a_k nu + l2)^2 - 1 by Newton from nu_0 = (||u|| - l2) / max a -- over ALL variables in ascending
order (no active set), all nodes of a stack and all penalty pairs advancing together.  It ends when a sweep changes
nothing, when the largest change falls to 1e-18 or when it has not decreased for 5 sweeps (in the last bits a longdouble loop
can cycle for ever), or at a sweep limit.  It is never the twin and never the device, and its own optimality residual is
asserted <= 1e-15 before anything is compared with it.

Notation: u = 2^-53; for node j, instance k, variable i:  A_ki = w_k (|s^(k)_ji| + sum_m |S^(k)_im| |beta^(k)_m|), which bounds
g^(k)_i and every partial sum of it; ngrp the number of groups of the returned B with a non-zero member.

1. The optimality residual (``residual``): the vector r^(.)_i with g - r in the subdifferential of the penalty at b,
       b = 0:   r = soft(g, l1) max(1 - l2 / ||soft(g, l1)||, 0)     (g - r = l1 s + l2 t, |s_k| <= 1, ||t|| <= 1)
       b != 0:  r_k = g_k - l1 sign(b_k) - l2 b_k / ||b|| where b_k != 0,  soft(g_k, l1) where b_k = 0,
   with g formed from the returned B in longdouble: independent of any solver.  Its norm over the instances is compared with
       ||r^(.)_i||_2 <= || (T_ki + E_ki)_k ||_2 + ROOT                                                      (``residual_bound``)
   T_ki = tol sum_{m in a non-zero group, m != i} |S^(k)_im| / S^(k)_mm.  The solver ends in a state where the last sweep changed
     every beta^(k)_m by at most tol / (w_k S^(k)_mm).  Block i's own update leaves the three conditions true up to rounding;
     the blocks m behind it in that sweep move g^(k)_i by w_k S^(k)_im d^(k)_m.  (mb_ref's first term, per instance.)
   E_ki = C_ROUND (ngrp + 4) u A_ki, C_ROUND = 4.  The g the last sweep starts from is recomputed in a fixed order,
     g = w s - sum_m (w beta_m) S_m over at most ngrp groups: three roundings per term (w beta_m, the product, the subtraction;
     two with a fused multiply-add) on partial sums bounded by A: 3 ngrp u A.  The updates of the sweep in front of block i:
     at most ngrp more subtractions on a value bounded by A (their products are of size tol and their rounding of second
     order): ngrp u A.  The initial w s: u A.  So the g_k block i reads is within (4 ngrp + 1) u A of the true one.  The update:
     a = fl(w S_ii), a b, z = g + a b: u A + u A + 2 u A (|z| <= 2 A); u = soft(z, l1): 2 u A; the stored
     b_k = fl(u_k nu / fl(fl(a_k nu) + l2)) has four roundings and a_k |b_k| <= |u_k| <= 2 A: 8 u A.  Sum: (4 ngrp + 15) u A
     <= 4 (ngrp + 4) u A.  For a zero group the final screen saw soft(g^, l1) with the same error, and soft is 1-Lipschitz.
   ROOT = l2 (K + 28) u / 2: the termination of the root and the norm.  With b_k = u_k nu / (a_k nu + l2) EXACTLY,
     u_k - a_k b_k = l2 b_k / nu and ||b|| = nu sqrt(1 + phi(nu)), so the condition is missed by the vector
     l2 b (1 / nu - 1 / ||b||), of norm l2 |1 - 1 / sqrt(1 + phi)| ~ l2 |phi(nu)| / 2.  phi + 1 = sum_k (u_k t_k)^2 is computed
     with t_k = 1 / (a_k nu + l2) (3 roundings), u_k t_k (1), the square (1): 9 u per term, and K - 1 additions: within
     (K + 9) u of the true value near the root.  Newton's iteration moves up from nu_0 where phi >= 0 (phi is convex and
     decreasing) and ends when a step no longer increases nu: computed phi <= |phi'| nu u <= 2 u (|phi'| nu <= 2 (1 + phi)); a step
     computed from a phi that is (K + 9) u too large overshoots to phi >= -(K + 9) u.  So |phi(nu)| <= (K + 12) u.  The four
     roundings of the stored b change b / ||b|| by at most 8 u: l2 8 u.  The zero test compares a computed ||u|| (relative
     error (K + 3) u / 2) with l2: a group set to zero wrongly misses by at most l2 (K + 3) u / 2, covered.
   None of the constants is fitted; the largest observed fraction of the bound is printed by every check.

2. The distance to the solution: the smooth part is mu-strongly convex with mu = min_k w_k lambda_min(S^(k)) and r is a
   subgradient of the objective at the returned B, so ||B - B*||_F <= ||r||_2 / mu per node; the comparison value's own
   residual is added in the same way.

3. The residual variance tau^2_k = S^(k)_jj - sum_i beta^(k)_i (s^(k)_ji + g^(k)_i / w_k) over the non-zero groups, against its
   longdouble value at the returned B (``resvar_reference``), mb_ref's bound with the g above and one more rounding for
   the division:  |d tau^2| <= sum_i |beta_i| (4 ngrp + 2) u A_ki / w_k + (ngrp + 3) u (S_jj + sum_i |beta_i| (|s_ji| + |g_i| / w_k)).
"""
import functools

import numpy as np

import mb_ref

U = 2.0 ** -53
LD = np.longdouble
C_ROUND = 4
MARGIN = 1e-5
PAIRS = ((0.05, 0.2), (0.1, 0.05), (0.0, 0.15), (0.1, 0.0))
KINDS = ('corr', 'scaled', 'weighted')


@functools.lru_cache(maxsize=None)
def stack(p, K, kind):
    """(S (K,p,p), omega (K,) or None), read-only.  'corr': the correlation matrices mb_ref.case(p, seed), seeds 0..K-1 (equal
    a_k: the closed-form root).  'scaled': the same rescaled per (instance, variable) by factors in [1, 1.5] from a seeded
    generator, built bitwise symmetric -- the upper triangle mirrored (unequal a_k: the Newton root).  'weighted': the scaled
    stack with the instance weights 0.5, 0.75, 1, ..."""
    assert kind in KINDS
    S = np.stack([mb_ref.case(p, seed) for seed in range(K)])
    om = None
    if kind != 'corr':
        c = np.random.default_rng([77, p, K]).uniform(1.0, 1.5, size=(K, p))
        up = np.triu(S * c[:, :, None] * c[:, None, :])
        S = up + np.swapaxes(np.triu(up, 1), 1, 2)
    if kind == 'weighted':
        om = 0.5 + 0.25 * np.arange(K)
        om.setflags(write=False)
    assert np.array_equal(S, np.swapaxes(S, 1, 2))
    S.setflags(write=False)
    return S, om


def _soft(z, l):
    return np.sign(z) * np.maximum(np.abs(z) - l, 0)


def solve(S, om, pairs, sweep_limit=20000):
    """The comparison value: B (P,K,p,p) longdouble for the P pairs (each on its own, from zero), column j = beta of node j."""
    with np.errstate(all='ignore'):                                         # (rows a where() masks out divide by zero)
        return _solve(S, om, pairs, sweep_limit)


def _solve(S, om, pairs, sweep_limit):
    Sl = np.asarray(S).astype(LD)
    K, p, _ = Sl.shape
    w = np.ones(K, dtype=LD) if om is None else np.asarray(om).astype(LD)
    P = len(pairs)
    l1 = np.repeat(np.array([a for a, _ in pairs], dtype=LD), p)[:, None]          # unit (pair, node) -> (n,1)
    l2 = np.repeat(np.array([b for _, b in pairs], dtype=LD), p)
    node = np.tile(np.arange(p), P)
    n = P * p
    wS = w[:, None, None] * Sl                                                   # (K,p,p): w_k S^(k)
    B = np.zeros((n, K, p), dtype=LD)
    G = np.ascontiguousarray(np.tile(np.swapaxes(wS, 0, 1), (P, 1, 1)))          # G[unit,k,:] = w_k S^(k)[j,:]
    best, stall = np.inf, 0
    for _ in range(sweep_limit):
        dmax = 0.0
        for i in range(p):
            a = wS[:, i, i]                                                      # (K,)
            bo = B[:, :, i]
            z = G[:, :, i] + a * bo
            u = _soft(z, l1)
            un = np.sqrt((u * u).sum(axis=1))
            live = np.flatnonzero(((un > l2) | (bo != 0).any(axis=1)) & (node != i))
            if live.size == 0:
                continue
            ul, l2l = u[live], l2[live][:, None]
            pos = (un[live] > l2[live])[:, None]
            nu = ((un[live] - l2[live]) / a.max())[:, None]
            go = (l2l > 0) & pos
            if go.any():
                for _it in range(200):
                    t = 1 / (a * nu + l2l)
                    ut = ul * t
                    f = (ut * ut).sum(axis=1, keepdims=True) - 1
                    fp = -2 * (ut * ut * a * t).sum(axis=1, keepdims=True)
                    nn = np.where(go, nu - f / np.where(fp != 0, fp, 1), nu)
                    up = nn > nu
                    if not up.any():
                        break
                    nu = np.where(up, nn, nu)
            b = np.where(pos, np.where(l2l > 0, ul * nu / (a * nu + l2l), ul / a), 0)
            d = b - bo[live]
            if d.any():
                G[live] -= d[:, :, None] * wS[None, :, i, :]
                B[live, :, i] = b
                dmax = max(dmax, float(np.abs(d).max()))
        if dmax == 0.0 or dmax <= 1e-18:
            break
        if dmax < best:
            best, stall = dmax, 0
        else:
            stall += 1
            if stall >= 5:
                break
    return np.ascontiguousarray(B.reshape(P, p, K, p).transpose(0, 2, 3, 1))


def gradient(S, om, coef):
    """G (K,p,p) longdouble, G[k,:,j] = w_k (s^(k)_j - S^(k) coef[k,:,j]), through the supports."""
    Sl = np.asarray(S).astype(LD)
    G = mb_ref.gradient_stack(Sl, np.asarray(coef).astype(LD))
    return G if om is None else G * np.asarray(om).astype(LD)[:, None, None]


def residual(S, om, coef, l1, l2):
    """(r (K,p,p) longdouble with r[:,i,j] the vector of step 1 for node j and variable i, 0 at i = j; G)."""
    C = np.asarray(coef).astype(LD)
    G = gradient(S, om, C)
    l1, l2 = LD(l1), LD(l2)
    sg = _soft(G, l1)
    ns = np.sqrt((sg * sg).sum(axis=0))
    nb = np.sqrt((C * C).sum(axis=0))
    zero = sg * np.maximum(1 - l2 / np.where(ns > 0, ns, 1), 0)
    act = np.where(C != 0, G - l1 * np.sign(C) - l2 * C / np.where(nb > 0, nb, 1), sg)
    R = np.where(nb > 0, act, zero)
    i = np.arange(C.shape[1])
    R[:, i, i] = 0
    return R, G


def group_norm(R):
    return np.sqrt((R * R).sum(axis=0))


def _magnitudes(S, om, coef):
    """(A (K,p,p) with A[k,i,j] = A_ki of node j, ngrp (1,p) per node, Z (p,p) the non-zero groups) in float64."""
    S = np.asarray(S, dtype=np.float64)
    w = np.ones(S.shape[0]) if om is None else np.asarray(om, dtype=np.float64)
    aS, C = np.abs(S), np.abs(np.asarray(coef, dtype=np.float64))
    A = w[:, None, None] * (aS + aS @ C)
    Z = (C != 0).any(axis=0).astype(np.float64)
    return A, Z.sum(axis=0, keepdims=True), Z


def residual_bound(S, om, coef, l2, tol):
    """(p,p): step 1's bound for ||r[:,i,j]||_2."""
    S = np.asarray(S, dtype=np.float64)
    K = S.shape[0]
    A, ngrp, Z = _magnitudes(S, om, coef)
    W1 = np.abs(S) / np.diagonal(S, axis1=1, axis2=2)[:, None, :]               # |S_im| / S_mm
    T = tol * (W1 @ Z - Z[None])                                                # W1_ii = 1: the term m = i leaves
    E = C_ROUND * (ngrp[None] + 4) * U * A
    return np.sqrt(((T + E) ** 2).sum(axis=0)) + float(l2) * (K + 28) * U / 2


def resvar_reference(S, om, coef, G):
    """(tau^2 (K,p) in longdouble at the given coefficients, step 3's bound)."""
    Sl = np.asarray(S).astype(LD)
    K = Sl.shape[0]
    w = np.ones(K) if om is None else np.asarray(om, dtype=np.float64)
    wl = w.astype(LD)[:, None, None]
    C = np.asarray(coef).astype(LD)
    tau = np.diagonal(Sl, axis1=1, axis2=2) - (C * (Sl + G / wl)).sum(axis=1)
    S64, C64 = np.abs(np.asarray(S, dtype=np.float64)), np.abs(np.asarray(coef, dtype=np.float64))
    G64 = np.abs((G / wl).astype(np.float64))
    A, ngrp, _ = _magnitudes(S, om, coef)
    bound = (C64 * A / w[:, None, None]).sum(axis=1) * (4 * ngrp + 2) * U + \
        (ngrp + 3) * U * (np.diagonal(S64, axis1=1, axis2=2) + (C64 * (S64 + G64)).sum(axis=1))
    return tau, bound


def strong_convexity(S, om):
    w = np.ones(len(S)) if om is None else np.asarray(om, dtype=np.float64)
    return float(min(w[k] * np.linalg.eigvalsh(S[k])[0] for k in range(len(S))))


@functools.lru_cache(maxsize=None)
def _reference(p, K, kind):
    S, om = stack(p, K, kind)
    Bs = solve(S, om, PAIRS)
    mu = strong_convexity(S, om)
    off = ~np.eye(p, dtype=bool)
    out = []
    for (l1, l2), B in zip(PAIRS, Bs):
        R, G = residual(S, om, B, l1, l2)
        rn = group_norm(R)
        assert float(rn.max()) <= 1e-15, f"the comparison value is not optimal: residual {float(rn.max()):.3g} (p={p}, K={K}, {kind})"
        sg = _soft(G, LD(l1))
        nb = group_norm(B)
        zero_slack = np.where((nb == 0) & off, LD(l2) - group_norm(sg), np.inf).min(axis=0, initial=np.inf)
        member_slack = np.where((B == 0) & (nb > 0)[None], LD(l1) - np.abs(G), np.inf).min(axis=(0, 1), initial=np.inf)
        small = np.where(B != 0, np.abs(B), np.inf).min(axis=(0, 1), initial=np.inf)
        margin = np.minimum(np.minimum(zero_slack, member_slack), small).astype(np.float64)
        for a in (B, rn, margin):
            a.setflags(write=False)
        out.append((B, rn, margin, mu))
    return out


def reference(p, K, kind, ip):
    """(B (K,p,p) longdouble, the group norms (p,p) of its residual, margin (p,) per node, mu) of ``stack(p, K, kind)`` at
    ``PAIRS[ip]``, computed once for the four pairs together.  The margin of a node: the smallest of l2 - ||soft(g_i, l1)|| over
    the zero groups, l1 - |g_k| over the zero members of non-zero groups and |beta_k| over the non-zeros."""
    return _reference(p, K, kind)[ip]


def check_case(p, K, kind, ip, coef, resvar, status, tol, what=""):
    """Checks 1, 2, 3 and the supports of one stack at one pair: coef (K,p,p) raw columns, resvar (K,p), status (p,) of the twin
    or the device.  Returns the largest observed fractions (residual, distance, resvar) of their bounds; asserts everything."""
    S, om = stack(p, K, kind)
    l1, l2 = PAIRS[ip]
    B, rn_ref, margin, mu = reference(p, K, kind, ip)
    assert np.all(np.asarray(status) == 0), f"{what}: a node did not converge (status {np.unique(status)})"
    coef = np.asarray(coef)
    assert coef.shape == (K, p, p) and np.all(np.isfinite(coef)) and np.all(np.diagonal(coef, axis1=1, axis2=2) == 0)
    R, G = residual(S, om, coef, l1, l2)
    rn = group_norm(R)
    bound = residual_bound(S, om, coef, l2, tol)
    fr = float((rn / bound).max())
    dist = np.sqrt(((coef.astype(LD) - B) ** 2).sum(axis=(0, 1))).astype(np.float64)
    dbound = (np.sqrt((rn * rn).sum(axis=0)) + np.sqrt((rn_ref * rn_ref).sum(axis=0))).astype(np.float64) / mu
    fd = float(np.max(np.where(dbound > 0, dist / np.where(dbound > 0, dbound, 1.0), np.where(dist > 0, np.inf, 0.0))))
    tau, tb = resvar_reference(S, om, coef, G)
    ft = float(np.max(np.abs(np.asarray(resvar).astype(LD) - tau).astype(np.float64) / tb))
    print(f"{what} p={p} K={K} {kind} pair={PAIRS[ip]}: residual {fr:.3f}, distance {fd:.3f}, resvar {ft:.3f} of their bounds")
    assert fr <= 1.0 and fd <= 1.0 and ft <= 1.0, (fr, fd, ft)
    ok = margin >= MARGIN
    same = ((coef != 0) == (B != 0)).all(axis=(0, 1))
    assert np.all(same[ok]), f"{what}: supports differ at nodes {np.flatnonzero(~same & ok)[:5]}"
    return (fr, fd, ft), ok


def check_residual(S, om, coef, status, l1, l2, tol, what=""):
    """Check 1 alone on any stack, over the nodes with status 0 (no longdouble solve).  Returns (the largest fraction of the
    bound, the longdouble gradient)."""
    R, G = residual(S, om, coef, l1, l2)
    rn = group_norm(R)
    bound = residual_bound(S, om, coef, l2, tol)
    conv = (np.asarray(status) == 0)[None, :]
    fr = float(np.max(np.where(conv, (rn / bound).astype(np.float64), 0.0)))
    print(f"{what}: residual {fr:.3f} of its bound over {int(conv.sum())} converged nodes")
    assert fr <= 1.0, fr
    return fr, G
