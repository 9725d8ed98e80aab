"""Inputs, comparison values and derived error bounds of neighbourhood selection with penalty weights and of the scaled lasso
(the WEIGHTED / SCALED instantiations of csrc/neighborhood.hip, the ``weights`` / ``scaled`` arguments of utils.neighborhood_selection and of its twin),
shared by test_cpu_mb_weighted.py and test_gpu_mb_weighted.py.  Inputs, ``gradient``, ``residual_bound``, ``resvar_reference``
and ``and_or`` come from mb_ref.py, whose notation is used: u = 2^-53, g = s_j - S beta.

Node j of S with the weights w_k = Wt[j,k] in [0, +inf] and the penalty lambda0:

    plain:   min 1/2 beta' S beta - s_j' beta + lambda0 sum_k w_k |beta_k|        thr_k = lambda0 w_k
    scaled:  min sqrt(tau^2(beta)) + lambda0 sum_k w_k |beta_k|                    thr_k = lambda0 sigma w_k
             tau^2(beta) = S_jj - 2 s_j' beta + beta' S beta,  sigma = sqrt(tau^2(beta))
    optimal (sigma > 0)  <=>  g_k = thr_k sign(beta_k) where beta_k != 0,  |g_k| <= thr_k where beta_k = 0

Comparison value (``solve_w``): mb_ref.solve's longdouble loop with a threshold per (node, k); in scaled mode the alternation
lasso at lambda0 sigma_t w -> sigma = sqrt(tau^2) around it, until sigma moves by at most 1e-18 relative.  Never the twin,
never the device; its own residual is asserted <= 1e-15 before use.

1. Residual r_k = g_k - thr_k sign(beta_k) on the support, max(|g_k| - thr_k, 0) off it, with g, tau^2 and sigma formed in
   longdouble from the RETURNED beta.  A coordinate with w_k = inf has r_k = 0 and must hold beta_k = 0 exactly.
   plain:   |r_k| <= mb_ref.residual_bound + 2 u thr_k.  mb_ref's derivation holds with thr_k in place of lambda; what is new
            is the threshold itself: fl(lambda0 w_k), and in scaled mode fl(fl(lambda0 sigma_t) w_k), one and two roundings.
   scaled:  in addition  lambda0 w_k (sig_tol sigma^ + tb / (2 sigma^) + 4 u sigma^),  sigma^ = sqrt(RESVAR) as returned, tb
            the bound of mb_ref.resvar_reference.  The returned state is lasso-optimal at sigma_t, the residual is measured at
            sigma(beta): |sigma(beta) - sigma_t| <= |sigma^ - sigma_t| + |sigma(beta) - sigma^|.  The first part is at most
            sig_tol sigma^ by the stopping test, which compared these very numbers.  The second: RESVAR is within tb of
            tau^2(beta), and |sqrt(a) - sqrt(b)| = |a - b| / (sqrt(a) + sqrt(b)) ~ tb / (2 sigma^); the rounding of the
            square root, of the difference and of the two products of the threshold are the 4 u sigma^.
2. Distance, plain mode only: weights leave the strong convexity alone, ||beta - beta*||_2 <= (||r|| + ||r*||) / lambda_min(S).
3. RESVAR against mb_ref.resvar_reference at the returned beta, with its bound, in both modes.
4. Supports and AND / OR graphs against the comparison value where its margin (the smaller of thr_k - |g_k| over the zeros and
   |beta_k| over the non-zeros) is >= 1e-5; at most 1 % of the (lambda, node) of a seed may be left out.
"""
import functools

import numpy as np

import mb_ref
from mb_ref import GRID, LD, MARGIN, U, and_or, gradient, gradient_stack, residual_bound, resvar_reference, stack

SIG_TOL = 1e-7
TOL = 1e-7
SCALED_REF_MAX_P = 65           # the scaled comparison value costs 20 s at p = 130, 91 s at 257: beyond 65 the residual alone


def weights(p, seed):
    """Wt (p,p) of ``mb_ref.case(p, seed)``: row j holds node j's weights, uniform on [0.5, 2]."""
    return np.random.default_rng([77, seed, p]).uniform(0.5, 2.0, (p, p))


@functools.lru_cache(maxsize=None)
def weight_stack(p):
    W = np.stack([weights(p, seed) for seed in range(3)])
    W.setflags(write=False)
    return W


def _tau2_nodes(Sl, Bn, Gn, mi, ji):
    """tau^2 (n,) of node-major beta and gradient."""
    return Sl[mi, ji, ji] - (Bn * (Sl[mi, :, ji] + Gn)).sum(axis=1)


def solve_w(S, lam, Wt, scaled=False, sweep_limit=2000, round_limit=100, polish_at=1e-4, sweeps_after=4, outer_limit=400,
            sig_stop=1e-18):
    """The comparison value: (B ([M,]L,p,p) longdouble, column j = beta^(j); sigma ([M,]L,p) longdouble, sqrt(tau^2(beta)))
    along the descending grid with warm starts.  ``mb_ref.solve`` with the threshold lambda0 [sigma_n] Wt[m][j,k] of node
    n = (m, j) and coordinate k; ``scaled``: the alternation on sigma around it, to ``sig_stop`` relative."""
    S = np.asarray(S)
    single = S.ndim == 2
    Sl = (S[None] if single else S).astype(LD)
    M, p, _ = Sl.shape
    n = M * p
    Wt = np.asarray(Wt, dtype=np.float64)
    Wn = np.broadcast_to(Wt if Wt.ndim == 3 else Wt[None], (M, p, p)).reshape(n, p).astype(LD)
    mi, ji = np.repeat(np.arange(M), p), np.tile(np.arange(p), M)      # node -> (matrix, variable)
    dg = np.diagonal(Sl, axis1=1, axis2=2)
    member = np.zeros((n, p), dtype=bool)                               # [node, k]
    rows = np.arange(n)[:, None]

    def grad(Bn):
        G = gradient_stack(Sl, np.ascontiguousarray(Bn.reshape(M, p, p).transpose(0, 2, 1)))
        return G.transpose(0, 2, 1).reshape(n, p)

    def stage(Bn, TH):
        for rnd in range(round_limit):
            Gn = grad(Bn)
            viol = (np.abs(Gn) > TH) & ~member
            viol[rows[:, 0], ji] = False
            if rnd > 0 and not viol.any():
                break
            member[:] |= viol
            amax = int(member.sum(axis=1).max())
            if amax == 0:
                break
            order = np.argsort(~member, axis=1, kind='stable')[:, :amax]         # (node, position): ascending active set
            valid = member[rows, order]
            Bt, Gr, Sd = Bn[rows, order], Gn[rows, order], dg[mi[:, None], order]
            THo = np.where(valid, TH[rows, order], 0)
            SA = Sl[mi[:, None, None], order[:, :, None], order[:, None, :]]     # (node, position, position)
            sA = Sl[mi[:, None], order, ji[:, None]]
            polished, left = False, sweep_limit
            while left > 0:
                left -= 1
                dmax = 0.0
                for i in range(amax):
                    z = Gr[:, i] + Sd[:, i] * Bt[:, i]
                    b = np.where(valid[:, i], np.sign(z) * np.maximum(np.abs(z) - THo[:, i], 0) / Sd[:, i], 0)
                    d = b - Bt[:, i]
                    if d.any():
                        Gr -= d[:, None] * SA[:, i, :]
                        Bt[:, i] = b
                        dmax = max(dmax, float(np.abs(d).max()))
                if dmax == 0.0:
                    break
                if not polished and dmax <= polish_at:
                    polished, left = True, sweeps_after
                    Bt = mb_ref._polish(SA, sA - THo * np.sign(Bt), Bt != 0)
                    Gr = sA - np.einsum('nab,nb->na', SA, Bt)
            Bn = Bn.copy()
            Bn[rows, order] = Bt
        return Bn

    Bn = np.zeros((n, p), dtype=LD)
    out = np.zeros((M, len(lam), p, p), dtype=LD)
    sig_out = np.zeros((M, len(lam), p), dtype=LD)
    for l, lv in enumerate(lam):
        lv = LD(lv)
        if not scaled:
            Bn = stage(Bn, lv * Wn)
            sig = np.sqrt(_tau2_nodes(Sl, Bn, grad(Bn), mi, ji))
        else:
            sig = np.sqrt(_tau2_nodes(Sl, Bn, grad(Bn), mi, ji))
            for it in range(outer_limit):
                Bn = stage(Bn, (lv * sig)[:, None] * Wn)
                sn = np.sqrt(_tau2_nodes(Sl, Bn, grad(Bn), mi, ji))
                done = float(np.max(np.abs(sn - sig) / sn)) <= sig_stop
                sig = sn
                if done:
                    break
        out[:, l] = Bn.reshape(M, p, p).transpose(0, 2, 1)
        sig_out[:, l] = sig.reshape(M, p)
    return (out[0], sig_out[0]) if single else (out, sig_out)


def thresholds(S, coef, lam, Wt, scaled):
    """(thr (L,p,p) longdouble with thr[l,k,j] = lambda_l [sigma_lj] Wt[j,k], G, tau^2 (L,p), sigma (L,p)) at the given
    coefficients, everything in longdouble; sigma is 1 in plain mode."""
    G = gradient(S, coef)
    C = np.asarray(coef).astype(LD)
    Sl = np.asarray(S).astype(LD)
    tau = np.diagonal(Sl)[None, :] - (C * (Sl[None] + G)).sum(axis=1)
    sigma = np.sqrt(tau) if scaled else np.ones_like(tau)
    lv = np.asarray(lam, dtype=LD)[:, None, None]
    thr = lv * sigma[:, None, :] * np.asarray(Wt).astype(LD).T[None]
    return thr, G, tau, sigma


def residual_w(S, coef, lam, Wt, scaled):
    """(r (L,p,p) longdouble, r[l,k,j] of node j, 0 at k = j and where the weight is inf; thr; G; sigma (L,p))."""
    thr, G, tau, sigma = thresholds(S, coef, lam, Wt, scaled)
    C = np.asarray(coef).astype(LD)
    with np.errstate(invalid='ignore'):
        R = np.where(C != 0, G - thr * np.sign(C), np.maximum(np.abs(G) - thr, 0))
    R = np.where(np.isinf(thr), 0, R)
    i = np.arange(C.shape[1])
    R[:, i, i] = 0
    return R, thr, G, sigma


def residual_bound_w(S, coef, lam, Wt, scaled, tol, sig_tol, resvar):
    """(L,p,p): check 1's bound for r[l,k,j] (module docstring)."""
    thr, G, _, _ = thresholds(S, coef, lam, Wt, scaled)
    bound = residual_bound(S, coef, tol) + 2 * U * thr.astype(np.float64)
    if scaled:
        sh = np.sqrt(np.asarray(resvar, dtype=np.float64))                              # (L,p): sigma^ as returned
        tb = resvar_reference(S, coef, G)[1]
        lw = np.asarray(lam, dtype=np.float64)[:, None, None] * np.asarray(Wt, dtype=np.float64).T[None]
        bound = bound + lw * (sig_tol * sh + tb / (2 * sh) + 4 * U * sh)[:, None, :]
    return bound


def check_residual(S, lam, Wt, scaled, coef, resvar, tol=TOL, sig_tol=SIG_TOL, nodes=None, what=""):
    """Check 1 of one matrix, for the nodes in the boolean (L,p) mask ``nodes`` (default: all).  Returns the largest fraction."""
    p = S.shape[-1]
    coef = np.asarray(coef)
    R, thr, G, _ = residual_w(S, coef, lam, Wt, scaled)
    assert np.all(coef[np.isinf(thr) & ~np.eye(p, dtype=bool)[None]] == 0), f"{what}: a coordinate of infinite weight is not zero"
    with np.errstate(invalid='ignore'):
        bound = residual_bound_w(S, coef, lam, Wt, scaled, tol, sig_tol, resvar)
        frac = np.abs(R).astype(np.float64) / bound
    keep = np.broadcast_to(~np.eye(p, dtype=bool)[None], R.shape).copy()
    if nodes is not None:
        keep &= np.asarray(nodes)[:, None, :]
    fr = float(frac[keep].max()) if keep.any() else 0.0
    print(f"{what} {'scaled' if scaled else 'plain'} p={p}: residual {fr:.4f} of its bound")
    assert fr <= 1.0, fr
    return fr


def check_resvar(S, coef, resvar, what=""):
    """Check 3 of one matrix."""
    tau, tb = resvar_reference(S, coef, gradient(S, coef))
    ft = float(np.max(np.abs(np.asarray(resvar).astype(LD) - tau).astype(np.float64) / tb))
    print(f"{what} p={S.shape[-1]}: resvar {ft:.3f} of its bound")
    assert ft <= 1.0, ft
    return ft


@functools.lru_cache(maxsize=None)
def _reference_stack(p, grid, scaled):
    lam = np.asarray(grid, dtype=np.float64)
    Bs, Sg = solve_w(stack(p), lam, weight_stack(p), scaled)
    out = []
    for seed in range(3):
        S, B, Wt = stack(p)[seed], Bs[seed], weight_stack(p)[seed]
        R, thr, G, sigma = residual_w(S, B, lam, Wt, scaled)
        worst = float(np.abs(R).max())
        assert worst <= 1e-15, f"the comparison value is not optimal: residual {worst:.3g}"
        off = ~np.eye(p, dtype=bool)[None]
        slack = np.where((B == 0) & off, thr - np.abs(G), np.inf).min(axis=1, initial=np.inf)
        small = np.where(B != 0, np.abs(B), np.inf).min(axis=1, initial=np.inf)
        margin = np.minimum(slack, small).astype(np.float64)
        for a in (B, R, margin, sigma):
            a.setflags(write=False)
        out.append((B, R, margin, float(np.linalg.eigvalsh(S)[0]), sigma))
    return out


def reference(p, seed, scaled, grid=GRID):
    """(B (L,p,p) longdouble, r its residual, margin (L,p), lambda_min(S), sigma (L,p)) of ``mb_ref.case(p, seed)`` with
    ``weights(p, seed)``, computed once for the three seeds together."""
    return _reference_stack(p, tuple(grid), bool(scaled))[seed]


def check_case(p, seed, scaled, coef, resvar, status, what=""):
    """Checks 1, 2 (plain), 3 and, where the comparison value is affordable, 4 of one matrix: coef (L,p,p) raw columns, resvar
    and status (L,p) of the twin or the device on ``mb_ref.case(p, seed)`` with ``weights(p, seed)`` along GRID at tol =
    sig_tol = 1e-7.  Returns the (L,p) mask of the (lambda, node) whose supports were compared, or None."""
    S, Wt, lam = stack(p)[seed], weight_stack(p)[seed], np.asarray(GRID)
    coef = np.asarray(coef)
    assert np.all(status == 0), f"{what}: a node did not finish (status {np.unique(status)})"
    assert np.all(np.isfinite(coef)) and np.all(np.diagonal(coef, axis1=1, axis2=2) == 0) and np.all(np.isfinite(resvar))
    check_residual(S, lam, Wt, scaled, coef, resvar, what=f"{what} seed={seed}")
    check_resvar(S, coef, resvar, what=f"{what} seed={seed}")
    if scaled and p > SCALED_REF_MAX_P:
        return None
    B, Rref, margin, lmin, sigma = reference(p, seed, scaled)
    if not scaled:
        R = residual_w(S, coef, lam, Wt, False)[0]
        dist = np.sqrt(((coef.astype(LD) - B) ** 2).sum(axis=1)).astype(np.float64)
        dbound = (np.sqrt((R * R).sum(axis=1)) + np.sqrt((Rref * Rref).sum(axis=1))).astype(np.float64) / lmin
        fd = float(np.max(np.where(dbound > 0, dist / np.where(dbound > 0, dbound, 1.0), np.where(dist > 0, np.inf, 0.0))))
        print(f"{what} seed={seed} p={p}: distance {fd:.3f} of its bound")
        assert fd <= 1.0, fd
    else:                                                               # printed, not asserted
        nb = np.sqrt((B.astype(np.float64) ** 2).sum(axis=1))
        db = np.sqrt(((coef.astype(LD) - B) ** 2).sum(axis=1)).astype(np.float64)
        rel_b = float(np.max(db / np.where(nb > 0, nb, 1.0)))
        rel_s = float(np.max(np.abs(np.sqrt(np.asarray(resvar)) - sigma.astype(np.float64)) / sigma.astype(np.float64)))
        print(f"{what} seed={seed} p={p}: beta {rel_b:.3g}, sigma {rel_s:.3g} relative to the comparison value")
    ok = margin >= MARGIN
    assert (~ok).sum() <= 0.01 * ok.size, f"{what}: {(~ok).sum()} of {ok.size} (lambda, node) left out"
    same = ((coef != 0) == (B != 0)).all(axis=1)
    assert np.all(same[ok]), f"{what}: supports differ at (lambda, node) {np.argwhere(~same & ok)[:5]}"
    return ok


def check_graphs(p, seed, scaled, W, rule, ok):
    """The AND / OR graph of a symmetrised stack W (L,p,p) against the comparison value's, on the pairs whose two nodes both
    passed the margin rule."""
    nz = reference(p, seed, scaled)[0] != 0
    want = (nz & nz.transpose(0, 2, 1)) if rule == 'and' else (nz | nz.transpose(0, 2, 1))
    both = ok[:, :, None] & ok[:, None, :]
    assert np.array_equal((np.asarray(W) != 0) & both, want & both)


def check_rescaled(S, Sd, d, lam0, Theta, info, Theta_d, info_d, tol=TOL, sig_tol=SIG_TOL):
    """``scaled_lasso_precision`` (weights 'sd') of S and of Sd = D S D, D = diag(d) of powers of two.  In the units of S the
    second result is beta~_k = beta'_k d_k / d_j (exact).  Both are held to check 1 on their own problem.  Their distance: beta
    has the residual r for the lasso at the thresholds thr = lambda0 sigma(beta) w, beta~ has r~ at thr~ = lambda0 sigma(beta~)
    w; the gradient of the smooth part is lambda_min(S)-strongly monotone and the subdifferentials of the two weighted l1
    terms are monotone up to thr - thr~, so  ||beta - beta~||_2 <= (||r|| + ||r~|| + ||thr - thr~||) / lambda_min(S),  every
    term formed in longdouble from the returned numbers.  Theta against D^-1 Theta D^-1 is printed."""
    p = S.shape[0]
    lam = [lam0]
    W, Wd = np.broadcast_to(np.sqrt(np.diag(S))[None, :], (p, p)), np.broadcast_to(np.sqrt(np.diag(Sd))[None, :], (p, p))
    C, Cd = np.asarray(info['COEF']), np.asarray(info_d['COEF'])
    check_residual(S, lam, W, True, C[None], info['RESVAR'][None], tol, sig_tol, what="unscaled")
    check_residual(Sd, lam, Wd, True, Cd[None], info_d['RESVAR'][None], tol, sig_tol, what="rescaled")
    Ct = Cd * d[:, None] / d[None, :]
    R, thr, _, _ = residual_w(S, C[None], lam, W, True)
    Rt, thrt, _, _ = residual_w(S, Ct[None], lam, W, True)
    off = ~np.eye(p, dtype=bool)
    dthr = np.where(off, thr[0] - thrt[0], 0)
    lmin = float(np.linalg.eigvalsh(S)[0])
    norm = lambda a: np.sqrt((a * a).sum(axis=0)).astype(np.float64)
    dist, bound = norm((C - Ct).astype(LD)), (norm(R[0]) + norm(Rt[0]) + norm(dthr)) / lmin
    fd = float(np.max(np.where(bound > 0, dist / np.where(bound > 0, bound, 1.0), np.where(dist > 0, np.inf, 0.0))))
    back = Theta_d * d[:, None] * d[None, :]
    print(f"rescaled: distance {fd:.3f} of its bound; Theta differs by {float(np.abs(back - Theta).max() / np.abs(Theta).max()):.3g} relative")
    assert fd <= 1.0, fd


def duplicate_case(p=17, N=108):
    """The correlation matrix of data whose variable 5 is a copy of variable 3: the degenerate square-root problem."""
    X = mb_ref.stars_data(seed=5, p=p, N=N).copy()
    X[5] = X[3]
    S = np.corrcoef(X)
    S = 0.5 * (S + S.T)
    S[np.arange(p), np.arange(p)] = 1.0
    S[3, 5] = S[5, 3] = 1.0
    return S
