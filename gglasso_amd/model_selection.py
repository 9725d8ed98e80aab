"""Model selection for the Single Graphical Lasso with the WHOLE grid solved as one batch on the GPU.

The reference's ``single_grid_search`` (helper/model_selection.py:505-692) walks the (lambda1, mu1) grid
sequentially, one ``ADMM_SGL``/``block_SGL`` call per grid point with a warm start from the previous point
(:619-633).  Grid points are independent problems on the same S, so here all L*M of them advance together
as the instances of one (L*M, p, p) stack (``gglasso_amd.batch.ADMM_SGL_batch``: one batched Omega-step and one
elementwise Theta-step per iteration, every instance with its own rho and stopping decision).  The optimum of
a grid point does not depend on its start, so the selection statistics agree with the sequential walk to the
solver tolerance; the bookkeeping below (AIC / eBIC tables, sparsity, rank, best point) follows the
reference's definitions (:769-894, helper/utils.py:17-23) and its return layout.

``grid_search`` (lambda1 x lambda2 grid of the multiple-graph problems, :55-298) is at the end of this module: the whole
grid as one batch on the GPU (``gglasso_amd.batch.ADMM_MGL_batch``), or -- for any other solver callable -- the
reference's sequential warm-started walk.  The reference's own ``grid_search`` also takes ``gglasso_amd.ADMM_MGL``
as its ``solver`` argument unchanged (tests/test_reference_dropin.py).
"""
import numpy as np

from .batch import ADMM_SGL_batch
from .solver import ADMM_SGL, latent_rank

DEFAULT_GAMMAS = (0.1, 0.3, 0.5, 0.7)        # model_selection.py:17
_NUMBER = (int, float, np.integer, np.floating)


def robust_logdet(A, t=1e-12):
    """log det A, or -inf when the smallest eigenvalue is not above ``t`` (model_selection.py:884-894)."""
    d = np.linalg.eigvalsh(A)
    if d.min() <= t:
        return -np.inf
    sign, val = np.linalg.slogdet(A)
    return sign * val


def sparsity(A):
    """ratio of non-zero off-diagonal entries (helper/utils.py:17-23)."""
    assert A.ndim == 2
    p = A.shape[0]
    return (np.count_nonzero(A) - p) / (p ** 2 - p)


def _edges(Theta, lambda1_mask=None):
    p = Theta.shape[0]
    if lambda1_mask is None:
        return (np.count_nonzero(Theta) - p) / 2          # non-zeros above the diagonal
    assert lambda1_mask.shape == Theta.shape
    E = (Theta != 0) * lambda1_mask                        # weighted by the mask, diagonal not counted
    np.fill_diagonal(E, 0)
    return E.sum() / 2


def aic_single(S, Theta, N):
    """AIC after Danaher et al. (model_selection.py:812-820)."""
    assert isinstance(N, _NUMBER)
    return N * np.sum(S * Theta) - N * robust_logdet(Theta) + _edges(Theta)


def ebic_single(S, Theta, N, gamma, lambda1_mask=None):
    """extended BIC after Drton et al. (model_selection.py:840-856)."""
    assert isinstance(N, _NUMBER)
    p = S.shape[0]
    E = _edges(Theta, lambda1_mask)
    return N * np.sum(S * Theta) - N * robust_logdet(Theta) + E * (np.log(N) + 4 * np.log(p) * gamma)


def aic(S, Theta, N):
    """(p,p) or (K,p,p) stacks (model_selection.py:769-810)."""
    if S.ndim == 2:
        return aic_single(S, Theta, N)
    Nk = np.ones(S.shape[0]) * N if isinstance(N, _NUMBER) else N
    return sum(aic_single(S[k], Theta[k], Nk[k]) for k in range(S.shape[0]))


def ebic(S, Theta, N, gamma=0.5):
    """(p,p), (K,p,p) stacks, or dicts (keys 0..K-1) of instances of different dimension (model_selection.py:824-882)."""
    if not isinstance(S, dict) and S.ndim == 2:
        return ebic_single(S, Theta, N, gamma)
    K = len(S)
    Nk = np.ones(K) * N if isinstance(N, _NUMBER) else N
    return sum(ebic_single(S[k], Theta[k], Nk[k], gamma) for k in range(K))


def _solve_grid(S, lam, mu, latent, tol, rtol, max_iter, tau_range=None, fetch=None, select=None):
    """All (lambda1[, mu1]) instances as ONE batch from the reference's start (Omega_0 = X_0 = identity,
    model_selection.py:595-596).  S: (p,p) shared, or (n,p,p) one covariance matrix per instance.  ``tau_range``: also
    score every instance's estimate thresholded at every tau on the GPU (tune_threshold, :707-737)."""
    eye = np.eye(S.shape[-1])
    # fetch / select: a grid walk reads Theta (and L) of every point; only the point it selects is returned whole, so only
    # that point's Omega and X are downloaded (ADMM_SGL_batch)
    res = ADMM_SGL_batch(S, lam, Omega_0=eye, X_0=eye, tol=tol, rtol=rtol, latent=latent, mu1=mu, max_iter=max_iter,
                         selection_stats=True, tau_range=tau_range, fetch=fetch, select=select)
    # per instance: the solution, and <S,Theta>, log det Theta, non-zero count computed on the GPU
    return [s for s, _ in res], [info['selection'] for _, info in res]


def _grid_tables(S, N, sols, dev, lambda_range, mu_range, latent, method, gamma, gammas, store_all, lambda1_mask,
                 thresholding=False, return_index=False):
    """AIC / eBIC / sparsity / rank tables, best point and stored estimates of one (lambda1, mu1) grid
    (model_selection.py:583-690); sols[j*M+m] solves (lambda_range[j], mu_range[m]).  thresholding: every point's
    Theta is replaced by its best thresholded version (tune_threshold, :641-650) before the criteria are taken."""
    p = S.shape[0]
    nl, nm = len(lambda_range), len(mu_range)
    MU, LAMB = np.meshgrid(mu_range, lambda_range)
    BIC = {g: np.full((nl, nm), np.nan) for g in gammas}
    AIC = np.full((nl, nm), np.nan)
    SP = np.full((nl, nm), np.nan)
    RANK = np.zeros((nl, nm))
    TAU = np.zeros((nl, nm)) if thresholding else None
    estimates = np.zeros((nl, nm, p, p)) if store_all else None
    lowrank = np.zeros((nl, nm, p, p)) if store_all else None
    best_sol, curr_min, best_k = dict(), np.inf, None
    for j in range(nl):
        for m in range(nm):
            sol = sols[j * nm + m]
            Theta = sol['Theta']
            if latent:
                if store_all:
                    lowrank[j, m] = sol['L']
            d = dev[j * nm + m] if dev is not None else None
            if latent:
                # matrix_rank(L) of :638: from the batch (the device's eigenvalue count where it rebuilt L, numpy's rule
                # otherwise), or numpy's rule on the host for the point-by-point walk
                RANK[j, m] = d['rank'] if (d is not None and 'rank' in d) else latent_rank(sol['L'])
            if thresholding and d is not None and 'threshold' in d:
                # scored on the GPU for every tau of the default range; the statistics of the chosen one become the point's
                jt = _pick_threshold(d['threshold'], N, p, method, gamma)
                TAU[j, m] = default_tau_range()[jt]
                sol['Theta'] = Theta = _apply_threshold(Theta, TAU[j, m])
                d = dict(zip(('Sdot', 'logdet', 'nnz'), d['threshold'][jt, :3]))
            elif thresholding:
                sol['Theta'], TAU[j, m], _ = tune_threshold(Theta, S, N, tau_range=None, method=method, gamma=gamma)
                Theta = sol['Theta']
                d = None
            # the criteria share the expensive terms <S,Theta> and log det Theta: from the
            # device statistics of the batch, or on the host for the point-by-point (mask) walk
            if d is not None:
                fit = N * d['Sdot'] - N * d['logdet']
                E0 = (d['nnz'] - p) / 2
                E = E0
                SP[j, m] = (d['nnz'] - p) / (p ** 2 - p)
            else:
                fit = N * np.sum(S * Theta) - N * robust_logdet(Theta)
                E0, E = _edges(Theta), _edges(Theta, lambda1_mask)
                SP[j, m] = sparsity(Theta)
            AIC[j, m] = fit + E0
            for g in gammas:
                BIC[g][j, m] = fit + E * (np.log(N) + 4 * np.log(p) * g)
            if store_all:
                estimates[j, m] = Theta
            score = BIC[gamma][j, m] if method == 'eBIC' else AIC[j, m]
            if score < curr_min:
                curr_min = score
                best_sol = dict(sol)
                best_k = j * nm + m
    AIC[AIC == -np.inf] = np.nan
    for g in gammas:
        BIC[g][BIC[g] == -np.inf] = np.nan
    table = AIC if method == 'AIC' else BIC[gamma]
    ix = np.unravel_index(np.nanargmin(table), table.shape)
    stats = {'BIC': BIC, 'AIC': AIC, 'SP': SP, 'RANK': RANK, 'LAMBDA': LAMB, 'MU': MU, 'TAU': TAU,
             'BEST': {'lambda1': LAMB[ix], 'mu1': MU[ix]}, 'GAMMA': gammas}
    if return_index:
        return best_sol, estimates, lowrank, stats, best_k
    return best_sol, estimates, lowrank, stats


def single_grid_search(S, lambda_range, N, method='eBIC', gamma=0.3, latent=False, mu_range=None,
                       thresholding=False, use_block=True, store_all=True, tol=1e-7, rtol=1e-7, lambda1_mask=None,
                       max_iter=1000):
    """Grid search over lambda1 (and mu1 when ``latent``) for the SGL problem with selection by eBIC or AIC:
    arguments and the returned ``(best_sol, estimates, lowrank, stats)`` as model_selection.py:505-692.

    All grid points are solved as ONE batch from the reference's start (Omega_0 = X_0 = identity, :595-596);
    ``use_block`` is accepted and ignored (block splitting changes how a point is solved, not its optimum).
    ``lambda1_mask`` grids run point by point with the reference's warm start (the mask is a per-problem
    array).  ``thresholding``: each point's estimate is replaced by its best thresholded version (tune_threshold,
    :698-737) before the criteria are taken, as in the reference; the 20 candidate thresholds of every grid point are scored
    on the GPU (``ggl_threshold_scan``), the mask walk scores them on the host."""
    assert method in ('AIC', 'eBIC')
    S = np.ascontiguousarray(S, dtype=np.float64)
    p = S.shape[0]
    lambda_range = np.atleast_1d(np.asarray(lambda_range, dtype=np.float64))
    if latent:
        assert mu_range is not None
        mu_range = np.atleast_1d(np.asarray(mu_range, dtype=np.float64))
    else:
        mu_range = np.array([0])
    nl, nm = len(lambda_range), len(mu_range)
    gammas = sorted(set(DEFAULT_GAMMAS) | {gamma})

    # instance j*nm + m solves (lambda_range[j], mu_range[m])
    if lambda1_mask is None:
        # the tables are taken while the batch's device state is still there (``select``): Theta (and L) of all points come
        # down, Omega and X of the selected one only -- what the reference returns as best_sol (:652-660)
        out = {}

        def select(results):
            tabs = _grid_tables(S, N, [sol for sol, _ in results], [info['selection'] for _, info in results], lambda_range,
                                mu_range, latent, method, gamma, gammas, store_all, None, thresholding, return_index=True)
            out['tables'] = tabs[:4]
            return tabs[4], tabs[0]

        _solve_grid(S, np.repeat(lambda_range, nm), np.tile(mu_range, nl) if latent else None, latent, tol, rtol, max_iter,
                    default_tau_range() if thresholding else None, fetch=('Theta', 'L'), select=select)
        return out['tables']
    else:
        sols, dev = [], None
        Om0 = np.eye(p)
        for j in range(nl):
            for m in range(nm):
                kw = dict(latent=True, mu1=mu_range[m]) if latent else {}
                sol, _ = ADMM_SGL(S, lambda_range[j], Om0, X_0=np.eye(p), tol=tol, rtol=rtol, verbose=False,
                                  lambda1_mask=lambda1_mask, max_iter=max_iter, **kw)
                Om0 = sol['Omega'].copy()
                sols.append(sol)
    return _grid_tables(S, N, sols, dev, lambda_range, mu_range, latent, method, gamma, gammas, store_all, lambda1_mask,
                        thresholding)


def _K_single_grid_dict(S, lambda_range, N, method, gamma, latent, mu_range, thresholding, use_block, store_all, tol,
                        rtol, max_iter):
    """K_single_grid for a dict of instances of DIFFERENT dimension (model_selection.py:300-503 with dict S): every
    instance's (lambda1, mu1) grid is its own batch (``single_grid_search``); the selection across instances follows
    the reference (:443-466)."""
    K = len(S.keys())
    assert len(N) == K, f"N must be given as array, is given as {N}."
    lambda_range = np.atleast_1d(np.asarray(lambda_range, dtype=np.float64))
    mu_r = np.atleast_1d(np.asarray(mu_range, dtype=np.float64)) if latent else np.array([0])
    nl, nm = len(lambda_range), len(mu_r)
    MU, LAMB = np.meshgrid(mu_r, lambda_range)
    BIC, AIC = np.full((K, nl, nm), np.nan), np.full((K, nl, nm), np.nan)
    SP, RANK = np.full((K, nl, nm), np.nan), np.zeros((K, nl, nm))
    estimates, lowrank, indv_T, indv_L = dict(), dict(), dict(), dict()
    for k in range(K):
        best, estimates[k], lowrank[k], st = single_grid_search(S[k], lambda_range, N[k], method, gamma, latent, mu_range,
                                                                thresholding, use_block, True, tol, rtol, None, max_iter)
        indv_T[k] = best['Theta']
        if latent:
            indv_L[k] = best['L']
        BIC[k], AIC[k], SP[k], RANK[k] = st['BIC'][gamma], st['AIC'], st['SP'], st['RANK']
    table = AIC if method == 'AIC' else BIC
    ix_mu = np.zeros((K, nl), dtype=int)
    score = np.full((K, nl), np.nan)
    for k in range(K):
        for j in range(nl):
            ix_mu[k, j] = np.nanargmin(table[k, j, :])
            score[k, j] = table[k, j, ix_mu[k, j]]
    score[score == -np.inf] = np.nan
    ix_uniform = np.nanargmin(score.sum(axis=0))
    ix_indv = np.nanargmin(score, axis=1)
    est_indv = {'Theta': indv_T}
    est_uniform = {'Theta': {k: estimates[k][ix_uniform, ix_mu[k, ix_uniform]] for k in range(K)}}
    if latent:
        est_indv['L'] = indv_L
        est_uniform['L'] = {k: lowrank[k][ix_uniform, ix_mu[k, ix_uniform]] for k in range(K)}
    statistics = {'BIC': BIC, 'AIC': AIC, 'SP': SP, 'RANK': RANK, 'LAMB': LAMB, 'MU': MU, 'ix_uniform': ix_uniform,
                  'ix_indv': ix_indv, 'ix_mu': ix_mu}
    return est_uniform, est_indv, statistics


def K_single_grid(S, lambda_range, N, method='eBIC', gamma=0.3, latent=False, mu_range=None, thresholding=False,
                  use_block=True, store_all=True, tol=1e-7, rtol=1e-7, max_iter=1000, max_batch_bytes=8 << 30):
    """Model selection for K independent Single Graphical Lasso problems on a common (lambda1, mu1) grid:
    arguments and the returned ``(est_uniform, est_indv, statistics)`` as model_selection.py:300-503 (array S only).

    The reference runs ``single_grid_search`` instance after instance; here the K x L x M problems are the
    instances of as few batches as ``max_batch_bytes`` of device stacks allow (one, typically)."""
    assert method in ('AIC', 'eBIC')
    if isinstance(S, dict):
        return _K_single_grid_dict(S, lambda_range, N, method, gamma, latent, mu_range, thresholding, use_block, store_all,
                                   tol, rtol, max_iter)
    S = np.ascontiguousarray(S, dtype=np.float64)
    K, p = S.shape[0], S.shape[1]
    assert len(N) == K, f"N must be given as array, is given as {N}."
    lambda_range = np.atleast_1d(np.asarray(lambda_range, dtype=np.float64))
    if latent:
        assert mu_range is not None
        mu_range = np.atleast_1d(np.asarray(mu_range, dtype=np.float64))
    else:
        mu_range = np.array([0])
    nl, nm = len(lambda_range), len(mu_range)
    gammas = sorted(set(DEFAULT_GAMMAS) | {gamma})
    MU, LAMB = np.meshgrid(mu_range, lambda_range)

    # instances in the order (k, j, m); ~14 (K',p,p) stacks live on the device per batch
    per_k = nl * nm
    k_per_batch = max(1, int(max_batch_bytes // (14 * per_k * p * p * 8)))
    sols, dev = [], []
    for k0 in range(0, K, k_per_batch):
        ks = range(k0, min(K, k0 + k_per_batch))
        S_inst = np.repeat(S[list(ks)], per_k, axis=0)
        lam = np.tile(np.repeat(lambda_range, nm), len(ks))
        mu = np.tile(np.tile(mu_range, nl), len(ks)) if latent else None
        s_, d_ = _solve_grid(S_inst, lam, mu, latent, tol, rtol, max_iter, default_tau_range() if thresholding else None,
                             fetch=('Theta', 'L'))            # (K_single_grid uses Theta and L of the points, nothing else)
        sols += s_
        dev += d_

    BIC = {g: np.full((K, nl, nm), np.nan) for g in gammas}
    AIC = np.full((K, nl, nm), np.nan)
    SP = np.full((K, nl, nm), np.nan)
    RANK = np.zeros((K, nl, nm))
    estimates, lowrank = dict(), dict()
    indv_T, indv_L = [], []
    for k in range(K):
        sl = slice(k * per_k, (k + 1) * per_k)
        best, est_k, lr_k, st = _grid_tables(S[k], N[k], sols[sl], dev[sl], lambda_range, mu_range, latent, method, gamma,
                                             gammas, store_all, None, thresholding)
        indv_T.append(best['Theta'])
        if latent:
            indv_L.append(best['L'])
        if store_all:
            estimates[k], lowrank[k] = est_k, lr_k
        for g in gammas:
            BIC[g][k] = st['BIC'][g]
        AIC[k], SP[k], RANK[k] = st['AIC'], st['SP'], st['RANK']

    # for each lambda1 the best mu1 per instance, then the best lambda1 uniformly and individually (:443-466)
    table = AIC if method == 'AIC' else BIC[gamma]
    ix_mu = np.zeros((K, nl), dtype=int)
    score = np.full((K, nl), np.nan)
    for k in range(K):
        for j in range(nl):
            ix_mu[k, j] = np.nanargmin(table[k, j, :])
            score[k, j] = table[k, j, ix_mu[k, j]]
    score[score == -np.inf] = np.nan
    ix_uniform = np.nanargmin(score.sum(axis=0))
    ix_indv = np.nanargmin(score, axis=1)

    est_indv = {'Theta': np.stack(indv_T)}
    if latent:
        est_indv['L'] = np.stack(indv_L)
    est_uniform = None
    if store_all:
        est_uniform = {'Theta': np.stack([estimates[k][ix_uniform, ix_mu[k, ix_uniform]] for k in range(K)])}
        if latent:
            est_uniform['L'] = np.stack([lowrank[k][ix_uniform, ix_mu[k, ix_uniform]] for k in range(K)])
    statistics = {'BIC': BIC[gamma], 'AIC': AIC, 'SP': SP, 'RANK': RANK, 'LAMB': LAMB, 'MU': MU,
                  'ix_uniform': ix_uniform, 'ix_indv': ix_indv, 'ix_mu': ix_mu}
    return est_uniform, est_indv, statistics


# -----------------------------------------------------------------------------------------------------------------
# lambda1 x lambda2 grid for the multiple-graph problems
# -----------------------------------------------------------------------------------------------------------------
N_TAU = 20      # model_selection.py:18


def lambda_parametrizer(l1=0.05, w2=0.5):
    """model_selection.py:20-25."""
    a = 1 / np.sqrt(2)
    return (w2 * l1) / (a * (1 - w2))


def lambda_grid(l1, l2=None, w2=None):
    """model_selection.py:32-52: lambda1 changes over the columns, lambda2 over the rows.  (The reference squeezes
    the meshgrid, which breaks its own MAIN LOOP for one-row or one-column grids; the grids stay 2-D here.)"""
    assert np.all(l2 is not None) | np.all(w2 is not None), \
        "Either a range of lambda2 or w2 values have to be specified"
    if np.all(l2 is not None):
        L1, L2 = np.meshgrid(l1, l2)
    else:
        l1grid, w2grid = np.meshgrid(l1, w2)
        L2 = lambda_parametrizer(l1grid, w2grid)
        L1 = l1grid.copy()
    return np.atleast_2d(L1), np.atleast_2d(L2)


def mean_sparsity(Theta):
    """helper/utils.py:25-31."""
    if isinstance(Theta, dict):
        return np.mean([sparsity(Theta[k]) for k in Theta.keys()])
    return np.mean([sparsity(Theta[k]) for k in range(Theta.shape[0])])


def thresholding(A, tau):
    """model_selection.py:698-705: entries with |a| <= tau are set to zero, the diagonal is kept."""
    mask = (np.abs(A) > tau)
    np.fill_diagonal(mask, 1.)
    return A * mask


_apply_threshold = thresholding        # the functions above take a flag of that name


def default_tau_range():
    return np.logspace(-12, -1, N_TAU)             # model_selection.py:714


def _pick_threshold(table, N, p, method, gamma):
    """tune_threshold's choice (model_selection.py:718-735) from the (ntau, 4) device table of
    {<S,T>, log det T, count_nonzero(T), lambda_min(T)}: index of the best tau (first of equals, nan = not definite)."""
    E = (table[:, 2] - p) / 2
    scores = N * table[:, 0] - N * table[:, 1] + E * ((np.log(N) + 4 * np.log(p) * gamma) if method == 'eBIC' else 1.0)
    scores[scores == np.inf] = np.nan
    return int(np.nanargmin(scores))


def tune_threshold(Theta, S, N, tau_range=None, method='eBIC', gamma=0.1):
    """model_selection.py:707-737."""
    if tau_range is None:
        tau_range = default_tau_range()
    assert np.all(tau_range > 0)
    scores = np.zeros(len(tau_range))
    for j in range(len(tau_range)):
        T = thresholding(Theta, tau_range[j])
        scores[j] = ebic_single(S, T, N, gamma) if method == 'eBIC' else aic_single(S, T, N)
    scores[scores == np.inf] = np.nan
    opt_tau = tau_range[np.nanargmin(scores)]
    return thresholding(Theta, opt_tau), opt_tau, scores


def tune_multiple_threshold(Theta, S, N, tau_range, method='eBIC', gamma=0.1):
    """model_selection.py:739-765 (arrays or dicts)."""
    K = len(S.keys()) if isinstance(S, dict) else S.shape[0]
    t_Theta = Theta.copy()
    score = dict()
    tau = np.zeros(K)
    for k in range(K):
        t_Theta[k], tau[k], score[k] = tune_threshold(Theta[k], S[k], N[k], tau_range, method, gamma)
    return t_Theta, tau, score


def _criteria(S, Theta, N, K):
    """Per-instance fit term N (<S,Theta> - log det Theta) and edge count of aic_single / ebic_single (:812-856)."""
    fit = np.array([N[k] * np.sum(S[k] * Theta[k]) - N[k] * robust_logdet(Theta[k]) for k in range(K)])
    E = np.array([_edges(Theta[k]) for k in range(K)])
    return fit, E


def grid_search(solver, S, N, p, reg, l1, l2=None, w2=None, method='eBIC', gamma=0.3, G=None, latent=False,
                mu_range=None, ix_mu=None, thresholding=False, tol=1e-7, rtol=1e-7, verbose=False, group=None,
                max_batch_bytes=8 << 30, batched=None):
    """Model selection for the multiple-graph problems over a lambda1 x lambda2 grid with AIC / eBIC -- arguments and
    the returned ``(stats, ix, curr_best)`` as the reference's ``grid_search`` (helper/model_selection.py:55-298).

    With ``solver`` = ``gglasso_amd.ADMM_MGL`` and S an array, the WHOLE grid is solved as one batch on the GPU
    (``gglasso_amd.batch.ADMM_MGL_batch``: grid points are independent problems on the same S; one batched Omega-step
    over all (grid points x K) matrices and one Theta-step launch per iteration, every point with its own rho and
    stopping decision) from the identity start, and the criteria's expensive terms <S,Theta>, log det Theta,
    count_nonzero come from the device.  The reference walks the grid column by column with a warm start from the
    previous point (:208-224); the optimum of a point does not depend on its start, so tables and selection agree
    to the solver tolerance.  ``group``: a torch.distributed process group -- the grid points are dealt round-robin
    over its ranks (``gglasso_amd.dist.shard_grid``; replicas only, results gathered on every rank).
    ``solver`` = ``gglasso_amd.ext_ADMM_MGL`` with dict S and G (instances of different dimension) is batched the same way
    (``gglasso_amd.ext_solver.ext_ADMM_MGL_batch``; the criteria then come from the host, per instance dimension).
    Any other solver callable (the reference's own solvers) and ``batched=False`` take the reference's sequential
    warm-started walk with that callable.  ``thresholding`` tunes a thresholded
    estimator per grid point on the host (tune_multiple_threshold, :739-765) in either mode."""
    from .solver import ADMM_MGL
    assert method in ['AIC', 'eBIC']
    assert reg in ['FGL', 'GGL']
    if isinstance(S, dict):
        K = len(S.keys())
    elif isinstance(S, np.ndarray):
        K = S.shape[0]
    else:
        raise Exception("S must be specified either as array or dict.")
    assert len(N) == K, f"N must be given as array, is given as {N}."
    if latent:
        assert np.all(mu_range > 0)
    L1, L2 = lambda_grid(l1, l2, w2)
    if verbose:
        print("Grid of lambda1/lambda2:")
        print(L1)
        print(L2)
    grid1, grid2 = L1.shape
    gammas = sorted(set(DEFAULT_GAMMAS) | {gamma})
    AIC = np.nan * np.zeros((grid1, grid2))
    BIC = {g: np.nan * np.zeros((grid1, grid2)) for g in gammas}
    SP = np.nan * np.zeros((grid1, grid2))
    RANK = np.nan * np.zeros((K, grid1, grid2))
    TAU = np.zeros((K, grid1, grid2)) if thresholding else None
    from .ext_solver import ext_ADMM_MGL as _ext_solver
    ext_batched = (batched is None or batched) and (solver is _ext_solver) and isinstance(S, dict) and reg == 'GGL' \
        and G is not None and group is None
    if ext_batched:
        batched = False
    if batched is None:
        # both penalties fall back to the sequential walk beyond what their batched Theta kernel takes (the library
        # exports the limits; ADVICE r2: FGL used to surface the limit as an AssertionError instead)
        from ._lib import theta_limits
        batched = (solver is ADMM_MGL) and isinstance(S, np.ndarray) and K <= theta_limits()[reg]
    order = [(g1, g2) for g2 in range(grid2) for g1 in range(grid1)]       # down the columns, as the reference

    sols = {}
    dev, dev_thr, dev_rank = {}, {}, {}
    if batched:
        from .batch import ADMM_MGL_batch
        pdim = S.shape[1]
        mine = list(range(len(order)))
        if group is not None:
            import torch.distributed as dist
            from .dist import shard_grid
            mine = shard_grid(len(order), dist.get_world_size(group), dist.get_rank(group))
        per_batch = max(1, int(max_batch_bytes // (14 * K * pdim * pdim * 8)))
        local = []
        for b0 in range(0, len(mine), per_batch):
            idx = mine[b0:b0 + per_batch]
            lam1 = np.array([L1[order[i]] for i in idx])
            lam2 = np.array([L2[order[i]] for i in idx])
            mu = np.stack([mu_range[ix_mu[:, order[i][1]]] for i in idx]) if latent else None
            # without thresholding the walk below reads Theta and L of the points and returns the whole solution of the best one
            # only: Theta and L of all points come down, Omega and X of each batch's best (the overall best is one of them)
            sel = None
            if not thresholding:
                pS_, Nk_ = S.shape[1], np.asarray(N, dtype=np.float64) * np.ones(K)

                def sel(results):
                    best, best_g = np.inf, None
                    for g, (_, info) in enumerate(results):
                        d = info['selection']
                        fit, E = Nk_ * d[:, 0] - Nk_ * d[:, 1], (d[:, 2] - pS_) / 2
                        sc = np.sum(fit + E * (np.log(Nk_) + 4 * np.log(pS_) * gamma)) if method == 'eBIC' else np.sum(fit + E)
                        if sc < best:
                            best, best_g = sc, g
                    return best_g, None
            res = ADMM_MGL_batch(S, lam1, lam2, reg, tol=tol, rtol=rtol, latent=latent, mu1=mu, selection_stats=True,
                                 tau_range=default_tau_range() if thresholding else None,
                                 fetch=None if thresholding else ('Theta', 'L'), select=sel)
            local += [(i, r) for i, r in zip(idx, res)]
        if group is not None:
            gathered = [None] * dist.get_world_size(group)
            dist.all_gather_object(gathered, local, group=group)
            local = [x for part in gathered for x in part]
        for i, (sol, info) in local:
            sols[order[i]] = sol
            dev[order[i]] = info['selection']
            if thresholding:
                dev_thr[order[i]] = info['threshold']
            if latent:
                dev_rank[order[i]] = info['rank']
    elif ext_batched:
        from .ext_solver import ext_ADMM_MGL_batch
        pmax = max(S[k].shape[0] for k in range(K))
        per_batch = max(1, int(max_batch_bytes // (17 * K * pmax * pmax * 8)))
        for b0 in range(0, len(order), per_batch):
            idx = order[b0:b0 + per_batch]
            lam1 = [L1[g] for g in idx]
            lam2 = np.array([L2[g] for g in idx])
            mu = np.stack([mu_range[ix_mu[:, g[1]]] for g in idx]) if latent else None
            res = ext_ADMM_MGL_batch(S, lam1, lam2, reg, G, tol=tol, rtol=rtol, latent=latent, mu1=mu)
            for g, (sol, info) in zip(idx, res):
                sols[g] = sol
    else:
        kwargs = {'reg': reg, 'S': S, 'tol': tol, 'rtol': rtol, 'verbose': False, 'measure': False}
        if isinstance(S, dict):
            kwargs['Omega_0'] = {k: np.eye(S[k].shape[0]) for k in range(K)}      # id_dict, ext_admm_helper.py:9-16
            kwargs['G'] = G
        else:
            kwargs['Omega_0'] = np.stack([np.eye(S.shape[1])] * K)               # id_array, utils.py:10-15
        for (g1, g2) in order:
            kwargs['lambda1'], kwargs['lambda2'] = L1[g1, g2], L2[g1, g2]
            if latent:
                kwargs['latent'] = True
                kwargs['mu1'] = mu_range[ix_mu[:, g2]].copy()
            sol, info = solver(**kwargs)
            kwargs['Omega_0'] = sol['Omega'].copy()                               # warm start (:224)
            sols[(g1, g2)] = sol

    curr_min, curr_best = np.inf, None
    no_thr_min, no_thr_params, no_thr_best = np.inf, None, None
    for (g1, g2) in order:
        sol = sols[(g1, g2)]
        d = dev.get((g1, g2))
        if d is not None:
            # the batch's device statistics; with thresholding also those of every instance's estimate at every tau
            pS = S.shape[1]
            fit = N * d[:, 0] - N * d[:, 1]
            nnz = d[:, 2].copy()
            E = (nnz - pS) / 2
            if thresholding:
                score0 = np.sum(fit + E * (np.log(N) + 4 * np.log(pS) * gamma))
                if score0 < no_thr_min:
                    no_thr_min, no_thr_best = score0, sol.copy()
                    no_thr_params = {'lambda1': L1[g1, g2], 'lambda2': L2[g1, g2]}
                sol['Theta'] = sol['Theta'].copy()
                for k in range(K):
                    tab = dev_thr[(g1, g2)][k]
                    jt = _pick_threshold(tab, N[k], pS, method, gamma)
                    TAU[k, g1, g2] = default_tau_range()[jt]
                    sol['Theta'][k] = _apply_threshold(sol['Theta'][k], TAU[k, g1, g2])
                    fit[k], nnz[k] = N[k] * tab[jt, 0] - N[k] * tab[jt, 1], tab[jt, 2]
                E = (nnz - pS) / 2
            SP[g1, g2] = np.mean((nnz - pS) / (pS ** 2 - pS))
        else:
            if thresholding:
                fit0, E0 = _criteria(S, sol['Theta'], N, K)
                pk = np.array([S[k].shape[0] for k in range(K)])
                score0 = np.sum(fit0 + E0 * (np.log(N) + 4 * np.log(pk) * gamma))
                if score0 < no_thr_min:
                    no_thr_min, no_thr_best = score0, sol.copy()
                    no_thr_params = {'lambda1': L1[g1, g2], 'lambda2': L2[g1, g2]}
                sol['Theta'], TAU[:, g1, g2], _ = tune_multiple_threshold(sol['Theta'], S, N, tau_range=None,
                                                                          method=method, gamma=gamma)
            fit, E = _criteria(S, sol['Theta'], N, K)
            SP[g1, g2] = mean_sparsity(sol['Theta'])
        pk = np.array([S[k].shape[0] for k in range(K)])
        Nk = np.asarray(N, dtype=np.float64)
        AIC[g1, g2] = np.sum(fit + E)
        for g in gammas:
            BIC[g][g1, g2] = np.sum(fit + E * (np.log(Nk) + 4 * np.log(pk) * g))
        if latent:
            if (g1, g2) in dev_rank:
                RANK[:, g1, g2] = dev_rank[(g1, g2)]
            else:
                RANK[:, g1, g2] = [latent_rank(sol['L'][k]) for k in range(K)]
        score = BIC[gamma][g1, g2] if method == 'eBIC' else AIC[g1, g2]
        if score < curr_min:
            curr_min = score
            curr_best = sol.copy()
        if verbose:
            print(f"Grid point: (l1,l2): {(L1[g1, g2], L2[g1, g2])}, sparsity: {np.round(SP[g1, g2], 3)}, "
                  f"best score: {np.round(curr_min, 1)}")
    if method == 'AIC':
        AIC[AIC == -np.inf] = np.nan
        ix = np.unravel_index(np.nanargmin(AIC), AIC.shape)
    else:
        for g in gammas:
            BIC[g][BIC[g] == -np.inf] = np.nan
        ix = np.unravel_index(np.nanargmin(BIC[gamma]), BIC[gamma].shape)
    if verbose:
        print(f"Best regularization parameters: (l1,l2): {(L1[ix], L2[ix])}")
    stats = {'BIC': BIC, 'AIC': AIC, 'SP': SP, 'RANK': RANK, 'TAU': TAU, 'L1': L1, 'L2': L2,
             'BEST': {'lambda1': L1[ix], 'lambda2': L2[ix]}, 'GAMMA': gammas}
    if thresholding:
        stats['NO_THRESHOLDING_SOL'] = no_thr_best
        stats['NO_THRESHOLDING_BEST'] = no_thr_params
    return stats, ix, curr_best


# -----------------------------------------------------------------------------------------------------------------
# StARS: stability selection of lambda1 from data (Liu, Roeder, Wasserman 2010, "Stability Approach to Regularization
# Selection"; the default of R's huge).  B subsamples x L lambdas are B * L independent single problems of one dimension:
# ONE batch (``ADMM_SGL_batch``'s machinery), instance l * B + r = subsample r at lambda l.  The data go to the device
# once, the B subset covariances are computed and replicated there, and what comes back is one integer per lambda.
# -----------------------------------------------------------------------------------------------------------------
def stars_subsamples(N, n_subsamples, subsample_size=None, seed=0):
    """The (n_subsamples, b) int32 array of sorted draws without replacement from range(N): row r comes from
    ``numpy.random.default_rng([seed, r])``.  Default b: ``int(10 sqrt(N))`` for N > 144, else ``int(0.8 N)`` (the rule of
    huge), at least 1."""
    N, B = int(N), int(n_subsamples)
    assert N >= 1 and B >= 1, "N and n_subsamples must be at least 1"
    if subsample_size is None:
        subsample_size = int(10 * np.sqrt(N)) if N > 144 else int(0.8 * N)
    b = max(1, int(subsample_size))
    assert b <= N, f"a subsample of {b} out of {N} observations cannot be drawn without replacement"
    return np.stack([np.sort(np.random.default_rng([int(seed), r]).choice(N, b, replace=False))
                     for r in range(B)]).astype(np.int32)


def stars_select(D, beta):
    """StARS' choice on the instabilities ``D`` of a grid in descending order (sparse to dense): ``(index, Dbar)`` with
    ``Dbar`` the running maximum of D and ``index`` the largest one with ``Dbar <= beta`` -- the densest graph that is still
    stable.  A NaN in D (a lambda with a failed point) is never chosen and does not enter the running maximum.  If no
    lambda qualifies: index 0 and a RuntimeWarning."""
    import warnings
    D = np.asarray(D, dtype=np.float64).reshape(-1)
    assert D.size >= 1
    Dbar = np.fmax.accumulate(D)
    ok = np.flatnonzero(~np.isnan(D) & (Dbar <= beta))
    if ok.size == 0:
        warnings.warn(f"StARS: no lambda1 of the grid has an instability of at most beta = {beta} (the smallest is "
                      f"{np.nanmin(D) if not np.all(np.isnan(D)) else np.nan}); the sparsest point of the grid is returned. "
                      f"Extend the grid to larger lambda1.", RuntimeWarning, stacklevel=2)
        return 0, Dbar
    return int(ok[-1]), Dbar


def _host_subset_covariances(X, idx, center, scale):
    """numpy counterpart of ``utils.sample_covariance_subsets`` for engines without the device route."""
    out = []
    for r in range(idx.shape[0]):
        Xr = X[:, idx[r]]
        S = np.atleast_2d(np.cov(Xr, bias=True)) if center else Xr @ Xr.T / Xr.shape[1]
        if scale:
            sd = np.sqrt(np.diag(S))
            S = S / (sd[:, None] * sd[None, :])
        out.append(S)
    return np.stack(out)


def _host_pairwise_covariances(X, idx, center, scale, min_pairs):
    """numpy counterpart of ``utils.sample_covariance_subsets(..., missing='pairwise')`` for engines without the device route."""
    from . import utils
    S, cnt = utils.host_pairwise_covariance(X, center, idx)
    assert int(min_pairs) >= 1 and cnt.min() >= int(min_pairs), f"a pair of variables shares fewer than min_pairs = {min_pairs} samples"
    if scale:
        sd = np.sqrt(np.diagonal(S, axis1=1, axis2=2))
        S = S / (sd[:, :, None] * sd[:, None, :])
    return S


def _host_edge_counts(Theta, t):
    """(L,p,p) int32 counts and (L,) int64 sums of StARS from a (L,B,p,p) stack: numpy counterpart of
    ``HipEngine.edge_stability`` (only the upper triangle of a Theta is read, a NaN is no edge)."""
    L, B, p, _ = Theta.shape
    with np.errstate(invalid='ignore'):
        up = np.triu(np.abs(Theta) >= t, 1).sum(axis=1).astype(np.int64)
    num = (up * (B - up)).sum(axis=(1, 2))
    return (up + up.transpose(0, 2, 1)).astype(np.int32), num.astype(np.int64)


def _mbw_kwargs(method, weights, scaled, X):
    """The keyword arguments ``weights`` / ``scaled`` add to every path call of a search ({} without them), and their
    refusals."""
    if weights is None and not scaled:
        return {}
    if method != 'mb':
        raise ValueError("weights= and scaled= belong to method='mb' (utils.neighborhood_selection): the node-wise lasso's "
                         "penalty weights and the scaled lasso.  The graphical lasso's per-entry penalties are lambda1_mask")
    kw = {'scaled': True} if scaled else {}
    if weights is not None:
        p = np.shape(X)[0]
        Wt = np.asarray(weights, dtype=np.float64)
        assert Wt.shape == (p, p), f"weights must be one ({p},{p}) table (row j: node j's weights) for every fit, got {Wt.shape}"
        kw['weights'] = Wt
    return kw


def stars_search(X, lambda_range, n_subsamples=20, subsample_size=None, beta=0.05, seed=0, indices=None, t=1e-8, center=True,
                 scale=False, tol=1e-7, rtol=1e-7, max_iter=1000, store_all=False, lambdas_per_batch=None, correlation=None,
                 missing=None, min_pairs=2, project=False, method='glasso', rule='and', refit=False, weights=None, scaled=False):
    """StARS for the Single Graphical Lasso from observations ``X`` (p,N), variables in rows.  Returns ``(sol, stats)``.

    * Subsamples: ``stars_subsamples(N, n_subsamples, subsample_size, seed)``, or ``indices`` (B,b) given by the caller
      (duplicates allowed: a bootstrap draw).  The grid is used in descending order, ``stats['LAMBDA']``.
    * ``S_r`` = ``numpy.cov(X[:, indices[r]], bias=True)`` (``scale``: each subsample's correlations); ``Theta[l,r]`` solves
      ``ADMM_SGL(S_r, lambda[l])`` from ``Omega_0 = X_0 = identity``; all B * L points run as one batch.
    * ``c[l,i,j]`` = #{r : |Theta[l,r,i,j]| >= t} for i < j; ``NUM[l] = sum_{i<j} c (B - c)`` (exact integers);
      ``INSTABILITY[l] = 2 NUM[l] / (B^2 p (p - 1) / 2)``; ``INSTABILITY_MONOTONE`` its running maximum along the grid;
      ``IX`` the largest index whose running maximum is at most ``beta`` (``stars_select``).
    * A lambda with a point that ended as 'solver error' gets NaN, is never chosen and is listed in ``FAILED``.
    * ``sol``: ``ADMM_SGL`` on the covariance of all N observations at the chosen lambda1 (``stats['BEST']``).

    With the device engine the data are uploaded once, the covariances never exist on the host and only the L integers come
    back; ``store_all`` also returns ``COUNTS`` (L,p,p) and ``THETA`` (L,B,p,p).  ``lambdas_per_batch``: run that many
    lambdas per batch (each its own ctx) where the whole grid does not fit in device memory.  An engine without
    ``set_data_subsets`` / ``edge_stability`` takes the same batch call on numpy covariances and counts on the host.

    ``correlation='kendall'``: every ``S_r``, and the matrix of the final fit, is the nonparanormal skeptic matrix
    ``sin(pi/2 tau-b)`` of the observations (``utils.skeptic_correlation``; on the device ``ggl_set_S_from_kendall``) instead of
    the Pearson covariance -- invariant under monotone transforms of the variables, robust to outliers and ties.  ``center`` and
    ``scale`` have no meaning then and must be left at their defaults.  The matrix may be indefinite; it is used as it is
    unless ``project=True``.

    ``missing='pairwise'``: a NaN in X is a missing value; every ``S_r`` and the matrix of the final fit are pairwise-complete
    covariances (``utils.sample_covariance_subsets(..., missing='pairwise')``; on the device
    ``ggl_set_S_from_subsets_pairwise``).  A subsample in which a pair of variables shares fewer than ``min_pairs`` samples is
    refused, naming it.  Together with ``correlation='kendall'`` or ``'mixed'`` it is a ValueError.

    ``correlation='mixed'``: every ``S_r``, and the matrix of the final fit, is the latent correlation matrix of mixed binary /
    continuous data (``utils.mixed_correlation``; on the device ``ggl_set_S_from_mixed``).  The types are fixed once, from all N
    observations: a variable with exactly two distinct values is binary.  A subsample over which a variable is constant is
    refused, naming both.  ``center`` and ``scale`` as with ``'kendall'``.

    ``project=True``: every ``S_r`` and the matrix of the final fit are replaced by their nearest-correlation projections
    (``utils.nearest_correlation`` with its defaults), after any ``correlation=`` and ``missing=`` choice.  On the device one
    ``engine.project_S(period=B)`` projects the B subset matrices where they lie, before they are used; an engine without
    ``project_S`` gets the numpy twin's matrices (``utils.host_nearest_correlation``).  ``stats['PROJECTION']`` is the info of
    the final fit's matrix.

    ``method='mb'``: the estimator at every point is Meinshausen-Buhlmann neighbourhood selection instead of the graphical
    lasso (``utils.neighborhood_selection``; ``method = "mb"`` of R's huge): one lasso per variable on ``S_r``, the grid walked
    in descending order with warm starts, and ``Theta[l,r]`` -- ``THETA`` with ``store_all`` -- is the coefficient matrix
    symmetrised by ``rule`` (``'and'`` / ``'or'``, ``utils.neighborhood_graph``), to which the same ``|.| >= t`` applies.
    Subsamples, ``correlation=``, ``missing=``, ``project=``, ``lambdas_per_batch`` (every batch starts its path anew),
    ``store_all``, the keys of ``stats`` and ``stars_select`` are those of the graphical lasso; ``tol`` is the path's tolerance,
    ``rtol`` and ``max_iter`` are not used.  On the device one ctx of B instances holds the subsample matrices and
    ``HipEngine.neighborhood_stability`` returns the integers; an engine without it gets ``utils.host_neighborhood_selection``
    on numpy matrices.  ``FAILED`` lists a lambda at which a node of a subsample met a non-finite value (status 2); nodes that
    reached a cap (status 1) raise a ``RuntimeWarning`` with their number and fail nothing.  ``sol`` is the path's result at the
    chosen lambda on the matrix of all N observations: ``{'adjacency', 'coef', 'resvar', 'lambda1'}`` -- the boolean graph under
    ``rule`` and ``t``, the raw coefficients (column j: node j's) and the residual variances.  The lasso is not invariant
    under rescaling a variable: ``mb`` works on whatever scale ``center`` / ``scale`` produce, and ``scale=True`` (correlations)
    is what huge does.  ``refit=True`` (``method='mb'`` only): ``sol`` gains ``coef_refit`` and ``resvar_refit``, the
    least-squares refit of every node on its neighbours in ``sol['adjacency']`` (``utils.neighborhood_refit``), and
    ``precision``, ``utils.neighborhood_precision`` of the two; with the default the keys and bits of ``sol`` stay.  With
    ``method='glasso'`` nothing of this applies.  ``weights`` ((p,p): row j holds node j's penalty weights) and ``scaled`` (the
    scaled lasso) are those of ``utils.neighborhood_selection`` (``method='mb'`` only; the graphical lasso's per-entry
    penalties are ``lambda1_mask``): they apply to every subsample fit and to the final fit, on the device and on the host
    route; statuses 2 and 3 put a lambda into ``FAILED``.  Without them the calls and the bits are what they were."""
    import warnings
    from . import solver as _solver, utils
    from .batch import _sgl_batch_impl
    assert method in ('glasso', 'mb'), "method must be 'glasso' or 'mb'"
    mb = method == 'mb'
    assert not mb or rule in ('and', 'or'), "rule must be 'and' or 'or'"
    mbw = _mbw_kwargs(method, weights, scaled, X)
    assert mb or not refit, "refit=True needs method='mb': the graphical lasso has no node-wise regressions to refit"
    assert correlation in (None, 'kendall', 'mixed'), "correlation must be None (Pearson), 'kendall' or 'mixed'"
    assert missing in (None, 'pairwise'), "missing must be None (complete data) or 'pairwise'"
    kendall, mixed = correlation == 'kendall', correlation == 'mixed'
    pairwise = missing == 'pairwise'
    if (kendall or mixed) and pairwise:
        raise ValueError(f"missing='pairwise' with correlation='{correlation}': ranks of data with holes are not implemented")
    if kendall or mixed:
        assert center is True and scale is False, \
            f"correlation='{correlation}' has no use for center / scale: leave them at their defaults"
    X = np.ascontiguousarray(X, dtype=np.float64)
    assert X.ndim == 2, f"data must be a (p,N) array with variables in rows, has shape {X.shape}"
    p, N = X.shape
    lam = np.sort(np.atleast_1d(np.asarray(lambda_range, dtype=np.float64)).reshape(-1))[::-1].copy()
    assert lam.size >= 1 and np.all(lam > 0), "lambda1 should be positive"
    assert t >= 0 and np.isfinite(t), "the edge threshold t must be finite and not negative"
    if indices is None:
        idx = stars_subsamples(N, n_subsamples, subsample_size, seed)
    else:
        idx = utils._subset_indices(indices)
        assert idx.shape[0] >= 1 and idx.shape[1] >= 1, "indices must hold at least one subsample of at least one observation"
        # (the library checks the range on the device route; the host route indexes numpy arrays, which would wrap)
        assert idx.min() >= 0 and idx.max() < N, f"indices must lie in [0, {N})"
    B, b = idx.shape
    L = lam.size
    per = L if lambdas_per_batch is None else max(1, int(lambdas_per_batch))
    route = "set_kendall_subsets" if kendall else ("set_mixed_subsets" if mixed else "set_data_subsets")
    on_device = hasattr(_solver.ENGINE, route) and \
        hasattr(_solver.ENGINE, "neighborhood_stability" if mb else "edge_stability") and \
        (not project or hasattr(_solver.ENGINE, "project_S"))
    capped = 0
    eye = np.eye(p)
    NUM = np.zeros(L, dtype=np.int64)
    failed = np.zeros(L, dtype=bool)
    COUNTS = np.zeros((L, p, p), dtype=np.int32) if store_all else None
    THETA = np.zeros((L, B, p, p)) if store_all else None
    types = utils.variable_types(X) if mixed else None          # of all observations: a subsample does not change a type
    if on_device:
        S_host = None
    elif mixed:
        S_host = utils.host_mixed_correlation(X, types, idx)
    elif pairwise:
        S_host = _host_pairwise_covariances(X, idx, center, scale, min_pairs)
    else:
        S_host = utils.host_skeptic_correlation(X, idx) if kendall else _host_subset_covariances(X, idx, center, scale)
    if project and S_host is not None:
        S_host = utils.host_nearest_correlation(S_host)
    for l0 in range(0, L, per):
        sl = slice(l0, min(L, l0 + per))
        nl = sl.stop - sl.start
        lam_k = np.repeat(lam[sl], B)                                   # instance (l - l0) * B + r
        got = {}

        def before(eng):
            if kendall:
                eng.set_kendall_subsets(X, idx)
            elif mixed:
                eng.set_mixed_subsets(X, idx, types=types)
            elif pairwise:
                eng.set_data_subsets(X, idx, center=center, scale=scale, missing='pairwise', min_pairs=min_pairs)
            else:
                eng.set_data_subsets(X, idx, center=center, scale=scale)
            if project:
                eng.project_S(period=B)

        def after(eng, results):
            got['edges'] = eng.edge_stability(B, t, counts=store_all)

        if mb:
            if on_device:
                # a ctx of B instances, shaped by ONE placeholder matrix; `before` writes the subsample matrices into its S
                ph = np.broadcast_to(eye, (B, p, p))
                eng = _solver.ENGINE(ph, ph, ph, np.broadcast_to(np.zeros((p, p)), (B, p, p)))
                try:
                    before(eng)
                    out = eng.neighborhood_stability(lam[sl], rule, tol=tol, t=t, counts=store_all, stack=store_all, **mbw)
                finally:
                    eng.close()
                NUM[sl], status = out['num'], out['status']
                if store_all:
                    COUNTS[sl], THETA[sl] = out['counts'], out['stack']
            else:
                W, inf = utils.host_neighborhood_selection(S_host, lam[sl], rule, tol=tol, return_info=True, **mbw)
                Th = np.ascontiguousarray(np.swapaxes(W, 0, 1))              # (B,nl,p,p) -> (nl,B,p,p)
                cnt, NUM[sl] = _host_edge_counts(Th, t)
                status = np.swapaxes(inf['STATUS'], 0, 1)
                if store_all:
                    COUNTS[sl], THETA[sl] = cnt, Th
            failed[sl] = (status >= 2).any(axis=(1, 2))
            capped += int((status == 1).sum())
            continue
        if on_device:
            # the S argument only shapes the ctx: ONE (p,p) matrix, which the batch hands to the engine as a broadcast view
            # (uploaded once, replicated on the device); `before` then writes the real S there
            res = _sgl_batch_impl(eye, lam_k, eye, None, eye, 1., max_iter, tol, rtol, True,
                                  False, False, None, None, False, None, None, True, ('Theta',) if store_all else (), None,
                                  None, _on_device=(before, after))
            if store_all:
                NUM[sl], COUNTS[sl] = got['edges']
            else:
                NUM[sl] = got['edges']
        else:
            res = _sgl_batch_impl(np.tile(S_host, (nl, 1, 1)), lam_k, eye, None, eye, 1., max_iter, tol, rtol, True, False,
                                  False, None, None, False, None, None, True, None, None, None)
            Th = np.stack([sol['Theta'] for sol, _ in res]).reshape(nl, B, p, p)
            cnt, NUM[sl] = _host_edge_counts(Th, t)
            if store_all:
                COUNTS[sl] = cnt
        if store_all:
            THETA[sl] = np.stack([sol['Theta'] for sol, _ in res]).reshape(nl, B, p, p)
        failed[sl] = np.array([info['status'] == 'solver error' for _, info in res]).reshape(nl, B).any(axis=1)
    pairs = p * (p - 1) // 2
    D = np.array([2 * int(n) / (B * B * pairs) for n in NUM]) if pairs else np.zeros(L)
    D[failed] = np.nan
    if failed.any():
        warnings.warn(f"StARS: a subsample failed at lambda1 = {[float(v) for v in lam[failed]]}; these grid points have no instability "
                      f"and are not chosen", RuntimeWarning, stacklevel=2)
    if capped:
        warnings.warn(f"StARS, method='mb': {capped} (subsample, lambda1, node) units reached a cap of the coordinate descent "
                      f"before tol = {tol}; their coefficients are used as they are", RuntimeWarning, stacklevel=2)
    ix, Dbar = stars_select(D, beta)
    if kendall:
        S_full = utils.skeptic_correlation(X) if on_device else utils.host_skeptic_correlation(X)
    elif mixed:
        S_full = utils.mixed_correlation(X, types) if on_device else utils.host_mixed_correlation(X, types)
    elif pairwise and not on_device:
        S_full = _host_pairwise_covariances(X, np.arange(N)[None], center, scale, min_pairs)[0]
    elif on_device:
        S_full = utils.sample_covariance(X, center=center, scale=scale, **(dict(missing='pairwise', min_pairs=min_pairs) if pairwise else {}))
        S_full = S_full[0] if scale else S_full
    else:
        S_full = _host_subset_covariances(X, np.arange(N)[None], center, scale)[0]
    projection = None
    if project:
        S_full, projection = (utils.nearest_correlation if on_device else utils.host_nearest_correlation)(S_full, return_info=True)
    if mb and not np.all(np.isfinite(S_full)):
        # (the stateless call refuses such a matrix; the subsamples that draw the observation behind it are in FAILED)
        warnings.warn("StARS, method='mb': the matrix of all N observations holds a non-finite value; there is no final fit and "
                      "sol holds NaN", RuntimeWarning, stacklevel=2)
        sol = {'adjacency': np.zeros((p, p), dtype=bool), 'coef': np.full((p, p), np.nan), 'resvar': np.full(p, np.nan),
               'lambda1': lam[ix]}
    elif mb:
        path = utils.neighborhood_selection if on_device else utils.host_neighborhood_selection
        W, inf = path(S_full, lam[:ix + 1], rule, tol=tol, return_info=True, **mbw)
        with np.errstate(invalid='ignore'):
            sol = {'adjacency': (np.abs(W[ix]) >= t) & (W[ix] != 0), 'coef': inf['COEF'][ix],
                   'resvar': inf['RESVAR'][ix], 'lambda1': lam[ix]}
        if refit:
            rf = (utils.neighborhood_refit if on_device else utils.host_neighborhood_refit)(S_full, W[ix], t)
            sol['coef_refit'], sol['resvar_refit'] = rf['COEF'], rf['RESVAR']
            sol['precision'] = utils.neighborhood_precision(rf['COEF'], rf['RESVAR'])[0]
    else:
        sol, _ = _solver.ADMM_SGL(S_full, lam[ix], eye, X_0=eye, tol=tol, rtol=rtol, max_iter=max_iter, verbose=False)
    stats = {'LAMBDA': lam, 'INSTABILITY': D, 'INSTABILITY_MONOTONE': Dbar, 'NUM': [int(n) for n in NUM], 'IX': ix,
             'BEST': {'lambda1': lam[ix]}, 'INDICES': idx, 'subsample_size': b, 'n_subsamples': B,
             'FAILED': [int(l) for l in np.flatnonzero(failed)]}
    if project:
        stats['PROJECTION'] = projection
    if store_all:
        stats['COUNTS'], stats['THETA'] = COUNTS, THETA
    return sol, stats


# -----------------------------------------------------------------------------------------------------------------
# K-fold cross-validation of lambda1 from data: held-out Gaussian likelihood (the default of scikit-learn's
# GraphicalLassoCV and of R's CVglasso).  F folds x L lambdas are F * L independent single problems of one dimension: ONE
# batch, instance l * F + f = fold f at lambda l (the layout of StARS with B = F).  The data go to the device once for the
# train covariances and once for the test covariances; what comes back is four numbers per point.
# -----------------------------------------------------------------------------------------------------------------
def cv_folds(N, n_folds=5, seed=0):
    """``(train (F, N - m), test (F, m))`` int32 with sorted rows, ``m = N // F``: ONE permutation of range(N) from
    ``numpy.random.default_rng([seed, F])``; test fold f is the permuted positions ``f m .. (f + 1) m - 1``, train set f every
    other index (the ``N - F m`` left-over observations included: they are never tested).  Both arrays are rectangular."""
    N, F = int(N), int(n_folds)
    if F < 2:
        raise ValueError(f"n_folds = {F}: cross-validation needs at least 2 folds")
    if F > N:
        raise ValueError(f"n_folds = {F} is more than the N = {N} observations")
    m = N // F
    if m < 2:
        raise ValueError(f"n_folds = {F} leaves m = N // n_folds = {m} observations per test fold: a covariance needs at least 2")
    perm = np.random.default_rng([int(seed), F]).permutation(N)
    test = np.stack([np.sort(perm[f * m:(f + 1) * m]) for f in range(F)]).astype(np.int32)
    train = np.stack([np.setdiff1d(np.arange(N), test[f]) for f in range(F)]).astype(np.int32)
    return train, test


def cv_select(CV, SE, rule='min'):
    """The choice of a cross-validation on the scores ``CV`` (and their standard errors ``SE``) of a grid in descending
    order: the index of the smallest usable CV, a tie going to the larger lambda (the smaller index) -- ``rule='min'`` -- or
    the largest lambda with ``CV[l] <= CV[min] + SE[min]`` -- ``rule='one_se'``.  NaN (a failed point) and +inf (a Theta that
    is not positive definite) are never chosen.  If no lambda is usable: index 0 and a RuntimeWarning."""
    import warnings
    if rule not in ('min', 'one_se'):
        raise ValueError(f"rule = {rule!r}: 'min' or 'one_se'")
    CV = np.asarray(CV, dtype=np.float64).reshape(-1)
    SE = np.asarray(SE, dtype=np.float64).reshape(-1)
    assert CV.size >= 1 and SE.shape == CV.shape
    ok = np.flatnonzero(np.isfinite(CV))
    if ok.size == 0:
        warnings.warn("cross-validation: no lambda1 of the grid has a finite held-out score; the sparsest point of the grid is "
                      "returned. Extend the grid to larger lambda1.", RuntimeWarning, stacklevel=2)
        return 0
    best = int(ok[np.argmin(CV[ok])])                         # (argmin: the first of equal values, i.e. the larger lambda)
    if rule == 'min':
        return best
    band = CV[best] + (SE[best] if np.isfinite(SE[best]) else 0.0)
    return int(ok[CV[ok] <= band][0])


def _host_heldout_scores(Theta, S_test):
    """numpy twin of ``HipEngine.heldout_scores``: Theta (K,p,p), S_test (F,p,p), instance k = fold k % F."""
    import math
    F = S_test.shape[0]
    out = np.zeros((Theta.shape[0], 4))
    for k, T in enumerate(Theta):
        if not np.all(np.isfinite(T)):
            out[k] = np.nan
            continue
        out[k] = (math.fsum((S_test[k % F] * T).ravel()), robust_logdet(T), np.count_nonzero(T), np.linalg.eigvalsh(T).min())
    return out


def cv_search(X, lambda_range, n_folds=5, seed=0, folds=None, rule='min', center=True, scale=False, tol=1e-7, rtol=1e-7,
              max_iter=1000, store_all=False, lambdas_per_batch=None, correlation=None, missing=None, project=False,
              latent=False, lambda1_mask=None, method='glasso', graph_rule='and', refit=True, score='pseudo', t=1e-8,
              weights=None, scaled=False):
    """K-fold cross-validation of lambda1 for the Single Graphical Lasso from observations ``X`` (p,N), variables in rows.
    Returns ``(sol, stats)``.

    * Folds: ``cv_folds(N, n_folds, seed)``, or ``folds = (train (F,a), test (F,m))`` given by the caller.  The grid is used in
      descending order, ``stats['LAMBDA']``.
    * ``Theta[l,f]`` solves ``ADMM_SGL(S_train_f, lambda[l])`` from ``Omega_0 = X_0 = identity``, ``S_train_f =
      numpy.cov(X[:, train[f]], bias=True)`` (without ``center`` the raw second moment); all F * L points run as one batch.
    * ``NLL[l,f] = <S_test_f, Theta[l,f]> - log det Theta[l,f]``: twice the negative log-likelihood per held-out observation,
      up to a constant.  Theta is scored, not Omega: the sparse iterate is the estimate the package returns and the one its
      information criteria (``ebic_single``) score.  A Theta that is not positive definite (``robust_logdet`` = -inf) scores
      +inf and is listed in ``NOT_PD``; a lambda with a point that ended as 'solver error' gets NaN and is listed in ``FAILED``.
    * ``CV[l]`` = mean over the folds, ``SE[l] = std(NLL[l], ddof=1) / sqrt(F)``, ``IX = cv_select(CV, SE, rule)``.
    * ``scale=True``: every variable is divided by its standard deviation over all N observations, once, before the split (the
      folds share one scale); the solution is that of the scaled data and ``stats['scale']`` holds the variances.
    * ``sol``: ``ADMM_SGL`` on the covariance of all N observations at the chosen lambda1 (``stats['BEST']``).

    With the device engine the data are uploaded, the covariances never exist on the host and four numbers per point come
    back (``HipEngine.heldout_scores``); ``store_all`` also returns ``THETA`` (L,F,p,p).  ``lambdas_per_batch`` as in
    ``stars_search``.  An engine without ``set_data_subsets`` / ``heldout_scores`` takes the same batch call on numpy
    covariances and scores on the host (``math.fsum``, ``robust_logdet``).

    Not implemented, each a ValueError: ``correlation=``, ``missing=``, ``project=`` (a held-out Gaussian likelihood against a
    rank matrix is a different estimator), latent variables, a ``lambda1_mask``, multiple-instance data.

    ``method='mb'``: the estimator is Meinshausen-Buhlmann neighbourhood selection and the score the held-out prediction error
    of its regressions -- a different statistic from the held-out likelihood above; the two are not comparable in value.
    Per (lambda, fold): the path on ``S_train_f`` symmetrised by ``graph_rule`` (``'and'`` / ``'or'``); with ``refit`` (the
    default) every node regressed by least squares on its neighbours in that graph (edges: ``|.| >= t``;
    ``utils.neighborhood_refit``), without it the lasso's own coefficients; ``tau_j^2`` the residual variance on the train
    matrix and ``r_j`` the same quadratic form on the test matrix.  ``score='pseudo'``: ``sum_j log tau_j^2 + r_j / tau_j^2``,
    the negative Gaussian pseudo-log-likelihood; ``score='mse'``: ``sum_j r_j``.  Both are summed on the host
    (``utils.mb_cv_scores``); a (lambda, fold) with a node that was not solved (refit status 1-3, a non-finite path) is +inf
    under ``'pseudo'`` and listed in ``NOT_SOLVED``.  ``CV``, ``SE`` and ``IX`` as above.  ``stats`` holds ``SCORE`` (L,F) in
    the place of ``NLL`` and the per-node arrays ``RESVAR``, ``HELDOUT``, ``STATUS`` (L,F,p); ``store_all`` adds ``THETA``, the
    symmetrised stack.  ``sol``: on all N observations at the chosen lambda ``{'adjacency', 'coef', 'resvar', 'lambda1'}`` of
    the path as in ``stars_search``, and with ``refit`` also ``coef_refit``, ``resvar_refit``; ``precision`` is
    ``utils.neighborhood_precision`` of the refit (without ``refit``: of the lasso's own pair).  On the device one ctx of F
    instances holds the train matrices and ``HipEngine.neighborhood_cv`` does the rest; the matrices never exist on the host.
    ``rtol``, ``max_iter`` are not used.  With ``method='glasso'`` nothing of this applies.  ``weights`` ((p,p): row j holds
    node j's penalty weights) and ``scaled`` (the scaled lasso) are those of ``utils.neighborhood_selection``, for
    ``method='mb'`` only (the graphical lasso's per-entry penalties are ``lambda1_mask``): they apply to every fold's path and
    to the final fit, on the device (``ggl_neighborhood_cv_w``) and on the host route; with ``scaled`` and without ``refit``
    ``tau_j^2`` is the scaled lasso's ``sigma_j^2``.  Without them the calls and the bits are what they were."""
    import warnings
    from . import solver as _solver, utils
    from .batch import _late_failures, _sgl_batch_impl
    if method not in ('glasso', 'mb'):
        raise ValueError(f"method = {method!r}: 'glasso' or 'mb'")
    mbw = _mbw_kwargs(method, weights, scaled, X)
    if method == 'mb':
        if graph_rule not in ('and', 'or'):
            raise ValueError(f"graph_rule = {graph_rule!r}: 'and' or 'or'")
        if score not in ('pseudo', 'mse'):
            raise ValueError(f"score = {score!r}: 'pseudo' or 'mse'")
        if not (np.isfinite(t) and t >= 0):
            raise ValueError(f"t = {t}: the edge threshold must be finite and not negative")
    for name, val in (('correlation', correlation), ('missing', missing)):
        if val is not None:
            raise ValueError(f"cv_search: {name}={val!r} is not implemented: a held-out Gaussian likelihood against such a matrix "
                             f"is a different estimator")
    if project:
        raise ValueError("cv_search: project=True is not implemented: a held-out Gaussian likelihood against a projected matrix "
                         "is a different estimator")
    if latent:
        raise ValueError("cv_search: latent variables are not implemented")
    if lambda1_mask is not None:
        raise ValueError("cv_search: a lambda1_mask is not implemented")
    if isinstance(X, (list, tuple, dict)) or np.ndim(X) != 2:
        raise ValueError("cv_search: data must be ONE (p,N) array with variables in rows; multiple-instance (GGL/FGL) problems "
                         "are not implemented")
    if rule not in ('min', 'one_se'):
        raise ValueError(f"rule = {rule!r}: 'min' or 'one_se'")
    X = np.ascontiguousarray(X, dtype=np.float64)
    p, N = X.shape
    lam = np.sort(np.atleast_1d(np.asarray(lambda_range, dtype=np.float64)).reshape(-1))[::-1].copy()
    assert lam.size >= 1 and np.all(lam > 0), "lambda1 should be positive"
    if folds is None:
        train, test = cv_folds(N, n_folds, seed)
    else:
        train, test = (utils._subset_indices(a) for a in folds)
        assert train.shape[0] == test.shape[0] >= 1, "folds = (train, test) must hold the same number of rows"
        assert train.shape[1] >= 1 and test.shape[1] >= 1, "every fold needs at least one train and one test observation"
        # (the library checks the range on the device route; the host route indexes numpy arrays, which would wrap)
        assert min(train.min(), test.min()) >= 0 and max(train.max(), test.max()) < N, f"folds must lie in [0, {N})"
    F, L = test.shape[0], lam.size
    var = None
    if scale:
        var = X.var(axis=1) if center else (X * X).mean(axis=1)
        for i in np.flatnonzero(~(var > 0)):
            raise ValueError(f"cv_search: variable {int(i)} is constant over the N = {N} observations (variance {var[i]}): "
                             f"it cannot be scaled")
        X = np.ascontiguousarray(X / np.sqrt(var)[:, None])
    per = L if lambdas_per_batch is None else max(1, int(lambdas_per_batch))
    if method == 'mb':
        return _cv_search_mb(X, lam, train, test, rule, graph_rule, bool(refit), score, float(t), center, var, tol, store_all, per,
                             mbw)
    on_device = hasattr(_solver.ENGINE, "set_data_subsets") and hasattr(_solver.ENGINE, "heldout_scores")
    eye = np.eye(p)
    OUT = np.zeros((L, F, 4))
    failed = np.zeros(L, dtype=bool)
    THETA = np.zeros((L, F, p, p)) if store_all else None
    if not on_device:
        S_train = _host_subset_covariances(X, train, center, False)
        S_test = _host_subset_covariances(X, test, center, False)
    for l0 in range(0, L, per):
        sl = slice(l0, min(L, l0 + per))
        nl = sl.stop - sl.start
        lam_k = np.repeat(lam[sl], F)                                   # instance (l - l0) * F + f
        got = {}

        def before(eng):
            eng.set_data_subsets(X, train, center=center)

        def after(eng, results):
            got['scores'] = eng.heldout_scores(X, test, center=center)
            _late_failures(eng, results, 1)        # (the eigenvalues of the statistics may mark a point)

        if on_device:
            # (the S argument only shapes the ctx, as in stars_search: `before` writes the real S on the device)
            res = _sgl_batch_impl(eye, lam_k, eye, None, eye, 1., max_iter, tol, rtol, True,
                                  False, False, None, None, False, None, None, True, ('Theta',) if store_all else (), None,
                                  None, _on_device=(before, after))
            OUT[sl] = got['scores'].reshape(nl, F, 4)
        else:
            res = _sgl_batch_impl(np.tile(S_train, (nl, 1, 1)), lam_k, eye, None, eye, 1., max_iter, tol, rtol, True, False,
                                  False, None, None, False, None, None, True, None, None, None)
            OUT[sl] = _host_heldout_scores(np.stack([sol['Theta'] for sol, _ in res]), S_test).reshape(nl, F, 4)
        if store_all:
            THETA[sl] = np.stack([sol['Theta'] for sol, _ in res]).reshape(nl, F, p, p)
        failed[sl] = np.array([info['status'] == 'solver error' for _, info in res]).reshape(nl, F).any(axis=1)
    with np.errstate(invalid='ignore'):
        NLL = OUT[:, :, 0] - OUT[:, :, 1]                               # (log det = -inf: +inf)
    not_pd = np.isneginf(OUT[:, :, 1]) & ~failed[:, None]
    NLL[not_pd] = np.inf
    NLL[failed] = np.nan
    with np.errstate(invalid='ignore'):
        CV = NLL.mean(axis=1)
        SE = NLL.std(axis=1, ddof=1) / np.sqrt(F) if F > 1 else np.full(L, np.nan)
    if failed.any():
        warnings.warn(f"cross-validation: a fold failed at lambda1 = {[float(v) for v in lam[failed]]}; these grid points have no "
                      f"score and are not chosen", RuntimeWarning, stacklevel=2)
    ix = cv_select(CV, SE, rule)
    if on_device:
        S_full = utils.sample_covariance(X, center=center)
    else:
        S_full = _host_subset_covariances(X, np.arange(N)[None], center, False)[0]
    sol, _ = _solver.ADMM_SGL(S_full, lam[ix], eye, X_0=eye, tol=tol, rtol=rtol, max_iter=max_iter, verbose=False)
    NNZ = OUT[:, :, 2].copy()
    NNZ[failed] = np.nan
    stats = {'LAMBDA': lam, 'NLL': NLL, 'CV': CV, 'SE': SE, 'IX': ix, 'BEST': {'lambda1': lam[ix]}, 'TRAIN': train,
             'TEST': test, 'n_folds': F, 'rule': rule, 'NNZ': NNZ, 'FAILED': [int(l) for l in np.flatnonzero(failed)],
             'NOT_PD': [(int(l), int(f)) for l, f in zip(*np.nonzero(not_pd))]}
    if scale:
        stats['scale'] = var
    if store_all:
        stats['THETA'] = THETA
    return sol, stats


def _cv_search_mb(X, lam, train, test, rule, graph_rule, refit, score, t, center, var, tol, store_all, per, mbw={}):
    """``cv_search(method='mb')`` behind its argument checks: X scaled already, the grid descending."""
    import warnings
    from . import solver as _solver, utils
    p, N = X.shape
    F, L = test.shape[0], lam.size
    on_device = hasattr(_solver.ENGINE, "set_data_subsets") and hasattr(_solver.ENGINE, "neighborhood_cv")
    TAU, R = np.zeros((L, F, p)), np.zeros((L, F, p))
    STATUS = np.zeros((L, F, p), dtype=np.int64)
    THETA = np.zeros((L, F, p, p)) if store_all else None
    if not on_device:
        S_train = _host_subset_covariances(X, train, center, False)
        S_test = _host_subset_covariances(X, test, center, False)
    eye = np.eye(p)
    for l0 in range(0, L, per):
        sl = slice(l0, min(L, l0 + per))
        if on_device:
            ph = np.broadcast_to(eye, (F, p, p))                            # (shapes the ctx, as in stars_search)
            eng = _solver.ENGINE(ph, ph, ph, np.broadcast_to(np.zeros((p, p)), (F, p, p)))
            try:
                eng.set_data_subsets(X, train, center=center)
                out = eng.neighborhood_cv(X, test, lam[sl], graph_rule, tol=tol, t=t, refit=refit, center=center, stack=store_all,
                                          **mbw)
            finally:
                eng.close()
            TAU[sl], R[sl], STATUS[sl] = out['resvar'], out['heldout'], out['status']
            if store_all:
                THETA[sl] = out['stack']
            continue
        W, inf = utils.host_neighborhood_selection(S_train, lam[sl], graph_rule, tol=tol, return_info=True, **mbw)     # (F,nl,..)
        if refit:
            rf = utils.host_neighborhood_refit(S_train, W, t, S_test)
            tau, r, st = rf['RESVAR'], rf['HELDOUT'], rf['STATUS']
        else:
            tau, st = inf['RESVAR'], inf['STATUS']
            r = np.full(tau.shape, np.nan)
            with np.errstate(all='ignore'):
                for f in range(F):
                    for l in range(W.shape[1]):
                        for j in range(p):
                            b = inf['COEF'][f, l][:, j]
                            A = np.flatnonzero(b != 0)
                            r[f, l, j] = utils._host_quad(S_test[f], j, A, b[A])
        TAU[sl], R[sl], STATUS[sl] = (np.swapaxes(a, 0, 1) for a in (tau, r, st))
        if store_all:
            THETA[sl] = np.swapaxes(W, 0, 1)
    bad = (STATUS != 0) if refit else (STATUS >= 2)
    SC = utils.mb_cv_scores(TAU, R, bad, score)
    capped = 0 if refit else int((STATUS == 1).sum())
    if capped:
        warnings.warn(f"cross-validation, method='mb': {capped} (lambda1, fold, node) units reached a cap of the coordinate "
                      f"descent before tol = {tol}; their coefficients are used as they are", RuntimeWarning, stacklevel=3)
    failed = np.isnan(SC).any(axis=1)
    with np.errstate(invalid='ignore'):
        CV = SC.mean(axis=1)
        SE = SC.std(axis=1, ddof=1) / np.sqrt(F) if F > 1 else np.full(L, np.nan)
    ix = cv_select(CV, SE, rule)
    if on_device:
        S_full = utils.sample_covariance(X, center=center)
    else:
        S_full = _host_subset_covariances(X, np.arange(N)[None], center, False)[0]
    path = utils.neighborhood_selection if on_device else utils.host_neighborhood_selection
    W, inf = path(S_full, lam[:ix + 1], graph_rule, tol=tol, return_info=True, **mbw)
    with np.errstate(invalid='ignore'):
        sol = {'adjacency': (np.abs(W[ix]) >= t) & (W[ix] != 0), 'coef': inf['COEF'][ix], 'resvar': inf['RESVAR'][ix],
               'lambda1': lam[ix]}
    if refit:
        rf = (utils.neighborhood_refit if on_device else utils.host_neighborhood_refit)(S_full, W[ix], t)
        sol['coef_refit'], sol['resvar_refit'] = rf['COEF'], rf['RESVAR']
        sol['precision'] = utils.neighborhood_precision(rf['COEF'], rf['RESVAR'])[0]
    else:
        sol['precision'] = utils.neighborhood_precision(sol['coef'], sol['resvar'])[0]
    stats = {'LAMBDA': lam, 'SCORE': SC, 'CV': CV, 'SE': SE, 'IX': ix, 'BEST': {'lambda1': lam[ix]}, 'TRAIN': train,
             'TEST': test, 'n_folds': F, 'rule': rule, 'method': 'mb', 'graph_rule': graph_rule, 'refit': refit, 'score': score,
             'RESVAR': TAU, 'HELDOUT': R, 'STATUS': STATUS, 'FAILED': [int(l) for l in np.flatnonzero(failed)],
             'NOT_SOLVED': [(int(l), int(f)) for l, f in zip(*np.nonzero(bad.any(axis=2)))]}
    if var is not None:
        stats['scale'] = var
    if store_all:
        stats['THETA'] = THETA
    return sol, stats


def bandwidth_search(X, bandwidths, rule='min', times=None, kernel='gaussian', cutoff=2.0 ** -53, center=True, ridge=0.0,
                     eval_index=None, device=0, chunk=0):
    """The bandwidth of a kernel-smoothed covariance stack (``utils.kernel_covariance``, ``glasso_problem.from_time_series``)
    chosen from the series itself by the leave-one-out Gaussian predictive likelihood (Yin, Geng, Li, Wang 2010; Monti et al.
    2014).  Returns ``(h, stats)``.

    * The grid is used in descending order, widest first: ``stats['BANDWIDTH']``.
    * ``SCORE[b,r]`` = ``utils.loo_bandwidth_scores``: minus twice the log density (up to ``p log 2 pi``) of the evaluation
      sample r under the weighted mean and covariance of all OTHER samples at bandwidth b; ``CV = SCORE.mean(axis=1)``,
      ``SE = SCORE.std(axis=1, ddof=1) / sqrt(M)``.
    * ``IX = cv_select(CV, SE, rule)``: the smallest CV (``'min'``), or the widest bandwidth within one standard error of it
      (``'one_se'``, the smoother estimate).  A bandwidth with a covariance that is not positive definite has ``CV = +inf``, is
      never chosen and its ``(bandwidth index, sample)`` pairs are listed in ``NOT_PD``; ``ridge`` > 0 regularises them.
    * ``N_EFF`` (H,): the smallest Kish effective sample size over the weight rows of each bandwidth -- below p the covariances
      are singular.  ``EVAL``: the evaluation samples.

    ``times``, ``kernel``, ``cutoff``, ``center``, ``ridge``, ``eval_index``, ``chunk`` as ``utils.loo_bandwidth_scores``.  With the
    device engine X goes up once per bandwidth and the M covariances of a bandwidth never leave the device; an engine without
    the weighted-covariance route takes the numpy twin."""
    from . import solver as _solver, utils
    if rule not in ('min', 'one_se'):
        raise ValueError(f"rule = {rule!r}: 'min' or 'one_se'")
    h = np.sort(np.atleast_1d(np.asarray(bandwidths, dtype=np.float64)).reshape(-1))[::-1].copy()
    host = not hasattr(_solver.ENGINE, "set_data_weighted")
    SCORE, STATUS, N_EFF, ev = utils._loo_scores(X, h, times, kernel, cutoff, center, ridge, eval_index, device, chunk, host)
    M = SCORE.shape[1]
    with np.errstate(invalid='ignore'):
        CV = SCORE.mean(axis=1)
        SE = SCORE.std(axis=1, ddof=1) / np.sqrt(M) if M > 1 else np.full(h.size, np.nan)
    ix = cv_select(CV, SE, rule)
    stats = {'BANDWIDTH': h, 'SCORE': SCORE, 'CV': CV, 'SE': SE, 'IX': ix, 'BEST': {'bandwidth': float(h[ix])},
             'NOT_PD': [(int(b), int(ev[r])) for b, r in zip(*np.nonzero(STATUS >= 0))], 'N_EFF': N_EFF, 'EVAL': ev,
             'rule': rule}
    return float(h[ix]), stats


# -----------------------------------------------------------------------------------------------------------------
# Joint neighbourhood selection of K instances (utils.joint_neighborhood_selection): the (lambda1, lambda2) grid
# in ONE device call with the refit, only tables downloaded, scored on the host by the extended BIC of every regression.
# -----------------------------------------------------------------------------------------------------------------
def joint_neighborhood_score(refit_resvar, degree, N, p, method='eBIC', gamma=0.1, bad=None):
    """(...) scores from ``refit_resvar`` and ``degree`` (...,K,p): ``sum_k sum_j [ N_k log tau_jk^2 + deg_jk (log N_k + 2 gamma
    log(p - 1)) ]`` -- the extended BIC of each regression (Chen & Chen 2008) summed over nodes and instances; ``'BIC'``:
    ``gamma = 0``; ``'AIC'``: ``2 deg`` in place of ``deg log N_k``.  NaN where ``bad`` (...) is set or a ``tau^2`` is not positive."""
    assert method in ('eBIC', 'BIC', 'AIC'), f"method = {method!r}: 'eBIC', 'BIC' or 'AIC'"
    tau, deg = np.asarray(refit_resvar, dtype=np.float64), np.asarray(degree, dtype=np.float64)
    K = tau.shape[-2]
    Nk = np.broadcast_to(np.asarray(N, dtype=np.float64).reshape(-1), (K,))[:, None]
    per_edge = 2.0 if method == 'AIC' else np.log(Nk)
    if method == 'eBIC' and p > 1:
        per_edge = per_edge + 2.0 * float(gamma) * np.log(p - 1.0)
    with np.errstate(all='ignore'):
        score = (Nk * np.log(tau) + deg * per_edge).sum(axis=(-1, -2))
        score = np.where(np.all(tau > 0, axis=(-1, -2)), score, np.nan)
    if bad is not None:
        score = np.where(np.asarray(bad, dtype=bool), np.nan, score)
    return score


def joint_neighborhood_search(S, N, lambda1_range, lambda2_range, rule='and', method='eBIC', gamma=0.1, instance_weights=None,
                              host=None, **kw):
    """Pick ``(lambda1, lambda2)`` of ``utils.joint_neighborhood_selection`` on a grid: one device call with the refit (only
    tables come back), then ``joint_neighborhood_score`` on the host from the refit's residual variances and degrees.  A grid
    point with any node of non-zero path or refit status scores NaN and is never chosen.  ``N``: one number or (K,).  ``kw``:
    ``tol``, ``max_sweeps``, ``t``, ``device``.  ``host``: through the numpy twin (default: when the engine has no
    neighbourhood route).

    Returns ``(sol, stats)``.  ``stats``: ``SCORE`` (L1,L2), ``IX`` (i1, i2), ``BEST`` ``{'lambda1', 'lambda2'}``, ``LAMBDA1``
    (descending), ``LAMBDA2``, ``STATUS``, ``SWEEPS``, ``NEWTON`` (L1,L2,p), ``REFIT_STATUS``, ``DEGREE`` (L1,L2,K,p).  ``sol``:
    ``coef`` (K,p,p) and ``resvar`` (K,p) of the refit at the chosen point, ``adjacency`` (K,p,p), ``common_adjacency`` (p,p:
    the edges present in every instance), ``precision`` (K,p,p: ``utils.joint_neighborhood_precision``), ``W`` the symmetrised
    lasso coefficients.  They come from one further call, the chosen ``lambda2``'s chain down to the chosen ``lambda1``, whose
    bits are that point's part of the grid call; only the chosen point's two coefficient stacks are downloaded."""
    return _joint_search('group', S, N, lambda1_range, lambda2_range, rule, method, gamma, instance_weights, host, kw)


def _joint_search(coupling, S, N, lambda1_range, lambda2_range, rule, method, gamma, instance_weights, host, kw):
    """``joint_neighborhood_search`` (``coupling='group'``) and ``fused_neighborhood_search`` (``'fused'``)."""
    from . import solver as _solver, utils
    who = 'fused_neighborhood_search' if coupling == 'fused' else 'joint_neighborhood_search'
    assert rule in ('and', 'or'), f"rule = {rule!r}: 'and' or 'or'"
    assert method in ('eBIC', 'BIC', 'AIC'), f"method = {method!r}: 'eBIC', 'BIC' or 'AIC'"
    assert 0 <= gamma <= 1, "gamma needs to be chosen as a parameter in [0,1]."
    unknown = set(kw) - {'tol', 'max_sweeps', 't', 'device'}
    assert not unknown, f"{who}: unknown arguments {sorted(unknown)}"
    tol, max_sweeps, t, device = kw.get('tol', 1e-7), kw.get('max_sweeps', 10000), kw.get('t', 1e-8), kw.get('device', 0)
    if host is None:
        host = not hasattr(_solver.ENGINE, "neighborhood_stability")
    Sm, l1, l2, om = utils._mbj_args(S, lambda1_range, lambda2_range, rule, instance_weights, tol, max_sweeps, True, t, coupling)
    K, p = Sm.shape[0], Sm.shape[1]
    Nk = np.asarray(N, dtype=np.float64).reshape(-1)
    assert Nk.size in (1, K) and np.all(Nk >= 1), f"N must be one number or one per instance ({K}), each at least 1"
    out = utils._joint_run(Sm, l1, l2, om, rule, tol, max_sweeps, True, t, device, host, want_coef=False, coupling=coupling)
    status, rstatus = out['INFO'][..., 1].astype(np.int64), out['REFIT_INFO'][..., 1].astype(np.int64)
    degree = out['REFIT_INFO'][..., 0].astype(np.int64)
    bad = np.any(status != 0, axis=-1) | np.any(rstatus != 0, axis=(-1, -2))
    score = joint_neighborhood_score(out['REFIT_RESVAR'], degree, Nk, p, method, gamma, bad)
    if np.all(np.isnan(score)):
        raise ValueError(f"{who}: no grid point finished with every node's status 0")
    i1, i2 = (int(v) for v in np.unravel_index(int(np.nanargmin(score)), score.shape))
    stats = {'SCORE': score, 'IX': (i1, i2), 'BEST': {'lambda1': float(l1[i1]), 'lambda2': float(l2[i2])}, 'LAMBDA1': l1,
             'LAMBDA2': l2, 'STATUS': status, 'SWEEPS': out['INFO'][..., 0].astype(np.int64),
             'NEWTON': out['INFO'][..., 2].astype(np.int64), 'REFIT_STATUS': rstatus, 'DEGREE': degree, 'method': method}
    fin = utils._joint_run(Sm, l1[:i1 + 1], l2[i2:i2 + 1], om, rule, tol, max_sweeps, True, t, device, host, last_only=True,
                           coupling=coupling)
    W, coef, resvar = fin['W'][0], fin['REFIT_COEF'][0], fin['REFIT_RESVAR'][i1, 0]
    with np.errstate(invalid='ignore'):
        adj = (np.abs(W) >= t) & ~np.eye(p, dtype=bool)[None]
    import warnings
    with warnings.catch_warnings():
        warnings.simplefilter('ignore', RuntimeWarning)                     # not positive definite by construction (utils)
        Theta, lmin = utils.joint_neighborhood_precision(coef, resvar)
    sol = {'coef': coef, 'resvar': resvar, 'W': W, 'adjacency': adj, 'common_adjacency': np.all(adj, axis=0), 'precision': Theta,
           'lambda_min': lmin, 'lambda1': float(l1[i1]), 'lambda2': float(l2[i2])}
    if coupling == 'fused':
        sol['changed_edges'] = np.sum(np.triu(adj[1:] != adj[:-1], 1), axis=(1, 2)).astype(np.int64)
    return sol, stats


def fused_neighborhood_search(S, N, lambda1_range, lambda2_range, rule='and', method='eBIC', gamma=0.1, instance_weights=None,
                              host=None, **kw):
    """Pick ``(lambda1, lambda2)`` of ``utils.fused_neighborhood_selection`` (K ordered instances, ``lambda2`` on the
    differences between consecutive ones) on a grid, by the table of ``joint_neighborhood_search``: the eBIC / BIC / AIC of the
    regressions REFITTED on the selected graphs.  The refit is per instance and unfused, so ``lambda2`` acts on the score through
    the supports it produces only, never through shrinkage of the differences.  Arguments, ``stats`` and ``sol`` as there
    (``NEWTON`` is all 0); ``sol`` additionally carries ``changed_edges`` (K-1,): the number of edges that differ between the
    graphs of instance k and k + 1."""
    return _joint_search('fused', S, N, lambda1_range, lambda2_range, rule, method, gamma, instance_weights, host, kw)
