"""The refit of neighbourhood selection on the device (csrc/mb_refit.hip behind ``ggl_neighborhood_refit`` and
``ggl_neighborhood_cv``): the checks of tests/mbrefit_ref.py against the longdouble comparison value on the graphs of the path
and on engineered graphs (every boundary of the kernel's two degree bins, the cap), the statuses, the bits, the refusals of the
C ABI, and ``cv_search(method='mb')`` / ``stars_search(refit=True)`` / ``glasso_problem.neighborhood_selection`` end to end."""
import warnings

import numpy as np
import pytest

import mb_ref
import mbrefit_ref as ref

pytestmark = pytest.mark.gpu

T_EDGE = 1e-8
TOL = 1e-7
SIZES = (1, 2, 3, 5, 17, 63, 64, 65, 130, 257)
WAVE_DEG = 32                      # csrc/mb_refit.hip: a wave per unit up to this degree, a workgroup per unit above


@pytest.fixture(scope="module")
def cap():
    from gglasso_amd import utils
    c = utils.mb_refit_max_degree()
    assert c >= 128 and c == utils.MB_REFIT_MAX_DEG
    return c


@pytest.fixture(scope="module")
def device():
    from gglasso_amd import utils
    cache = {}

    def run(p):
        if p not in cache:
            S, T, W = mb_ref.stack(p), ref.heldout_stack(p), ref.graphs(p)
            cache[p] = (S, T, W, utils.neighborhood_refit(S, W, T_EDGE, T))
        return cache[p]
    return run


@pytest.mark.parametrize("p", SIZES)
def test_device_against_the_comparison_value(device, p):
    """AND, OR and raw supports of the path along the grid, three seeds as one stack, T of other seeds: the list, the
    normal-equation residual, the distance to the solution, tau^2 and r at the returned coefficients."""
    from gglasso_amd import utils
    S, T, W, out = device(p)
    assert out['COEF'].shape == W.shape and out['RESVAR'].shape == W.shape[:3] == out['HELDOUT'].shape
    ref.check_stack(S, T, W, T_EDGE, out, "device")
    i = np.arange(p)
    assert np.all(out['COEF'][..., i, i] == 0)
    if p <= 65:
        twin = utils.host_neighborhood_refit(S, W, T_EDGE, T)
        assert np.array_equal(twin['DEGREE'], out['DEGREE']) and np.array_equal(twin['STATUS'], out['STATUS'])


@pytest.mark.parametrize("p", (17, 65))
def test_device_bits(device, p):
    """Two calls; T = S; a matrix of the stack alone; some graphs of the stack alone."""
    from gglasso_amd import utils
    S, T, W, out = device(p)
    again = utils.neighborhood_refit(S, W, T_EDGE, T)
    assert all(np.array_equal(out[k], again[k]) for k in out)
    same = utils.neighborhood_refit(S, W, T_EDGE, S)
    assert np.array_equal(same['HELDOUT'], same['RESVAR']) and np.array_equal(same['COEF'], out['COEF'])
    one = utils.neighborhood_refit(S[1], W[1], T_EDGE, T[1])
    assert all(np.array_equal(one[k], out[k][1]) for k in out)
    some = utils.neighborhood_refit(S, W[:, 3:6], T_EDGE, T)
    assert all(np.array_equal(some[k], out[k][:, 3:6]) for k in out)
    single = utils.neighborhood_refit(S[2], W[2, 7], T_EDGE)
    assert single['HELDOUT'] is None and np.array_equal(single['COEF'], out['COEF'][2, 7])
    assert np.array_equal(single['RESVAR'], out['RESVAR'][2, 7])


def test_device_engineered_graphs():
    from gglasso_amd import utils
    p = 17
    S, T = mb_ref.case(p, 0), mb_ref.case(p, 7)
    out = utils.neighborhood_refit(S, np.zeros((p, p)), T_EDGE, T)         # the empty graph
    assert not out['COEF'].any() and not out['DEGREE'].any() and not out['STATUS'].any()
    assert np.array_equal(out['RESVAR'], np.diagonal(S)) and np.array_equal(out['HELDOUT'], np.diagonal(T))
    Wn = np.zeros((p, p))                                                   # a NaN, a value below t, a sign, t itself
    Wn[3, 5], Wn[3, 6], Wn[3, 7], Wn[3, 8] = np.nan, 0.5e-8, -1.0, 1e-8
    out = utils.neighborhood_refit(S, Wn, T_EDGE)
    assert out['DEGREE'][3] == 2 and sorted(np.flatnonzero(out['COEF'][:, 3])) == [7, 8]
    Wa = np.zeros((p, p))                                                   # not symmetric: 2 regresses on 9 and 11, 9 on nothing
    Wa[2, 9] = Wa[2, 11] = 1.0
    out = utils.neighborhood_refit(S, Wa, T_EDGE, T)
    assert out['DEGREE'][2] == 2 and out['DEGREE'][9] == 0 and out['COEF'][2, 9] == 0
    ref.check_stack(S[None], T[None], Wa[None, None], T_EDGE, {k: v[None, None] for k, v in out.items()}, "device, not symmetric")


@pytest.mark.parametrize("p", (17, 65, 129))
def test_device_complete_graph_is_the_inverse(cap, p):
    """Every piece at once: the precision matrix of the complete graph's refit is inv(S), within the derived bound.  p = 129
    (cap + 1) puts every node at the cap, in the workgroup bin."""
    from gglasso_amd import utils
    assert cap == 128
    S = mb_ref.case(p, 1)
    out = utils.neighborhood_refit(S, np.ones((p, p)), T_EDGE, S)
    assert np.all(out['DEGREE'] == p - 1) and not out['STATUS'].any() and np.array_equal(out['HELDOUT'], out['RESVAR'])
    Theta, lmin = utils.neighborhood_precision(out['COEF'], out['RESVAR'])
    assert np.array_equal(Theta, Theta.T) and lmin > 0
    err = np.abs(Theta.astype(ref.LD) - ref.precision_reference(S)).astype(np.float64)
    bound = ref.precision_bound(S, out['COEF'], out['RESVAR'])
    print(f"device, complete graph p={p}: {float((err / bound).max()):.3f} of the bound")
    assert np.all(err <= bound)


def test_device_bin_boundaries_and_the_cap(cap):
    """Stars whose hub has 31, 32, 33 neighbours (the wave bin ends at 32) and cap - 1, cap, cap + 1: one stack.  Only the hub
    of cap + 1 is refused, with status 3."""
    from gglasso_amd import utils
    p = cap + 3
    S, T = mb_ref.case(p, 2), mb_ref.case(p, 8)
    degs = (WAVE_DEG - 1, WAVE_DEG, WAVE_DEG + 1, cap - 1, cap, cap + 1)
    W = np.stack([ref.star(p, 1, d) for d in degs])
    out = utils.neighborhood_refit(S, W, T_EDGE, T)
    assert list(out['DEGREE'][:, 1]) == list(degs)
    assert list(out['STATUS'][:, 1]) == [0, 0, 0, 0, 0, 3] and not np.delete(out['STATUS'], 1, axis=1).any()
    g = len(degs) - 1
    assert np.all(np.isnan(np.delete(out['COEF'][g][:, 1], 1))) and out['COEF'][g][1, 1] == 0
    assert np.isnan(out['RESVAR'][g, 1]) and np.isnan(out['HELDOUT'][g, 1])
    worst = np.zeros(4)
    for gi in range(len(degs)):
        for j in range(p):
            if gi == g and j == 1:
                continue
            worst = np.maximum(worst, ref.check_node(S, T, W[gi, j], j, T_EDGE, out['COEF'][gi][:, j], out['RESVAR'][gi, j],
                                                     out['HELDOUT'][gi, j], int(out['DEGREE'][gi, j]), 0, f"star {degs[gi]}"))
    print(f"device, stars: residual {worst[0]:.3f}, distance {worst[1]:.3f}, resvar {worst[2]:.3f}, heldout {worst[3]:.3f}")
    alone = utils.neighborhood_refit(S, W[4], T_EDGE, T)                   # the workgroup bin's bits do not depend on the stack
    assert all(np.array_equal(alone[k], out[k][4]) for k in out)


def test_device_statuses_one_and_two():
    from gglasso_amd import utils
    p = 9
    S = mb_ref.case(p, 0).copy()
    S[4, :], S[:, 4] = S[3, :], S[:, 3]                                      # variable 4 = variable 3
    S[4, 4] = S[3, 3]
    W = np.zeros((p, p))
    W[0, [3, 4, 6]] = 1.0                                                    # node 0 holds both
    W[3, [0, 6]] = W[4, [0, 6]] = W[6, [0, 3]] = 1.0
    T = mb_ref.case(p, 7)
    out = utils.neighborhood_refit(S, W, T_EDGE, T)
    assert list(out['STATUS']) == [1, 0, 0, 0, 0, 0, 0, 0, 0] and list(out['DEGREE']) == [3, 0, 0, 2, 2, 0, 2, 0, 0]
    assert np.all(np.isnan(np.delete(out['COEF'][:, 0], 0))) and out['COEF'][0, 0] == 0
    assert np.isnan(out['RESVAR'][0]) and np.isnan(out['HELDOUT'][0])
    assert np.all(np.isfinite(out['COEF'][:, 1:])) and np.all(np.isfinite(out['RESVAR'][1:]))
    for j in (3, 4, 6):
        ref.check_node(S, T, W[j], j, T_EDGE, out['COEF'][:, j], out['RESVAR'][j], out['HELDOUT'][j], 2, 0, "beside the duplicate")
    Tn = T.copy()
    Tn[6, 3] = Tn[3, 6] = np.inf
    out = utils.neighborhood_refit(mb_ref.case(p, 0), W, T_EDGE, Tn)
    assert list(out['STATUS']) == [2, 0, 0, 2, 0, 0, 2, 0, 0]
    assert np.isnan(out['HELDOUT'][[0, 3, 6]]).all() and np.isfinite(out['HELDOUT'][[1, 2, 4, 5, 7, 8]]).all()
    twin = utils.host_neighborhood_refit(mb_ref.case(p, 0), W, T_EDGE, Tn)
    assert np.array_equal(twin['STATUS'], out['STATUS'])


def test_device_wide_matrix():
    """p = 513 (nine steps of the list's 64-lane scan, the last one ragged) with a two-lambda graph."""
    from gglasso_amd import utils
    p = 513
    S, T = mb_ref.case(p, 0), mb_ref.case(p, 7)
    W = utils.neighborhood_selection(S, (0.2, 0.1), 'and', tol=TOL)
    out = utils.neighborhood_refit(S, W, T_EDGE, T)
    assert out['DEGREE'].max() >= 2 and out['DEGREE'][:, -1].max() >= 1
    ref.check_stack(S[None], T[None], W[None], T_EDGE, {k: v[None] for k, v in out.items()}, "device")


def _refit_call(S, W, T=None, t=T_EDGE, M=None, G=None, p=None, held=True, null=()):
    """One raw ``ggl_neighborhood_refit`` call with sentinel-filled outputs: (rc, message, coef, resvar, heldout, info)."""
    from gglasso_amd import _lib
    lib = _lib.load()
    S, W = np.ascontiguousarray(S, dtype=np.float64), np.ascontiguousarray(W, dtype=np.float64)
    T = None if T is None else np.ascontiguousarray(T, dtype=np.float64)
    n = W.shape[0] * W.shape[1] * W.shape[2]
    C, R, H = np.full(n * W.shape[2], -7.5), np.full(n, -7.5), np.full(n, -7.5)
    I = np.full(n * 2, -7, dtype=np.int32)
    arg = lambda name, a: None if name in null else a
    rc = lib.ggl_neighborhood_refit(0, W.shape[0] if M is None else M, W.shape[2] if p is None else p, arg('S', _lib.ptr(S)),
                                    W.shape[1] if G is None else G, arg('W', _lib.ptr(W)), t, _lib.ptr(T),
                                    arg('coef', _lib.ptr(C)), arg('resvar', _lib.ptr(R)), _lib.ptr(H) if held else None,
                                    arg('info', I.ctypes.data_as(_lib._ip)))
    return rc, _lib.last_error(), C, R, H, I


def test_refusals_write_nothing():
    from gglasso_amd import _lib
    S, T = mb_ref.stack(5).copy(), ref.heldout_stack(5)
    W = np.ones((3, 2, 5, 5))
    bad_S, neg_d = S.copy(), S.copy()
    bad_S[1, 2, 3] = np.inf
    neg_d[2, 4, 4] = -1.0
    cases = {
        "M": dict(M=0), "G": dict(G=0), "p": dict(p=0), "p max": dict(p=2049), "S NULL": dict(null=('S',)),
        "W NULL": dict(null=('W',)), "coef NULL": dict(null=('coef',)), "resvar NULL": dict(null=('resvar',)),
        "info NULL": dict(null=('info',)), "heldout without T": dict(T=None), "t < 0": dict(t=-1e-9), "t nan": dict(t=np.nan),
        "t inf": dict(t=np.inf), "S inf": dict(S=bad_S), "diagonal": dict(S=neg_d),
    }
    for name, kw in cases.items():
        args = dict(S=S, W=W, T=T)
        args.update(kw)
        rc, msg, C, R, H, I = _refit_call(**args)
        assert rc == _lib.E_ARG, (name, rc, msg)
        assert np.all(C == -7.5) and np.all(R == -7.5) and np.all(H == -7.5) and np.all(I == -7), name
        if name == "S inf":
            assert "matrix 1" in msg and "(2, 3)" in msg, msg
        if name == "diagonal":
            assert "matrix 2" in msg and "variable 4" in msg, msg
        if name == "heldout without T":
            assert "heldout_out" in msg, msg
    rc, msg, C, R, H, I = _refit_call(S, W, T)
    assert rc == 0 and not np.any(C == -7.5) and not np.any(R == -7.5) and not np.any(H == -7.5) and not np.any(I == -7)
    rc, msg, C, R, H, I = _refit_call(S, W, T, held=False)                  # T without heldout_out: not an error, r not written
    assert rc == 0 and np.all(H == -7.5) and not np.any(R == -7.5)
    lim = (np.zeros(2, dtype=np.int32))
    _lib.load().ggl_mb_refit_limits(lim.ctypes.data_as(_lib._ip))
    assert list(lim) == [128, 2048]


# ---- end to end: p = 17, N = 120, F = 3, L = 4 -------------------------------------------------------------------------
def _cv_inputs():
    from gglasso_amd import model_selection as ms
    X = mb_ref.stars_data()
    return X, np.array(mb_ref.GRID), ms.cv_folds(X.shape[1], 3, 4)


def _score_reference(S_tr, S_te, nodes):
    """(score, bound) of one (lambda, fold) under 'pseudo' from the comparison value: ``nodes`` yields (j, A, beta, tau^2).
    With beta None the coefficients are the reference's own solve, and the device's tau^2 and r may differ from the
    reference's by steps 2-4 of mbrefit_ref (for r: the gradient of q(T; .) at beta* times the distance, plus the second-order
    term).  With beta given (the lasso's own, whose tau^2 -- the path's, checked by test_gpu_neighborhood -- comes with it)
    only r is new, and differs by step 3."""
    total, bound = ref.LD(0), 0.0
    for j, A, b, tau_given in nodes:
        solved = b is None
        bs = ref.solve_node(S_tr, j, A) if solved else b
        tau, r = ref.quad(S_tr, j, A, bs), ref.quad(S_te, j, A, bs)
        b64 = np.asarray(bs, dtype=np.float64)
        dt, dr = ref.quad_bound(S_tr, j, A, b64), ref.quad_bound(S_te, j, A, b64)
        if solved and A.size:
            D, _, lmax = ref.distance_bound(S_tr, j, A, b64 * (1 + 1e-6), bs)
            grad = 2 * float(np.linalg.norm((ref.residual(S_te, j, A, bs)).astype(np.float64)))
            dt += lmax * D * D
            dr += grad * D + float(np.linalg.eigvalsh(S_te[np.ix_(A, A)])[-1]) * D * D
        elif not solved:
            tau, dt = tau_given, 0.0
        tau, r = float(tau), float(r)
        lo = tau - dt
        total += np.log(ref.LD(tau)) + ref.LD(r) / ref.LD(tau)
        bound += dt / lo + dr / lo + abs(r) * dt / (tau * lo) + 4 * ref.U * (abs(np.log(tau)) + abs(r / tau))
    return float(total), bound


@pytest.mark.parametrize("refit", (True, False))
def test_cv_search_on_the_device(refit):
    """The per-node arrays recomputed by the comparison value from the stack the device returns; the scores and the choice."""
    from gglasso_amd import model_selection as ms, utils
    X, lam, (train, test) = _cv_inputs()
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        sol, st = ms.cv_search(X, lam, n_folds=3, seed=4, method='mb', graph_rule='or', refit=refit, tol=TOL, store_all=True)
    p, F, L = 17, 3, 4
    assert st['THETA'].shape == (L, F, p, p) and not st['STATUS'].any() and st['FAILED'] == [] and st['NOT_SOLVED'] == []
    S_tr, S_te = utils.sample_covariance_subsets(X, train), utils.sample_covariance_subsets(X, test)
    Wd, infd = utils.neighborhood_selection(S_tr, lam, 'or', tol=TOL, return_info=True)
    assert np.array_equal(st['THETA'], np.swapaxes(Wd, 0, 1))               # the ctx path has the stateless path's bits
    SC, B = np.zeros((L, F)), np.zeros((L, F))
    for l in range(L):
        for f in range(F):
            if refit:
                nodes = [(j, ref.neighbours(st['THETA'][l, f, j], j, T_EDGE), None, None) for j in range(p)]
            else:
                raw = infd['COEF'][f, l]
                nodes = [(j, np.flatnonzero(raw[:, j]), raw[np.flatnonzero(raw[:, j]), j], infd['RESVAR'][f, l, j]) for j in range(p)]
            SC[l, f], B[l, f] = _score_reference(S_tr[f], S_te[f], nodes)
    print(f"cv, refit={refit}: scores within {float((np.abs(st['SCORE'] - SC) / B).max()):.3f} of their bounds")
    assert np.all(np.abs(st['SCORE'] - SC) <= B)
    assert np.array_equal(st['SCORE'], utils.mb_cv_scores(st['RESVAR'], st['HELDOUT'], st['STATUS'] != 0, 'pseudo'))
    CV = SC.mean(axis=1)
    assert st['IX'] == ms.cv_select(CV, SC.std(axis=1, ddof=1) / np.sqrt(F), 'min')
    # the test-fold matrices have the bits of ggl_heldout_scores' route (ggl_covariance_subsets shares it): the stateless
    # refit on them and on the stack gives the per-node arrays bit for bit
    if refit:
        rf = utils.neighborhood_refit(S_tr, Wd, T_EDGE, S_te)
        assert np.array_equal(st['RESVAR'], np.swapaxes(rf['RESVAR'], 0, 1))
        assert np.array_equal(st['HELDOUT'], np.swapaxes(rf['HELDOUT'], 0, 1))
        assert np.array_equal(sol['coef_refit'] != 0, sol['adjacency'])
    else:
        assert np.array_equal(st['RESVAR'], np.swapaxes(infd['RESVAR'], 0, 1))
    assert np.array_equal(sol['precision'], sol['precision'].T)


def test_cv_empty_graph_shows_the_test_matrices():
    """At a lambda above every |S_ij| no node has a neighbour: r_j is T_jj, the diagonal of the matrices ggl_heldout_scores'
    route builds."""
    from gglasso_amd import solver, utils
    X, _, (train, test) = _cv_inputs()
    p, F = 17, 3
    eye = np.broadcast_to(np.eye(p), (F, p, p))
    eng = solver.HipEngine(eye, eye, eye, np.zeros((F, p, p)))
    try:
        eng.set_data_subsets(X, train)
        out = eng.neighborhood_cv(X, test, [50.0], 'and', tol=TOL)
        for kw in (dict(rule='raw'), dict(t=-1.0), dict(tol=-1.0), dict(max_sweeps=0), dict(lambda_range=[0.1, 0.2])):
            args = dict(X=X, test_idx=test, lambda_range=[0.2, 0.1])
            args.update(kw)
            with pytest.raises(AssertionError):
                eng.neighborhood_cv(**args)
        with pytest.raises(AssertionError):                                 # what ggl_heldout_scores refuses about the folds
            eng.neighborhood_cv(X, np.full((F, 4), 120, dtype=np.int32), [0.2])
        with pytest.raises(AssertionError):                                 # F must be K
            eng.neighborhood_cv(X, test[:1], [0.2])
    finally:
        eng.close()
    S_tr, S_te = utils.sample_covariance_subsets(X, train), utils.sample_covariance_subsets(X, test)
    assert not out['degree'].any() and not out['status'].any()
    assert np.array_equal(out['heldout'][0], np.diagonal(S_te, axis1=1, axis2=2))
    assert np.array_equal(out['resvar'][0], np.diagonal(S_tr, axis1=1, axis2=2))


def test_cv_nan_in_one_train_fold():
    """A NaN planted in S through the ctx route: an observation that only train fold 1 holds.  The nodes it reaches get status
    2 -- with the path dead on that matrix nobody has a neighbour, so that is the variable itself -- and the other folds keep
    the bits of the run without it."""
    from gglasso_amd import solver
    X = mb_ref.stars_data()
    p, F, N = 17, 3, 120
    rng = np.random.default_rng(6)
    train = np.stack([np.sort(rng.choice(N - 1, 70, replace=False)) for _ in range(F)]).astype(np.int32)
    test = np.stack([np.setdiff1d(np.arange(N - 1), train[f])[:40] for f in range(F)]).astype(np.int32)
    train[1, -1] = N - 1
    Xn = X.copy()
    Xn[3, N - 1] = np.nan
    lam = np.array(mb_ref.GRID)
    eye = np.broadcast_to(np.eye(p), (F, p, p))
    got = []
    for data in (X, Xn):
        eng = solver.HipEngine(eye, eye, eye, np.zeros((F, p, p)))
        try:
            eng.set_data_subsets(data, train)
            got.append(eng.neighborhood_cv(data, test, lam, 'and', tol=TOL, stack=True))
        finally:
            eng.close()
    clean, out = got
    assert not clean['status'].any()
    st = out['status']
    assert np.all(st[:, 1, 3] == 2) and not np.delete(st[:, 1], 3, axis=1).any() and not st[:, [0, 2]].any()
    assert np.isnan(out['resvar'][:, 1, 3]).all() and np.isnan(out['heldout'][:, 1, 3]).all()
    assert np.isfinite(np.delete(out['resvar'][:, 1], 3, axis=1)).all() and not out['degree'][:, 1].any()
    for k in ('resvar', 'heldout', 'status', 'degree', 'stack'):
        assert np.array_equal(out[k][:, [0, 2]], clean[k][:, [0, 2]]), k


def test_front_end_and_untouched_routes():
    from gglasso_amd import model_selection as ms, utils
    from gglasso_amd.problem import glasso_problem
    X, lam, _ = _cv_inputs()
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        P = glasso_problem.from_data(X, reg=None)
        P.neighborhood_selection(lam, select='cv', rule='and', n_folds=3, seed=4, tol=TOL)
        sol, st = ms.cv_search(X, lam, n_folds=3, seed=4, method='mb', graph_rule='and', tol=TOL)
    assert np.array_equal(P.solution.precision_, sol['precision']) and np.array_equal(P.solution.adjacency_, sol['adjacency'])
    assert P.reg_params['lambda1'] == st['BEST']['lambda1'] and P.modelselect_stats['IX'] == st['IX']
    assert np.array_equal(P.solution.precision_, P.solution.precision_.T)
    assert np.array_equal(P.solution.adjacency_, (P.solution.precision_ != 0) & ~np.eye(17, dtype=bool))
    # stars_search: refit only adds keys
    kw = dict(n_subsamples=6, seed=5, beta=0.1, scale=True, tol=TOL, method='mb')
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        sol0, st0 = ms.stars_search(X, lam, **kw)
        sol1, st1 = ms.stars_search(X, lam, refit=True, **kw)
        P.neighborhood_selection(lam, select='stars', rule='and', n_subsamples=6, seed=5, beta=0.1, tol=TOL)
    assert sorted(sol0) == ['adjacency', 'coef', 'lambda1', 'resvar'] and st0['NUM'] == st1['NUM']
    assert all(np.array_equal(sol0[k], sol1[k]) for k in sol0)
    S_full = utils.sample_covariance(X, center=True, scale=True)[0]
    rf = utils.neighborhood_refit(S_full, sol1['adjacency'].astype(float), T_EDGE)
    assert np.array_equal(sol1['coef_refit'], rf['COEF']) and np.array_equal(sol1['resvar_refit'], rf['RESVAR'])
    # the glasso routes with default arguments against the same routes called the old way
    Xs = mb_ref.stars_data(p=6, N=60)
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        a = ms.cv_search(Xs, (0.4, 0.2), n_folds=3, seed=2, store_all=True, tol=1e-6, rtol=1e-6)
        b = ms.cv_search(Xs, (0.4, 0.2), 3, 2, None, 'min', True, False, 1e-6, 1e-6, 1000, True, None, None, None, False, False, None)
        c = ms.stars_search(Xs, (0.4, 0.2), n_subsamples=3, seed=2, beta=0.2, store_all=True, tol=1e-6, rtol=1e-6)
        d = ms.stars_search(Xs, (0.4, 0.2), 3, None, 0.2, 2, None, 1e-8, True, False, 1e-6, 1e-6, 1000, True, None, None, None, 2,
                            False, 'glasso', 'and')
    for (sa, ta), (sb, tb) in ((a, b), (c, d)):
        assert sorted(ta) == sorted(tb) and sorted(sa) == sorted(sb)
        for k in ta:
            if isinstance(ta[k], np.ndarray):
                assert np.array_equal(ta[k], tb[k], equal_nan=True), k
            else:
                assert ta[k] == tb[k], k
        for k in sa:
            assert np.array_equal(sa[k], sb[k]), k
    assert 'SCORE' not in a[1] and 'precision' not in c[0]
