"""K-fold cross-validation of lambda1 on the device: the held-out scores of the snapshots of a batch (ggl_heldout_scores,
k_heldout_dot) and the drivers on top (model_selection.cv_search, glasso_problem.cross_validation).

There is no reference program for this; the yardsticks are ``math.fsum`` on the downloaded snapshots with the library's own
test covariances (the any-order summation bound), the library's selection statistics (bitwise: the same route), and the
driver's host route on the test-only oracle engine.

Sizes: p on both sides of the Jacobi limit 8, of the LDS Omega-step limit 64, of a 64-wide tile edge and of the
eigenvalue-route switch at 128; p = 95 beside them for the inner product alone (an odd p * p above one workgroup's 8192
elements: the 8-byte loads with more than one partial per instance; p = 130 is the 16-byte counterpart).  N = 23 with F = 5
leaves three observations that are never tested."""
import math
import warnings

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

U = 2.0 ** -53
LAM4 = [1.0, 0.6, 0.4, 0.25]


def cv_data(p, N, seed):
    """Observations (p,N) of a sparse precision matrix of gglasso_amd.synth."""
    from gglasso_amd import synth
    Th = synth.make_precisions('SGL', 1, p, M=max(1, p // 8), seed=seed)[0]
    Z = np.random.default_rng([seed, p, N]).standard_normal((p, N))
    return np.ascontiguousarray(np.linalg.solve(np.linalg.cholesky(Th).T, Z))


def planted(K, p, seed):
    """(K,p,p) symmetric positive definite, about half of the off-diagonal entries zero; instance 1 (if there is one and
    p > 1) gets a negative eigenvalue: its log det is -inf."""
    rng = np.random.default_rng([K, p, seed])
    T = rng.uniform(-1.0, 1.0, (K, p, p)) * (rng.random((K, p, p)) < 0.5)
    T = np.triu(T, 1)
    T = T + T.transpose(0, 2, 1)
    T[:, np.arange(p), np.arange(p)] = np.abs(T).sum(axis=2) + rng.uniform(0.5, 2.0, (K, p))
    if K > 1 and p > 1:
        T[1, 0, 0] = -1.0
    return np.ascontiguousarray(T)


def engine_with_snapshots(T):
    from gglasso_amd.solver import HipEngine
    K, p, _ = T.shape
    eye = np.broadcast_to(np.eye(p), (K, p, p))
    eng = HipEngine(eye, eye, eye, 0 * eye)
    eng.set_state(np.ascontiguousarray(eye), T, np.zeros((K, p, p)))
    for k in range(K):
        eng.snapshot_k(k)
    return eng


def inner_bound(S, T):
    """(p^2 + 8) u sum |S o T|: p^2 products summed in any order."""
    return (S.size + 8) * U * math.fsum(np.abs(S * T).ravel())


# ---------------------------------------------------------------------------------------------------------------------
# 1. the entry point on planted snapshots
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("p", [1, 2, 9, 33, 65, 95, 130])
def test_heldout_scores_on_planted_snapshots(p):
    from gglasso_amd import model_selection as ms, utils
    for N, F, L in ((23, 5, 1), (40, 2, 4), (23, 3, 4), (40, 5, 4)):
        what = (p, N, F, L)
        K = L * F
        X = cv_data(p, N, 3)
        X += np.arange(p)[:, None]                                      # (row means: centring shows)
        train, test = ms.cv_folds(N, F, seed=2)
        T = planted(K, p, N)
        eng = engine_with_snapshots(T)
        try:
            eng.set_data_subsets(X, train)
            S_ctx = eng.get_S()
            for center in (True, False):
                out = eng.heldout_scores(X, test, center=center)
                assert out.shape == (K, 4)
                S_test = utils.sample_covariance_subsets(X, test, center=center)
                Th = eng.snapshots(names=('Theta',))['Theta']
                assert np.array_equal(Th, T)
                for k in range(K):
                    S = S_test[k % F]
                    ref = math.fsum((S * Th[k]).ravel())
                    bound = inner_bound(S, Th[k])
                    print(what, center, k, "diff", abs(out[k, 0] - ref), "bound", bound)
                    assert abs(out[k, 0] - ref) <= bound, what + (center, k)
                # columns 1-3: the bits of the selection statistics (whose column 0 is the ctx's own S)
                st = eng.selection_stats()
                assert np.array_equal(out[:, 1:], st[:, 1:]), what
                if K > 1 and p > 1:
                    assert out[1, 1] == -np.inf and out[1, 3] < 0
                assert np.all(np.isfinite(np.delete(out[:, 1], 1 if K > 1 and p > 1 else [])))
                assert np.array_equal(out[:, 2], np.count_nonzero(Th, axis=(1, 2)))
                # the same bits from a second call
                assert np.array_equal(eng.heldout_scores(X, test, center=center), out), what
            # the ctx's S was neither read nor written
            assert np.array_equal(eng.get_S(), S_ctx), what
        finally:
            eng.close()


@pytest.mark.parametrize("p", [9, 65, 130])
def test_an_instance_does_not_depend_on_the_others_in_the_batch(p):
    """The F snapshots of one lambda alone (K = F) and as lambda 2 of a grid of 4 among other matrices: the same bits."""
    from gglasso_amd import model_selection as ms
    N, F = 40, 5
    X = cv_data(p, N, 4)
    _, test = ms.cv_folds(N, F, seed=0)
    own = planted(F, p, 1)
    alone = engine_with_snapshots(own)
    try:
        a = alone.heldout_scores(X, test)
    finally:
        alone.close()
    for seed in (2, 3):
        T = planted(4 * F, p, seed)
        T[2 * F:3 * F] = own
        grid = engine_with_snapshots(T)
        try:
            g = grid.heldout_scores(X, test)
        finally:
            grid.close()
        assert np.array_equal(g[2 * F:3 * F, 0], a[:, 0]), (p, seed)
        assert not np.array_equal(g[:F, 0], a[:, 0])


def test_heldout_scores_refusals_write_nothing():
    from gglasso_amd import _lib, model_selection as ms
    from gglasso_amd.solver import HipEngine
    p, N, F, L = 5, 23, 3, 2
    K = L * F
    X = cv_data(p, N, 6)
    train, test = ms.cv_folds(N, F, seed=0)
    m = test.shape[1]
    lib = _lib.load()
    ip = lambda a: a.ctypes.data_as(_lib._ip)
    eye = np.broadcast_to(np.eye(p), (K, p, p))
    sentinel = np.full((K, 4), -7.25)
    out = sentinel.copy()

    def refused(eng, word, *args):
        S = eng.get_S()
        assert lib.ggl_heldout_scores(eng.h, *args) == _lib.E_ARG, word
        msg = _lib.last_error()
        assert word in msg, (word, msg)
        assert np.array_equal(out, sentinel), word
        assert np.array_equal(eng.get_S(), S), word

    eng = HipEngine(eye, eye, eye, 0 * eye)
    try:
        eng.set_data_subsets(X, train)
        good = (_lib.ptr(X), N, F, m, ip(test), _lib.COV_CENTER, _lib.ptr(out))
        refused(eng, "no snapshot", *good)
        with pytest.raises(AssertionError, match=r"no snapshot"):
            eng.heldout_scores(X, test, out=out)
        assert np.array_equal(out, sentinel)
        for k in range(K):
            eng.snapshot_k(k)
        assert lib.ggl_heldout_scores(None, *good) == _lib.E_ARG and np.array_equal(out, sentinel)
        refused(eng, "X", None, N, F, m, ip(test), _lib.COV_CENTER, _lib.ptr(out))
        refused(eng, "idx_test", _lib.ptr(X), N, F, m, None, _lib.COV_CENTER, _lib.ptr(out))
        assert lib.ggl_heldout_scores(eng.h, _lib.ptr(X), N, F, m, ip(test), _lib.COV_CENTER, None) == _lib.E_ARG
        assert "out" in _lib.last_error()
        for bad_F in (0, -1, 4, 5, 7):
            refused(eng, f"F = {bad_F} folds do not divide the K = {K}", _lib.ptr(X), N, bad_F, m, ip(test), _lib.COV_CENTER,
                    _lib.ptr(out))
        for bad_m in (0, -3):
            refused(eng, f"m = {bad_m}", _lib.ptr(X), N, F, bad_m, ip(test), _lib.COV_CENTER, _lib.ptr(out))
        for flags in (_lib.COV_SCALE, _lib.COV_CENTER | _lib.COV_SCALE, _lib.COV_TILE32, 1 << 9):
            refused(eng, f"flags = {flags}", _lib.ptr(X), N, F, m, ip(test), flags, _lib.ptr(out))
        bad = test.copy()
        bad[2, 4] = N
        refused(eng, f"fold 2, position 4 holds the index {N}, outside [0, {N})", _lib.ptr(X), N, F, m, ip(bad), _lib.COV_CENTER,
                _lib.ptr(out))
        bad[2, 4], bad[0, 1] = 0, -1
        refused(eng, "fold 0, position 1 holds the index -1", _lib.ptr(X), N, F, m, ip(bad), _lib.COV_CENTER, _lib.ptr(out))
        # ... and the call that is not refused writes all of it
        assert lib.ggl_heldout_scores(eng.h, *good) == 0
        assert np.all(out != sentinel)
        assert np.array_equal(out, eng.heldout_scores(X, test))
    finally:
        eng.close()
    dims = HipEngine(eye, eye, eye, 0 * eye)
    try:
        dims.set_instance_dims(np.full(K, p - 1))
        for k in range(K):
            dims.snapshot_k(k)
        out[:] = sentinel
        assert lib.ggl_heldout_scores(dims.h, *good) == _lib.E_ARG
        assert "instance dimensions" in _lib.last_error() and np.array_equal(out, sentinel)
    finally:
        dims.close()


# ---------------------------------------------------------------------------------------------------------------------
# 2. the search: device route against the host route (oracle engine) on the same folds
# ---------------------------------------------------------------------------------------------------------------------
def host_route(X, lam, **kw):
    from gglasso_amd import solver, model_selection as ms
    from oracle_engine import OracleEngine
    keep, solver.ENGINE = solver.ENGINE, OracleEngine
    try:
        return ms.cv_search(X, lam, store_all=True, **kw)
    finally:
        solver.ENGINE = keep


@pytest.mark.parametrize("p,N,F,L", [(2, 23, 5, 4), (9, 40, 2, 4), (33, 23, 3, 4), (65, 40, 5, 1), (65, 23, 5, 4), (130, 40, 3, 4)])
def test_cv_search_device_against_host_route(p, N, F, L, monkeypatch):
    from gglasso_amd import model_selection as ms, utils
    from gglasso_amd.solver import HipEngine
    X = cv_data(p, N, 8)
    # (p = 2: two weakly correlated variables, every lambda of LAM4 gives the empty graph and the same score)
    lam = [0.5] if L == 1 else ([0.3, 0.15, 0.08, 0.04] if p == 2 else LAM4)
    kw = dict(n_folds=F, seed=5, tol=1e-8, rtol=1e-8)
    seen = []
    real = HipEngine.heldout_scores

    def spy(self, X_, test_idx, center=True, out=None):
        seen.append(self.get_S())                                       # what the `before` hook left in the ctx
        return real(self, X_, test_idx, center=center, out=out)

    monkeypatch.setattr(HipEngine, "heldout_scores", spy)
    with warnings.catch_warnings():
        warnings.simplefilter("error")
        sol, st = ms.cv_search(X, lam, store_all=True, **kw)
        sol_h, st_h = host_route(X, lam, **kw)
    train, test = ms.cv_folds(N, F, seed=5)
    assert np.array_equal(st['TRAIN'], train) and np.array_equal(st['TEST'], test)
    # the train matrices: bitwise the subset covariances, tiled over the lambdas
    assert len(seen) == 1 and np.array_equal(seen[0], np.tile(utils.sample_covariance_subsets(X, train), (L, 1, 1)))
    assert st['FAILED'] == st_h['FAILED'] == [] and st['NOT_PD'] == st_h['NOT_PD'] == []
    assert sorted(st) == sorted(st_h)
    S_test = ms._host_subset_covariances(X, test, True, False)
    slack = np.zeros((L, F))
    for l in range(L):
        for f in range(F):
            Th = st_h['THETA'][l, f]
            slack[l, f] = inner_bound(S_test[f], Th) + 1e-9 * (np.linalg.norm(S_test[f]) + np.linalg.norm(np.linalg.inv(Th)))
    diff = np.abs(st['NLL'] - st_h['NLL'])
    print((p, N, F, L), "max NLL diff", diff.max(), "smallest bound", slack.min(), "max Theta diff",
          np.abs(st['THETA'] - st_h['THETA']).max())
    assert np.all(diff <= slack)
    assert np.array_equal(st['NNZ'], st_h['NNZ'])
    assert np.array_equal(st['NNZ'], np.count_nonzero(st['THETA'], axis=(2, 3)))
    order = np.sort(st_h['CV'])
    if L == 1 or order[1] - order[0] > slack.max():
        assert st['IX'] == st_h['IX'] and st['BEST'] == st_h['BEST']
        assert np.abs(sol['Theta'] - sol_h['Theta']).max() <= 1e-9
    if L > 1:
        assert order[1] - order[0] > slack.max(), "the grid of this test was chosen so that the choice is clear"
    assert np.array_equal(st['CV'], st['NLL'].mean(axis=1))
    assert st['IX'] == ms.cv_select(st['CV'], st['SE'], 'min')


def test_cv_search_chunks_give_the_same_bits():
    from gglasso_amd import model_selection as ms
    p, N, F = 33, 40, 3
    X = cv_data(p, N, 8)
    sol, st = ms.cv_search(X, LAM4, n_folds=F, seed=5, rule='one_se')
    sol2, st2 = ms.cv_search(X, LAM4, n_folds=F, seed=5, rule='one_se', lambdas_per_batch=3)
    assert np.array_equal(st2['NLL'], st['NLL']) and np.array_equal(st2['NNZ'], st['NNZ']) and st2['IX'] == st['IX']
    assert 'THETA' not in st and st['rule'] == 'one_se' and st['IX'] <= ms.cv_select(st['CV'], st['SE'], 'min')
    assert np.array_equal(sol2['Theta'], sol['Theta'])


def test_cv_search_with_one_poisoned_instance(monkeypatch):
    """A non-finite observation reaches ONE instance, fold 1 at lambda 2, through its train covariance only: that lambda has
    no score, is named and not chosen.

    Where every lambda runs as its own batch (``lambdas_per_batch=1``) the other lambdas' scores are the bits of the clean
    run.  Where the whole grid is ONE batch they are not, and cannot be without changing the solver: a point that fails falls
    out of the fused LDS Omega-step, which the launches it shares then sit out for some iterations, so the other points take
    another route to the same optimum (tests/test_gpu_batch_isolation.py states 1e-9 on Theta for them).  There the scores
    agree within that parity, propagated as in the comparison with the host route."""
    from gglasso_amd import _lib, model_selection as ms, utils
    from gglasso_amd.solver import HipEngine
    p, N, F, L = 33, 40, 3, 4
    X = cv_data(p, N, 8)
    kw = dict(n_folds=F, seed=5)
    with warnings.catch_warnings():
        warnings.simplefilter("error")
        sol, st = ms.cv_search(X, LAM4, store_all=True, **kw)
        sol_c, st_c = ms.cv_search(X, LAM4, lambdas_per_batch=1, **kw)
    train, test = ms.cv_folds(N, F, seed=5)
    bad = X.copy()
    bad[7, train[1, 3]] = np.inf
    S_bad = utils.sample_covariance_subsets(bad, train[1:2])[0]
    assert not np.all(np.isfinite(S_bad))
    real = HipEngine.set_data_subsets
    calls = []

    def poisoned(self, X_, indices, **k):
        real(self, X_, indices, **k)
        calls.append(self.K)
        if self.K == L * F or len(calls) == 3:                          # the whole grid, or the batch of lambda 2
            S = self.get_S()
            S[(2 * F if self.K == L * F else 0) + 1] = S_bad
            _lib.check(_lib.load().ggl_set_S(self.h, _lib.ptr(np.ascontiguousarray(S))))

    monkeypatch.setattr(HipEngine, "set_data_subsets", poisoned)
    keep = [0, 1, 3]
    for chunked in (True, False):
        del calls[:]
        with pytest.warns(RuntimeWarning) as rec:
            sol2, st2 = ms.cv_search(X, LAM4, lambdas_per_batch=1 if chunked else None, **kw)
        assert calls == ([F] * L if chunked else [L * F])
        assert any(f"cross-validation: a fold failed at lambda1 = [{LAM4[2]}]" in str(w.message) for w in rec)
        assert st2['FAILED'] == [2] and np.all(np.isnan(st2['NLL'][2])) and np.isnan(st2['CV'][2]) and st2['NOT_PD'] == []
        assert st2['IX'] != 2 and st2['IX'] == ms.cv_select(st2['CV'], st2['SE'], 'min')
        assert np.array_equal(st2['NNZ'][keep], st['NNZ'][keep])
        if chunked:
            assert np.array_equal(st2['NLL'][keep], st_c['NLL'][keep])
            continue
        S_test = ms._host_subset_covariances(X, test, True, False)
        for l in keep:
            for f in range(F):
                Th = st['THETA'][l, f]
                slack = inner_bound(S_test[f], Th) + 1e-9 * (np.linalg.norm(S_test[f]) + np.linalg.norm(np.linalg.inv(Th)))
                print("poisoned batch", (l, f), "NLL diff", abs(st2['NLL'][l, f] - st['NLL'][l, f]), "bound", slack)
                assert abs(st2['NLL'][l, f] - st['NLL'][l, f]) <= slack


# ---------------------------------------------------------------------------------------------------------------------
# 3. the front end
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("do_scaling", [False, True])
def test_cross_validation_front_end(do_scaling):
    from gglasso_amd import model_selection as ms
    from gglasso_amd.problem import glasso_problem
    p, N = 33, 40
    X = cv_data(p, N, 8) * np.linspace(0.5, 3.0, p)[:, None]
    grid = {'lambda1_range': np.array(LAM4[::-1])}
    P = glasso_problem.from_data(X, reg_params={'lambda1': 0.3}, do_scaling=do_scaling)
    P.cross_validation(grid, n_folds=3, seed=5)
    st = P.modelselect_stats
    sol, st_s = ms.cv_search(X, LAM4, n_folds=3, seed=5, scale=do_scaling)
    assert np.array_equal(st['NLL'], st_s['NLL']) and st['IX'] == st_s['IX']
    assert P.reg_params['lambda1'] == st['BEST']['lambda1'] == LAM4[st['IX']]
    Theta = P.solution.precision_
    assert Theta.shape == (p, p) and np.all(np.isfinite(Theta)) and np.array_equal(Theta, Theta.T)
    if do_scaling:
        assert np.allclose(st['scale'], X.var(axis=1), rtol=1e-12, atol=0)
        sd = np.sqrt(P._scale)
        assert np.allclose(Theta, sol['Theta'] / (sd[:, None] * sd[None, :]), rtol=1e-9, atol=1e-12)
    else:
        assert 'scale' not in st and np.array_equal(Theta, sol['Theta'])
    P2 = glasso_problem.from_data(X, do_scaling=do_scaling)
    P2.cross_validation(grid, n_folds=3, seed=5, rule='one_se')
    assert P2.modelselect_stats['IX'] <= st['IX'] and P2.modelselect_stats['rule'] == 'one_se'
