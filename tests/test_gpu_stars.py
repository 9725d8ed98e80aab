"""StARS stability selection on the device: the column gather in front of the covariance kernels (ggl_covariance_subsets,
ggl_set_S_from_subsets), the edge-stability kernel over the snapshots of a batch (ggl_edge_stability), and the drivers on
top of them (model_selection.stars_search, glasso_problem.stability_selection).

There is no reference program for any of this; the yardsticks are the library's own covariance of host-gathered columns
(bitwise: same kernels, same bits in) and numpy on the host (exact: the statistics are integers)."""
import warnings

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

T_EDGE = 1e-8
LAM = [0.5, 0.35, 0.25, 0.18, 0.12, 0.08, 0.05, 0.02]
NUM = [154, 274, 593, 1154, 1931, 2626, 2929, 2202]          # the CPU oracle engine's at tol = rtol = 1e-8 (margins: see below)


def make_data(p, N, seed):
    """The generator of tests/test_gpu_covariance.py: row means up to 1e3, so a wrong column shows at once."""
    rng = np.random.default_rng([20241018, p, N, seed])
    mean = rng.uniform(-1e3, 1e3, (p, 1))
    std = rng.uniform(0.1, 10.0, (p, 1))
    return mean + std * rng.standard_normal((p, N))


def draws(N, B, b, rng):
    """(B, b) indices: row 0 sorted without repetition (the identity permutation for b = N), the others draws with
    replacement, row 1 with a forced duplicate and not in ascending order."""
    idx = rng.integers(0, N, (B, b))
    idx[0] = np.sort(rng.choice(N, b, replace=False))
    if b >= 2:
        idx[1, 1] = idx[1, 0]
        if np.all(np.diff(idx[1]) >= 0):
            idx[1] = idx[1, ::-1].copy()                                  # ... and out of order
    return idx.astype(np.int32)


# ---------------------------------------------------------------------------------------------------------------------
# 1. subset covariances
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("p", [1, 17, 65])
@pytest.mark.parametrize("N", [5, 33, 257])
def test_subset_covariance_is_the_covariance_of_gathered_columns(p, N):
    from gglasso_amd import _lib, utils
    X = np.ascontiguousarray(make_data(p, N, 0))
    B = 3
    rng = np.random.default_rng([p, N])
    for b in (1, 4, N):
        idx = draws(N, B, b, rng)
        if b == N:
            assert np.array_equal(idx[0], np.arange(N))
        for tile in (0, _lib.COV_TILE32, _lib.COV_TILE64):
            for center in (0, _lib.COV_CENTER):
                for scale in (0, _lib.COV_SCALE):
                    flags = tile | center | scale
                    what = (p, N, b, flags)
                    flat = [r for r in range(B) if len(set(idx[r])) == 1]
                    if scale and center and flat:
                        # one observation (b = 1, or one index drawn b times) has no variance: both routes refuse, naming
                        # the first such subset and its first variable
                        with pytest.raises(AssertionError, match=rf"instance {flat[0]}, variable 0"):
                            utils._covariance_subsets_call(X, idx, flags)
                        with pytest.raises(AssertionError, match=r"instance 0, variable 0"):
                            utils._covariance_call([np.ascontiguousarray(X[:, idx[flat[0]]])], flags)
                        continue
                    S, var = utils._covariance_subsets_call(X, idx, flags)
                    assert S.shape == (B, p, p) and (var is None) == (not scale)
                    for r in range(B):
                        Sr, vr = utils._covariance_call([np.ascontiguousarray(X[:, idx[r]])], flags)
                        assert np.array_equal(S[r], Sr[0]), what + (r,)
                        assert np.array_equal(S[r], S[r].T), what + (r,)
                        if scale:
                            assert np.array_equal(var[r], vr[0]), what + (r,)
    # all observations in their order: the covariance of X itself
    ident = np.broadcast_to(np.arange(N, dtype=np.int32), (B, N))
    S = utils.sample_covariance_subsets(X, ident)
    assert np.array_equal(S[0], utils.sample_covariance(X)) and np.array_equal(S[1], S[0]) and np.array_equal(S[2], S[0])
    C, var = utils.sample_covariance_subsets(X, ident[:1], center=False, scale=True)
    C1, var1 = utils.sample_covariance(X, center=False, scale=True)
    assert np.array_equal(C[0], C1) and np.array_equal(var[0], var1)
    if p > 1 and N > 5:
        assert np.abs(S[0] - np.cov(X, bias=True)).max() <= 1e-9 * np.abs(S[0]).max()


def test_subset_covariance_misuse():
    from gglasso_amd import utils
    X = make_data(5, 9, 1)
    ok = np.array([[0, 1, 2], [3, 4, 8]])
    utils.sample_covariance_subsets(X, ok)
    bad = ok.copy()
    bad[1, 2] = 9
    with pytest.raises(AssertionError, match=r"subset 1, position 2 holds the index 9, outside \[0, 9\)"):
        utils.sample_covariance_subsets(X, bad)
    bad[1, 2], bad[0, 1] = 8, -1
    with pytest.raises(AssertionError, match=r"subset 0, position 1 holds the index -1"):
        utils.sample_covariance_subsets(X, bad)
    with pytest.raises(AssertionError, match=r"b = 0"):
        utils.sample_covariance_subsets(X, np.zeros((2, 0), dtype=int))
    with pytest.raises(AssertionError, match=r"B = 0"):
        utils.sample_covariance_subsets(X, np.zeros((0, 3), dtype=int))
    with pytest.raises(AssertionError):
        utils.sample_covariance_subsets(X, ok.astype(float))


# ---------------------------------------------------------------------------------------------------------------------
# 2. straight into the S of a ctx
# ---------------------------------------------------------------------------------------------------------------------
def test_ctx_takes_its_S_from_subsets_and_keeps_it_when_a_call_is_refused():
    from gglasso_amd import utils
    from gglasso_amd.solver import HipEngine
    p, N, L, B, b = 17, 33, 2, 3, 11
    X = make_data(p, N, 2)
    idx = draws(N, B, b, np.random.default_rng(5))
    S_op = utils.sample_covariance_subsets(X, idx)
    eye = np.broadcast_to(np.eye(p), (L * B, p, p))
    eng = HipEngine(eye, eye, eye, 0 * eye)
    try:
        eng.set_data_subsets(X, idx)
        S = eng.get_S()
        for l in range(L):
            for r in range(B):
                assert np.array_equal(S[l * B + r], S_op[r]), (l, r)
        bad = idx.copy()
        bad[2, 7] = N
        with pytest.raises(AssertionError, match=rf"subset 2, position 7 holds the index {N}"):
            eng.set_data_subsets(X, bad)
        assert np.array_equal(eng.get_S(), S)
        with pytest.raises(AssertionError, match=r"do not divide"):
            eng.set_data_subsets(X, np.concatenate([idx, idx[:1]]))          # 4 subsets, 6 instances
        assert np.array_equal(eng.get_S(), S)
        # correlations: the variances are kept, per instance
        C_op, var_op = utils.sample_covariance_subsets(X, idx, scale=True)
        eng.set_data_subsets(X, idx, scale=True)
        C, var = eng.get_S()
        assert np.array_equal(C, np.tile(C_op, (L, 1, 1))) and np.array_equal(var, np.tile(var_op, (L, 1)))
        # a refusal found on the device (a variable without variance in subset 1) leaves S and the variances alone too
        flat = X.copy()
        flat[4, idx[1]] = 2.5
        with pytest.raises(AssertionError, match=r"instance 1, variable 4"):
            eng.set_data_subsets(flat, idx, scale=True)
        C2, var2 = eng.get_S()
        assert np.array_equal(C2, C) and np.array_equal(var2, var)
        eng.set_data_subsets(X, idx, center=False)
        assert np.array_equal(eng.get_S(), np.tile(utils.sample_covariance_subsets(X, idx, center=False), (L, 1, 1)))
    finally:
        eng.close()
    dims = HipEngine(eye, eye, eye, 0 * eye)
    try:
        dims.set_instance_dims(np.full(L * B, p - 1))
        with pytest.raises(AssertionError, match=r"instance dimensions"):
            dims.set_data_subsets(X, idx)
    finally:
        dims.close()


# ---------------------------------------------------------------------------------------------------------------------
# 3. edge stability on planted snapshots
# ---------------------------------------------------------------------------------------------------------------------
def planted(L, B, p, seed):
    """(L*B,p,p) stacks with entries from {0, +-t/10, +-t, +-1, NaN}, NOT symmetric: only the upper triangle may count."""
    values = np.array([0.0, T_EDGE / 10, -T_EDGE / 10, T_EDGE, -T_EDGE, 1.0, -1.0, np.nan])
    rng = np.random.default_rng([L, B, p, seed])
    return values[rng.integers(0, len(values), (L * B, p, p))]


def numpy_edges(T, L, B, t):
    p = T.shape[-1]
    with np.errstate(invalid='ignore'):
        hit = np.abs(T.reshape(L, B, p, p)) >= t
    c = np.triu(hit.sum(axis=1), 1).astype(np.int64)
    num = [int(np.sum(c[l] * (B - c[l]))) for l in range(L)]
    return (c + c.transpose(0, 2, 1)).astype(np.int32), num


@pytest.mark.parametrize("p", [1, 2, 15, 16, 17, 64, 65, 130])
@pytest.mark.parametrize("LB", [(1, 1), (3, 2), (2, 7), (1, 64)])
def test_edge_stability_counts_are_exact(p, LB):
    from gglasso_amd.solver import HipEngine
    L, B = LB
    K = L * B
    T = planted(L, B, p, 0)
    eye = np.broadcast_to(np.eye(p), (K, p, p))
    eng = HipEngine(eye, eye, eye, 0 * eye)
    try:
        eng.set_state(np.ascontiguousarray(eye), T, np.zeros((K, p, p)))
        for k in range(K):
            eng.snapshot_k(k)
        counts, num = numpy_edges(T, L, B, T_EDGE)
        got_num, got_counts = eng.edge_stability(B, T_EDGE, counts=True)
        assert got_num.dtype == np.int64 and got_counts.dtype == np.int32 and got_counts.shape == (L, p, p)
        assert np.array_equal(got_counts, counts)
        assert list(got_num) == num
        assert np.array_equal(got_counts, got_counts.transpose(0, 2, 1))
        assert not got_counts[:, np.arange(p), np.arange(p)].any()
        if B == 1 or p == 1:
            assert not got_num.any()
        elif p >= 15:
            assert got_num.all()                         # (planted values on both sides of t: every lambda is unstable)
        # the same bits from a second call, with and without the tables
        again_num, again_counts = eng.edge_stability(B, T_EDGE, counts=True)
        assert np.array_equal(again_num, got_num) and np.array_equal(again_counts, got_counts)
        assert np.array_equal(eng.edge_stability(B), got_num)
        # t = 0: every entry that is a number is an edge
        counts0, num0 = numpy_edges(T, L, B, 0.0)
        n0, c0 = eng.edge_stability(B, 0.0, counts=True)
        assert np.array_equal(c0, counts0) and list(n0) == num0
        # the other layout of the same stack: one lambda of K subsamples
        counts1, num1 = numpy_edges(T, 1, K, T_EDGE)
        n1, c1 = eng.edge_stability(K, counts=True)
        assert np.array_equal(c1, counts1) and list(n1) == num1
    finally:
        eng.close()


def test_edge_stability_misuse():
    from gglasso_amd.solver import HipEngine
    p, K = 5, 6
    eye = np.broadcast_to(np.eye(p), (K, p, p))
    eng = HipEngine(eye, eye, eye, 0 * eye)
    try:
        with pytest.raises(AssertionError, match=r"no snapshot taken"):
            eng.edge_stability(3)
        eng.snapshot_k(0)
        assert list(eng.edge_stability(3)) == [0, 0]                 # (slots never snapshotted read as zeros)
        for B in (0, -1, 4, 7):
            with pytest.raises(AssertionError, match=r"do not divide"):
                eng.edge_stability(B)
        for t in (-1e-8, float('nan'), float('inf'), -float('inf')):
            with pytest.raises(AssertionError, match=r"finite and not negative"):
                eng.edge_stability(3, t)
    finally:
        eng.close()


# ---------------------------------------------------------------------------------------------------------------------
# 4. end to end.  The problem: a chain graph with one extra edge, p = 16, N = 400, B = 12 subsamples of 200.  Its integer sums
# on the CPU oracle engine at tol = rtol = 1e-8 are NUM; the cuts are 432 for beta = 0.05 and 864 for beta = 0.1, so the
# choice has a margin of 158 resp. 271 counts, and the last sum (2202 after 2929) shows why the running maximum matters.
# ---------------------------------------------------------------------------------------------------------------------
def stars_problem():
    p, N, B = 16, 400, 12
    Th = np.eye(p)
    Th[np.arange(p - 1), np.arange(1, p)] = Th[np.arange(1, p), np.arange(p - 1)] = 0.4
    Th[0, 5] = Th[5, 0] = 0.3
    X = np.linalg.cholesky(np.linalg.inv(Th)) @ np.random.default_rng(7).standard_normal((p, N))
    indices = np.stack([np.sort(np.random.default_rng([3, r]).choice(N, 200, replace=False)) for r in range(B)])
    return X, indices


@pytest.fixture(scope="module")
def device_run():
    from gglasso_amd import model_selection as ms
    X, indices = stars_problem()
    sol, stats = ms.stars_search(X, LAM, beta=0.05, indices=indices, tol=1e-8, rtol=1e-8, store_all=True)
    return X, indices, sol, stats


def test_stars_search_statistics_are_numpy_on_the_returned_theta(device_run):
    from gglasso_amd import model_selection as ms
    X, indices, sol, stats = device_run
    p, B, L = 16, 12, len(LAM)
    assert np.array_equal(stats['LAMBDA'], LAM) and stats['THETA'].shape == (L, B, p, p)
    counts, num = numpy_edges(stats['THETA'].reshape(L * B, p, p), L, B, T_EDGE)
    print("NUM", stats['NUM'])
    assert np.array_equal(stats['COUNTS'], counts) and stats['NUM'] == num
    D = np.array([2 * n / (B * B * (p * (p - 1) // 2)) for n in num])
    assert np.array_equal(stats['INSTABILITY'], D)
    assert np.array_equal(stats['INSTABILITY_MONOTONE'], np.maximum.accumulate(D))
    assert stats['IX'] == 1 and stats['BEST'] == {'lambda1': LAM[1]}
    assert ms.stars_select(stats['INSTABILITY'], 0.1)[0] == 2
    assert stats['NUM'] == NUM
    assert stats['FAILED'] == [] and stats['n_subsamples'] == B and stats['subsample_size'] == 200
    assert np.array_equal(stats['INDICES'], indices)


def test_stars_search_solution_is_the_single_solve_on_all_observations(device_run):
    from gglasso_amd import solver, utils
    X, indices, sol, stats = device_run
    p = X.shape[0]
    ref, _ = solver.ADMM_SGL(utils.sample_covariance(X), stats['LAMBDA'][stats['IX']], np.eye(p), X_0=np.eye(p), tol=1e-8,
                             rtol=1e-8)
    assert sorted(sol) == sorted(ref)
    for nm in ref:
        assert np.array_equal(sol[nm], ref[nm]), nm


def test_stars_search_points_are_the_batch_on_downloaded_covariances(device_run):
    """S written on the device or uploaded: the same bits, the same batch, the same Theta."""
    from gglasso_amd import utils
    from gglasso_amd.batch import ADMM_SGL_batch
    X, indices, sol, stats = device_run
    p, B, L = 16, 12, len(LAM)
    S_sub = utils.sample_covariance_subsets(X, indices)
    res = ADMM_SGL_batch(np.tile(S_sub, (L, 1, 1)), np.repeat(LAM, B), Omega_0=np.eye(p), X_0=np.eye(p), tol=1e-8, rtol=1e-8)
    for l in range(L):
        for r in range(B):
            assert res[l * B + r][1]['status'] == 'optimal'
            assert np.array_equal(stats['THETA'][l, r], res[l * B + r][0]['Theta']), (l, r)


def test_stars_search_is_reproducible_and_chunks_agree(device_run):
    from gglasso_amd import model_selection as ms
    X, indices, sol, stats = device_run
    # the same draws from their seed: the same bits everywhere
    sol2, st2 = ms.stars_search(X, LAM, n_subsamples=12, subsample_size=200, seed=3, beta=0.05, tol=1e-8, rtol=1e-8,
                                store_all=True)
    assert sorted(st2) == sorted(stats)
    for nm in ('LAMBDA', 'INSTABILITY', 'INSTABILITY_MONOTONE', 'INDICES', 'COUNTS', 'THETA'):
        assert np.array_equal(st2[nm], stats[nm]), nm
    for nm in ('NUM', 'IX', 'BEST', 'FAILED', 'subsample_size', 'n_subsamples'):
        assert st2[nm] == stats[nm], nm
    for nm in sol:
        assert np.array_equal(sol2[nm], sol[nm]), nm
    sol3, st3 = ms.stars_search(X, LAM, beta=0.1, indices=indices, tol=1e-8, rtol=1e-8, lambdas_per_batch=3)
    assert st3['NUM'] == stats['NUM'] and st3['IX'] == 2
    assert 'THETA' not in st3 and 'COUNTS' not in st3
    assert ms.stars_search(X, LAM, beta=0.05, indices=indices, tol=1e-8, rtol=1e-8, lambdas_per_batch=3)[1]['IX'] == stats['IX']


# ---------------------------------------------------------------------------------------------------------------------
# 5. the front end
# ---------------------------------------------------------------------------------------------------------------------
def test_glasso_problem_stability_selection(device_run):
    from gglasso_amd import model_selection as ms
    from gglasso_amd.problem import glasso_problem
    X, indices, sol, stats = device_run
    grid = {'lambda1_range': np.array(LAM)}
    P = glasso_problem.from_data(X)
    P.stability_selection(grid, n_subsamples=12, subsample_size=200, seed=3, beta=0.05, tol=1e-8, rtol=1e-8)
    assert P.reg_params['lambda1'] == LAM[1] == stats['BEST']['lambda1']
    assert np.array_equal(P.solution.precision_, sol['Theta'])
    assert np.array_equal(P.solution.adjacency_, (np.abs(sol['Theta']) >= 1e-8) * (1 - np.eye(16, dtype=int)))
    assert sorted(P.modelselect_stats) == sorted(k for k in stats if k not in ('COUNTS', 'THETA'))
    assert P.modelselect_stats['NUM'] == stats['NUM'] and P.modelselect_stats['IX'] == stats['IX']
    assert np.array_equal(P.modelselect_stats['INSTABILITY'], stats['INSTABILITY'])
    assert np.array_equal(P.modelselect_stats['INDICES'], indices)
    # do_scaling: every subsample's own correlations, and the solution back on the covariances' scale as in solve()
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        Q = glasso_problem.from_data(X, do_scaling=True)
    Q.stability_selection(grid, n_subsamples=12, subsample_size=200, seed=3, beta=0.05, tol=1e-8, rtol=1e-8)
    sol_c, st_c = ms.stars_search(X, LAM, n_subsamples=12, subsample_size=200, seed=3, beta=0.05, scale=True, tol=1e-8,
                                  rtol=1e-8)
    assert Q.reg_params['lambda1'] == st_c['BEST']['lambda1'] and Q.modelselect_stats['NUM'] == st_c['NUM']
    assert np.array_equal(Q.solution.precision_, Q._from_correlations(sol_c['Theta']))
    # the refusals
    with pytest.raises(AssertionError, match=r"build the problem with glasso_problem.from_data"):
        glasso_problem(np.cov(X, bias=True), 400).stability_selection(grid)
    with pytest.raises(AssertionError, match=r"Single Graphical Lasso problems only"):
        glasso_problem.from_data(np.stack([X, X])).stability_selection(grid)
    with pytest.raises(AssertionError, match=r"latent variables"):
        glasso_problem.from_data(X, latent=True).stability_selection(grid)
    with pytest.raises(AssertionError, match=r"lambda1_mask"):
        glasso_problem.from_data(X).stability_selection({**grid, 'lambda1_mask': np.ones((16, 16))})
