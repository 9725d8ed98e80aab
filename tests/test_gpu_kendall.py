"""Rank correlation on the device: the counts G = Z Z^T of Kendall's tau on the int8 matrix cores (ggl_kendall_counts), the
skeptic matrix sin(pi/2 tau-b) (ggl_kendall_skeptic, ggl_set_S_from_kendall) and the drivers on top of them.

The yardstick of G is the numpy brute force of tests/kendall_ref.py, compared as integers: a fragment loaded from the wrong
row, a wrong C/D map, a pair counted twice or a float accumulation changes some integer.  Tile side 64, pair block 64,
a-chunk 1024 of the kernel: the shapes take a point on each side of every one of them.

The skeptic matrix is compared with numpy's sin(pi/2 G_ij / sqrt(G_ii G_jj)) on the SAME integers.  Largest deviation
measured on the MI355X over the shapes of this file: see SKEPTIC_MEASURED; the bound is 4 times that, and it must stay
below 1e-13 (a wrong constant or a missing square root is off by far more)."""
import ctypes
import warnings

import numpy as np
import pytest

from kendall_ref import counts_ref, make_data, skeptic_ref

pytestmark = pytest.mark.gpu

P_ALL = (1, 2, 15, 16, 17, 63, 64, 65, 130)
N_ALL = (2, 3, 17, 63, 64, 65, 129, 300)
SHAPES = sorted({(p, N) for p in P_ALL for N in (17, 65)} | {(p, N) for p in (17, 65) for N in N_ALL}
                | {(1, 2), (2, 3), (130, 300), (3, 1025), (17, 1027)})
KINDS = ('continuous', 'tied', 'constant')
SKEPTIC_MEASURED = 1.1103e-16              # 2^-53: one rounding of a value below 1 (MI355X, every shape of this file)
SKEPTIC_BOUND = 4 * SKEPTIC_MEASURED

_cache = {}


def reference(p, N, kind):
    """(X, G) of a shape and kind: computed once, shared, read-only."""
    key = (p, N, kind)
    if key not in _cache:
        X = make_data(p, N, kind)
        G = counts_ref(X)
        X.setflags(write=False)
        G.setflags(write=False)
        _cache[key] = (X, G)
    return _cache[key]


@pytest.mark.parametrize("p,N", SHAPES)
def test_counts_are_the_exact_integers(p, N):
    from gglasso_amd import utils
    for kind in KINDS:
        X, G_ref = reference(p, N, kind)
        G = utils.kendall_counts(X)
        assert G.dtype == np.int64 and G.shape == (p, p)
        assert np.array_equal(G, G_ref), (p, N, kind, int(np.abs(G - G_ref).max()))
        if kind == 'constant':
            assert not G[p // 2].any() and not G[:, p // 2].any()
            with pytest.raises(AssertionError, match=rf"variable {p // 2} is constant over subset 0"):
                utils.skeptic_correlation(X)


def test_counts_are_invariant_under_monotone_transforms():
    from gglasso_amd import utils
    X, G = reference(65, 129, 'continuous')
    assert np.array_equal(utils.kendall_counts(np.exp(X)), G)
    assert np.array_equal(utils.kendall_counts(X ** 3), G)
    flip = np.where(np.arange(65) % 3 == 0, -1.0, 1.0)
    assert np.array_equal(utils.kendall_counts(X * flip[:, None]), G * np.outer(flip, flip).astype(np.int64))
    Xt, Gt = reference(17, 65, 'tied')
    assert np.array_equal(utils.kendall_counts(np.exp(Xt)), Gt) and np.array_equal(utils.kendall_counts(-Xt), Gt)


@pytest.mark.parametrize("B,b", [(1, 2), (1, 100), (3, 31), (3, 64), (5, 2), (5, 100)])
def test_subsets_are_the_counts_of_gathered_columns(B, b):
    from gglasso_amd import utils
    p, N = 17, 150
    X = make_data(p, N, 'tied', seed=1) + (make_data(p, N, 'continuous', seed=1) if B == 3 else 0.0)
    rng = np.random.default_rng([B, b])
    idx = rng.integers(0, N, (B, b)).astype(np.int32)
    idx[0] = np.sort(rng.choice(N, b, replace=False))[::-1]             # reversed order
    if B > 1:
        idx[1, 1] = idx[1, 0]                                            # a duplicated index: a tied pair in every variable
    G = utils.kendall_counts(X, idx)
    assert G.shape == (B, p, p) and G.dtype == np.int64
    for r in range(B):
        Xr = np.ascontiguousarray(X[:, idx[r]])
        assert np.array_equal(G[r], counts_ref(Xr)), (B, b, r)
        assert np.array_equal(G[r], utils.kendall_counts(Xr)), (B, b, r)
    assert np.array_equal(utils.kendall_counts(X, idx), G)              # two calls, the same bits
    # a stack and a dict of instances take one call each
    G2 = utils.kendall_counts(np.stack([X, -X]), idx)
    assert G2.shape == (2, B, p, p) and np.array_equal(G2[0], G) and np.array_equal(G2[1], G)
    Gd = utils.kendall_counts({0: X, 1: X[:5, :40]})
    assert np.array_equal(Gd[0], utils.kendall_counts(X)) and np.array_equal(Gd[1], counts_ref(X[:5, :40]))


def test_counts_beyond_32_bits():
    """p = 3, N = 70 000: 2.45e9 pairs.  Increasing, decreasing and floor(n / 1000): closed forms, no reference run."""
    from gglasso_amd import utils
    N = 70000
    n = np.arange(N, dtype=np.float64)
    X = np.stack([n, -n, np.floor(n / 1000)])
    G = utils.kendall_counts(X)
    full = N * (N - 1) // 2
    assert full > 2 ** 31
    block = full - 70 * (1000 * 999 // 2)
    want = np.array([[full, -full, block], [-full, full, -block], [block, -block, block]], dtype=np.int64)
    assert np.array_equal(G, want), (G, want)


def numpy_skeptic(G):
    d = np.diag(G).astype(np.float64)
    return np.sin(np.pi / 2 * (G / np.sqrt(np.outer(d, d))))


def test_skeptic_matrix():
    from gglasso_amd import utils
    worst = 0.0
    for p, N in SHAPES:
        for kind in ('continuous', 'tied'):
            X, G = reference(p, N, kind)
            if not np.all(np.diag(G) > 0):
                continue
            S = utils.skeptic_correlation(X)
            assert np.array_equal(np.diag(S), np.ones(p)) and np.array_equal(S, S.T), (p, N, kind)
            off = ~np.eye(p, dtype=bool)
            dev = float(np.abs(S - numpy_skeptic(G))[off].max()) if p > 1 else 0.0
            worst = max(worst, dev)
            T = utils.kendall_tau(X)
            assert np.array_equal(np.diag(T), np.ones(p))
            d = np.diag(G).astype(np.float64)
            assert np.array_equal(T[off], (G / np.sqrt(np.outer(d, d)))[off])
    print(f"skeptic: largest deviation from numpy on the same integers {worst:.3e} (bound {SKEPTIC_BOUND:.3e})")
    assert SKEPTIC_BOUND < 1e-13
    assert worst <= SKEPTIC_BOUND, worst
    # subsets: each its own matrix; a variable constant over ONE subset is refused, naming both
    X, _ = reference(17, 129, 'tied')
    idx = np.stack([np.arange(0, 60), np.arange(60, 120)]).astype(np.int32)
    S = utils.skeptic_correlation(X, idx)
    for r in range(2):
        assert np.array_equal(S[r], utils.skeptic_correlation(np.ascontiguousarray(X[:, idx[r]])))
    flat = X.copy()
    flat[4, idx[1]] = 2.0
    with pytest.raises(AssertionError, match=r"variable 4 is constant over subset 1"):
        utils.skeptic_correlation(flat, idx)


def test_ctx_takes_its_S_from_kendall_and_keeps_it_when_a_call_is_refused():
    from gglasso_amd import utils
    from gglasso_amd.solver import HipEngine
    p, N, L, B, b = 17, 65, 2, 3, 40
    X, _ = reference(p, N, 'continuous')                                # (ties come from the repeated indices only)
    rng = np.random.default_rng(9)
    idx = rng.integers(0, N, (B, b)).astype(np.int32)
    S_op = utils.skeptic_correlation(X, idx)
    eye = np.broadcast_to(np.eye(p), (L * B, p, p))
    eng = HipEngine(eye, eye, eye, 0 * eye)
    try:
        eng.set_kendall_subsets(X, idx)
        S = eng.get_S()
        assert np.array_equal(S, np.tile(S_op, (L, 1, 1)))
        flat = X.copy()
        flat[6, idx[2]] = -1.0
        with pytest.raises(AssertionError, match=r"variable 6 is constant over subset 2"):
            eng.set_kendall_subsets(flat, idx)
        assert np.array_equal(eng.get_S(), S)
        bad = idx.copy()
        bad[1, 7] = N
        with pytest.raises(AssertionError, match=rf"subset 1, position 7 holds the index {N}"):
            eng.set_kendall_subsets(X, bad)
        assert np.array_equal(eng.get_S(), S)
        eng.set_kendall_subsets(X)                                       # all observations, every instance
        assert np.array_equal(eng.get_S(), np.tile(utils.skeptic_correlation(X)[None], (L * B, 1, 1)))
    finally:
        eng.close()


def test_misuse_is_refused_and_a_valid_call_follows():
    from gglasso_amd import _lib, utils
    from gglasso_amd.solver import HipEngine
    lib = _lib.load()
    p, N, B, b = 5, 9, 2, 4
    X, _ = reference(17, 17, 'continuous')
    R = utils.dense_ranks(X[:p, :N])
    idx = np.array([[0, 1, 2, 3], [8, 4, 4, 5]], dtype=np.int32)
    G = np.empty((B, p, p), dtype=np.int64)
    S = np.empty((B, p, p))
    ip = lambda a: a.ctypes.data_as(_lib._ip)
    gp, sp = G.ctypes.data_as(ctypes.POINTER(ctypes.c_longlong)), _lib.ptr(S)

    def valid():
        assert lib.ggl_kendall_counts(0, p, N, ip(R), B, b, ip(idx), gp) == 0
        assert lib.ggl_kendall_skeptic(0, p, N, ip(R), B, b, ip(idx), sp, gp) == 0
        assert np.array_equal(G[1], counts_ref(X[:p, :N][:, idx[1]]))

    valid()
    bad = idx.copy()
    bad[1, 0] = N
    neg = idx.copy()
    neg[0, 3] = -1
    for args in ((p, N, ip(R), B, b, ip(bad)), (p, N, ip(R), B, b, ip(neg)), (p, N, ip(R), B, 1, ip(idx)),
                 (p, N, ip(R), 0, b, ip(idx)), (p, N, None, B, b, ip(idx)), (p, N, ip(R), 2, b, None), (p, 1, ip(R), 1, 1, None)):
        assert lib.ggl_kendall_counts(0, *args, gp) == _lib.E_ARG, args[:2] + args[3:5]
        valid()
        assert lib.ggl_kendall_skeptic(0, *args, sp, None) == _lib.E_ARG
        valid()
    assert lib.ggl_kendall_counts(0, p, N, ip(R), B, b, ip(bad), gp) == _lib.E_ARG
    assert "subset 1, position 0 holds the index 9" in _lib.last_error()
    valid()
    assert lib.ggl_kendall_counts(0, p, N, ip(R), B, b, ip(idx), None) == _lib.E_ARG
    assert lib.ggl_kendall_skeptic(0, p, N, ip(R), B, b, ip(idx), None, gp) == _lib.E_ARG
    # a shape beyond one launch (b-blocks x a-chunks >= 2^24) is an argument error, found on the host
    Nbig = 1100000
    Rbig = np.zeros((1, Nbig), dtype=np.int32)
    Gbig = np.empty((1, 1, 1), dtype=np.int64)
    assert lib.ggl_kendall_counts(0, 1, Nbig, ip(Rbig), 1, Nbig, None, Gbig.ctypes.data_as(ctypes.POINTER(ctypes.c_longlong))) == _lib.E_ARG
    assert "one launch" in _lib.last_error()
    valid()
    Rbad = R.copy()
    Rbad[2, 3] = N
    assert lib.ggl_kendall_counts(0, p, N, ip(Rbad), B, b, ip(idx), gp) == _lib.E_ARG
    valid()
    # the ctx route: K % B != 0, instance dimensions, and the cases above
    eye = np.broadcast_to(np.eye(p), (3, p, p))
    eng = HipEngine(eye, eye, eye, 0 * eye)
    try:
        one = idx[:1]
        assert lib.ggl_set_S_from_kendall(None, ip(R), N, 1, b, ip(one)) == _lib.E_ARG
        assert lib.ggl_set_S_from_kendall(eng.h, ip(R), N, 1, b, ip(one)) == 0
        S0 = eng.get_S()
        assert lib.ggl_set_S_from_kendall(eng.h, ip(R), N, B, b, ip(idx)) == _lib.E_ARG       # 2 subsets, 3 instances
        assert "do not divide" in _lib.last_error()
        assert lib.ggl_set_S_from_kendall(eng.h, ip(R), N, 1, 1, ip(one)) == _lib.E_ARG       # b < 2
        assert lib.ggl_set_S_from_kendall(eng.h, ip(R), N, 0, b, ip(one)) == _lib.E_ARG       # B < 1
        assert lib.ggl_set_S_from_kendall(eng.h, ip(R), N, 1, b, ip(bad[1:])) == _lib.E_ARG   # an index outside
        eng.set_instance_dims(np.full(3, p - 1))
        assert lib.ggl_set_S_from_kendall(eng.h, ip(R), N, 1, b, ip(one)) == _lib.E_ARG
        assert "instance dimensions" in _lib.last_error()
        eng.set_instance_dims(None)
        assert np.array_equal(eng.get_S(), S0)
        assert lib.ggl_set_S_from_kendall(eng.h, ip(R), N, 1, N, None) == 0
        assert np.array_equal(eng.get_S()[2], utils.skeptic_correlation(X[:p, :N]))
    finally:
        eng.close()


def e2e_problem():
    p, N, B = 12, 60, 4
    Th = np.eye(p)
    Th[np.arange(p - 1), np.arange(1, p)] = Th[np.arange(1, p), np.arange(p - 1)] = 0.4
    Th[0, 5] = Th[5, 0] = 0.3
    X = np.exp(np.linalg.cholesky(np.linalg.inv(Th)) @ np.random.default_rng(13).standard_normal((p, N)))
    idx = np.stack([np.sort(np.random.default_rng([2, r]).choice(N, 45, replace=False)) for r in range(B)])
    return X, idx


def test_stars_search_kendall_device_and_host_routes_agree(monkeypatch):
    from gglasso_amd import model_selection as ms, solver
    X, idx = e2e_problem()
    lam = [0.5, 0.3, 0.15]
    with warnings.catch_warnings():
        warnings.simplefilter("ignore", RuntimeWarning)
        sol, st = ms.stars_search(X, lam, indices=idx, beta=0.1, correlation='kendall', tol=1e-8, rtol=1e-8)
        monkeypatch.delattr(solver.HipEngine, "set_kendall_subsets")     # an engine without the route: the numpy fallback
        assert not hasattr(solver.ENGINE, "set_kendall_subsets")
        sol_h, st_h = ms.stars_search(X, lam, indices=idx, beta=0.1, correlation='kendall', tol=1e-8, rtol=1e-8)
    assert st['NUM'] == st_h['NUM'] and st['IX'] == st_h['IX']
    assert np.abs(sol['Theta'] - sol_h['Theta']).max() <= 1e-12


def test_from_data_kendall_solves_the_problem_of_the_skeptic_matrix():
    from gglasso_amd import glasso_problem, solver
    X, _ = e2e_problem()
    p, N = X.shape
    S_ref = skeptic_ref(counts_ref(X))
    P = glasso_problem.from_data(X, correlation='kendall', reg_params={'lambda1': 0.2})
    # (the bound of tests/test_gpu_problem.py for a from_data S against the host's)
    assert np.abs(P.S - S_ref).max() <= 1e-12 and np.array_equal(np.diag(P.S), np.ones(p))
    P.solve(tol=1e-9, rtol=1e-9)
    Q = glasso_problem(S_ref, N, reg_params={'lambda1': 0.2})
    Q.solve(tol=1e-9, rtol=1e-9)
    assert np.abs(P.solution.precision_ - Q.solution.precision_).max() <= 1e-12
    # ADMM_SGL on the reference's matrix: both are optima of one strictly convex problem, each within its stopping tolerance
    eye = np.eye(p)
    sol, _ = solver.ADMM_SGL(S_ref, 0.2, eye, X_0=eye, tol=1e-9, rtol=1e-9, verbose=False)
    assert np.abs(P.solution.precision_ - sol['Theta']).max() <= 1e-6
