"""Latent correlation of mixed binary / continuous data on the device (ggl_mixed_correlation, ggl_set_S_from_mixed; kernels
k_bridge_zero_counts and k_bridge_invert of csrc/bridge.hip) and the drivers on top of them.

The yardstick is tests/bridge_ref.py: scipy's quad, ndtri and brentq.  Integers (the counts G, the zero counts, the number of
clipped pairs) are compared exactly.  For every pair with a binary variable that the reference does not clip,

    |F_ref(r; Delta_ref) - tau| <= TOL_F     and     |r - r_ref| <= TOL_F / F'_ref(r_ref) + 4 u.

TOL_F is 4 times the largest residual measured on the MI355X over the shapes of this file (RESIDUAL_MEASURED; the factor is
for differences between math-library versions), and it may never exceed 1e-12: there the error in r is far below the sampling
error wherever F' >= 1e-3.  Measured: 4.58e-16 at (33, 40, binary), (33, 150, interleaved) and (65, 40, binary), and
4.66e-16 for |r - r_ref| F'(r_ref); the numpy twin reaches the same 4.6e-16 on the same data (the reference's own quadrature
and the rounding of tau are part of both figures).

Shapes: one wave solves one pair and a workgroup holds four, the diagonal is written by the waves behind the last pair; p = 1
(no pair), 2 (one), 7, 33, 65 put the pair count off every multiple of 4 and 64, with one and several workgroups."""
import ctypes
import warnings

import numpy as np
import pytest

from bridge_ref import CLIP, F_ref, dF_ref, make_mixed, pair_table, types_ref
from kendall_ref import counts_ref

pytestmark = pytest.mark.gpu

U = 2.0 ** -53
P_ALL = (1, 2, 7, 33, 65)
N_ALL = (40, 150)
KINDS = ('binary', 'continuous', 'interleaved')
RESIDUAL_MEASURED = 4.58e-16               # MI355X, every shape of this file (profiles/mixed_correlation.txt): 33/8 of 2^-53
TOL_F = 4 * RESIDUAL_MEASURED
# the drawn inputs on which the reference clips no pair (asserted below): there the residual check covers every pair
NO_CLIP = {(p, 150, 'interleaved') for p in P_ALL} | {(p, N, 'continuous') for p in P_ALL for N in N_ALL}

_cache = {}


def n_binary(p, kind):
    return {'binary': p, 'continuous': 0, 'interleaved': (p + 1) // 2}[kind]


def reference(p, N, kind):
    """(X, rows, n0, G) of a shape and kind (bridge_ref.pair_table): computed once, shared, read-only."""
    key = (p, N, kind)
    if key not in _cache:
        X = make_mixed(p, N, n_binary(p, kind), 1)
        rows, n0, G = pair_table(X)
        for a in (X, n0, G):
            a.setflags(write=False)
        _cache[key] = (X, rows, n0, G)
    return _cache[key]


def check_against_reference(X, S, info, rows, n0, G_dev, G):
    """The exact parts, and (largest residual, largest |r - r_ref| F'(r_ref)) over the pairs the reference does not clip."""
    p = X.shape[0]
    t = types_ref(X)
    assert np.array_equal(info['types'], t)
    assert G_dev.dtype == np.int64 and np.array_equal(G_dev, G)
    assert info['zero_counts'].dtype == np.int32 and np.array_equal(info['zero_counts'], n0)
    assert np.array_equal(S, S.T) and np.array_equal(np.diag(S), np.ones(p))
    assert info['clipped'] == sum(q['clipped'] for q in rows)
    res = err = 0.0
    for q in rows:
        r = S[q['i'], q['j']]
        if q['clipped']:
            assert r == q['r'], q                                        # +-clip, exactly
            continue
        f = abs(F_ref(r, q['h'], q['k'], q['bb']) - q['tau'])
        d = dF_ref(q['r'], q['h'], q['k'], q['bb'])
        assert f <= TOL_F, (q, r, f)
        assert abs(r - q['r']) <= TOL_F / d + 4 * U, (q, r)
        res, err = max(res, f), max(err, abs(r - q['r']) * d)
    return res, err


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("p,N", [(p, N) for p in P_ALL for N in N_ALL])
def test_matrix_against_the_reference(p, N, kind):
    from gglasso_amd import utils
    X, rows, n0, G = reference(p, N, kind)
    S, info = utils.mixed_correlation(X, return_info=True)
    assert S.shape == (p, p) and S.dtype == np.float64
    res, err = check_against_reference(X, S, info, rows, n0, utils.kendall_counts(X), G)
    print(f"mixed ({p}, {N}, {kind}): {len(rows)} bridged pairs, {info['clipped']} clipped, largest |F_ref(r) - tau| {res:.3e}, "
          f"largest |r - r_ref| F' {err:.3e} (bound {TOL_F:.3e})")
    assert TOL_F <= 1e-12
    if (p, N, kind) in NO_CLIP:
        assert info['clipped'] == 0
    S2, info2 = utils.mixed_correlation(X, return_info=True)              # two calls, the same bits
    assert np.array_equal(S2, S) and info2['clipped'] == info['clipped']
    # a pair of continuous variables on data without ties: the skeptic entry
    t = info['types']
    if p > 1 and not t.all():
        cc = np.outer(t == 0, t == 0) & ~np.eye(p, dtype=bool)
        Sk = utils.skeptic_correlation(X[t == 0]) if (t == 0).sum() > 1 else np.ones((1, 1))
        assert np.abs(S[cc] - Sk[~np.eye(Sk.shape[0], dtype=bool)]).max(initial=0.0) <= 4 * U
    # increasing transforms, a recoding of the binary variables included, change nothing
    Y = X.copy()
    Y[t == 1] = 3.0 * X[t == 1] - 1.0
    Y[t == 0] = np.log(X[t == 0]) ** 3
    assert np.array_equal(utils.mixed_correlation(Y), S)


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("p,N", [(p, N) for p in P_ALL for N in N_ALL])
def test_subsets_are_the_matrices_of_the_gathered_columns(p, N, kind):
    from gglasso_amd import utils
    X = reference(p, N, kind)[0]
    B, b = 3, int(0.8 * N)
    rng = np.random.default_rng([p, N, 7])
    idx = np.stack([rng.choice(N, b, replace=False) for _ in range(B)]).astype(np.int32)
    idx[1, :4] = idx[1, 4:8]                                             # duplicated indices in one subset
    S, info = utils.mixed_correlation(X, indices=idx, return_info=True)
    assert S.shape == (B, p, p) and info['zero_counts'].shape == (B, p) and info['clipped'].shape == (B,)
    G = utils.kendall_counts(X, idx)
    for r in range(B):
        Xr = np.ascontiguousarray(X[:, idx[r]])
        assert np.array_equal(G[r], counts_ref(Xr))
        assert np.array_equal(info['zero_counts'][r], (Xr == X.min(axis=1, keepdims=True)).sum(axis=1))   # rank 0 of ALL samples
        S1, i1 = utils.mixed_correlation(Xr, types=info['types'], return_info=True)
        assert np.array_equal(S[r], S1) and info['clipped'][r] == i1['clipped'], (p, N, kind, r)
    S2 = utils.mixed_correlation(X, indices=idx)
    assert np.array_equal(S2, S)
    # a stack of instances takes one call each
    S3 = utils.mixed_correlation(np.stack([X, X]), indices=idx)
    assert S3.shape == (2, B, p, p) and np.array_equal(S3[0], S) and np.array_equal(S3[1], S)


def test_an_iteration_that_ends_within_a_bit_of_its_tolerance():
    """n = 2000, n0 = 1426, G = 22916 (a pair of tools/bench_mixed.py's data): the second Newton iterate has |H - tau| =
    4.39e-16 against the 4.44e-16 at which the iteration ends.  Lanes whose sums differed in the last bit disagreed there,
    some went on over a part of the wave and returned 0.0596 for 0.0298."""
    from gglasso_amd import utils
    y = np.r_[np.zeros(732), np.ones(22), np.zeros(1), np.ones(552), np.zeros(693)]        # the binary variable along the
    X = np.stack([y, np.exp(np.arange(2000) / 500.0)])                                      # order of the continuous one
    rows, n0, G = pair_table(X)
    assert n0[0] == 1426 and G[0, 1] == 22916 and not rows[0]['clipped']
    S, info = utils.mixed_correlation(X, return_info=True)
    check_against_reference(X, S, info, rows, n0, utils.kendall_counts(X), G)
    assert abs(S[0, 1] - 0.029823945575486687) <= 1e-14


def test_duplicated_and_complemented_binary_rows_are_clipped():
    from gglasso_amd import utils
    X = reference(7, 150, 'interleaved')[0]
    Y = np.concatenate([X, X[:1], 1.0 - X[:1]])                          # rows 7, 8: variable 0 and its complement
    for clip in (CLIP, 0.9):
        S, info = utils.mixed_correlation(Y, clip=clip, return_info=True)
        assert S[0, 7] == clip and S[0, 8] == -clip and S[7, 8] == -clip
        rows, n0, _ = pair_table(Y, clip=clip)
        assert info['clipped'] == sum(q['clipped'] for q in rows) >= 3
        for q in rows:
            if q['clipped']:
                assert S[q['i'], q['j']] == q['r'] and S[q['j'], q['i']] == q['r']
        assert np.array_equal(S, S.T) and np.array_equal(np.diag(S), np.ones(9))
        Sh, ih = utils.host_mixed_correlation(Y, clip=clip, return_info=True)
        assert ih['clipped'] == info['clipped'] and np.abs(Sh - S).max() <= 1e-12


def test_ctx_takes_its_S_from_mixed_and_keeps_it_when_a_call_is_refused():
    from gglasso_amd import utils
    from gglasso_amd.solver import HipEngine
    p, N, L, B = 7, 150, 2, 3
    X = reference(p, N, 'interleaved')[0]
    b = 120
    idx = np.random.default_rng(9).integers(0, N, (B, b)).astype(np.int32)
    S_op = utils.mixed_correlation(X, indices=idx)
    eye = np.broadcast_to(np.eye(p), (L * B, p, p))
    eng = HipEngine(eye, eye, eye, 0 * eye)
    try:
        eng.set_mixed_subsets(X, idx)
        S = eng.get_S()
        assert np.array_equal(S, np.tile(S_op, (L, 1, 1)))               # instance k: subset k % B
        flat = X.copy()
        flat[3] = 2.5                                                     # a constant variable: found on the host
        with pytest.raises(AssertionError, match=r"variable 3 is constant"):
            eng.set_mixed_subsets(flat, idx)
        assert np.array_equal(eng.get_S(), S)
        one = X.copy()                                                    # binary variable 2: one value only over subset 1
        one[2] = 0.0
        one[2, np.setdiff1d(np.arange(N), idx[1])] = 1.0
        assert all(len(set(one[2, idx[r]])) == 2 for r in (0, 2))
        with pytest.raises(AssertionError, match=r"variable 2 is constant over subset 1"):
            eng.set_mixed_subsets(one, idx)
        assert np.array_equal(eng.get_S(), S)
        with pytest.raises(AssertionError, match=r"variable 2 is constant over subset 1"):
            utils.mixed_correlation(one, indices=idx)
        bad = utils.variable_types(X)
        bad[4] = 2
        with pytest.raises(AssertionError, match=r"types\[4\] = 2"):
            eng.set_mixed_subsets(X, idx, types=bad)
        assert np.array_equal(eng.get_S(), S)
        with pytest.raises(AssertionError, match=r"variable 1 is marked binary"):
            eng.set_mixed_subsets(X, idx, types=np.ones(p, dtype=np.int32))
        assert np.array_equal(eng.get_S(), S)
        for clip in (0.0, 1.0, -0.3, float('nan')):
            with pytest.raises(AssertionError, match=r"clip"):
                eng.set_mixed_subsets(X, idx, clip=clip)
            assert np.array_equal(eng.get_S(), S)
        eng.set_mixed_subsets(X)                                          # all observations, every instance
        assert np.array_equal(eng.get_S(), np.tile(utils.mixed_correlation(X)[None], (L * B, 1, 1)))
    finally:
        eng.close()


def test_a_refused_call_writes_nothing():
    from gglasso_amd import _lib, utils
    lib = _lib.load()
    p, N = 7, 40
    X = reference(p, N, 'interleaved')[0]
    R, t = utils.dense_ranks(X), utils.variable_types(X)
    ip = lambda a: None if a is None else a.ctypes.data_as(_lib._ip)
    S = np.full((1, p, p), 7.0)
    G = np.full((1, p, p), 7, dtype=np.int64)
    n0, cl = np.full((1, p), 7, dtype=np.int32), np.full(1, 7, dtype=np.int32)
    gp = G.ctypes.data_as(ctypes.POINTER(ctypes.c_longlong))
    call = lambda R_, t_, clip: lib.ggl_mixed_correlation(0, p, N, ip(R_), ip(t_), 1, N, None, clip, _lib.ptr(S), gp, ip(n0), ip(cl))
    t_bad = t.copy()
    t_bad[0] = -1
    R_flat = R.copy()
    R_flat[5] = 0
    for args, text in (((R, t_bad, CLIP), "types[0] = -1"), ((R, np.ones(p, dtype=np.int32), CLIP), "marked binary"),
                       ((R, t, 1.0), "clip"), ((R, t, 0.0), "clip"), ((R_flat, t, CLIP), "variable 5 is constant"),
                       ((R, None, CLIP), "types"), ((None, t, CLIP), "ranks")):
        assert call(*args) == _lib.E_ARG and text in _lib.last_error(), (text, _lib.last_error())
        assert (S == 7.0).all() and (G == 7).all() and (n0 == 7).all() and (cl == 7).all()
    assert call(R, t, CLIP) == 0
    assert np.array_equal(S[0], utils.mixed_correlation(X)) and np.array_equal(G[0], counts_ref(X))
    # the optional outputs may be NULL
    S1 = np.empty((1, p, p))
    assert lib.ggl_mixed_correlation(0, p, N, ip(R), ip(t), 1, N, None, CLIP, _lib.ptr(S1), None, None, None) == 0
    assert np.array_equal(S1, S)
    assert lib.ggl_mixed_correlation(0, p, N, ip(R), ip(t), 1, N, None, CLIP, None, None, None, None) == _lib.E_ARG


def e2e_problem():
    p, N, B = 12, 80, 4
    X = make_mixed(p, N, 6, 13)
    idx = np.stack([np.sort(np.random.default_rng([2, r]).choice(N, 60, replace=False)) for r in range(B)])
    return X, idx


def test_stars_search_mixed_device_route_is_the_host_route_on_the_devices_matrices(monkeypatch):
    """p = 12, N = 80, B = 4, L = 3: the device route (S never on the host) against the host route of the same driver, fed
    with the matrices the device computes: the same integers, the same choice, the same bits of the solution."""
    from gglasso_amd import model_selection as ms, solver, utils
    X, idx = e2e_problem()
    lam = [0.5, 0.3, 0.15]
    with warnings.catch_warnings():
        warnings.simplefilter("ignore", RuntimeWarning)
        sol, st = ms.stars_search(X, lam, indices=idx, beta=0.1, correlation='mixed', tol=1e-8, rtol=1e-8)
        monkeypatch.delattr(solver.HipEngine, "set_mixed_subsets")       # an engine without the route ...
        assert not hasattr(solver.ENGINE, "set_mixed_subsets")
        monkeypatch.setattr(utils, "host_mixed_correlation",             # ... whose host matrices are the device's
                            lambda X_, types=None, indices=None, clip=0.999: utils.mixed_correlation(X_, types, indices, clip))
        sol_h, st_h = ms.stars_search(X, lam, indices=idx, beta=0.1, correlation='mixed', tol=1e-8, rtol=1e-8)
    assert st['NUM'] == st_h['NUM'] and st['IX'] == st_h['IX']
    assert np.array_equal(sol['Theta'], sol_h['Theta'])


def test_from_data_mixed_solves_the_problem_of_the_latent_correlation():
    from gglasso_amd import glasso_problem, utils
    X, _ = e2e_problem()
    p, N = X.shape
    S = utils.mixed_correlation(X)
    P = glasso_problem.from_data(X, correlation='mixed', reg_params={'lambda1': 0.2})
    assert np.array_equal(P.S, S) and np.abs(P.S - utils.host_mixed_correlation(X)).max() <= 1e-12
    P.solve(tol=1e-9, rtol=1e-9)
    Q = glasso_problem(S, N, reg_params={'lambda1': 0.2})
    Q.solve(tol=1e-9, rtol=1e-9)
    assert np.array_equal(P.solution.precision_, Q.solution.precision_)
    assert not np.array_equal(P.S, glasso_problem.from_data(X, correlation='kendall').S)
