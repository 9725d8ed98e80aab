"""Pairwise-complete covariance of data with missing values on the device (covariance_missing.hip behind
ggl_covariance_pairwise, ggl_covariance_pairwise_subsets, ggl_set_S_from_data_pairwise, ggl_set_S_from_subsets_pairwise) and
what is built on it (utils.sample_covariance(missing='pairwise'), HipEngine.set_data, glasso_problem.from_data, stars_search).

Comparison value, bound and data: tests/pairwise_ref.py --  |S_dev - S_ref|_ij <= (3 n_ij + 16) u D_ij elementwise against the
definition evaluated in numpy.longdouble; row means in +-1e3 and std in 0.1-10, so a wrong centring, a leaked padded column
or a NaN taken for a value is ~1e6 (or NaN) against a bound of ~1e-13.  Largest |S_dev - S_ref| / bound measured over this
file on the MI355X: see DESIGN.md section 18 (the last test prints it).
"""
import contextlib
import ctypes
import functools
import io

import numpy as np
import pytest

import pairwise_ref as pr

pytestmark = pytest.mark.gpu

U = 2.0 ** -53
P_ALL = (1, 2, 15, 17, 33, 65, 70)
N_ALL = (1, 3, 16, 17, 33, 65, 130)
TILES = (4, 8, 0)                                   # GGL_COV_TILE32, GGL_COV_TILE64, the library's choice
WORST = {"ratio": 0.0, "where": None, "checked": 0}


@functools.lru_cache(maxsize=None)
def case(p, N, pattern, seed=0):
    """(X, reference centred, reference raw) of one case, computed once; None where the shape has no room for the pattern."""
    X = pr.make_case(p, N, pattern, seed)
    if X is None:
        return None
    X.setflags(write=False)
    return X, pr.reference(X, True), pr.reference(X, False)


def pw(Xs, flags, min_pairs=2, counts=True):
    from gglasso_amd import utils
    return utils._covariance_pairwise_call([np.ascontiguousarray(x) for x in Xs], flags, min_pairs, counts)


def check(S, cnt, ref, what):
    assert np.array_equal(cnt, ref[1]), what                         # n_ij, exact
    assert np.array_equal(S, S.T), what                               # one evaluation per pair
    r = pr.ratio(S, ref)
    WORST["checked"] += 1
    if r > WORST["ratio"]:
        WORST["ratio"], WORST["where"] = r, what
    print(what, "max |S - S_ref| / bound =", r)
    assert r <= 1.0, (what, r)


@pytest.mark.parametrize("N", N_ALL)
@pytest.mark.parametrize("p", P_ALL)
def test_pairwise_covariance_within_derived_bound(p, N):
    from gglasso_amd import _lib
    mp = 1 if N == 1 else 2                                           # one sample: every pair shares exactly one
    ran = 0
    for pattern in pr.PATTERNS:
        c = case(p, N, pattern)
        if c is None:
            continue
        X, ref_c, ref_r = c
        for tile in TILES:
            S, _, cnt = pw([X], _lib.COV_CENTER | tile, mp)
            check(S[0], cnt[0], ref_c, (p, N, pattern, tile, "centred"))
            S2, _, cnt2 = pw([X], _lib.COV_CENTER | tile, mp)
            assert np.array_equal(S, S2) and np.array_equal(cnt, cnt2)            # fixed reduction order: the same bits
            R, _, rcnt = pw([X], tile, mp)
            check(R[0], rcnt[0], ref_r, (p, N, pattern, tile, "raw"))
            if N == 1:
                assert not S.any()                                    # x - mean(x) = 0 exactly
            ran += 1
    assert ran >= 3


@pytest.mark.parametrize("tile", (4, 8))
def test_ragged_batch_equals_single_instances(tile):
    from gglasso_amd import _lib
    p = 33
    cases = [case(p, 17, "r30"), case(p, 65, "lastcol"), case(p, 130, "slab")]
    S, _, cnt = pw([c[0] for c in cases], _lib.COV_CENTER | tile)
    for k, (X, ref_c, _) in enumerate(cases):
        check(S[k], cnt[k], ref_c, (p, "K=3", k, tile))
        alone, _, acnt = pw([X], _lib.COV_CENTER | tile)
        assert np.array_equal(S[k], alone[0]) and np.array_equal(cnt[k], acnt[0]), k         # no cross-instance leakage
    # nine instances take the other branch of the tile decoding
    nine = [case(17, 5 + k, "r60", 10 + k) for k in range(9)]
    S9, _, cnt9 = pw([c[0] for c in nine], _lib.COV_CENTER | tile)
    for k, (X, ref_c, _) in enumerate(nine):
        check(S9[k], cnt9[k], ref_c, (17, "K=9", k, tile))
        alone, _, _ = pw([X], _lib.COV_CENTER | tile)
        assert np.array_equal(S9[k], alone[0]), k


@pytest.mark.parametrize("p,N", [(17, 33), (65, 130), (70, 65)])
def test_complete_data_agrees_with_the_complete_route(p, N):
    """Without a NaN every count is N and the two estimators are the same number: the two device results differ by at most
    the sum of their bounds (this file's and tests/test_gpu_covariance.py's, each against its own longdouble value)."""
    import test_gpu_covariance as tgc
    from gglasso_amd import _lib, utils
    X, ref_c, ref_r = case(p, N, "none")
    for center, ref in ((True, ref_c), (False, ref_r)):
        flags = _lib.COV_CENTER if center else 0
        S, _, cnt = pw([X], flags)
        assert np.all(cnt == N)
        full, _ = utils._covariance_call([np.ascontiguousarray(X)], flags)
        _, cov_bound = tgc.reference(X, center)
        assert np.all(np.abs(S[0].astype(np.longdouble) - full[0]) <= pr.bound(ref[1], ref[2]) + cov_bound), (p, N, center)


@pytest.mark.parametrize("p,N,K", [(33, 70, 3), (65, 17, 1)])
def test_complete_raw_data_gives_the_bits_of_the_complete_route(p, N, K):
    """Without a NaN and uncentred the pairwise kernel is the plain one: both run the one tile body (gram_nt_tile.hpp), P
    accumulates the same products in the same order and C = N is exact, so P / C has the bits of acc / N.  (Centred, the
    pairwise formula is another expression: test_complete_data_agrees_with_the_complete_route bounds it.)"""
    from gglasso_amd import utils
    Xs = [np.ascontiguousarray(pr.make_case(p, N, "none", 20 + k)) for k in range(K)]
    full, _ = utils._covariance_call(Xs, 0)
    for tile in TILES:
        S, _, cnt = pw(Xs, tile)
        assert np.all(cnt == N), tile
        assert np.array_equal(S, full), tile


def test_missing_none_is_the_complete_data_path_bit_for_bit():
    from gglasso_amd import _lib, utils
    X = np.ascontiguousarray(case(33, 65, "none")[0])
    assert np.array_equal(utils.sample_covariance(X), utils._covariance_call([X], _lib.COV_CENTER)[0][0])
    assert np.array_equal(utils.sample_covariance(X, center=False, missing=None), utils._covariance_call([X], 0)[0][0])
    C, var = utils.sample_covariance(X, scale=True, missing=None, min_pairs=7)
    C2, var2 = utils._covariance_call([X], _lib.COV_CENTER | _lib.COV_SCALE)
    assert np.array_equal(C, C2[0]) and np.array_equal(var, var2[0])
    idx = np.stack([np.arange(0, 40), np.arange(20, 60)])
    assert np.array_equal(utils.sample_covariance_subsets(X, idx, missing=None),
                          utils._covariance_subsets_call(X, idx.astype(np.int32), _lib.COV_CENTER)[0])
    hole = np.array(case(33, 65, "r30")[0])                            # and a NaN still spreads over its row and column there
    assert np.isnan(utils.sample_covariance(hole)).any()


def test_scale_divides_by_the_diagonal_of_this_S():
    from gglasso_amd import _lib, utils
    X = case(33, 130, "r30")[0]
    S, _, _ = pw([X], _lib.COV_CENTER)
    C, var, cnt = pw([X], _lib.COV_CENTER | _lib.COV_SCALE)
    d = np.diag(S[0])
    assert np.array_equal(var[0], d)                                  # each variable's variance over all its observed entries
    assert np.all(np.abs(np.diag(C[0]) - 1.0) <= 4 * U)
    want = S[0] / (np.sqrt(d)[:, None] * np.sqrt(d)[None, :])
    assert np.all(np.abs(C[0] - want) <= 8 * U * np.abs(want))
    assert np.array_equal(C[0], C[0].T)
    C1, var1 = utils.sample_covariance(X, scale=True, missing='pairwise')
    assert np.array_equal(C1, C[0]) and np.array_equal(var1, var[0])
    C3, var3, cnt3 = utils.sample_covariance(X, scale=True, missing='pairwise', return_counts=True)
    assert np.array_equal(C3, C[0]) and np.array_equal(cnt3, cnt[0]) and cnt3.dtype == np.int32


def test_sample_covariance_kinds():
    from gglasso_amd import utils
    X3 = np.stack([case(15, 33, "r30", k)[0] for k in range(3)])
    S3, n3 = utils.sample_covariance(X3, missing='pairwise', return_counts=True)
    assert S3.shape == n3.shape == (3, 15, 15)
    one = utils.sample_covariance(X3[1], missing='pairwise')
    assert one.shape == (15, 15) and np.array_equal(one, S3[1])
    ragged = [case(15, 33, "r30")[0], case(17, 65, "lastcol")[0], case(15, 17, "r60")[0]]
    Sd, nd = utils.sample_covariance(ragged, missing='pairwise', return_counts=True)
    assert sorted(Sd) == sorted(nd) == [0, 1, 2] and [Sd[k].shape[0] for k in range(3)] == [15, 17, 15]
    for k, (pN, pattern) in enumerate((((15, 33), "r30"), ((17, 65), "lastcol"), ((15, 17), "r60"))):
        check(Sd[k], nd[k], case(*pN, pattern)[1], ("dict", k))
    R = utils.sample_covariance(ragged[1], center=False, missing='pairwise')
    check(R, nd[1], case(17, 65, "lastcol")[2], ("raw", 1))


def test_subsets_route_is_the_call_on_host_gathered_columns():
    from gglasso_amd import _lib, utils
    X = case(15, 65, "r30")[0]
    idx = np.stack([np.sort(np.random.default_rng([5, r]).choice(65, 33, replace=False)) for r in range(4)])
    idx[:, :2] = (0, 1)                                               # the two observed columns: every pair shares them
    idx[1, 7] = idx[1, 8]                                             # duplicates: a bootstrap draw
    idx[3, ::-1] = idx[3].copy()                                      # any order
    for flags in (_lib.COV_CENTER, 0, _lib.COV_CENTER | _lib.COV_SCALE, _lib.COV_CENTER | _lib.COV_TILE64):
        S, var, cnt = utils._covariance_pairwise_subsets_call(np.ascontiguousarray(X), idx.astype(np.int32), flags)
        S2, var2, cnt2 = pw([X[:, idx[r]] for r in range(4)], flags)
        assert np.array_equal(S, S2) and np.array_equal(cnt, cnt2), flags
        assert (var is None and var2 is None) or np.array_equal(var, var2)
    Sg, ng = utils.sample_covariance_subsets(X, idx, missing='pairwise', return_counts=True)
    assert np.array_equal(Sg, pw([X[:, idx[r]] for r in range(4)], _lib.COV_CENTER)[0])
    for r in range(4):
        check(Sg[r], ng[r], pr.reference(X[:, idx[r]], True), ("subset", r))


def test_ctx_routes_equal_the_standalone_calls():
    from gglasso_amd import _lib
    from gglasso_amd.solver import HipEngine
    p = 33
    Xs = [case(p, 65, "r30")[0], case(p, 130, "slab")[0]]
    S, _, _ = pw(Xs, _lib.COV_CENTER)
    eye = np.stack([np.eye(p)] * 2)
    eng = HipEngine(eye, eye, eye, 0 * eye)
    four = HipEngine(np.stack([np.eye(p)] * 4), np.stack([np.eye(p)] * 4), np.stack([np.eye(p)] * 4), np.zeros((4, p, p)))
    try:
        eng.set_data(Xs, missing='pairwise')
        got = eng.get_S()
        assert isinstance(got, np.ndarray) and np.array_equal(got, S)
        eng.set_data(Xs, [65, 130], scale=True, missing='pairwise')
        C, var = eng.get_S()
        C2, var2, _ = pw(Xs, _lib.COV_CENTER | _lib.COV_SCALE)
        assert np.array_equal(C, C2) and np.array_equal(var, var2)
        eng.set_data(Xs, center=False, missing='pairwise')
        assert np.array_equal(eng.get_S(), pw(Xs, 0)[0])
        # subsets, B = 2 replicated over K = 4
        X = Xs[0]
        idx = np.stack([np.arange(0, 40), np.r_[0, 1, np.arange(27, 65)]])
        four.set_data_subsets(X, idx, missing='pairwise')
        sub = pw([X[:, idx[r]] for r in range(2)], _lib.COV_CENTER)[0]
        assert np.array_equal(four.get_S(), np.concatenate([sub, sub]))
        four.set_data_subsets(X, idx, scale=True, missing='pairwise')
        C, var = four.get_S()
        C2, var2, _ = pw([X[:, idx[r]] for r in range(2)], _lib.COV_CENTER | _lib.COV_SCALE)
        assert np.array_equal(C, np.concatenate([C2, C2])) and np.array_equal(var, np.concatenate([var2, var2]))
    finally:
        eng.close()
        four.close()


# ---------------------------------------------------------------------------------------------------------------------
# refusals
# ---------------------------------------------------------------------------------------------------------------------
def bad_inputs():
    """[(data of K = 2 instances, min_pairs, what the message must name)]"""
    p, N = 17, 33
    good = [np.array(case(p, N, "r30", k)[0]) for k in range(2)]
    empty = [good[0], good[1].copy()]
    empty[1][3, :] = np.nan                                           # instance 1, variable 3: no observation at all
    disjoint = [good[0].copy(), good[1]]
    disjoint[0][2, :16] = np.nan                                      # instance 0: variables 2 and 5 share nothing
    disjoint[0][5, 16:] = np.nan
    few = [good[0], np.array(case(p, N, "minpairs", 1)[0])]           # instance 1: variables 0 and 1 share two samples
    return [(empty, 2, r"instance 1, variable 3 has no observed entry"),
            (disjoint, 1, r"instance 0, the pair of variables \(2, 5\) shares 0 samples"),
            (few, 3, r"instance 1, the pair of variables \(0, 1\) shares 2 samples, min_pairs = 3"),
            (good, 0, r"min_pairs = 0")]


def test_refused_calls_name_the_offender_and_write_nothing():
    from gglasso_amd import _lib
    lib = _lib.load()
    p = 17
    for Xs, mp, message in bad_inputs():
        with pytest.raises(AssertionError, match=message):
            pw(Xs, _lib.COV_CENTER, mp)
        Xs = [np.ascontiguousarray(x) for x in Xs]
        S = np.full((2, p, p), -77.0)
        var = np.full((2, p), -77.0)
        cnt = np.full((2, p, p), -7, dtype=np.int32)
        rc = lib.ggl_covariance_pairwise(0, 2, p, (ctypes.c_int * 2)(33, 33), (_lib._dp * 2)(*[_lib.ptr(x) for x in Xs]),
                                         _lib.COV_CENTER | _lib.COV_SCALE, mp, _lib.ptr(S), _lib.ptr(var),
                                         cnt.ctypes.data_as(_lib._ip))
        assert rc == _lib.E_ARG
        assert np.all(S == -77.0) and np.all(var == -77.0) and np.all(cnt == -7), message
        # the subsets route: the two instances as two subsets of their concatenation
        X = np.ascontiguousarray(np.concatenate(Xs, axis=1))
        idx = np.ascontiguousarray(np.stack([np.arange(33), np.arange(33, 66)]), dtype=np.int32)
        rc = lib.ggl_covariance_pairwise_subsets(0, p, 66, _lib.ptr(X), 2, 33, idx.ctypes.data_as(_lib._ip), _lib.COV_CENTER, mp,
                                                 _lib.ptr(S), None, cnt.ctypes.data_as(_lib._ip))
        assert rc == _lib.E_ARG and __import__("re").search(message.replace("instance", "subset"), _lib.last_error())
        assert np.all(S == -77.0) and np.all(cnt == -7), message
    # the pair that shares exactly min_pairs samples is accepted
    few = bad_inputs()[2][0]
    S, _, cnt = pw(few, _lib.COV_CENTER, 2)
    assert cnt[1, 0, 1] == 2 and np.isfinite(S).all()
    check(S[1], cnt[1], case(17, 33, "minpairs", 1)[1], "shares exactly min_pairs")
    # a zero variance under GGL_COV_SCALE is refused like in ggl_covariance, and writes nothing either
    const = [np.array(x) for x in bad_inputs()[3][0]]
    const[1][4, ~np.isnan(const[1][4])] = 2.5
    with pytest.raises(AssertionError, match=r"instance 1, variable 4"):
        pw(const, _lib.COV_CENTER | _lib.COV_SCALE)


def test_refused_ctx_calls_leave_the_ctx_as_it_was():
    from gglasso_amd.solver import HipEngine
    p = 17
    good = [np.array(case(p, 33, "r30", k)[0]) for k in range(2)]
    eye = np.stack([np.eye(p)] * 2)
    eng = HipEngine(eye, eye, eye, 0 * eye)
    try:
        eng.set_data(good, scale=True, missing='pairwise')
        S0, var0 = eng.get_S()
        for Xs, mp, message in bad_inputs():
            with pytest.raises(AssertionError, match=message):
                eng.set_data(Xs, missing='pairwise', min_pairs=mp)
            S1, var1 = eng.get_S()                                    # still the pair: the variances are kept as well
            assert np.array_equal(S1, S0) and np.array_equal(var1, var0), message
            X = np.concatenate(Xs, axis=1)
            idx = np.stack([np.arange(33), np.arange(33, 66)])
            with pytest.raises(AssertionError, match=message.replace("instance", "subset")):
                eng.set_data_subsets(X, idx, missing='pairwise', min_pairs=mp)
            S1, var1 = eng.get_S()
            assert np.array_equal(S1, S0) and np.array_equal(var1, var0), message
    finally:
        eng.close()


def test_misuse_of_the_four_pairwise_entry_points():
    from gglasso_amd import _lib
    from gglasso_amd.solver import HipEngine
    lib = _lib.load()
    X = np.ascontiguousarray(case(15, 17, "r30")[0])
    p, N = X.shape
    Xp = (_lib._dp * 1)(_lib.ptr(X))
    Nn = (ctypes.c_int * 1)(N)
    S, sc, cnt = np.empty((1, p, p)), np.empty((1, p)), np.empty((1, p, p), dtype=np.int32)
    good = (0, 1, p, Nn, Xp, 1, 2, _lib.ptr(S), _lib.ptr(sc), cnt.ctypes.data_as(_lib._ip))

    def bad(fn, args, i, v):
        a = list(args)
        a[i] = v
        assert fn(*a) == _lib.E_ARG and _lib.last_error(), (i, v)
    assert lib.ggl_covariance_pairwise(*good) == 0
    for i, v in ((1, 0), (2, 0), (3, None), (4, None), (5, 16), (5, 4 | 8), (6, 0), (6, -1), (7, None),
                 (3, (ctypes.c_int * 1)(0)), (4, (_lib._dp * 1)(None))):
        bad(lib.ggl_covariance_pairwise, good, i, v)
    a = list(good)
    a[5], a[8] = 3, None                                              # GGL_COV_SCALE without scale_out
    assert lib.ggl_covariance_pairwise(*a) == _lib.E_ARG
    a = list(good)
    a[9] = None                                                       # the counts are optional
    assert lib.ggl_covariance_pairwise(*a) == 0
    idx = np.ascontiguousarray(np.arange(10)[None], dtype=np.int32)
    ip = idx.ctypes.data_as(_lib._ip)
    sgood = (0, p, N, _lib.ptr(X), 1, 10, ip, 1, 2, _lib.ptr(S), _lib.ptr(sc), cnt.ctypes.data_as(_lib._ip))
    assert lib.ggl_covariance_pairwise_subsets(*sgood) == 0
    out_of_range = np.ascontiguousarray(np.r_[np.arange(9), N][None], dtype=np.int32)
    for i, v in ((1, 0), (2, 0), (3, None), (4, 0), (5, 0), (6, None), (7, 16), (8, 0), (9, None),
                 (6, out_of_range.ctypes.data_as(_lib._ip))):
        bad(lib.ggl_covariance_pairwise_subsets, sgood, i, v)
    assert lib.ggl_set_S_from_data_pairwise(None, Xp, Nn, 1, 2) == _lib.E_ARG
    assert lib.ggl_set_S_from_subsets_pairwise(None, _lib.ptr(X), N, 1, 10, ip, 1, 2) == _lib.E_ARG
    eye = np.stack([np.eye(p)] * 3)
    eng = HipEngine(eye, eye, eye, 0 * eye)
    X3 = (_lib._dp * 3)(*[_lib.ptr(X)] * 3)
    N3 = (ctypes.c_int * 3)(N, N, N)
    try:
        h = eng.h
        assert lib.ggl_set_S_from_data_pairwise(h, X3, N3, 1, 2) == 0
        before = eng.get_S()
        assert lib.ggl_set_S_from_data_pairwise(h, None, N3, 1, 2) == _lib.E_ARG
        assert lib.ggl_set_S_from_data_pairwise(h, X3, None, 1, 2) == _lib.E_ARG
        assert lib.ggl_set_S_from_data_pairwise(h, X3, N3, 32, 2) == _lib.E_ARG
        assert lib.ggl_set_S_from_data_pairwise(h, X3, N3, 1, 0) == _lib.E_ARG
        assert lib.ggl_set_S_from_subsets_pairwise(h, None, N, 1, 10, ip, 1, 2) == _lib.E_ARG
        assert lib.ggl_set_S_from_subsets_pairwise(h, _lib.ptr(X), N, 1, 10, None, 1, 2) == _lib.E_ARG
        assert lib.ggl_set_S_from_subsets_pairwise(h, _lib.ptr(X), N, 1, 10, ip, 1, 0) == _lib.E_ARG
        two = np.ascontiguousarray(np.stack([np.arange(10)] * 2), dtype=np.int32)
        assert lib.ggl_set_S_from_subsets_pairwise(h, _lib.ptr(X), N, 2, 10, two.ctypes.data_as(_lib._ip), 1, 2) == _lib.E_ARG   # 2 does not divide 3
        eng.set_instance_dims(np.array([p - 1, p, p]))
        assert lib.ggl_set_S_from_data_pairwise(h, X3, N3, 1, 2) == _lib.E_ARG
        assert lib.ggl_set_S_from_subsets_pairwise(h, _lib.ptr(X), N, 1, 10, ip, 1, 2) == _lib.E_ARG
        eng.set_instance_dims(None)
        assert np.array_equal(eng.get_S(), before)
        assert lib.ggl_set_S_from_subsets_pairwise(h, _lib.ptr(X), N, 1, 10, ip, 1, 2) == 0
    finally:
        eng.close()


# ---------------------------------------------------------------------------------------------------------------------
# end to end: p = 20, N = 120, 20 % missing
# ---------------------------------------------------------------------------------------------------------------------
def holed_problem():
    p, N = 20, 120
    Th = np.eye(p)
    Th[np.arange(p - 1), np.arange(1, p)] = Th[np.arange(1, p), np.arange(p - 1)] = 0.4
    Th[0, 5] = Th[5, 0] = 0.3
    rng = np.random.default_rng(11)
    X = np.linalg.cholesky(np.linalg.inv(Th)) @ rng.standard_normal((p, N))
    hole = rng.random((p, N)) < 0.2
    hole[:, :2] = False
    X[hole] = np.nan
    return X


def quiet(fn, *a, **k):
    buf = io.StringIO()
    with contextlib.redirect_stdout(buf):
        out = fn(*a, **k)
    return out, buf.getvalue()


def test_problem_from_data_with_holes_solves():
    from gglasso_amd import utils
    from gglasso_amd.problem import glasso_problem
    X = holed_problem()
    P = glasso_problem.from_data(X, missing='pairwise', reg_params={'lambda1': 0.1})
    S, n = utils.sample_covariance(X, missing='pairwise', return_counts=True)
    assert P.N == 120 and np.array_equal(P.S, S) and np.array_equal(P.pair_counts, n) and n.min() >= 2
    # the KKT residual as the stopping test: 'optimal' is the solver's own verdict on the Theta it returns
    _, out = quiet(P.solve, tol=1e-6, rtol=1e-6, solver_params={'stopping_criterion': 'kkt'})
    Theta = P.solution.precision_
    assert np.isfinite(Theta).all() and np.array_equal(Theta, Theta.T)
    assert "with status: optimal" in out and "max iterations" not in out and "solver error" not in out, out
    # the same data without missing=: the NaNs spread over S and nothing usable comes back
    try:
        Q = glasso_problem.from_data(X, reg_params={'lambda1': 0.1})
        _, out = quiet(Q.solve, tol=1e-6, rtol=1e-6, solver_params={'stopping_criterion': 'kkt'})
        usable = np.isfinite(Q.solution.precision_).all() and "with status: optimal" in out
    except Exception:      # noqa: BLE001  (a refusal is as good as a NaN)
        usable = False
    assert not usable
    # three instances of one dimension become a stack, the counts with them
    P3 = glasso_problem.from_data([X, X[:, :100], X[:, 10:]], missing='pairwise', reg_params={'lambda1': 0.1, 'lambda2': 0.05})
    assert P3.S.shape == P3.pair_counts.shape == (3, 20, 20) and list(P3.N) == [120, 100, 110]


def test_stars_search_with_holes_equals_the_host_route():
    import warnings
    from gglasso_amd import model_selection as ms, solver
    from gglasso_amd.problem import glasso_problem
    from oracle_engine import OracleEngine
    X = holed_problem()
    lam = [0.5, 0.3, 0.15]
    kw = dict(missing='pairwise', n_subsamples=4, seed=2, beta=0.15, tol=1e-8, rtol=1e-8, store_all=True)
    with warnings.catch_warnings():
        warnings.simplefilter("ignore", RuntimeWarning)               # (no lambda below beta: not what is compared)
        sol, stats = ms.stars_search(X, lam, **kw)
        real = solver.ENGINE
        solver.ENGINE = OracleEngine                                  # no set_data_subsets: numpy matrices, host counts
        try:
            hsol, hstats = ms.stars_search(X, lam, **kw)
        finally:
            solver.ENGINE = real
        assert stats['FAILED'] == [] and hstats['FAILED'] == []
        assert stats['IX'] == hstats['IX'] and stats['NUM'] == hstats['NUM'] and stats['BEST'] == hstats['BEST']
        assert np.array_equal(stats['COUNTS'], hstats['COUNTS']) and np.array_equal(stats['INDICES'], hstats['INDICES'])
        assert np.isfinite(sol['Theta']).all() and np.abs(sol['Theta'] - hsol['Theta']).max() <= 1e-6
        # the front end hands the same arguments on
        P = glasso_problem.from_data(X, missing='pairwise')
        P.stability_selection({'lambda1_range': np.array(lam)}, n_subsamples=4, seed=2, beta=0.15, tol=1e-8, rtol=1e-8)
        assert P.modelselect_stats['NUM'] == stats['NUM'] and P.reg_params['lambda1'] == stats['BEST']['lambda1']
        assert np.array_equal(P.solution.precision_, sol['Theta'])


def test_zz_largest_ratio_of_this_run():
    """Prints the largest |S_dev - S_ref| / bound over every comparison this run made (DESIGN.md section 18 quotes it)."""
    if not WORST["checked"]:
        from gglasso_amd import _lib
        X, ref_c, _ = case(33, 65, "r30")
        S, _, cnt = pw([X], _lib.COV_CENTER)
        check(S[0], cnt[0], ref_c, (33, 65, "r30"))
    print("pairwise covariance: largest |S_dev - S_ref| / bound =", WORST["ratio"], "at", WORST["where"], "over", WORST["checked"],
          "comparisons")
    assert 0.0 < WORST["ratio"] <= 1.0
