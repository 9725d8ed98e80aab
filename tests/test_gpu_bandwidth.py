"""The batched Cholesky on the device (``ggl_cholesky_predict``: k_chol_predict of csrc/cholesky.hip) against the longdouble
reference at the bounds derived in tests/chol_ref.py, its bitwise guarantees, failure rule and refusals, and the bandwidth
search built on it (``ggl_weighted_predictive_scores``, ``utils.loo_bandwidth_scores``, ``model_selection.bandwidth_search``,
``glasso_problem.from_time_series_cv``).

Shapes: p = 1, 2 and 15 / 16 / 17 are one block column and its edges (with d the border row falls into the diagonal block's
16 rows, or opens a second row block); 31 / 32 / 33 and 63 / 64 / 65 the edges of two block columns and of the 64 rows of a
round (p = 64 with d: the border row is the first row of a second round); p = 129 has nine block columns and three rounds."""
import os
import re
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import chol_ref as cr  # noqa: E402

pytestmark = pytest.mark.gpu

PS = [1, 2, 15, 16, 17, 31, 32, 33, 63, 64, 65, 129]
KS = [1, 3, 9]
SENTINEL = -12345.678


def same(a, b):
    """two results of cholesky_predict, bit for bit (NaN equal to NaN)"""
    return all(np.array_equal(x, y, equal_nan=True) for x, y in zip(a, b))


@pytest.mark.parametrize("p", PS)
def test_device_against_the_longdouble_reference(p):
    from gglasso_amd import utils
    S, d = cr.spd_stack(9, p, 0)
    full = None
    for K in KS:
        res = utils.cholesky_predict(S[:K], d[:K])
        assert np.all(res[3] == -1), (K, res[3])
        fr = cr.fractions(res, S[:K], d[:K])
        print(f"device p={p} K={K} fractions of the bounds (log det, q, pivot)", fr)
        assert np.all(fr <= 1.0), (K, fr)
        nod = utils.cholesky_predict(S[:K])
        assert np.array_equal(nod[0], res[0]) and np.all(nod[1] == 0.0) and np.array_equal(nod[2], res[2])
        assert same(res, utils.cholesky_predict(S[:K], d[:K]))                        # two calls, the same bits
        full = res
    for k in (0, 4, 8):                                                                # instance k alone
        one = utils.cholesky_predict(S[k], d[k])
        assert all(one[i] == full[i][k] for i in range(4)), k
    rid = utils.cholesky_predict(S[:3], d[:3], ridge=0.25)
    assert same(rid, utils.cholesky_predict(S[:3] + 0.25 * np.eye(p), d[:3]))
    assert not np.array_equal(rid[0], full[0][:3])


@pytest.mark.parametrize("p", [17, 33, 65])
def test_not_positive_definite_is_a_status(p):
    from gglasso_amd import utils
    S, d = cr.spd_stack(3, p, 1)
    good = utils.cholesky_predict(S, d)
    lam, Q = np.linalg.eigh(S[1])
    lam[0] = -0.1
    bad = S.copy()
    bad[1] = (Q * lam) @ Q.T
    bad[1] = 0.5 * (bad[1] + bad[1].T)
    nan = S.copy()
    nan[1, p - 3, 5] = nan[1, 5, p - 3] = np.nan
    for M in (bad, nan):
        res = utils.cholesky_predict(M, d)
        twin = utils.host_cholesky_predict(M, d)
        assert res[3][1] >= 0 and res[3][1] == twin[3][1], (res[3], twin[3])
        assert res[0][1] == -np.inf and np.isnan(res[1][1])
        for k in (0, 2):
            assert all(res[i][k] == good[i][k] for i in range(4)), k
    assert utils.cholesky_predict(bad, d)[2][1] <= 0.0 and utils.cholesky_predict(nan, d)[3][1] == p - 3
    up = S.copy()
    up[1, 5, p - 3] = np.nan                                      # the upper triangle is not read
    assert same(utils.cholesky_predict(up, d), good)
    res = utils.cholesky_predict(bad, d, ridge=0.2)
    assert np.all(res[3] == -1) and np.isfinite(res[0]).all() and np.isfinite(res[1]).all()


def raw_chol(S, d, ridge, K=None, p=None, null=()):
    from gglasso_amd import _lib
    out = np.full((S.shape[0], 4), SENTINEL)
    rc = _lib.load().ggl_cholesky_predict(0, S.shape[0] if K is None else K, S.shape[1] if p is None else p,
                                          None if 'S' in null else _lib.ptr(S), None if d is None else _lib.ptr(d), ridge,
                                          None if 'out' in null else _lib.ptr(out))
    return rc, _lib.last_error(), out


def raw_scores(X, w, target, ridge=0.0, flags=1, chunk=0, M=None, p=None, null=()):
    from gglasso_amd import _lib
    X, w = np.ascontiguousarray(X, dtype=np.float64), np.ascontiguousarray(w, dtype=np.float64)
    target = np.ascontiguousarray(target, dtype=np.int32)
    out = np.full((w.shape[0], 4), SENTINEL)
    rc = _lib.load().ggl_weighted_predictive_scores(
        0, X.shape[0] if p is None else p, X.shape[1], None if 'X' in null else _lib.ptr(X), w.shape[0] if M is None else M,
        None if 'w' in null else _lib.ptr(w), None if 'target' in null else target.ctypes.data_as(_lib._ip), ridge, flags, chunk,
        None if 'out' in null else _lib.ptr(out))
    return rc, _lib.last_error(), out


def test_misuse_is_refused_and_writes_nothing():
    from gglasso_amd import _lib, utils
    S, d = cr.spd_stack(3, 17, 2)
    for kw, text in (({'K': 0}, "K >= 1"), ({'p': 0}, "p >= 1"), ({'null': ('S',)}, "NULL"), ({'null': ('out',)}, "NULL")):
        rc, msg, out = raw_chol(S, d, 0.0, **kw)
        assert rc == _lib.E_ARG and re.search(text, msg) and np.all(out == SENTINEL), (kw, rc, msg)
    for ridge in (-1e-9, np.nan, np.inf):
        rc, msg, out = raw_chol(S, d, ridge)
        assert rc == _lib.E_ARG and "ridge" in msg and np.all(out == SENTINEL), (ridge, rc, msg)
    rc, msg, out = raw_chol(S, d, 0.0)
    assert rc == 0 and not np.any(out == SENTINEL)
    with pytest.raises(AssertionError, match="ridge"):
        utils.cholesky_predict(S, d, ridge=-1.0)

    X, _ = cr.case_a(0)
    ev = np.arange(0, 240, 24)
    w = utils.loo_weights(np.arange(240.0), ev, 16.0)
    cases = [({'M': 0}, "M >= 1"), ({'p': 0}, "p >= 1"), ({'null': ('X',)}, "X, w"), ({'null': ('w',)}, "X, w"),
             ({'null': ('target',)}, "NULL"), ({'null': ('out',)}, "NULL"), ({'ridge': -1.0}, "ridge"), ({'ridge': np.nan}, "ridge"),
             ({'flags': 32}, "unknown bits"), ({'flags': 1 | 2}, "GGL_COV_SCALE"), ({'flags': 1 | 4 | 8}, "exclude each other"),
             ({'chunk': -1}, "chunk")]
    for kw, text in cases:
        rc, msg, out = raw_scores(X, w, ev, **kw)
        assert rc == _lib.E_ARG and re.search(text, msg) and np.all(out == SENTINEL), (kw, rc, msg)
    for bad, row in ((240, 3), (-1, 7)):
        t = ev.copy(); t[row] = bad
        rc, msg, out = raw_scores(X, w, t)
        assert rc == _lib.E_ARG and re.search(rf"row {row} scores the sample {bad}", msg) and np.all(out == SENTINEL), msg
    w2 = w.copy(); w2[4, 100] = -0.5
    rc, msg, out = raw_scores(X, w2, ev)
    assert rc == _lib.E_ARG and re.search(r"instance 4, sample 100 holds the weight -0\.5", msg) and np.all(out == SENTINEL), msg
    w2 = w.copy(); w2[6] = 0.0
    rc, msg, out = raw_scores(X, w2, ev)
    assert rc == _lib.E_ARG and re.search(r"weights of instance 6 sum to 0", msg) and np.all(out == SENTINEL), msg
    rc, msg, out = raw_scores(X, w, ev)
    assert rc == 0 and np.all(out[:, 3] == -1)


def test_scores_are_those_of_the_weighted_covariance():
    """Row r of the call is cholesky_predict on row r of ggl_covariance_weighted's S, with d = x_target - m_r: bit for bit in
    the log det (the same S, the same kernel) and, without centring (d = x_target exactly), in everything."""
    from gglasso_amd import utils
    X, times, ev = cr.case_b()
    w = utils.loo_weights(times, ev, 90.0, 'epanechnikov')
    for center in (True, False):
        rc, msg, out = raw_scores(X, w, ev, flags=1 if center else 0)
        assert rc == 0, msg
        S = utils.weighted_covariance(X, w, center=center)
        d = X[:, ev].T - ((w @ X.T) / w.sum(axis=1, keepdims=True) if center else 0.0)
        ref = utils.cholesky_predict(S, np.ascontiguousarray(d))
        assert np.array_equal(out[:, 0], ref[0]) and np.array_equal(out[:, 2], ref[2]) and np.all(out[:, 3] == -1)
        if not center:
            assert np.array_equal(out[:, 1], ref[1])
        rc, msg, o2 = raw_scores(X, w, ev, flags=16 | (1 if center else 0))          # GGL_COV_FULL_RANGE: the same bits
        assert rc == 0 and np.array_equal(o2, out), msg
        for flags in (4, 8):                                                         # a forced tile shape is served
            rc, msg, o2 = raw_scores(X, w, ev, flags=flags | (1 if center else 0))
            assert rc == 0 and np.allclose(o2, out, rtol=1e-10, atol=0), (flags, msg)


@pytest.fixture(scope="module")
def search_a():
    """seed -> ((h, stats) on the swinging series, (h, stats) on the stationary one) of the device search, computed once"""
    from gglasso_amd import model_selection
    out = {}
    for seed in range(4):
        X, Xs = cr.case_a(seed)
        out[seed] = (X, Xs, model_selection.bandwidth_search(X, cr.CASE_A_BANDWIDTHS),
                     model_selection.bandwidth_search(Xs, cr.CASE_A_BANDWIDTHS))
    return out


def test_case_a_choices(search_a):
    from gglasso_amd import model_selection, utils
    for seed in range(4):
        X, Xs, (h, st), (hs, sts) = search_a[seed]
        assert st['NOT_PD'] == [] and sts['NOT_PD'] == []
        for data, stats in ((X, st), (Xs, sts)):
            SC, _ = utils.host_loo_bandwidth_scores(data, stats['BANDWIDTH'])
            CV, SE = SC.mean(axis=1), SC.std(axis=1, ddof=1) / np.sqrt(240)
            assert stats['IX'] == model_selection.cv_select(CV, SE, 'min'), seed
            assert np.abs(stats['SCORE'] - SC).max() <= 1e-9 * np.abs(SC).max()
        assert h == 32.0 and hs == 200.0, (seed, st['CV'], sts['CV'])
        assert [round(float(v), 1) for v in st['N_EFF']] == [229.9, 113.0, 56.3, 27.9, 13.8, 6.7]
        h1, st1 = model_selection.bandwidth_search(X, cr.CASE_A_BANDWIDTHS, rule='one_se')
        assert h1 >= h and st1['IX'] <= st['IX'] and np.array_equal(st1['SCORE'], st['SCORE'])


def test_case_a_scores_against_the_longdouble_formula(search_a):
    from gglasso_amd import utils
    X, _, (_, st), _ = search_a[0]
    ev = np.arange(240)
    worst = 0.0
    for b, h in enumerate(st['BANDWIDTH']):
        worst = max(worst, cr.score_fraction(st['SCORE'][b], X, utils.loo_weights(np.arange(240.0), ev, h), ev))
    print("device, case A: largest fraction of the score bound", worst)
    assert worst <= 1.0


def test_chunks_and_eval_index_do_not_change_a_bit(search_a):
    from gglasso_amd import utils
    X, _, (_, st), _ = search_a[1]
    hs = st['BANDWIDTH']
    for chunk in (1, 7, 0):
        SC, STAT = utils.loo_bandwidth_scores(X, hs, chunk=chunk)
        assert np.array_equal(SC, st['SCORE']) and np.all(STAT == -1), chunk
    SC, STAT = utils.loo_bandwidth_scores(X, hs, eval_index=40)
    ev = utils._loo_setup(X, hs, None, 40)[3]
    assert SC.shape == (6, 40) and ev.size == 40 and np.array_equal(SC, st['SCORE'][:, ev])


def test_case_b_epanechnikov_unsorted_times_no_centring():
    from gglasso_amd import utils
    X, times, ev = cr.case_b()
    hs = [120.0, 100.0]
    SC, STAT = utils.loo_bandwidth_scores(X, hs, times=times, kernel='epanechnikov', center=False, eval_index=ev)
    assert SC.shape == (2, 25) and np.all(STAT == -1)
    worst = 0.0
    for b, h in enumerate(hs):
        W = utils.loo_weights(times, ev, h, 'epanechnikov')
        assert utils.effective_sample_size(W).min() > 33
        worst = max(worst, cr.score_fraction(SC[b], X, W, ev, center=False))
    print("device, case B: largest fraction of the score bound", worst)
    assert worst <= 1.0
    tw, _ = utils.host_loo_bandwidth_scores(X, hs, times=times, kernel='epanechnikov', center=False, eval_index=ev)
    assert np.abs(SC - tw).max() <= 1e-9 * np.abs(tw).max()


def test_case_b_fewer_effective_samples_than_variables():
    """Gaussian kernel at h = 3 on times of mean spacing 2: N_eff < 7 and at most 26 samples carry a weight (the cutoff ends
    the Gaussian at 8.6 h), fewer than p = 33, so every covariance is singular up to rounding.  The call returns; a row is flagged or its smallest pivot is rounding noise; a ridge makes every row regular."""
    from gglasso_amd import utils
    X, times, ev = cr.case_b()
    W = utils.loo_weights(times, ev, 3.0)
    assert utils.effective_sample_size(W).max() < 33 and (W > 0).sum(axis=1).max() < 33
    rc, msg, out = raw_scores(X, W, ev)
    assert rc == 0, msg
    S = utils.host_weighted_covariance(X, W)
    for r in range(25):
        assert out[r, 3] >= 0 or out[r, 2] < 1e-10 * np.diagonal(S[r]).max(), (r, out[r])
        assert out[r, 3] < 33
    SC, STAT = utils.loo_bandwidth_scores(X, [3.0], times=times, eval_index=ev)
    assert np.array_equal(STAT[0], out[:, 3].astype(np.int64)) and np.all(np.isinf(SC[0][STAT[0] >= 0]))
    SC, STAT = utils.loo_bandwidth_scores(X, [3.0], times=times, eval_index=ev, ridge=1e-3)
    assert np.all(STAT == -1) and np.isfinite(SC).all()


def test_a_bandwidth_without_neighbours_is_refused_before_the_device(monkeypatch):
    from gglasso_amd import _lib, model_selection, utils
    X, _ = cr.case_a(0)

    def no_device(*a, **k):
        raise AssertionError("a refused search must not reach the device")
    monkeypatch.setattr(_lib, "require_gpu", no_device)
    monkeypatch.setattr(_lib, "load", no_device)
    with pytest.raises(ValueError, match=r"bandwidth 0\.4: the evaluation sample 0 has no neighbour"):
        utils.loo_bandwidth_scores(X, [16.0, 0.4], kernel='epanechnikov')
    with pytest.raises(ValueError, match=r"bandwidth 0\.4: the evaluation sample 12 has no neighbour"):
        model_selection.bandwidth_search(X, [16.0, 0.4], kernel='epanechnikov', eval_index=np.array([12, 50]))


def test_from_time_series_cv(search_a):
    from gglasso_amd import model_selection, problem
    X = search_a[2][0]
    ev = np.arange(0, 240, 3)
    P = problem.glasso_problem.from_time_series_cv(X, 6, [64, 32, 16], eval_index=ev)
    h, st = model_selection.bandwidth_search(X, [64, 32, 16], eval_index=ev)
    assert P.bandwidth_ == h and P.bandwidth_stats['IX'] == st['IX'] and np.array_equal(P.bandwidth_stats['SCORE'], st['SCORE'])
    Q = problem.glasso_problem.from_time_series(X, 6, P.bandwidth_)
    assert np.array_equal(P.S, Q.S) and np.array_equal(P.N, Q.N) and P.S.shape == (6, 6, 6)
