"""Neighbourhood selection with penalty weights and the scaled lasso on the device (``k_mb_path`` of csrc/neighborhood.hip behind
``ggl_neighborhood_path_w``, ``ggl_neighborhood_stability_w`` and ``ggl_neighborhood_cv_w``): the checks of tests/mbw_ref.py
against the longdouble comparison value at every size at which the kernel takes another path or a lane falls off an edge, the
arithmetic its instantiations share, the plain entries as forwards into the _w entries' host path, the bits, the edges of the method, the refusals of the C ABI, and the searches and the
front end end to end."""
import warnings

import numpy as np
import pytest

import mb_ref
import mbw_ref
from mbw_ref import SIG_TOL, TOL

pytestmark = pytest.mark.gpu

SIZES = (1, 2, 3, 5, 17, 63, 64, 65, 130, 257)
MODES = pytest.mark.parametrize("scaled", (False, True), ids=("plain", "scaled"))


@pytest.fixture(scope="module")
def device():
    from gglasso_amd import utils
    cache = {}

    def run(p, scaled):
        if (p, scaled) not in cache:
            cache[p, scaled] = utils.neighborhood_selection(mb_ref.stack(p), mb_ref.GRID, 'and', tol=TOL, return_info=True,
                                                            weights=mbw_ref.weight_stack(p), scaled=scaled, sig_tol=SIG_TOL)
        return cache[p, scaled]
    return run


@MODES
@pytest.mark.parametrize("p", SIZES)
def test_device_against_the_comparison_value(device, p, scaled):
    """Checks 1-4 for the stack of three seeds, one weight table per matrix (scaled mode beyond p = 65: checks 1 and 3)."""
    from gglasso_amd import utils
    W, info = device(p, scaled)
    assert W.shape == (3, 4, p, p) and np.array_equal(info['LAMBDA'], mb_ref.GRID)
    assert np.all(info['OUTER'] >= 1) if scaled else not info['OUTER'].any()
    assert ('SIGMA' in info) == scaled
    Wor = utils.neighborhood_selection(mb_ref.stack(p), mb_ref.GRID, 'or', tol=TOL, weights=mbw_ref.weight_stack(p),
                                       scaled=scaled, sig_tol=SIG_TOL)
    for seed in range(3):
        ok = mbw_ref.check_case(p, seed, scaled, info['COEF'][seed], info['RESVAR'][seed], info['STATUS'][seed], "device")
        for rule, Wr in (('and', W[seed]), ('or', Wor[seed])):
            assert np.array_equal(Wr, utils.neighborhood_graph(info['COEF'][seed], rule))
            if ok is not None:
                mbw_ref.check_graphs(p, seed, scaled, Wr, rule, ok)
    if p <= 65:
        assert np.array_equal(W[1], mbw_ref.and_or(info['COEF'][1], 'and'))     # the definition, entry by entry


@MODES
@pytest.mark.parametrize("p", (513, 1025))
def test_device_wide_variants(p, scaled):
    """The instantiations with 16 and 32 values per lane, 80 KiB of LDS per workgroup: every node finishes and check 1 -- the
    optimality certificate, which needs no comparison value -- holds on a two-lambda grid."""
    from gglasso_amd import utils
    S, Wt, lam = mb_ref.case(p, 0), mbw_ref.weights(p, 0), (0.2, 0.1)
    W, info = utils.neighborhood_selection(S, lam, 'and', tol=TOL, return_info=True, weights=Wt, scaled=scaled, sig_tol=SIG_TOL)
    assert not info['STATUS'].any() and W[1].any()
    mbw_ref.check_residual(S, lam, Wt, scaled, info['COEF'], info['RESVAR'], what="wide")
    assert np.array_equal(W, utils.neighborhood_graph(info['COEF'], 'and'))


def _path_w_call(S, lam, rule=1, tol=TOL, max_sweeps=100, weights=None, per_matrix=0, mode=0, sig_tol=SIG_TOL, max_outer=100,
                 M=None, p=None, L=None, coef=True, info=True, s_null=False, lam_null=False):
    """One raw ``ggl_neighborhood_path_w`` call with sentinel-filled outputs: (rc, message, coef, resvar, info)."""
    from gglasso_amd import _lib
    lib = _lib.load()
    S = np.ascontiguousarray(S, dtype=np.float64)
    lam = np.ascontiguousarray(lam, dtype=np.float64)
    Wt = None if weights is None else np.ascontiguousarray(weights, dtype=np.float64)
    M = S.shape[0] if M is None else M
    p = S.shape[-1] if p is None else p
    L = lam.size if L is None else L
    n = max(1, S.shape[0]) * max(1, lam.size) * S.shape[-1]
    C, R = np.full(n * S.shape[-1], -7.5), np.full(n, -7.5)
    I = np.full(n * 3, -7, dtype=np.int32)
    rc = lib.ggl_neighborhood_path_w(0, M, p, None if s_null else _lib.ptr(S), L, None if lam_null else _lib.ptr(lam), rule,
                                     tol, max_sweeps, _lib.ptr(Wt), per_matrix, mode, sig_tol, max_outer,
                                     _lib.ptr(C) if coef else None, _lib.ptr(R), I.ctypes.data_as(_lib._ip) if info else None)
    return rc, _lib.last_error(), C, R, I


@pytest.mark.parametrize("p", (17, 65, 257, 513, 1025))
def test_same_arithmetic_as_the_existing_kernel(p):
    """``ggl_neighborhood_path_w`` without weights (the unweighted instantiation of ``k_mb_path``), and with a table of ones
    (the weighted one), in plain mode: bit for bit the COEF, RESVAR, SWEEPS, STATUS and the AND and OR stacks of
    ``ggl_neighborhood_path``, OUTER all zero.  p = 513 and 1025 are the smallest sizes of the instantiations with 16 and 32
    values per lane (at 32, 2 waves per workgroup): one matrix there, and the two-lambda grid of ``test_device_wide_variants``."""
    from gglasso_amd import utils
    S, lam = (mb_ref.stack(p), np.array(mb_ref.GRID)) if p <= 257 else (mb_ref.case(p, 0)[None], np.array((0.2, 0.1)))
    M, L = S.shape[0], lam.size
    want = {r: utils.neighborhood_selection(S, lam, r, tol=TOL, return_info=True) for r in ('and', 'or')}
    info0 = want['and'][1]
    for rule, code in (('raw', 0), ('and', 1), ('or', 2)):
        for Wt in (None, np.ones((p, p))):
            rc, msg, C, R, I = _path_w_call(S, lam, rule=code, max_sweeps=10000, weights=Wt)
            assert rc == 0, msg
            C, R, I = C.reshape(M, L, p, p), R.reshape(M, L, p), I.reshape(M, L, p, 3)
            assert np.array_equal(C, info0['COEF'] if rule == 'raw' else want[rule][0])
            assert np.array_equal(R, info0['RESVAR']) and np.array_equal(I[..., 0], info0['SWEEPS'])
            assert np.array_equal(I[..., 1], info0['STATUS']) and not I[..., 2].any()
    Wa, ia = utils.neighborhood_selection(S, lam, 'and', tol=TOL, return_info=True, weights=np.ones((p, p)))
    assert np.array_equal(Wa, want['and'][0]) and all(np.array_equal(ia[k], info0[k]) for k in info0)


@MODES
@pytest.mark.parametrize("p", (17, 65, 257))
def test_device_bits(device, p, scaled):
    """Two calls, one matrix of a stack alone, the leading part of a grid, a shared table against its copies."""
    from gglasso_amd import utils
    S, Wt = mb_ref.stack(p), mbw_ref.weight_stack(p)
    kw = dict(rule='and', tol=TOL, return_info=True, scaled=scaled, sig_tol=SIG_TOL)
    W, info = device(p, scaled)
    W2, info2 = utils.neighborhood_selection(S, mb_ref.GRID, weights=Wt, **kw)
    assert np.array_equal(W, W2) and all(np.array_equal(info[k], info2[k]) for k in info)
    W1, info1 = utils.neighborhood_selection(S[1], mb_ref.GRID, weights=Wt[1], **kw)
    assert np.array_equal(W1, W[1]) and all(np.array_equal(info1[k], info[k][1]) for k in info if k != 'LAMBDA')
    Wh, infoh = utils.neighborhood_selection(S, mb_ref.GRID[:2], weights=Wt, **kw)
    assert np.array_equal(Wh, W[:, :2]) and all(np.array_equal(infoh[k], info[k][:, :2]) for k in info if k != 'LAMBDA')
    Ws, infos = utils.neighborhood_selection(S, mb_ref.GRID, weights=Wt[0], **kw)
    Wr, infor = utils.neighborhood_selection(S, mb_ref.GRID, weights=np.stack([Wt[0]] * 3), **kw)
    assert np.array_equal(Ws, Wr) and all(np.array_equal(infos[k], infor[k]) for k in infos)
    assert np.array_equal(Ws[0], W[0]) and not np.array_equal(Ws[1], W[1])


def test_device_edges_of_the_method():
    from gglasso_amd import utils
    p = 17
    S, Wt = mb_ref.stack(p)[0], mbw_ref.weights(p, 0)
    off = ~np.eye(p, dtype=bool)
    top = float((np.abs(S) / (Wt * np.sqrt(np.diag(S))[:, None]))[off].max())
    for scaled in (False, True):
        kw = dict(tol=TOL, return_info=True, scaled=scaled, sig_tol=SIG_TOL)
        W, info = utils.neighborhood_selection(S, (top * 1.01, 0.1), 'or', weights=Wt, **kw)
        assert not W[0].any() and not info['COEF'][0].any() and not info['SWEEPS'][0].any() and not info['STATUS'].any()
        assert np.array_equal(info['RESVAR'][0], np.diag(S)) and np.all(info['OUTER'][0] == (1 if scaled else 0)) and W[1].any()
        W, info = utils.neighborhood_selection(np.array([[2.0]]), mb_ref.GRID, 'and', weights=np.ones((1, 1)), **kw)
        assert W.shape == (4, 1, 1) and not W.any() and not info['STATUS'].any() and np.all(info['RESVAR'] == 2.0)
        Wz = Wt.copy()
        Wz[:, 4], Wz[:, 9] = 0.0, np.inf
        W, info = utils.neighborhood_selection(S, mb_ref.GRID, 'and', weights=Wz, **kw)
        C = info['COEF']
        assert not info['STATUS'].any() and np.all(C[:, 9, :] == 0) and np.all(C[:, 4, :][:, np.arange(p) != 4] != 0)
        mbw_ref.check_residual(S, mb_ref.GRID, Wz, scaled, C, info['RESVAR'], what="free and excluded columns")
    W, info = utils.neighborhood_selection(S, mb_ref.GRID[-1:], 'and', tol=TOL, return_info=True, weights=Wt, scaled=True,
                                           max_outer=1)
    assert np.all(info['STATUS'] == 1) and np.all(info['OUTER'] == 1) and np.all(np.isfinite(info['COEF']))
    assert np.all(np.isfinite(info['RESVAR'])) and np.all(np.isfinite(W))


def test_device_duplicated_variable():
    """The degenerate square-root problem: the floor on tau^2 and the cap end the two nodes' loops, the call returns, and
    nobody else is touched."""
    from gglasso_amd import utils
    S = mbw_ref.duplicate_case()
    p = S.shape[0]
    W, info = utils.neighborhood_selection(S, mb_ref.GRID, 'raw', tol=TOL, return_info=True, scaled=True, sig_tol=SIG_TOL)
    dup = np.zeros(p, dtype=bool)
    dup[[3, 5]] = True
    assert np.all(info['STATUS'][:, dup] == 3) and np.all(info['OUTER'][0, dup] <= 20) and not info['STATUS'][:, ~dup].any()
    for j in (3, 5):
        col = info['COEF'][:, :, j]
        assert np.all(col[:, j] == 0) and np.all(np.isnan(np.delete(col, j, axis=1))) and np.all(np.isnan(info['RESVAR'][:, j]))
    keep = np.broadcast_to(~dup[None, :], info['STATUS'].shape)
    C = np.where(np.isnan(info['COEF']), 0.0, info['COEF'])
    R = np.where(np.isnan(info['RESVAR']), 1.0, info['RESVAR'])
    mbw_ref.check_residual(S, mb_ref.GRID, np.ones((p, p)), True, C, R, nodes=keep, what="beside a duplicated variable")


@MODES
def test_nan_in_one_matrix_of_a_stack(scaled):
    """The C ABI refuses a non-finite S_host, so the NaN reaches the kernel on a ctx: status 2 for the nodes that read it, the
    other matrices' stack bit for bit that of the clean call."""
    from gglasso_amd import solver
    p, B = 5, 3
    S, Wt = mb_ref.stack(p).copy(), mbw_ref.weights(p, 0)
    eye = np.broadcast_to(np.eye(p), (B, p, p))
    out = []
    for nan in (False, True):
        if nan:
            S[1, 2, 3] = S[1, 3, 2] = np.nan
        eng = solver.HipEngine(S, eye, eye, np.zeros((B, p, p)))
        try:
            out.append(eng.neighborhood_stability(mb_ref.GRID, 'and', tol=TOL, stack=True, weights=Wt, scaled=scaled))
        finally:
            eng.close()
    clean, dirty = out
    assert not clean['status'].any() and set(np.unique(dirty['status'][:, 1])) <= {0, 2}
    assert np.all(dirty['status'][:, 1][:, [2, 3]] == 2) and not dirty['status'][:, [0, 2]].any()
    assert np.array_equal(dirty['stack'][:, [0, 2]], clean['stack'][:, [0, 2]])


def test_refusals_write_nothing():
    """GGL_E_ARG before any device work on ``ggl_neighborhood_path_w``: the outputs keep their sentinel, the message names the
    offender."""
    from gglasso_amd import _lib
    S = mb_ref.stack(5).copy()
    lam = np.array(mb_ref.GRID)
    bad_S, neg_d = S.copy(), S.copy()
    bad_S[1, 2, 3] = np.nan
    neg_d[2, 4, 4] = 0.0
    Wt = mbw_ref.weight_stack(5).copy()
    w_neg, w_nan, w_inf = Wt.copy(), Wt.copy(), Wt.copy()
    w_neg[2, 1, 3], w_nan[1, 4, 0], w_inf[0, 1, 2] = -0.25, np.nan, np.inf
    cases = {
        "M": dict(M=0), "L": dict(L=0), "p": dict(p=0), "p max": dict(p=2049), "S NULL": dict(s_null=True),
        "lam NULL": dict(lam_null=True), "coef NULL": dict(coef=False), "info NULL": dict(info=False),
        "lambda 0": dict(lam=[0.4, 0.0]), "lambda nan": dict(lam=[0.4, np.nan]), "ascending": dict(lam=[0.1, 0.4]),
        "tol < 0": dict(tol=-1e-9), "tol nan": dict(tol=np.nan), "sweeps": dict(max_sweeps=0),
        "rule": dict(rule=3), "S nan": dict(S=bad_S), "diagonal": dict(S=neg_d),
        "weight < 0": dict(weights=w_neg, per_matrix=1), "weight nan": dict(weights=w_nan, per_matrix=1),
        "shared weight < 0": dict(weights=w_neg[2]), "mode": dict(mode=2), "mode < 0": dict(mode=-1),
        "sig_tol < 0": dict(sig_tol=-1e-9), "sig_tol nan": dict(sig_tol=np.nan), "sig_tol inf": dict(sig_tol=np.inf),
        "max_outer": dict(max_outer=0),
    }
    for mode in (0, 1):
        for name, kw in cases.items():
            args = dict(S=S, lam=lam, mode=mode)
            args.update(kw)
            rc, msg, C, R, I = _path_w_call(**args)
            assert rc == _lib.E_ARG, (name, rc, msg)
            assert np.all(C == -7.5) and np.all(R == -7.5) and np.all(I == -7), name
            expect = {"S nan": ("matrix 1", "(2, 3)"), "diagonal": ("matrix 2", "variable 4"), "weight < 0": ("matrix 2", "(1, 3)"),
                      "weight nan": ("matrix 1", "(4, 0)"), "shared weight < 0": ("matrix 0", "(1, 3)"), "mode": ("mode = 2",),
                      "sig_tol < 0": ("sig_tol",), "max_outer": ("max_outer = 0",)}.get(name, ())
            assert all(e in msg for e in expect), (name, msg)
        rc, msg, C, R, I = _path_w_call(S, lam, mode=mode, weights=w_inf, per_matrix=1)
        assert rc == 0 and not np.any(C == -7.5) and not np.any(I == -7), msg


def _ctx_refusal_cases():
    Wt = mbw_ref.weight_stack(5).copy()
    w_neg, w_nan = Wt.copy(), Wt.copy()
    w_neg[2, 1, 3], w_nan[1, 4, 0] = -0.25, np.nan
    lam = np.array(mb_ref.GRID)
    return {
        "weight < 0": (dict(weights=w_neg, per_matrix=1), ("matrix 2", "(1, 3)")),
        "weight nan": (dict(weights=w_nan, per_matrix=1), ("matrix 1", "(4, 0)")),
        "shared weight < 0": (dict(weights=w_neg[2]), ("matrix 0", "(1, 3)")),
        "mode": (dict(mode=2), ("mode = 2",)), "sig_tol < 0": (dict(sig_tol=-1e-9), ("sig_tol",)),
        "sig_tol nan": (dict(sig_tol=np.nan), ("sig_tol",)), "max_outer": (dict(max_outer=0), ("max_outer = 0",)),
        "rule raw": (dict(rule=0), ("rule = 0",)), "t < 0": (dict(t=-1.0), ("t = -1",)), "tol": (dict(tol=-1.0), ("tol",)),
        "sweeps": (dict(max_sweeps=0), ("max_sweeps",)), "ascending": (dict(lam=lam[::-1].copy()), ("descending",)),
        "lambda nan": (dict(lam=np.array([0.4, np.nan])), ("lam[1]",)), "L": (dict(L=0), ()),
    }


def test_ctx_refusals_write_nothing():
    """The refusals of ``ggl_neighborhood_stability_w`` and ``ggl_neighborhood_cv_w``: GGL_E_ARG, sentinel-filled outputs
    unchanged, the offender named; then one accepted call of each, which fills them."""
    import ctypes
    from gglasso_amd import _lib, solver
    from gglasso_amd import model_selection as ms
    p, F, L = 5, 3, 4
    X = mb_ref.stars_data(p=p, N=60)
    train, test = ms.cv_folds(60, F, 4)
    test = np.ascontiguousarray(test, dtype=np.int32)
    eye = np.broadcast_to(np.eye(p), (F, p, p))
    eng = solver.HipEngine(eye, eye, eye, np.zeros((F, p, p)))
    lib = _lib.load()

    def call(entry, lam=np.array(mb_ref.GRID), rule=1, tol=TOL, max_sweeps=100, t=1e-8, weights=None, per_matrix=0, mode=0,
             sig_tol=SIG_TOL, max_outer=100, L=None):
        lam = np.ascontiguousarray(lam, dtype=np.float64)
        Wt = None if weights is None else np.ascontiguousarray(weights, dtype=np.float64)
        nL = lam.size if L is None else L
        n = 4 * F * p
        num, cnt = np.full(4, -7, dtype=np.int64), np.full(4 * p * p, -7, dtype=np.int32)
        stack, info = np.full(n * p, -7.5), np.full(n * 3, -7, dtype=np.int32)
        res, held = np.full(n, -7.5), np.full(n, -7.5)
        ip = lambda a: a.ctypes.data_as(_lib._ip)
        if entry == 'stability':
            rc = lib.ggl_neighborhood_stability_w(eng.h, nL, _lib.ptr(lam), rule, tol, max_sweeps, t, _lib.ptr(Wt), per_matrix, mode,
                                                  sig_tol, max_outer, num.ctypes.data_as(ctypes.POINTER(ctypes.c_longlong)),
                                                  ip(cnt), _lib.ptr(stack), ip(info))
            outs = (num, cnt, stack, info)
        else:
            rc = lib.ggl_neighborhood_cv_w(eng.h, _lib.ptr(X), X.shape[1], F, test.shape[1], ip(test), _lib.COV_CENTER, nL,
                                           _lib.ptr(lam), rule, tol, max_sweeps, t, 0, _lib.ptr(Wt), per_matrix, mode, sig_tol,
                                           max_outer, _lib.ptr(res), _lib.ptr(held), ip(info), _lib.ptr(stack))
            outs = (res, held, stack, info)
        return rc, _lib.last_error(), outs

    try:
        eng.set_data_subsets(X, train)
        for entry in ('stability', 'cv'):
            for mode in (0, 1):
                for name, (kw, expect) in _ctx_refusal_cases().items():
                    args = dict(mode=mode)
                    args.update(kw)
                    rc, msg, outs = call(entry, **args)
                    assert rc == _lib.E_ARG, (entry, name, rc, msg)
                    assert all(np.all((a == -7) | (a == -7.5)) for a in outs), (entry, name)
                    assert all(e in msg for e in expect), (entry, name, msg)
                Wi = mbw_ref.weights(p, 0)
                Wi[0, 1] = np.inf
                rc, msg, outs = call(entry, mode=mode, weights=Wi)
                assert rc == 0 and not any(np.any((a == -7) | (a == -7.5)) for a in outs), (entry, msg)
    finally:
        eng.close()


def test_ctx_entries_have_the_stateless_bits():
    """``ggl_neighborhood_stability_w`` on a ctx of three matrices: the stack of the stateless call, the counts of the host
    definition, a shared table and one per matrix; what the engine refuses raises."""
    from gglasso_amd import model_selection as ms, solver, utils
    p, B = 17, 3
    S, Wt = mb_ref.stack(p), mbw_ref.weight_stack(p)
    eye = np.broadcast_to(np.eye(p), (B, p, p))
    lam = np.array(mb_ref.GRID)
    eng = solver.HipEngine(S, eye, eye, np.zeros((B, p, p)))
    try:
        for scaled in (False, True):
            for W_arg in (Wt, Wt[0], None):
                if W_arg is None and not scaled:
                    continue
                out = eng.neighborhood_stability(lam, 'or', tol=TOL, counts=True, stack=True, weights=W_arg, scaled=scaled)
                W, info = utils.neighborhood_selection(S, lam, 'or', tol=TOL, return_info=True, weights=W_arg, scaled=scaled)
                assert np.array_equal(out['stack'], np.swapaxes(W, 0, 1)) and not out['status'].any()
                assert np.array_equal(out['sweeps'], np.swapaxes(info['SWEEPS'], 0, 1))
                assert np.array_equal(out['outer'], np.swapaxes(info['OUTER'], 0, 1))
                cnt, num = ms._host_edge_counts(out['stack'], 1e-8)
                assert np.array_equal(out['counts'], cnt) and np.array_equal(out['num'], num)
        for kw in (dict(weights=-Wt), dict(scaled=True, sig_tol=-1.0), dict(scaled=True, max_outer=0), dict(weights=np.ones((2, p, p)))):
            with pytest.raises((AssertionError, ValueError)):
                eng.neighborhood_stability(lam, 'and', **kw)
    finally:
        eng.close()


def test_plain_ctx_entries_are_forwards():
    """``HipEngine.neighborhood_stability`` and ``neighborhood_cv`` (with and without ``refit``) on a ctx of three matrices,
    p = 65: without weights (``ggl_neighborhood_stability`` / ``_cv``) and with a table of ones in plain mode (their _w
    siblings) every array both return is the same bit for bit, and the _w dicts' ``outer`` is all zero."""
    from gglasso_amd import model_selection as ms, solver
    p, B = 65, 3
    X, lam, ones = mb_ref.stars_data(p=p, N=240), np.array(mb_ref.GRID), np.ones((p, p))
    train, test = ms.cv_folds(X.shape[1], B, 4)
    eye = np.broadcast_to(np.eye(p), (B, p, p))
    eng = solver.HipEngine(eye, eye, eye, np.zeros((B, p, p)))

    def same(a, b, more):
        assert set(b) == set(a) | more and all(np.array_equal(a[k], b[k]) for k in a)
        assert not b['status'].any() and a['stack'][-1].any() and all(not b[k].any() for k in more)

    try:
        eng.set_data_subsets(X, train)
        kw = dict(rule='and', tol=TOL, counts=True, stack=True)
        a, b = eng.neighborhood_stability(lam, **kw), eng.neighborhood_stability(lam, weights=ones, **kw)
        assert {'num', 'counts', 'stack', 'sweeps', 'status'} <= set(a)
        same(a, b, {'outer'})
        for refit in (False, True):
            kw = dict(rule='and', tol=TOL, refit=refit, stack=True)
            a, b = eng.neighborhood_cv(X, test, lam, **kw), eng.neighborhood_cv(X, test, lam, weights=ones, **kw)
            assert {'resvar', 'heldout', 'stack', 'status', 'degree' if refit else 'sweeps'} <= set(a)
            same(a, b, set() if refit else {'outer'})
    finally:
        eng.close()


def _stars_inputs():
    from gglasso_amd import model_selection as ms
    X = mb_ref.stars_data()
    return X, ms.stars_subsamples(X.shape[1], 6, None, seed=5)


@MODES
def test_stars_on_the_device(scaled):
    """``stars_search(method='mb', weights=, scaled=)``: THETA[l, r] is the stateless call on subsample r's matrix, COUNTS and
    NUM the host definition's, the final fit the stateless call on all observations."""
    from gglasso_amd import model_selection as ms, utils
    X, idx = _stars_inputs()
    Wt = mbw_ref.weights(17, 0)
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        sol, stats = ms.stars_search(X, mb_ref.GRID, n_subsamples=6, seed=5, beta=0.1, tol=TOL, store_all=True, method='mb',
                                     weights=Wt, scaled=scaled)
    assert stats['FAILED'] == [] and np.array_equal(stats['INDICES'], idx)
    S_sub = utils.sample_covariance_subsets(X, idx)
    W = utils.neighborhood_selection(S_sub, mb_ref.GRID, 'and', tol=TOL, weights=Wt, scaled=scaled)
    assert np.array_equal(stats['THETA'], np.swapaxes(W, 0, 1))
    cnt, num = ms._host_edge_counts(stats['THETA'], 1e-8)
    assert np.array_equal(stats['COUNTS'], cnt) and stats['NUM'] == [int(v) for v in num]
    ix = stats['IX']
    S_full = utils.sample_covariance(X, center=True)
    Wf, info = utils.neighborhood_selection(S_full, mb_ref.GRID[:ix + 1], 'and', tol=TOL, return_info=True, weights=Wt, scaled=scaled)
    assert np.array_equal(sol['coef'], info['COEF'][ix]) and np.array_equal(sol['adjacency'], Wf[ix] != 0)
    assert np.array_equal(sol['resvar'], info['RESVAR'][ix])
    plain = utils.neighborhood_selection(S_sub, mb_ref.GRID, 'and', tol=TOL)
    assert not np.array_equal(plain, W)


def test_searches_without_the_new_arguments_keep_their_bits():
    """``stars_search(method='mb')`` and ``cv_search(method='mb')`` called without the new arguments, and with their
    defaults spelled out, return the bits of the stateless unweighted entries -- the parent's calling convention."""
    from gglasso_amd import model_selection as ms, utils
    X, idx = _stars_inputs()
    lam = np.array(mb_ref.GRID)
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        _, a = ms.stars_search(X, lam, n_subsamples=6, seed=5, beta=0.1, tol=TOL, store_all=True, method='mb')
        _, b = ms.stars_search(X, lam, n_subsamples=6, seed=5, beta=0.1, tol=TOL, store_all=True, method='mb', weights=None,
                               scaled=False)
        _, c = ms.cv_search(X, lam, n_folds=3, seed=4, method='mb', graph_rule='or', refit=False, tol=TOL, store_all=True)
        _, d = ms.cv_search(X, lam, n_folds=3, seed=4, method='mb', graph_rule='or', refit=False, tol=TOL, store_all=True,
                            weights=None, scaled=False)
    S_sub = utils.sample_covariance_subsets(X, idx)
    W = utils.neighborhood_selection(S_sub, lam, 'and', tol=TOL)
    assert np.array_equal(a['THETA'], np.swapaxes(W, 0, 1)) and np.array_equal(a['THETA'], b['THETA']) and a['NUM'] == b['NUM']
    train, _ = ms.cv_folds(X.shape[1], 3, 4)
    Wc, ic = utils.neighborhood_selection(utils.sample_covariance_subsets(X, train), lam, 'or', tol=TOL, return_info=True)
    assert np.array_equal(c['THETA'], np.swapaxes(Wc, 0, 1)) and np.array_equal(c['RESVAR'], np.swapaxes(ic['RESVAR'], 0, 1))
    assert np.array_equal(c['THETA'], d['THETA']) and np.array_equal(c['SCORE'], d['SCORE'])
    for method_kw in (dict(weights=np.ones((17, 17))), dict(scaled=True)):
        with pytest.raises(ValueError, match="lambda1_mask"):
            ms.stars_search(X, lam, n_subsamples=3, **method_kw)
        with pytest.raises(ValueError, match="lambda1_mask"):
            ms.cv_search(X, lam, n_folds=3, **method_kw)


@MODES
@pytest.mark.parametrize("refit", (True, False))
def test_cv_search_on_the_device(refit, scaled):
    """``cv_search(method='mb', weights=, scaled=)`` against a by-hand call of the stateless entries on the fold matrices: the
    stack and the train-side numbers bit for bit, the scores within the bounds of tests/mbrefit_ref.py."""
    import mbrefit_ref as ref
    from test_gpu_mbrefit import _score_reference
    from gglasso_amd import model_selection as ms, utils
    X, lam = mb_ref.stars_data(), np.array(mb_ref.GRID)
    train, test = ms.cv_folds(X.shape[1], 3, 4)
    Wt = mbw_ref.weights(17, 1)
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        sol, st = ms.cv_search(X, lam, n_folds=3, seed=4, method='mb', graph_rule='or', refit=refit, tol=TOL, store_all=True,
                               weights=Wt, scaled=scaled)
    p, F, L = 17, 3, 4
    assert st['THETA'].shape == (L, F, p, p) and not st['STATUS'].any() and st['FAILED'] == [] and st['NOT_SOLVED'] == []
    S_tr, S_te = utils.sample_covariance_subsets(X, train), utils.sample_covariance_subsets(X, test)
    Wd, infd = utils.neighborhood_selection(S_tr, lam, 'or', tol=TOL, return_info=True, weights=Wt, scaled=scaled)
    assert np.array_equal(st['THETA'], np.swapaxes(Wd, 0, 1))
    SC, B = np.zeros((L, F)), np.zeros((L, F))
    for l in range(L):
        for f in range(F):
            if refit:
                nodes = [(j, ref.neighbours(st['THETA'][l, f, j], j, 1e-8), None, None) for j in range(p)]
            else:
                raw = infd['COEF'][f, l]
                nodes = [(j, np.flatnonzero(raw[:, j]), raw[np.flatnonzero(raw[:, j]), j], infd['RESVAR'][f, l, j]) for j in range(p)]
            SC[l, f], B[l, f] = _score_reference(S_tr[f], S_te[f], nodes)
    print(f"cv, refit={refit}, scaled={scaled}: scores within {float((np.abs(st['SCORE'] - SC) / B).max()):.3f} of their bounds")
    assert np.all(np.abs(st['SCORE'] - SC) <= B)
    assert np.array_equal(st['SCORE'], utils.mb_cv_scores(st['RESVAR'], st['HELDOUT'], st['STATUS'] != 0, 'pseudo'))
    if refit:
        rf = utils.neighborhood_refit(S_tr, Wd, 1e-8, S_te)
        assert np.array_equal(st['RESVAR'], np.swapaxes(rf['RESVAR'], 0, 1))
        assert np.array_equal(st['HELDOUT'], np.swapaxes(rf['HELDOUT'], 0, 1))
    else:
        assert np.array_equal(st['RESVAR'], np.swapaxes(infd['RESVAR'], 0, 1))
    ix = st['IX']
    S_full = utils.sample_covariance(X, center=True)
    Wf, inff = utils.neighborhood_selection(S_full, lam[:ix + 1], 'or', tol=TOL, return_info=True, weights=Wt, scaled=scaled)
    assert np.array_equal(sol['coef'], inff['COEF'][ix]) and np.array_equal(sol['adjacency'], Wf[ix] != 0)


def test_scaled_lasso_precision_and_the_front_end():
    from gglasso_amd import utils
    from gglasso_amd.problem import glasso_problem
    p, n = 17, 108
    S = mb_ref.stack(p)[1]
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        Theta, info = utils.scaled_lasso_precision(S, n=n)
        lam0 = utils.scaled_lasso_lambda(p, n)
        _, raw = utils.neighborhood_selection(S, [lam0], 'raw', return_info=True, scaled=True, weights=np.ones((p, p)))
        assert info['LAMBDA0'] == lam0 and not info['STATUS'].any()
        assert np.array_equal(Theta, utils.neighborhood_precision(raw['COEF'][0], raw['RESVAR'][0])[0])
        assert np.array_equal(Theta, Theta.T)
        d = 2.0 ** np.random.default_rng(4).integers(-3, 4, p)
        Sd = S * d[:, None] * d[None, :]
        Theta_d, info_d = utils.scaled_lasso_precision(Sd, n=n)
        mbw_ref.check_rescaled(S, Sd, d, lam0, Theta, info, Theta_d, info_d)
        X = mb_ref.stars_data()
        P = glasso_problem.from_data(X, reg=None)
        P.neighborhood_selection(select='scaled')
        S_full = utils.sample_covariance(X, center=True)
        want, winfo = utils.scaled_lasso_precision(S_full, n=X.shape[1])
    assert np.array_equal(P.solution.precision_, want) and P.reg_params['lambda1'] == utils.scaled_lasso_lambda(17, X.shape[1])
    assert np.array_equal(P.solution.adjacency_, (want != 0) & ~np.eye(17, dtype=bool)) and P.solution.adjacency_.any()
    assert np.array_equal(P.modelselect_stats['SIGMA'], winfo['SIGMA']) and not P.modelselect_stats['STATUS'].any()
    assert P.modelselect_stats['LAMBDA0'] == winfo['LAMBDA0']
    with pytest.raises(AssertionError, match="searches nothing"):
        P.neighborhood_selection(mb_ref.GRID, select='scaled')
    with pytest.raises(AssertionError, match="lambda_range"):
        P.neighborhood_selection(select='stars')
