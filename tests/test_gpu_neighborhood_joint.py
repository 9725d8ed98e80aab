"""Joint neighbourhood selection on the device (csrc/neighborhood_joint.hip behind ``ggl_neighborhood_joint_path``): the
checks of tests/mbj_ref.py against the longdouble comparison value at the small sizes, the optimality residual alone at the
sizes that reach every instantiated variant of the kernel (slots per lane x instances per wave), the bits, the identities that
tie it to the single-problem path, the rule and the refit behind it, status 2, the refusals of the C ABI, the limits, and
``joint_neighborhood_search`` against the host route."""
import warnings

import numpy as np
import pytest

import mb_ref
import mbj_ref as ref

pytestmark = pytest.mark.gpu

TOL = 1e-7


def _dev(S, om, l1, l2, rule='raw', **kw):
    from gglasso_amd import utils
    W, info = utils.joint_neighborhood_selection(S, [l1], [l2], rule=rule, instance_weights=om, tol=TOL, return_info=True, **kw)
    return W[0, 0], info


def _same(a, b):
    return sorted(a) == sorted(b) and all(np.array_equal(a[k], b[k], equal_nan=True) for k in a)


@pytest.mark.parametrize("kind", ("corr", "scaled"))
@pytest.mark.parametrize("K", (1, 2, 3, 5))
@pytest.mark.parametrize("p", (1, 2, 3, 5, 17, 63, 64, 65))
def test_device_against_the_comparison_value(p, K, kind):
    """Residual bound, distance bound, residual variance, statuses all 0, supports where the comparison value has a margin --
    all nodes, the four penalty pairs."""
    S, om = ref.stack(p, K, kind)
    for ip, (l1, l2) in enumerate(ref.PAIRS):
        coef, info = _dev(S, om, l1, l2)
        ref.check_case(p, K, kind, ip, coef, info['RESVAR'][0, 0], info['STATUS'][0, 0], TOL, "device")
        assert info['NEWTON'].max() <= 12


@pytest.mark.parametrize("p,K", ((5, 2), (17, 3)))
def test_device_with_unequal_instance_weights(p, K):
    S, om = ref.stack(p, K, 'weighted')
    for ip, (l1, l2) in enumerate(ref.PAIRS):
        coef, info = _dev(S, om, l1, l2)
        ref.check_case(p, K, 'weighted', ip, coef, info['RESVAR'][0, 0], info['STATUS'][0, 0], TOL, "device")


# every instantiated variant (slots per lane, instances per wave) and every remainder of the ownership k = w (mod 8):
# p <= 256: 4 slots; p <= 384 with more than 32 instances: 6; p <= 512: 8; beyond: 16.  K <= 8: one instance per wave; <= 16: two;
# <= 32: four; <= 64: eight.  Where the gradients no longer fit the registers (K > 32 above p = 384, K > 16 above p = 512) they
# live in device memory: the variants with 8 slots ((385, 33), (385, 64)) and 16 slots ((513, 17), (513, 33), (513, 64),
# (1024, 17): all sixteen slots in use).
WIDE = [(130, 16), (130, 17), (130, 33), (130, 64), (257, 16), (257, 17), (257, 33), (257, 64), (300, 3), (513, 4), (1024, 4),
        (513, 9), (385, 33), (385, 64), (513, 17), (513, 33), (513, 64), (1024, 17)]


@pytest.mark.parametrize("p,K", WIDE)
def test_device_by_the_optimality_residual(p, K):
    """No longdouble solve: the residual of the returned B against its bound, every node converged."""
    S, om = ref.stack(p, K, 'scaled')
    l1, l2 = ref.PAIRS[1]
    coef, info = _dev(S, om, l1, l2)
    assert not info['STATUS'].any() and np.all(np.isfinite(coef)) and (coef != 0).any()
    G = ref.check_residual(S, om, coef, info['STATUS'][0, 0], l1, l2, TOL, f"p={p} K={K}")[1]
    tau, tb = ref.resvar_reference(S, om, coef, G)                          # (the longdouble gradient is formed once)
    assert np.all(np.abs(info['RESVAR'][0, 0].astype(ref.LD) - tau).astype(np.float64) <= tb)


def test_device_bits():
    """Two calls; one chain alone against its part of a call of three; the leading two pairs of a chain; the chunk budget."""
    from gglasso_amd import _lib, utils
    S, om = ref.stack(65, 5, 'weighted')
    l1, l2 = (0.2, 0.1, 0.05), (0.2, 0.05, 0.0)
    kw = dict(rule='and', instance_weights=om, tol=TOL, refit=True, return_info=True)
    W, info = utils.joint_neighborhood_selection(S, l1, l2, **kw)
    assert W.shape == (3, 3, 5, 65, 65) and not info['STATUS'].any()
    W2, info2 = utils.joint_neighborhood_selection(S, l1, l2, **kw)
    assert np.array_equal(W, W2) and _same(info, info2)
    for c in range(3):
        W1, info1 = utils.joint_neighborhood_selection(S, l1, l2[c:c + 1], **kw)
        assert np.array_equal(W1[:, 0], W[:, c])
        assert all(np.array_equal(info1[k][:, 0], info[k][:, c], equal_nan=True) for k in info if not k.startswith('LAMBDA'))
    Wh, infoh = utils.joint_neighborhood_selection(S, l1[:2], l2, **kw)
    assert np.array_equal(Wh, W[:2])
    assert all(np.array_equal(infoh[k], info[k][:2], equal_nan=True) for k in info if not k.startswith('LAMBDA'))
    lib = _lib.load()
    try:
        lib.ggl_mb_joint_chunk_budget(1)                                    # one chain per chunk
        W3, info3 = utils.joint_neighborhood_selection(S, l1, l2, **kw)
        lib.ggl_mb_joint_chunk_budget(2 * 2 * 3 * 5 * 65 * 65 * 8)          # two chains per chunk: 2 + 1
        W4, info4 = utils.joint_neighborhood_selection(S, l1, l2, **kw)
    finally:
        lib.ggl_mb_joint_chunk_budget(0)
    assert np.array_equal(W, W3) and _same(info, info3) and np.array_equal(W, W4) and _same(info, info4)


def _node_norm(a):
    a = np.asarray(a, dtype=np.float64)
    return np.sqrt((a * a).reshape(-1, a.shape[-1]).sum(axis=0))


def test_device_identities():
    """K = 1 is the single path at lambda1 + lambda2, lambda2 = 0 the K separate paths (both ``utils.neighborhood_selection``),
    K identical instances with lambda1 = 0 the lasso at lambda2 / sqrt(K): within the sum of the two distance bounds.  With
    lambda1 = 0 the K supports coincide exactly; with lambda1 > 0 an active group has a zero member; the null model."""
    from gglasso_amd import utils

    def lasso(S, lam):
        W, info = utils.neighborhood_selection(S, [lam], 'raw', tol=TOL, return_info=True)
        assert not info['STATUS'].any()
        return W[..., 0, :, :], W

    p = 17
    S, _ = ref.stack(p, 1, 'scaled')
    coef, info = _dev(S, None, 0.05, 0.1)
    one, Wl = lasso(S[0], 0.15)
    room = (_node_norm(ref.residual_bound(S, None, coef, 0.1, TOL)) + _node_norm(mb_ref.residual_bound(S[0], Wl, TOL)[0])) / ref.strong_convexity(S, None)
    assert not info['STATUS'].any() and np.all(_node_norm(coef[0] - one) <= room)
    S, _ = ref.stack(p, 3, 'scaled')
    coef, info = _dev(S, None, 0.1, 0.0)
    each, Wl = lasso(S, 0.1)
    lb = np.stack([mb_ref.residual_bound(S[k], Wl[k], TOL)[0] for k in range(3)])
    room = (_node_norm(ref.residual_bound(S, None, coef, 0.0, TOL)) + _node_norm(lb)) / ref.strong_convexity(S, None)
    assert not info['STATUS'].any() and np.all(_node_norm(coef - each) <= room)
    K, S1 = 4, mb_ref.case(p, 3)
    S = np.stack([S1] * K)
    coef, info = _dev(S, None, 0.0, 0.3)
    one, Wl = lasso(S1, 0.3 / np.sqrt(K))
    room = (_node_norm(ref.residual_bound(S, None, coef, 0.3, TOL)) + np.sqrt(K) * _node_norm(mb_ref.residual_bound(S1, Wl, TOL)[0])) \
        / ref.strong_convexity(S, None)
    assert not info['STATUS'].any() and np.all(_node_norm(coef - one[None]) <= room)
    assert np.array_equal(coef, np.broadcast_to(coef[0], coef.shape))       # identical instances in identical lanes' arithmetic
    for kind in ('corr', 'scaled'):
        S, om = ref.stack(p, 4, kind)
        coef, info = _dev(S, om, 0.0, 0.15)
        assert not info['STATUS'].any() and (coef != 0).any() and np.array_equal(coef != 0, np.broadcast_to((coef != 0)[0], coef.shape))
    S, om = ref.stack(p, 4, 'corr')
    coef, info = _dev(S, om, 0.1, 0.05)
    nz = coef != 0
    assert not info['STATUS'].any() and np.any(nz.any(axis=0) & ~nz.all(axis=0))
    S, om = ref.stack(p, 3, 'weighted')
    sg = np.maximum(np.abs(om[:, None, None] * S) - 0.05, 0.0)
    nrm = np.sqrt((sg * sg).sum(axis=0))
    nrm[np.arange(p), np.arange(p)] = 0.0
    coef, info = _dev(S, om, 0.05, float(nrm.max()) * (1 + 1e-12))
    assert not coef.any() and not info['STATUS'].any() and not info['SWEEPS'].any()
    assert np.array_equal(info['RESVAR'][0, 0], np.diagonal(S, axis1=1, axis2=2))
    coef, info = _dev(np.array([[[2.0]], [[3.0]]]), None, 0.1, 0.1)
    assert coef.shape == (2, 1, 1) and not coef.any() and not info['STATUS'].any() and np.array_equal(info['RESVAR'][0, 0], [[2.0], [3.0]])


def test_device_rule_and_refit():
    """The symmetrised outputs are bitwise symmetric with a zero diagonal and the definition's, per instance; with the refit
    the tables are those of ``utils.neighborhood_refit`` on the downloaded symmetrised stack, bit for bit."""
    from gglasso_amd import utils
    S, om = ref.stack(65, 3, 'scaled')
    l1, l2 = (0.1, 0.05), (0.05, 0.2)
    raw = utils.joint_neighborhood_selection(S, l1, l2, rule='raw', tol=TOL)
    for rule in ('and', 'or'):
        W, info = utils.joint_neighborhood_selection(S, l1, l2, rule=rule, tol=TOL, refit=True, return_info=True)
        assert np.array_equal(W, np.swapaxes(W, -1, -2)) and not np.diagonal(W, axis1=-2, axis2=-1).any()
        assert np.array_equal(W, mb_ref.and_or(raw, rule)) and np.array_equal(W, utils.neighborhood_graph(raw, rule))
        rf = utils.neighborhood_refit(S, np.ascontiguousarray(np.moveaxis(W.reshape(4, 3, 65, 65), 1, 0)))
        for key, name in (('COEF', 'REFIT_COEF'), ('RESVAR', 'REFIT_RESVAR'), ('DEGREE', 'DEGREE'), ('STATUS', 'REFIT_STATUS')):
            got = info[name].reshape((4, 3) + info[name].shape[3:])
            assert np.array_equal(np.moveaxis(rf[key], 0, 1), got, equal_nan=True), (rule, key)
        assert not info['REFIT_STATUS'].any() and np.array_equal(info['DEGREE'], (np.abs(W) >= 1e-8).sum(axis=-1))


def test_device_status_2():
    """One symmetric pair of entries (a, b) of one instance is finite but so large that its square overflows.  The first pair's
    lambda1 lies above it: every node is the null model.  From the second pair on the nodes that meet it -- a, b and whoever
    activates one of them -- are status 2: all K columns NaN with diagonal 0, tau^2 NaN.  Every other node never read the
    entry, and its bits are those of the call on the clean stack."""
    from gglasso_amd import utils
    p, K, a, b = 17, 3, 3, 4
    clean, _ = ref.stack(p, K, 'corr')
    dirty = clean.copy()
    dirty[1, a, b] = dirty[1, b, a] = 1e155
    l1, l2 = (1e156, 0.1, 0.05), (0.05,)
    kw = dict(rule='raw', tol=TOL, return_info=True)
    Wc, ic = utils.joint_neighborhood_selection(clean, l1, l2, **kw)
    Wd, idd = utils.joint_neighborhood_selection(dirty, l1, l2, **kw)
    st = idd['STATUS'][:, 0]                                                # (L,p)
    assert not ic['STATUS'].any() and not st[0].any() and not Wd[0].any() and set(np.unique(st)) == {0, 2}
    dead = st == 2                                                          # (L,p): a dead node stays dead, later pairs add to them
    assert dead[1, a] and dead[1, b] and np.all(dead[2][dead[1]]) and 2 <= dead[1].sum() <= dead[2].sum() < p
    off = ~np.eye(p, dtype=bool)
    for l in (0, 1, 2):
        cols = Wd[l, 0][:, :, dead[l]]                                      # (K,p,dead)
        assert np.all(np.isnan(cols[:, off[:, dead[l]]])) and np.all(Wd[l, 0][:, np.arange(p), np.arange(p)] == 0)
        assert np.all(np.isnan(idd['RESVAR'][l, 0][:, dead[l]]))
        live = ~dead[l]
        assert np.array_equal(Wd[l, 0][:, :, live], Wc[l, 0][:, :, live])
        assert np.array_equal(idd['RESVAR'][l, 0][:, live], ic['RESVAR'][l, 0][:, live])
        assert all(np.array_equal(idd[k][l, 0][live], ic[k][l, 0][live]) for k in ('SWEEPS', 'STATUS', 'NEWTON'))


def _raw_call(S, lam1, lam2, om=None, K=None, p=None, C=None, L=None, rule=1, tol=TOL, max_sweeps=100, refit=0, t=1e-8,
              s_null=False, l1_null=False, l2_null=False, info=True):
    """One raw ``ggl_neighborhood_joint_path`` call with sentinel-filled outputs: (rc, message, the six output arrays)."""
    from gglasso_amd import _lib
    lib = _lib.load()
    S = np.ascontiguousarray(S, dtype=np.float64)
    lam1, lam2 = np.ascontiguousarray(lam1, dtype=np.float64), np.ascontiguousarray(lam2, dtype=np.float64)
    om = None if om is None else np.ascontiguousarray(om, dtype=np.float64)
    Kb, pb = S.shape[0], S.shape[-1]
    Cb, Lb = lam1.shape
    n = Cb * Lb * Kb * pb
    outs = [np.full(n * pb, -7.5), np.full(n, -7.5), np.full(Cb * Lb * pb * 3, -7, dtype=np.int32), np.full(n * pb, -7.5),
            np.full(n, -7.5), np.full(n * 2, -7, dtype=np.int32)]
    ip = lambda x: x.ctypes.data_as(_lib._ip)
    rc = lib.ggl_neighborhood_joint_path(0, Kb if K is None else K, pb if p is None else p, None if s_null else _lib.ptr(S),
                                         _lib.ptr(om), Cb if C is None else C, Lb if L is None else L,
                                         None if l1_null else _lib.ptr(lam1), None if l2_null else _lib.ptr(lam2), rule, tol,
                                         max_sweeps, refit, t, _lib.ptr(outs[0]), _lib.ptr(outs[1]), ip(outs[2]) if info else None,
                                         _lib.ptr(outs[3]), _lib.ptr(outs[4]), ip(outs[5]))
    return rc, _lib.last_error(), outs


def test_refusals_write_nothing():
    """GGL_E_ARG before any device work: the outputs keep their sentinel, the message names the culprit, and the next valid
    call returns what it returned before."""
    from gglasso_amd import _lib
    S, _ = ref.stack(5, 3, 'scaled')
    S = S.copy()
    lam1, lam2 = np.array([[0.2, 0.1], [0.2, 0.1]]), np.array([[0.1, 0.1], [0.0, 0.0]])
    rc, msg, before = _raw_call(S, lam1, lam2, refit=1)
    assert rc == 0 and all(not np.any(o == (-7 if o.dtype == np.int32 else -7.5)) for o in before)
    nan_S, neg_d, asym = S.copy(), S.copy(), S.copy()
    nan_S[1, 2, 3] = nan_S[1, 3, 2] = np.inf
    neg_d[2, 4, 4] = 0.0
    asym[2, 1, 3] = np.nextafter(asym[2, 1, 3], 2.0)
    l1neg, l2nan, both0 = lam1.copy(), lam2.copy(), lam1.copy()
    l1neg[1, 0], l2nan[0, 1], both0[1, 1] = -0.1, np.nan, 0.0
    cases = {
        "K": (dict(K=0), "K = 0"), "p": (dict(p=0), "p = 0"), "C": (dict(C=0), "C = 0"), "L": (dict(L=0), "L = 0"),
        "K max": (dict(K=65), "K = 65"), "p max": (dict(p=1025), "p = 1025"), "S NULL": (dict(s_null=True), "S must not be NULL"),
        "lam1 NULL": (dict(l1_null=True), "lam1"), "lam2 NULL": (dict(l2_null=True), "lam2"), "info NULL": (dict(info=False), "info_out"),
        "lam1 < 0": (dict(lam1=l1neg), "lam1 of (chain 1, index 0)"), "lam2 nan": (dict(lam2=l2nan), "lam2 of (chain 0, index 1)"),
        "both 0": (dict(lam1=both0), "(chain 1, index 1)"), "omega 0": (dict(om=[1.0, 0.0, 1.0]), "omega[1]"),
        "omega inf": (dict(om=[1.0, 1.0, np.inf]), "omega[2]"), "tol < 0": (dict(tol=-1e-9), "tol"), "tol nan": (dict(tol=np.nan), "tol"),
        "sweeps": (dict(max_sweeps=0), "max_sweeps"), "rule": (dict(rule=3), "rule = 3"), "rule < 0": (dict(rule=-1), "rule = -1"),
        "raw refit": (dict(rule=0, refit=1), "GGL_MB_RAW with refit"), "t < 0": (dict(refit=1, t=-1.0), "threshold"),
        "t inf": (dict(refit=1, t=np.inf), "threshold"), "S inf": (dict(S=nan_S), "instance 1: the entry (2, 3)"),
        "diagonal": (dict(S=neg_d), "instance 2, variable 4"), "asymmetric": (dict(S=asym), "instance 2 is not bitwise symmetric: the entries (1, 3)"),
    }
    for name, (kw, culprit) in cases.items():
        args = dict(S=S, lam1=lam1, lam2=lam2)
        args.update(kw)
        rc, msg, outs = _raw_call(**args)
        assert rc == _lib.E_ARG and culprit in msg, (name, rc, msg)
        assert all(np.all(o == (-7 if o.dtype == np.int32 else -7.5)) for o in outs), name
    rc, msg, after = _raw_call(S, lam1, lam2, refit=1)
    assert rc == 0 and all(np.array_equal(x, y, equal_nan=True) for x, y in zip(before, after))


def test_limits():
    from gglasso_amd import _lib, utils
    Kmax, pmax = utils.mb_joint_limits()
    assert Kmax >= 64 and pmax >= 1024
    one = np.ones((1, 1))
    for kw, culprit in ((dict(K=Kmax + 1), f"K = {Kmax + 1}"), (dict(p=pmax + 1), f"p = {pmax + 1}")):
        rc, msg, outs = _raw_call(np.ones((1, 1, 1)), one, one, **kw)
        assert rc == _lib.E_ARG and culprit in msg and np.all(outs[2] == -7)
    # K at the limit
    S, om = ref.stack(17, Kmax, 'scaled')
    l1, l2 = ref.PAIRS[0]
    coef, info = _dev(S, om, l1, l2)
    assert not info['STATUS'].any() and (coef != 0).any()
    ref.check_residual(S, om, coef, info['STATUS'][0, 0], l1, l2, TOL, f"K={Kmax}")


def test_search_on_the_device_against_the_host_route():
    from gglasso_amd import model_selection as ms
    from gglasso_amd.problem import glasso_problem
    S, _ = ref.stack(17, 3, 'scaled')
    N = [400, 600, 500]
    l1, l2 = (0.2, 0.1, 0.05, 0.025), (0.1, 0.02)
    sol_d, st_d = ms.joint_neighborhood_search(S, N, l1, l2, tol=TOL, host=False)
    sol_h, st_h = ms.joint_neighborhood_search(S, N, l1, l2, tol=TOL, host=True)
    srt = np.sort(st_h['SCORE'].ravel())
    assert srt[1] - srt[0] > 1e-3 * abs(srt[0])                              # the choice has a margin
    assert st_d['IX'] == st_h['IX'] and st_d['BEST'] == st_h['BEST'] and np.array_equal(st_d['DEGREE'], st_h['DEGREE'])
    assert not st_d['STATUS'].any() and not st_d['REFIT_STATUS'].any()
    # With equal graphs (DEGREE above, adjacency below) both routes solve the same systems S_AA beta = s_A by Cholesky in
    # float64.  Higham, Accuracy and Stability, Thm 10.4 and (10.7): the computed solution solves (S_AA + E) x = s_A with
    # ||E||_2 <= d gamma_{3d+1} ||S_AA||_2, so each route is within REL = 2 d (3d + 1) u kappa of the exact beta in relative
    # norm, d the largest degree (at least 2) and kappa the largest condition number of an S^(k), which bounds that of every
    # principal submatrix.  Two routes: 2 REL.  tau^2 is stationary in beta at the solution (second order) and its evaluation
    # rounds (2d + 3) times on terms of at most S_jj + 2 |s' beta| + beta' S beta <= 3 kappa tau^2: within REL relative as well.
    # The score: |d log tau^2| <= 2 REL per regression, times N_k, summed.  Theta = (1, -beta) / tau^2: 4 REL of its largest entry.
    d = max(2, int(st_d['DEGREE'].max()))
    kappa = max(np.linalg.cond(S[k]) for k in range(3))
    REL = 2 * d * (3 * d + 1) * ref.U * kappa
    assert np.all(np.abs(st_d['SCORE'] - st_h['SCORE']) <= 2 * REL * 17 * sum(N))
    assert np.array_equal(sol_d['adjacency'], sol_h['adjacency']) and np.array_equal(sol_d['common_adjacency'], sol_h['common_adjacency'])
    assert np.all(np.abs(sol_d['coef'] - sol_h['coef']) <= 2 * REL * np.sqrt((sol_h['coef'] ** 2).sum(axis=1, keepdims=True)))
    assert np.all(np.abs(sol_d['resvar'] - sol_h['resvar']) <= 2 * REL * sol_h['resvar'])
    assert np.all(np.abs(sol_d['precision'] - sol_h['precision']) <= 4 * REL * np.abs(sol_h['precision']).max())
    # the chosen point's further call against its part of a grid call
    from gglasso_amd import utils
    W, info = utils.joint_neighborhood_selection(S, l1, l2, tol=TOL, refit=True, return_info=True)
    i1, i2 = st_d['IX']
    assert np.array_equal(sol_d['W'], W[i1, i2]) and np.array_equal(sol_d['coef'], info['REFIT_COEF'][i1, i2])
    assert np.array_equal(sol_d['resvar'], info['REFIT_RESVAR'][i1, i2])
    P = glasso_problem(S.copy(), N, reg='GGL')
    P.joint_neighborhood_selection(l1, l2, tol=TOL)
    assert np.array_equal(P.solution.precision_, sol_d['precision']) and np.array_equal(P.solution.adjacency_, sol_d['adjacency'].astype(int))
    assert P.reg_params['lambda1'] == st_d['BEST']['lambda1'] and P.reg_params['lambda2'] == st_d['BEST']['lambda2']


def test_other_routes_are_untouched():
    """One call each of the graphical lasso and of the single-problem path, before and after a joint call in the same process:
    the same keys and bits (the joint entry keeps no state that another entry reads)."""
    from gglasso_amd import solver, utils
    S = mb_ref.stack(17)

    def both():
        with warnings.catch_warnings():
            warnings.simplefilter("ignore")
            sol, info = solver.ADMM_MGL(S.copy(), 0.1, 0.05, 'GGL', np.tile(np.eye(17), (3, 1, 1)), tol=1e-7, rtol=1e-7, max_iter=50)
        W, inf = utils.neighborhood_selection(S, mb_ref.GRID, 'and', tol=TOL, return_info=True)
        return sol, W, inf

    sol_a, W_a, inf_a = both()
    _dev(ref.stack(17, 3, 'scaled')[0], None, 0.1, 0.05, rule='and', refit=True)
    sol_b, W_b, inf_b = both()
    assert sorted(sol_a) == sorted(sol_b) and all(np.array_equal(sol_a[k], sol_b[k]) for k in sol_a)
    assert np.array_equal(W_a, W_b) and _same(inf_a, inf_b)
