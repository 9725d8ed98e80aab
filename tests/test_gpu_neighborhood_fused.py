"""Fused joint neighbourhood selection on the device (csrc/neighborhood_fused.hip behind ``ggl_neighborhood_fused_path``): the
checks of tests/mbf_ref.py against the longdouble comparison value at the small sizes, the optimality residual alone at the
sizes that reach every instantiated variant of the kernel, the bits, statuses 1 and 2, the refusals of the C ABI, the limits,
and ``fused_neighborhood_search`` against the host route."""
import numpy as np
import pytest

import mbf_ref as ref

pytestmark = pytest.mark.gpu

TOL = 1e-7


def _dev(S, om, l1, l2, rule='raw', **kw):
    from gglasso_amd import utils
    W, info = utils.fused_neighborhood_selection(S, [l1], [l2], rule=rule, instance_weights=om, tol=TOL, return_info=True, **kw)
    return W[0, 0], info


def _same(a, b):
    return sorted(a) == sorted(b) and all(np.array_equal(a[k], b[k], equal_nan=True) for k in a)


@pytest.mark.parametrize("kind", ref.KINDS)
@pytest.mark.parametrize("K", (1, 2, 3, 5))
@pytest.mark.parametrize("p", (1, 2, 3, 5, 17, 63, 64, 65))
def test_device_against_the_comparison_value(p, K, kind):
    """Residual bound and residual variance at every node, distance bound at the nodes of the comparison value, statuses all 0,
    the third info column 0 -- the four penalty pairs."""
    S, om = ref.stack(p, K, kind)
    for ip, (l1, l2) in enumerate(ref.PAIRS):
        coef, info = _dev(S, om, l1, l2)
        ref.check_case(p, K, kind, ip, coef, info['RESVAR'][0, 0], info['STATUS'][0, 0], TOL, "device")
        assert not info['NEWTON'].any()


# Every instantiated variant (slots per lane x instances per wave) at the smallest (p, K) that selects it, then the sizes of the
# group route's list: 4 slots up to p = 256, 6 up to 384 with more than 32 instances, 8 up to 512, 16 beyond; K <= 8: one
# instance per wave, <= 16: two, <= 32: four, <= 64: eight.  (4,1) is every small case above.  Memory-resident: K > 32 above
# p = 384 (8 slots), K > 8 above p = 512 (16 slots; the group route keeps K <= 16 in registers there, this one does not).
WIDE = [(17, 9), (17, 17), (17, 33), (257, 3), (257, 9), (257, 17), (257, 33), (513, 4), (385, 33), (513, 9),
        (130, 16), (17, 64), (513, 17), (1024, 4)]


@pytest.mark.parametrize("p,K", WIDE)
def test_device_by_the_optimality_residual(p, K):
    """No longdouble solve: every node converged and finite; the residual of the returned B against its bound, at every node
    up to p = 130 and at ``mbf_ref.spread_nodes(p)`` beyond (the longdouble scan of every block of every node would take
    longer than everything else in this file)."""
    S, om = ref.stack(p, K, 'weighted')
    l1, l2 = ref.PAIRS[1]
    coef, info = _dev(S, om, l1, l2)
    assert not info['STATUS'].any() and np.all(np.isfinite(coef)) and (coef != 0).any()
    ref.check_residual(S, om, coef, info['STATUS'][0, 0], l1, l2, TOL, f"p={p} K={K}", None if p <= 130 else ref.spread_nodes(p))


def test_fused_segments_are_bitwise_constant():
    """Equal diagonals, equal weights: the block step is exact and writes the scan's one value per segment, so where the
    comparison value is fused (consecutive instances bitwise equal and not zero) the device's values are bitwise equal too; and
    the device never returns consecutive values that are nearly but not bitwise equal (apart by less than 2^-40 of their size: a
    segment value carries a few roundings, a jump is a property of the data)."""
    S, _ = ref.stack(65, 5, 'corr')
    nodes = ref.nodes_of(65)
    l1, l2 = 0.02, 0.02                                                     # small enough that segments end between non-zero values
    coef, info = _dev(S, None, l1, l2)
    assert not info['STATUS'].any()
    B = ref.solve(S, None, ((l1, l2),), nodes)[0]
    assert float(ref.group_norm(ref.residual(S, None, B, l1, l2, nodes)[0]).max()) <= 1e-15
    seg = (B[1:] == B[:-1]) & (B[1:] != 0)
    assert seg.sum() > 20 and ((B[1:] != B[:-1]) & (B[1:] != 0) & (B[:-1] != 0)).sum() > 20     # both kinds occur
    dev = coef[:, :, nodes]
    assert np.all((dev[1:] == dev[:-1])[seg])
    d = np.abs(np.diff(coef, axis=0))
    assert not np.any((d != 0) & (d <= 2.0 ** -40 * np.maximum(np.abs(coef[1:]), np.abs(coef[:-1]))))


def test_device_bits():
    """Two calls; one chain alone against its part of a call of three; the leading two pairs of a chain; the chunk budget;
    ``_last`` against the last pair of ``_path``."""
    from gglasso_amd import _lib, utils
    S, om = ref.stack(65, 5, 'weighted')
    l1, l2 = (0.2, 0.1, 0.05), (0.2, 0.05, 0.0)
    kw = dict(rule='and', instance_weights=om, tol=TOL, refit=True, return_info=True)
    W, info = utils.fused_neighborhood_selection(S, l1, l2, **kw)
    assert W.shape == (3, 3, 5, 65, 65) and not info['STATUS'].any()
    W2, info2 = utils.fused_neighborhood_selection(S, l1, l2, **kw)
    assert np.array_equal(W, W2) and _same(info, info2)
    for c in range(3):
        W1, info1 = utils.fused_neighborhood_selection(S, l1, l2[c:c + 1], **kw)
        assert np.array_equal(W1[:, 0], W[:, c])
        assert all(np.array_equal(info1[k][:, 0], info[k][:, c], equal_nan=True) for k in info if not k.startswith('LAMBDA'))
    Wh, infoh = utils.fused_neighborhood_selection(S, l1[:2], l2, **kw)
    assert np.array_equal(Wh, W[:2])
    assert all(np.array_equal(infoh[k], info[k][:2], equal_nan=True) for k in info if not k.startswith('LAMBDA'))
    lib = _lib.load()
    try:
        lib.ggl_mb_joint_chunk_budget(1)                                    # one chain per chunk
        W3, info3 = utils.fused_neighborhood_selection(S, l1, l2, **kw)
        lib.ggl_mb_joint_chunk_budget(2 * 2 * 3 * 5 * 65 * 65 * 8)          # two chains per chunk: 2 + 1
        W4, info4 = utils.fused_neighborhood_selection(S, l1, l2, **kw)
    finally:
        lib.ggl_mb_joint_chunk_budget(0)
    assert np.array_equal(W, W3) and _same(info, info3) and np.array_equal(W, W4) and _same(info, info4)
    Sm, a, b, w = utils._mbj_args(S, l1, l2, 'and', om, TOL, 10000, True, 1e-8, 'fused')
    last = utils._joint_run(Sm, a, b, w, 'and', TOL, 10000, True, 1e-8, 0, False, last_only=True, coupling='fused')
    assert np.array_equal(last['W'], W[-1]) and np.array_equal(last['REFIT_COEF'], info['REFIT_COEF'][-1])
    assert np.array_equal(last['RESVAR'], info['RESVAR']) and np.array_equal(last['INFO'][..., 1], info['STATUS'])


def test_device_status_1_and_2():
    """One sweep is a cap: status 1 with finite values, the nodes that finish within it unchanged.  Status 2 as the group
    route's test produces it: one symmetric pair of entries (a, b) of one instance is finite but overflows when squared; the
    first pair's lambda1 lies above it, from the second pair on the nodes that meet it are NaN with diagonal 0, and every other
    node has the bits of the call on the clean stack."""
    from gglasso_amd import utils
    p, K, a, b = 17, 3, 3, 4
    clean, _ = ref.stack(p, K, 'corr')
    kw = dict(rule='raw', tol=TOL, return_info=True)
    W1, i1 = utils.fused_neighborhood_selection(clean, [0.05], [0.05], max_sweeps=1, **kw)
    assert np.any(i1['STATUS'] == 1) and set(np.unique(i1['STATUS'])) <= {0, 1} and np.all(np.isfinite(W1)) and i1['SWEEPS'].max() == 1
    dirty = clean.copy()
    dirty[1, a, b] = dirty[1, b, a] = 1e155
    l1, l2 = (1e156, 0.1, 0.05), (0.05,)
    Wc, ic = utils.fused_neighborhood_selection(clean, l1, l2, **kw)
    Wd, idd = utils.fused_neighborhood_selection(dirty, l1, l2, **kw)
    st = idd['STATUS'][:, 0]                                                # (L,p)
    assert not ic['STATUS'].any() and not st[0].any() and not Wd[0].any() and set(np.unique(st)) == {0, 2}
    dead = st == 2
    assert dead[1, a] and dead[1, b] and np.all(dead[2][dead[1]]) and 2 <= dead[1].sum() <= dead[2].sum() < p
    off = ~np.eye(p, dtype=bool)
    for l in (0, 1, 2):
        cols = Wd[l, 0][:, :, dead[l]]
        assert np.all(np.isnan(cols[:, off[:, dead[l]]])) and np.all(Wd[l, 0][:, np.arange(p), np.arange(p)] == 0)
        assert np.all(np.isnan(idd['RESVAR'][l, 0][:, dead[l]]))
        live = ~dead[l]
        assert np.array_equal(Wd[l, 0][:, :, live], Wc[l, 0][:, :, live])
        assert np.array_equal(idd['RESVAR'][l, 0][:, live], ic['RESVAR'][l, 0][:, live])
        assert all(np.array_equal(idd[k][l, 0][live], ic[k][l, 0][live]) for k in ('SWEEPS', 'STATUS', 'NEWTON'))


def _raw_call(S, lam1, lam2, om=None, K=None, p=None, C=None, L=None, rule=1, tol=TOL, max_sweeps=100, refit=0, t=1e-8,
              s_null=False, l1_null=False, l2_null=False, info=True, last=False):
    """One raw ``ggl_neighborhood_fused_path`` (or ``_last``) call with sentinel-filled outputs: (rc, message, the outputs)."""
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
    entry = lib.ggl_neighborhood_fused_last if last else lib.ggl_neighborhood_fused_path
    rc = entry(0, Kb if K is None else K, pb if p is None else p, None if s_null else _lib.ptr(S), _lib.ptr(om),
               Cb if C is None else C, Lb if L is None else L, None if l1_null else _lib.ptr(lam1),
               None if l2_null else _lib.ptr(lam2), rule, tol, max_sweeps, refit, t, _lib.ptr(outs[0]), _lib.ptr(outs[1]),
               ip(outs[2]) if info else None, _lib.ptr(outs[3]), _lib.ptr(outs[4]), ip(outs[5]))
    return rc, _lib.last_error(), outs


def test_refusals_write_nothing():
    """GGL_E_ARG before any device work, from both entries: the outputs keep their sentinel, the message names the culprit, and
    the next valid call returns what it returned before.  lam2 > 0 with K = 1 is no refusal: it is inert."""
    from gglasso_amd import _lib
    S, _ = ref.stack(5, 3, 'weighted')
    S = S.copy()
    lam1, lam2 = np.array([[0.2, 0.1], [0.2, 0.1]]), np.array([[0.1, 0.1], [0.0, 0.0]])
    rc, msg, before = _raw_call(S, lam1, lam2, refit=1)
    assert rc == 0 and all(not np.any(o == (-7 if o.dtype == np.int32 else -7.5)) for o in before)
    assert np.all(before[2].reshape(-1, 3)[:, 2] == 0)                      # the third info column
    nan_S, neg_d, asym = S.copy(), S.copy(), S.copy()
    nan_S[1, 2, 3] = nan_S[1, 3, 2] = np.inf
    neg_d[2, 4, 4] = 0.0
    asym[2, 1, 3] = np.nextafter(asym[2, 1, 3], 2.0)
    l1neg, l2nan, both0 = lam1.copy(), lam2.copy(), lam1.copy()
    l1neg[1, 0], l2nan[0, 1], both0[1, 1] = -0.1, np.nan, 0.0
    cases = {
        "K": (dict(K=0), "K = 0"), "p": (dict(p=0), "p = 0"), "C": (dict(C=0), "C = 0"), "L": (dict(L=0), "L = 0"),
        "K max": (dict(K=65), "K = 65, k_mb_fused_path"), "p max": (dict(p=1025), "p = 1025, k_mb_fused_path"),
        "S NULL": (dict(s_null=True), "S must not be NULL"),
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
        for last in (False, True):
            args = dict(S=S, lam1=lam1, lam2=lam2, last=last)
            args.update(kw)
            rc, msg, outs = _raw_call(**args)
            assert rc == _lib.E_ARG and culprit in msg, (name, rc, msg)
            assert all(np.all(o == (-7 if o.dtype == np.int32 else -7.5)) for o in outs), name
    rc, msg, after = _raw_call(S, lam1, lam2, refit=1)
    assert rc == 0 and all(np.array_equal(x, y, equal_nan=True) for x, y in zip(before, after))
    one = _raw_call(S[:1], lam1, lam2)[2]
    zero = _raw_call(S[:1], lam1, np.zeros_like(lam2))[2]
    assert np.array_equal(one[0], zero[0]) and np.array_equal(one[1], zero[1]) and np.array_equal(one[2], zero[2])


def test_limits():
    from gglasso_amd import _lib, utils
    Kmax, pmax = utils.mb_fused_limits()
    assert Kmax >= 64 and pmax >= 1024
    one = np.ones((1, 1))
    for kw, culprit in ((dict(K=Kmax + 1), f"K = {Kmax + 1}"), (dict(p=pmax + 1), f"p = {pmax + 1}")):
        rc, msg, outs = _raw_call(np.ones((1, 1, 1)), one, one, **kw)
        assert rc == _lib.E_ARG and culprit in msg and np.all(outs[2] == -7)


def test_search_on_the_device_against_the_host_route():
    from gglasso_amd import model_selection as ms
    from gglasso_amd.problem import glasso_problem
    S, om = ref.stack(17, 3, 'weighted')
    N = [400, 600, 500]
    l1, l2 = (0.2, 0.1, 0.05, 0.025), (0.1, 0.02)
    sol_d, st_d = ms.fused_neighborhood_search(S, N, l1, l2, instance_weights=om, tol=TOL, host=False)
    sol_h, st_h = ms.fused_neighborhood_search(S, N, l1, l2, instance_weights=om, tol=TOL, host=True)
    srt = np.sort(st_h['SCORE'].ravel())
    assert srt[1] - srt[0] > 1e-3 * abs(srt[0])                              # the choice has a margin
    assert st_d['IX'] == st_h['IX'] and st_d['BEST'] == st_h['BEST'] and np.array_equal(st_d['DEGREE'], st_h['DEGREE'])
    assert not st_d['STATUS'].any() and not st_d['REFIT_STATUS'].any() and not st_d['NEWTON'].any()
    # The refit's backward error, as in the group route's test (Higham, Accuracy and Stability, Thm 10.4 and (10.7)): with
    # equal graphs both routes solve the same systems S_AA beta = s_A by Cholesky in float64, each within REL = 2 d (3d + 1) u
    # kappa of the exact beta in relative norm, d the largest degree (at least 2), kappa the largest condition number of an
    # S^(k).  Two routes: 2 REL; tau^2 within REL relative as well; the score: 2 REL per regression, times N_k, summed.
    d = max(2, int(st_d['DEGREE'].max()))
    kappa = max(np.linalg.cond(S[k]) for k in range(3))
    REL = 2 * d * (3 * d + 1) * ref.U * kappa
    assert np.all(np.abs(st_d['SCORE'] - st_h['SCORE']) <= 2 * REL * 17 * sum(N))
    assert np.array_equal(sol_d['adjacency'], sol_h['adjacency']) and np.array_equal(sol_d['changed_edges'], sol_h['changed_edges'])
    assert np.all(np.abs(sol_d['coef'] - sol_h['coef']) <= 2 * REL * np.sqrt((sol_h['coef'] ** 2).sum(axis=1, keepdims=True)))
    assert np.all(np.abs(sol_d['resvar'] - sol_h['resvar']) <= 2 * REL * sol_h['resvar'])
    P = glasso_problem(S.copy(), N, reg='FGL')
    P.fused_neighborhood_selection(l1, l2, instance_weights=om, tol=TOL)
    assert np.array_equal(P.solution.precision_, sol_d['precision']) and np.array_equal(P.solution.adjacency_, sol_d['adjacency'].astype(int))
    assert P.reg_params['lambda1'] == st_d['BEST']['lambda1'] and P.reg_params['lambda2'] == st_d['BEST']['lambda2']
    assert np.array_equal(P.neighborhood_['changed_edges'], sol_d['changed_edges'])
