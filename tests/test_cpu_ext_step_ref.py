"""tests/ext_step_ref.py pinned without a GPU.  Fed the oracle's own Omega, the helper reproduces iterations 1 AND 2 of
oracle.ext_ADMM_MGL on every case of the table (per problem for the batch cases) and iteration 1 of the G14 trajectories written by
the reference solver, to rounding: <= 1e-13 absolute on these O(1) problems.  The oracle starts from Theta = Lambda = Omega_0 and
L = 0, so iteration 1 runs from that start with the case's S, duals, groups and thresholds; iteration 2 then starts from a state
with Lambda != Theta and (latent) L != 0, which is the general form of the step.  The conditions the GPU test relies on are
asserted here with the oracle's Omega: nothing on a threshold, 10 % .. 90 % of the off-diagonal entries and of the groups zeroed for
every problem, two problems of a batch with different group patterns, sums 0, 1 and 3 positive."""
import numpy as np
import pytest

import ext_step_ref as xr
from conftest import load_golden
from oracle import ggl_oracle as orc

TOL = 1e-13
IDS = [c.name for c in xr.CASES]


def _pad(blocks, pk, P, identity):
    from gglasso_amd.ext_solver import _pad as pad
    return pad(blocks, len(pk), np.asarray(pk), P, identity)


def _sums_of(sol, prev, pk, rho, tol, rtol):
    """the five sums from the oracle's dicts with numpy's norms, and ext_stopping_criterion's four numbers"""
    K = len(pk)
    n2 = lambda A: float(np.linalg.norm(A) ** 2)          # noqa: E731
    sq = np.zeros(5)
    for k in range(K):
        sq += [n2(sol["Omega"][k]) + n2(sol["Lambda"][k]), n2(sol["Theta"][k] - sol["L"][k]) + n2(sol["Theta"][k]),
               n2(sol["X0"][k]) + n2(sol["X1"][k]), n2(sol["Omega"][k] - sol["Theta"][k] + sol["L"][k]) + n2(sol["Lambda"][k] - sol["Theta"][k]),
               n2(sol["Omega"][k] - prev["Omega"][k]) + n2(sol["Lambda"][k] - prev["Lambda"][k])]
    crit = orc.ext_stopping_criterion(sol["Omega"], prev["Omega"], sol["Theta"], sol["L"], sol["Lambda"], prev["Lambda"], sol["X0"],
                                      sol["X1"], rho, np.asarray(pk), tol, rtol)
    return sq, np.array(crit)


def _check_iteration(before, sol, prev, pk, P, G, rho, lambda1, lambda2, latent, mu1):
    """ext_ref from the padded state `before` and the oracle's Omega against the oracle's iterate `sol`; returns the padded state"""
    from gglasso_amd import solver
    K = len(pk)
    ref = xr.ext_ref(before, _pad(sol["Omega"], pk, P, True), np.asarray(pk), G, 1, rho, lambda1, [lambda2])
    after = {nm: _pad(sol[nm], pk, P, nm in ("Omega", "Theta", "Lambda")) for nm in ("Omega", "Theta", "L", "X0", "X1", "Lambda")}
    assert np.abs(ref.Theta - after["Theta"]).max() <= TOL
    if latent:
        assert np.abs(orc.rank_stack(ref.C(after["Theta"]), mu1 / rho) - after["L"]).max() <= TOL
    lm = ref.lam(after["Theta"])
    assert np.abs(lm["Lambda"] - after["Lambda"]).max() <= TOL
    assert np.abs(ref.X0n(after["Theta"], after["L"]) - after["X0"]).max() <= TOL
    assert np.abs(ref.X1n(after["Theta"], after["Lambda"]) - after["X1"]).max() <= TOL
    got, n_terms = ref.sums(after["Theta"], after["L"], after["Lambda"], after["X0"], after["X1"])
    want, crit = _sums_of(sol, prev, pk, rho, 1e-3, 1e-2)
    got = np.asarray(got[0], dtype=np.float64)
    assert got.shape == (5,) and np.abs(got - want).max() <= TOL * max(1.0, want.max())
    dim = ((np.asarray(pk) ** 2 + np.asarray(pk)) / 2).sum()
    assert np.allclose(solver.residuals_from_norms(got, rho, 1e-3, 1e-2, dim), crit, rtol=1e-12, atol=0)
    assert n_terms[0] == 2 * sum(int(q) ** 2 for q in pk)
    assert np.all(got[[0, 1, 3]] > 0)
    return after


def _two_iterations(c, b, g):
    """problem g of a built case: the oracle's iterations 1 and 2 against the helper"""
    pk, P, Kp = c.pk, c.P, c.Kp
    sl = slice(g * Kp, (g + 1) * Kp)
    S = xr.unpad(b["S"][sl], pk)
    st = b["state"]
    Om0, X0, X1 = (xr.unpad(st[nm][sl], pk) for nm in ("Theta", "X0", "X1"))
    lam1, lam2 = b["lambda1"][sl], float(b["lambda2"][g])
    mu1 = None if b["mu1"] is None else b["mu1"][sl]
    kw = dict(X0=X0, X1=X1, rho=b["rho"], tol=1e-20, rtol=1e-20, latent=c.latent, mu1=mu1)
    G_orc, lam2_orc = b["G"], lam2
    if c.L == 0:
        # the reference refuses an empty G: one group under a vanishing threshold is the identity map to rounding
        G_orc, lam2_orc = -np.ones((2, 1, Kp), dtype=int), 1e-300
        G_orc[:, 0, 0] = (0, 1)
    sol1, _ = orc.ext_ADMM_MGL(S, lam1, lam2_orc, "GGL", Om0, G_orc, max_iter=1, **kw)
    sol2, _ = orc.ext_ADMM_MGL(S, lam1, lam2_orc, "GGL", Om0, G_orc, max_iter=2, **kw)
    zero = {k: np.zeros((q, q)) for k, q in enumerate(pk)}
    start = dict(Omega=Om0, Theta=Om0, Lambda=Om0, L=zero, X0=X0, X1=X1)
    before = {nm: _pad(start[nm], pk, P, nm in ("Omega", "Theta", "Lambda")) for nm in start}
    args = (pk, P, b["G"], b["rho"], lam1, lam2, c.latent, mu1)
    after1 = _check_iteration(before, sol1, start, *args)
    _check_iteration(after1, sol2, sol1, *args)


@pytest.mark.parametrize("case", xr.SINGLE, ids=[c.name for c in xr.SINGLE])
def test_two_iterations_of_the_oracle(case):
    _two_iterations(case, xr.build_case(case), 0)


@pytest.mark.parametrize("case", xr.BATCH, ids=[c.name for c in xr.BATCH])
def test_two_iterations_of_the_oracle_per_problem_of_a_batch(case):
    b = xr.build_case(case)
    for g in range(case.nprob):
        _two_iterations(case, b, g)
    # ... and the batch reference is the single-problem reference per problem: slot and problem parameters are not mixed up
    ref = xr.ref_of(case, b, b["Omega_cpu"])
    lm = ref.lam(ref.Theta)
    X0n, X1n = ref.X0n(ref.Theta, b["state"]["L"]), ref.X1n(ref.Theta, lm["Lambda"])
    sq, n_terms = ref.sums(ref.Theta, b["state"]["L"], lm["Lambda"], X0n, X1n)
    assert sq.shape == (case.nprob, 5) and n_terms.shape == (case.nprob,)
    Kp = case.Kp
    for g in range(case.nprob):
        sl = slice(g * Kp, (g + 1) * Kp)
        one = xr.ext_ref({nm: A[sl] for nm, A in b["state"].items()}, b["Omega_cpu"][sl], b["pk_all"][sl], b["G"], 1, b["rho"],
                         b["lambda1"][sl], b["lambda2"][g:g + 1])
        l1 = one.lam(one.Theta)
        assert np.array_equal(one.Theta, ref.Theta[sl]) and np.array_equal(l1["Lambda"], lm["Lambda"][sl])
        s1, n1 = one.sums(one.Theta, b["state"]["L"][sl], l1["Lambda"], X0n[sl], X1n[sl])
        assert np.array_equal(s1[0], sq[g]) and n1[0] == n_terms[g]


@pytest.mark.parametrize("latent", [False, True])
def test_iteration_one_of_the_g14_trajectories(latent):
    import ext_checks
    from gglasso_amd import solver
    g = load_golden("g14_ext_admm_nonconforming")
    K, p, S, G, Om0 = ext_checks.g14_inputs(g)
    l1, l2, mu1 = (float(v) for v in g["params"])
    tag = ("lat" if latent else "nol") + "_it1"
    P = int(p.max())
    zero = {k: np.zeros((p[k], p[k])) for k in range(K)}
    start = dict(Omega=Om0, Theta=Om0, Lambda=Om0, L=zero, X0=zero, X1=zero)
    before = {nm: _pad(start[nm], p, P, nm in ("Omega", "Theta", "Lambda")) for nm in start}
    fix = {nm: _pad({k: g[f"{tag}_{nm}_{k}"] for k in range(K)}, p, P, nm in ("Omega", "Theta")) for nm in ext_checks.NAMES}
    ref = xr.ext_ref(before, fix["Omega"], p, G, 1, 1.0, np.full(K, l1), [l2])
    assert np.abs(ref.Theta - fix["Theta"]).max() <= TOL
    if latent:
        assert np.abs(orc.rank_stack(ref.C(fix["Theta"]), np.full(K, mu1)) - fix["L"]).max() <= TOL
    else:
        assert not fix["L"].any()
    Lam = ref.lam(fix["Theta"])["Lambda"]
    assert np.abs(ref.X0n(fix["Theta"], fix["L"]) - fix["X0"]).max() <= TOL
    assert np.abs(ref.X1n(fix["Theta"], Lam) - fix["X1"]).max() <= TOL
    sq, _ = ref.sums(fix["Theta"], fix["L"], Lam, fix["X0"], fix["X1"])
    r_t, s_t, _, _ = solver.residuals_from_norms([float(v) for v in sq[0]], 1.0, 1e-20, 1e-20, 1.0)
    assert abs(max(r_t, s_t) - float(g[f"{tag}_residual"][0])) <= TOL * max(1.0, float(g[f"{tag}_residual"][0]))


@pytest.mark.parametrize("case", xr.CASES, ids=IDS)
def test_case_inputs(case):
    b = xr.build_case(case)
    st = b["state"]
    cross, trailing = xr.padding_masks(b["pk_all"], case.P)
    eye = np.broadcast_to(np.eye(case.P), st["Omega"].shape)
    for nm, A in list(st.items()) + [("S", b["S"])]:
        assert np.array_equal(A, A.transpose(0, 2, 1)), nm
        assert not A[cross].any(), nm
        assert np.array_equal(A[trailing], eye[trailing] if nm in ("S", "Omega", "Theta", "Lambda") else 0 * eye[trailing]), nm
    assert trailing.any() == case.padded
    if case.latent:
        ev = np.linalg.eigvalsh(st["L"])
        assert ev.min() >= -1e-14 * ev.max() and np.linalg.matrix_rank(st["L"][0]) == 2
    else:
        assert not st["L"].any()
    G = b["G"]
    assert G.shape == (2, case.L, case.Kp)
    if case.L:
        orc.check_G(G, np.asarray(case.pk))
        assert orc._G_entries_distinct(G, np.asarray(case.pk))
        sizes = (G[0] >= 0).sum(axis=1)
        if case.L >= 10:
            # sizes 1 .. K, as far as the instances hold pairs to give (a 1 x 1 block holds none, a 2 x 2 block one)
            assert set(sizes) >= set(range(1, sum(q >= 3 for q in case.pk) + 1)) and sizes.max() <= case.Kp
    assert np.all(b["lambda1"] > 0) and np.all(b["lambda2"] > 0)
    if case.nprob > 1:
        # its own state, lambda1 per slot and lambda2 per problem
        Kp = case.Kp
        assert len(set(b["lambda2"])) == case.nprob and len(set(b["lambda1"])) == case.K
        assert not np.array_equal(st["Lambda"][:Kp], st["Lambda"][Kp:2 * Kp])
    ref = xr.ref_of(case, b, b["Omega_cpu"])
    lm = xr.check_inputs(case, b, ref)
    X0n, X1n = ref.X0n(ref.Theta, st["L"]), ref.X1n(ref.Theta, lm["Lambda"])
    sq, _ = ref.sums(ref.Theta, st["L"], lm["Lambda"], X0n, X1n)
    assert sq.shape == (case.nprob, 5) and np.all(sq[:, (0, 1, 3)] > 0)
    if case.L == 0:
        assert np.array_equal(lm["Lambda"], np.asarray(lm["Z"], dtype=np.float64))
    # the reference's padding is the fixed point
    for A, fill in ((ref.Theta, 1.0), (lm["Lambda"], 1.0), (X0n, 0.0), (X1n, 0.0)):
        assert not A[cross].any() and np.abs(np.where(trailing, A - fill * eye, 0.0)).max() <= 1e-12


def test_the_structure_the_case_table_claims():
    by = {c.name: c for c in xr.CASES}
    assert len(by) == len(xr.CASES)
    chunks = {c.name: xr.nblk(c.P) for c in xr.CASES}
    for lat in ("", "-latent"):
        assert chunks["P8-jacobi" + lat] == 1 and chunks["P32-one-full-chunk" + lat] == 1
        assert chunks["P33-two-chunks" + lat] == 2 and chunks["P46-three-chunks-L600" + lat] == 3
        assert (chunks["batch3x2-P20" + lat], chunks["batch2x3-P33" + lat], chunks["batch3x2-P46" + lat]) == (1, 2, 3)
    assert 32 * 32 == xr.XCHUNK and 33 * 33 - xr.XCHUNK == 65 and 2 * xr.XCHUNK < 46 * 46 <= 3 * xr.XCHUNK
    # the last chunk of the last instance of every problem of a batch holds elements of its leading block (a reduction that dropped
    # the last row of a problem's partial sums would drop something)
    for c in xr.BATCH:
        first = (xr.nblk(c.P) - 1) * xr.XCHUNK
        assert first // c.P < c.pk[-1]
    wgs = {c.name: -(-c.L // xr.GROUP_WG) for c in xr.CASES}
    assert {n for n, w in wgs.items() if w == 0} == {"P46-L0"}
    assert wgs["P46-L1"] == 1 and wgs["P46-L256"] == 1 and wgs["P46-L257"] == 2 and wgs["P46-three-chunks-L600"] == 3
    assert all(wgs[c.name] == 2 for c in xr.BATCH)
    assert by["P8-jacobi"].P <= 8 < by["K1-groups-of-one"].P            # GGL_NS_MIN_P = 8: the only case on the Jacobi Omega route
    assert min(c.P for c in xr.CASES) == 8 and xr.SPEC_CASE.P > 64       # above the LDS-resident chain (p <= 64): the launch chain
    assert by["K1-groups-of-one"].Kp == 1 and 1 in by["P8-jacobi"].pk
    assert {c.latent for c in xr.CASES} == {False, True}
