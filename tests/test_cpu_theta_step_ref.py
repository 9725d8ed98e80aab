"""tests/theta_step_ref.py pinned without a GPU: fed the oracle's own Omega, the helper reproduces one iteration of
oracle.ADMM_MGL (GGL and FGL, latent and not), of oracle.ADMM_SGL, and iteration 1 of the Functional SGL trajectories A and F of
the G20 fixtures (written by the reference solver) -- to rounding, <= 1e-13 absolute on these O(1) problems.  The cases of
tests/test_gpu_theta_routes.py are built here as well, with the oracle's Omega: between 10 % and 90 % of the off-diagonal
entries survive, and no element lies within 1e-10 max|V| of its threshold, so the GPU test's zero-pattern check leaves out none."""
import numpy as np
import pytest

import fsgl_fixtures as fx
import theta_step_ref as tsr
from oracle import ggl_oracle as orc

TOL = 1e-13
RHO = 1.7


def _sums_of(sol, Omega_prev):
    L = sol.get("L", 0.0)
    n2 = lambda A: float(np.linalg.norm(A) ** 2)          # noqa: E731  (ADMM_stopping_criterion's own norms)
    return np.array([n2(sol["Omega"]), n2(sol["Theta"] - L), n2(sol["X"]), n2(sol["Omega"] - sol["Theta"] + L),
                     n2(sol["Omega"] - Omega_prev)])


def _check(ref, sol, Omega_prev, latent, groups=1):
    L = sol["L"] if latent else None
    assert np.abs(ref.Theta - sol["Theta"]).max() <= TOL
    assert np.abs(ref.X(sol["Theta"], L) - sol["X"]).max() <= TOL
    got, n_terms = ref.sums(sol["Theta"], sol["X"], L, groups=groups)
    want = _sums_of(sol, Omega_prev)
    assert np.abs(np.asarray(got.sum(axis=0), dtype=np.float64) - want).max() <= TOL * max(1.0, want.max())
    assert int(n_terms.sum()) == sol["Omega"].size


@pytest.mark.parametrize("reg", ["GGL", "FGL"])
@pytest.mark.parametrize("latent", [False, True])
def test_one_iteration_of_admm_mgl(reg, latent):
    from gglasso_amd import synth
    K, p = 5, 13
    S, _ = synth.make_problem(reg, K, p, seed=3)
    Omega_0, Theta_0, X_0, _ = tsr.make_start(K, p, 4)
    mu1 = np.full(K, 0.2)
    sol, _ = orc.ADMM_MGL(S, 0.07, 0.03, reg, Omega_0, Theta_0=Theta_0, X_0=X_0, rho=RHO, max_iter=1, update_rho=False,
                          tol=1e-20, rtol=1e-20, latent=latent, mu1=mu1)
    ref = tsr.step_ref(reg, Omega_0, Theta_0, X_0, None, sol["Omega"], RHO, 0.07, 0.03, latent=latent)
    _check(ref, sol, Omega_0, latent)
    if latent:
        # C is what the L-step eats (admm_solver.py:197-205)
        assert np.abs(orc.rank_stack(ref.C(sol["Theta"]), mu1 / RHO) - sol["L"]).max() <= TOL
        return
    # two problems with their own parameters in one stack: each half is the single problem
    both = tsr.step_ref(reg, np.tile(Omega_0, (2, 1, 1)), None, np.tile(X_0, (2, 1, 1)), None, np.tile(sol["Omega"], (2, 1, 1)),
                        np.array([RHO, RHO]), np.array([0.07, 0.2]), np.array([0.03, 0.03]), G=2)
    assert np.array_equal(both.Theta[:K], ref.Theta) and not np.array_equal(both.Theta[K:], ref.Theta)
    s2, _ = both.sums(both.Theta, both.X(both.Theta), groups=2)
    s1, _ = ref.sums(ref.Theta, ref.X(ref.Theta))
    assert np.array_equal(s2[0], s1[0]) and s2[1, 1] < s1[0, 1]


@pytest.mark.parametrize("latent", [False, True])
@pytest.mark.parametrize("masked", [False, True])
def test_one_iteration_of_admm_sgl(latent, masked):
    from gglasso_amd import synth
    p = 17
    S, _ = synth.make_problem("SGL", 1, p, seed=5)
    Omega_0, Theta_0, X_0, _ = tsr.make_start(1, p, 6)
    mask0 = tsr.sym(np.random.default_rng(7).uniform(0.5, 1.5, (1, p, p)))[0] if masked else None
    sol, _ = orc.ADMM_SGL(S[0], 0.06, Omega_0[0], Theta_0=Theta_0[0], X_0=X_0[0], rho=RHO, max_iter=1, update_rho=False,
                          tol=1e-20, rtol=1e-20, latent=latent, mu1=0.2, lambda1_mask=mask0)
    sol = {k: v[None] for k, v in sol.items()}
    ref = tsr.step_ref("SGL", Omega_0, Theta_0, X_0, None, sol["Omega"], RHO, 0.06, latent=latent,
                       mask=None if mask0 is None else 0.06 * mask0)
    _check(ref, sol, Omega_0, latent)
    # sums over a leading block only
    got, n_terms = ref.sums(sol["Theta"], sol["X"], sol.get("L"), groups=1, pk=[p - 5])
    cut = {k: v[:, :p - 5, :p - 5] for k, v in sol.items()}
    assert np.abs(np.asarray(got[0], dtype=np.float64) - _sums_of(cut, Omega_0[:, :p - 5, :p - 5])).max() <= TOL
    assert n_terms[0] == (p - 5) ** 2


@pytest.mark.parametrize("tag", ["A", "F"])
def test_iteration_one_of_the_fsgl_trajectories(tag):
    from gglasso_amd import solver
    c, traj = fx.case(tag), fx.trajectory(tag)
    pM = c["p"] * c["M"]
    latent = "L" in c["runs"][0]
    eye, zero = np.eye(pM)[None], np.zeros((1, pM, pM))
    sol = {nm: traj[nm][0][None] for nm in traj}
    ref = tsr.step_ref("FSGL", eye, eye, zero, None, sol["Omega"], 1.0, c["lams"][0], M=c["M"], latent=latent)
    L = sol["L"] if latent else None
    assert np.abs(ref.Theta - sol["Theta"]).max() <= TOL
    assert np.array_equal(ref.Theta[0][ref.diag_blocks], ref.V[0][ref.diag_blocks])
    # the reference returns X after its rho rule (functional_sgl_admm.py:173-183), which the helper's sums decide
    sq, _ = ref.sums(sol["Theta"], ref.X(sol["Theta"], L), L)
    r_t, s_t, _, _ = solver.residuals_from_norms([float(v) for v in sq[0]], 1.0, 1e-20, 1e-20, 1.0)
    rho_new = solver.next_rho(1.0, r_t, s_t)
    assert np.abs((1.0 / rho_new) * ref.X(sol["Theta"], L) - sol["X"]).max() <= TOL


def test_the_cases_cover_every_dispatch_code():
    assert {c.code for c in tsr.CASES if c.code is not None} == tsr.ALL_CODES
    assert len({c.name for c in tsr.CASES}) == len(tsr.CASES)
    # the ragged K-chunk case, restated from ggl_chunks (theta_pair.hip): 6 tiles -> 21 pairs -> 49 chunks wanted -> 2 per chunk
    T = -(-161 // 32)
    kc = min(-(-1024 // (T * (T + 1) // 2)), 51)
    klen = -(-51 // kc)
    assert (klen, -(-51 // klen), 51 % klen) == (2, 26, 1)


@pytest.mark.parametrize("case", tsr.CASES, ids=[c.name for c in tsr.CASES])
def test_case_generators(case):
    b = tsr.build_case(case)
    for nm in ("S", "Omega_0", "Theta_0", "X_0", "L_0"):
        if b[nm] is not None:
            assert np.array_equal(b[nm], b[nm].transpose(0, 2, 1)), nm
    ref = tsr.ref_of(case, b, b["Omega_cpu"])
    assert 0.1 <= ref.nonzero_fraction() <= 0.9, ref.nonzero_fraction()
    assert not ref.near.any()
    assert np.all(np.asarray(b["lambda1"]) > 0)
    if case.latent:
        ev = np.linalg.eigvalsh(b["L_0"])
        assert ev.min() >= -1e-14 * ev.max() and np.linalg.matrix_rank(b["L_0"][0]) == 2
