"""The direct family of the Omega-step on the device (GGL_OPT_OMEGA_POLY, csrc/newton_schulz.hip ns_plan / ns_run): one
polynomial in A' evaluated by Paterson-Stockmeyer, its digits in the second affine operand (E2) of the product epilogue.

Every case runs ggl_admm_step with the reference's rho rule (solver/admm_solver.py:227-233) twice -- default, and
omega_poly = 0 (the Newton-Schulz schedule everywhere) -- and checks
  1. that the direct family really ran (ggl_omega_poly_stats), on the route the case names;
  2. the iterates against the Newton-Schulz run (<= 1e-10 at the default ns_tol of 2e-12; <= 100 ns_tol at a looser one);
  3. the last Omega-step against phi^+ of the Newton-Schulz run's W by eigh.
Routes: the headline's two concurrent speculative parts with early parts (fused start G in the B' launch, E2 = W), an odd p
on the direct-to-LDS and on the register-staged kernel, every speculation missed (spec_factor 0.9: the repeated step plans
after the bound, G from k_ns_start) and a grouped batch with the early part on."""
import numpy as np
import pytest

from oracle import ggl_oracle as orc

ITERS = 30
LAM1, LAM2 = 0.05, 0.01


def _problem(K, p, seed, spread=False):
    from gglasso_amd import synth
    S, _ = synth.make_problem("GGL", K, p, N=2 * p, seed=seed)
    return S * np.geomspace(0.2, 2.5, K)[:, None, None] if spread else S


def _run(S, options, iters=ITERS, mid=None):
    """ADMM iterations with the rho rule; returns the final state, the rho sequence, (ns, poly, group, pipeline) stats after
    every call and the state before the last step (if asked)."""
    from gglasso_amd import solver
    K, p = S.shape[0], S.shape[-1]
    eye = np.repeat(np.eye(p)[None], K, axis=0)
    eng = solver.HipEngine(S, eye, eye, np.zeros_like(S), options=options)
    nk = np.ones(K)
    rho, rhos, st_mid = 1.0, [], None
    trail = [(eng.ns_stats(), eng.poly_stats(), eng.group_stats(), eng.pipeline_stats())]
    try:
        for it in range(iters):
            if it == mid:
                st_mid = eng.state()
            if it == iters - 1:
                eng.hint_last_step()
            rhos.append(rho)
            sq = eng.step(rho, LAM1, LAM2, "GGL", False, None, nk).copy()
            trail.append((eng.ns_stats(), eng.poly_stats(), eng.group_stats(), eng.pipeline_stats()))
            r_t, s_t, _, _ = solver.residuals_from_norms(sq, rho, 1e-20, 1e-20, 1.0)
            new = solver.next_rho(rho, r_t, s_t)
            if new != rho and it < iters - 1:
                eng.scale_X(rho / new)
            rho = new
        return eng.state(), rhos, trail, st_mid
    finally:
        eng.close()


def _compare(S, opts):
    """the run with the direct family against the Newton-Schulz run; returns the first run's stats trail.  Both runs meet
    ns_tol: at the default 2e-12 they agree to 1e-10, at a looser ns_tol to 100 ns_tol."""
    lim = max(1e-10, 100.0 * opts.get("ns_tol", 2e-12))
    got, rhos, trail, _ = _run(S, opts)
    ref, rhos_r, trail_r, prev = _run(S, {**opts, "omega_poly": 0.0}, mid=ITERS - 1)
    assert trail_r[-1][1]["seqs"] == 0                                  # omega_poly = 0: never
    assert rhos == rhos_r
    for nm in ("Omega", "Theta", "X"):
        assert np.abs(got[nm] - ref[nm]).max() <= lim, nm
    assert np.array_equal(got["Omega"], got["Omega"].transpose(0, 2, 1))
    W = prev["Theta"] - prev["X"] - S / rhos[-1]
    Om, _ = orc.phiplus_stack(W, 1.0 / rhos[-1])
    assert np.abs(got["Omega"] - Om).max() <= max(1e-9, lim)
    return trail


@pytest.mark.gpu
def test_headline_two_parts_speculative():
    """(32, 500): two concurrent parts, speculative steps with the start G fused into the B' launch.  In the steady state
    most steps run the direct family in at least one part (at this seed the other part's interval is just too wide for
    degree 12), and a part that runs it costs 6 products against the schedule's 7: the steps' units (parts weighted by their
    share) are that mix."""
    trail = _compare(_problem(32, 500, 1239), {})
    ns, poly = trail[-1][0], trail[-1][1]
    assert ns["last_parts"] == 2 and ns["spec_calls"] >= ITERS // 2, ns
    assert poly["seqs"] > 0 and poly["last_deg"] == 12, poly
    # per step: units (A', B' included; parts weighted by their share of the batch) and direct sequences of that step
    steady = [(trail[t][0]["units"] - trail[t - 1][0]["units"], trail[t][1]["seqs"] - trail[t - 1][1]["seqs"],
               trail[t][1]["seqs_total"] - trail[t - 1][1]["seqs_total"]) for t in range(ITERS // 2, ITERS + 1)]
    # (calls whose stats cover a step of both parts; the announced last step runs no early part and may count differently)
    steady = [x for x in steady if x[2] == 2]
    assert len(steady) >= ITERS // 2 - 2 and sum(d >= 1 for u, d, n in steady) >= len(steady) // 2, steady
    # ns_stats rounds the running sum of the weighted units: compare the window's sum, parts of 16 instances each
    want = sum((6 * d + 7 * (n - d)) / n for u, d, n in steady)
    assert abs(sum(u for u, d, n in steady) - want) <= 1.0, (steady, want)


@pytest.mark.gpu
@pytest.mark.parametrize("odd_dl", [1, 0])
def test_odd_p(odd_dl):
    """odd p = 301: the direct-to-LDS kernel's odd last column, and (odd_dl = 0) the register-staged kernel with E2.  At this
    shape the spectrum is wider than the headline's; ns_tol = 1e-9 makes the direct family (degree 9 / 12 against the
    schedule's 6-8 products) the cheaper one."""
    from gglasso_amd import _lib
    lib = _lib.load()
    was = lib.ggl_set_odd_dl(odd_dl)
    try:
        trail = _compare(_problem(8, 301, 77), {"ns_tol": 1e-9})
    finally:
        lib.ggl_set_odd_dl(was)
    assert trail[-1][1]["seqs"] > 0, trail[-1][1]
    assert trail[-1][0]["last_variant"] == (20 if odd_dl else 9), trail[-1][0]


@pytest.mark.gpu
def test_speculation_missed():
    """spec_factor 0.9: every speculative step is rejected and repeated after its bound (G from k_ns_start)"""
    trail = _compare(_problem(16, 400, 2416), {"spec_factor": 0.9})
    ns, poly = trail[-1][0], trail[-1][1]
    assert ns["spec_misses"] >= 3, ns
    assert poly["seqs"] > 0, poly


@pytest.mark.gpu
def test_grouped_with_early_part():
    """heterogeneous instances cut into groups with their own plans (group_sched 13), early first parts resumed"""
    trail = _compare(_problem(16, 400, 2416, spread=True), {"group_sched": 13.0, "early_part": 1.0})
    ns, poly, gs, ps = trail[-1]
    assert gs["steps"] > 0 and ps["early_used"] > 0, (gs, ps)
    assert poly["seqs"] > 0, poly

