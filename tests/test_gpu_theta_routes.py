"""Every kernel route of the Theta-step (launch_theta_pair, launch_theta_batch, k_theta_sgl and its twin fused into the
LDS-resident iteration, k_theta_fsgl), named, proven taken by its dispatch code, and checked at STEP level: one iteration from a
non-trivial symmetric start, then Theta, the dual update and the five stopping-test sums against tests/theta_step_ref.py, which
forms every quantity from the device's own upstream outputs (its Omega for Theta, its Theta and L for X and the sums).

Bounds (derived, u = 2^-53; tests/theta_step_ref.py):
  Theta   max|dev - ref| <= 8 n u max(1, max|V|), n the reduction length behind one output (1 SGL, K GGL / FGL, M^2 FSGL)
  X       <= 4 u max(|X_0| + |Omega| + |Theta| + |L|)
  sums    relative deviation from the numpy.longdouble value <= (N + 4) u, N the number of terms
  Theta bitwise symmetric, its zero pattern the reference's (elements within 1e-10 max|V| of a threshold left out, at most
  1e-4 of them), FSGL diagonal blocks equal to V's bit for bit, and a second run from the same start gives the same bits.
The cases (shapes, seeds, thresholds) are tests/theta_step_ref.py CASES; tests/test_cpu_theta_step_ref.py builds them too."""
import numpy as np
import pytest

import theta_step_ref as tsr
from oracle import ggl_oracle as orc

pytestmark = pytest.mark.gpu

_SEEN = {}          # case name -> dispatch code asserted
_WORST = {}         # case name -> {quantity: (deviation, bound)}


def _run(case, b):
    """One iteration of the case on a fresh engine: (state, sums (rows,5), dispatch code, fsgl_stats, lds_stats)."""
    from gglasso_amd import solver
    K = case.K
    eng = solver.HipEngine(b["S"], b["Omega_0"], b["Theta_0"], b["X_0"], b["L_0"], options=case.opts)
    try:
        if b["mask"] is not None:
            (eng.set_lambda1_mask_k if b["mask"].ndim == 3 else eng.set_lambda1_mask)(b["mask"])
        if b["pk"] is not None:
            eng.set_instance_dims(b["pk"])
        if case.M:
            eng.set_block_size(case.M)
        if case.kind == "step":
            eng.hint_last_step()
            sq = eng.step(float(b["rho"]), float(b["lambda1"]), float(b["lambda2"] or 0.0), case.reg, case.latent, b["mu1"],
                          np.ones(K)).copy().reshape(1, 5)
        elif case.kind == "mgl_batch":
            sq = eng.mgl_batch_step(case.G, b["rho"], b["lambda1"], b["lambda2"], case.reg, case.latent, b["mu1"], None)
        else:
            sq = eng.sgl_batch_step(b["rho"], b["lambda1"], case.latent, b["mu1"])
        st = eng.state()
        return st, np.array(sq), eng.last_dispatch()["theta_kernel"], eng.fsgl_stats(), eng.lds_stats()
    finally:
        eng.close()


def _note(case, what, dev, bound):
    _WORST.setdefault(case.name, {})[what] = (float(dev), float(bound))
    print(f"{case.name:28s} {what:10s} deviation {float(dev):.3e}  bound {float(bound):.3e}")


@pytest.mark.parametrize("case", tsr.CASES, ids=[c.name for c in tsr.CASES])
def test_theta_route(case):
    from gglasso_amd import _lib
    if case.name == "fgl-Kmax-p6":
        assert _lib.theta_limits()["FGL"] == case.K == tsr.FGL_MAX_K
    b = tsr.build_case(case)
    st, sq, code, fs, lds = _run(case, b)
    K, p, latent = case.K, case.p, case.latent
    Om, Th, X = st["Omega"], st["Theta"], st["X"]
    L = st["L"] if latent else None

    # ---- the route ----
    if case.code is not None:
        assert code == case.code, (case.name, code, case.code)
        _SEEN[case.name] = code
    if case.reg == "FSGL":
        want = {"M": case.M, "pair_steps": int(case.M <= 32), "table_steps": int(case.M > 32), "fused_sgl_steps": 0}
        assert fs == want, (fs, want)
    elif case.kind == "sgl_batch":
        assert fs["fused_sgl_steps"] == int(case.fused), (case.name, fs, lds)
        assert (lds["calls"] >= 1) == case.fused, (case.name, lds)

    # ---- the state made it to the device and back: Omega against eigh (the Omega-step's own tests bound it tighter) ----
    assert np.abs(Om - b["Omega_cpu"]).max() <= 1e-9
    assert np.array_equal(Om, Om.transpose(0, 2, 1))

    # ---- Theta ----
    ref = tsr.ref_of(case, b, Om)
    assert 0.1 <= ref.nonzero_fraction() <= 0.9, ref.nonzero_fraction()
    d = np.abs(Th - ref.Theta).max()
    _note(case, "Theta", d, ref.theta_bound())
    assert d <= ref.theta_bound()
    assert np.array_equal(Th, Th.transpose(0, 2, 1))
    share = ref.near.mean()
    assert share <= 1e-4, share
    assert np.array_equal((Th == 0)[~ref.near], (ref.Theta == 0)[~ref.near])
    if case.reg == "FSGL":
        assert np.array_equal(Th[:, ref.diag_blocks], ref.V[:, ref.diag_blocks])

    # ---- L (latent): the Theta kernel's C = (Theta - X_0) - Omega is seen through the L-step, an iteration of its own
    # tolerance -- the parity bound of the suite, 1e-9, applies; X below is then formed with the device's own L ----
    if latent:
        rho_K = np.repeat(np.atleast_1d(b["rho"]), K // np.atleast_1d(b["rho"]).size)
        dL = np.abs(L - orc.rank_stack(ref.C(Th), b["mu1"] / rho_K)).max()
        _note(case, "L", dL, 1e-9)
        assert dL <= 1e-9

    # ---- X ----
    dX = np.abs(X - ref.X(Th, L)).max()
    _note(case, "X", dX, ref.x_bound(Th, L))
    assert dX <= ref.x_bound(Th, L)

    # ---- the five sums, as the entry point returns them ----
    groups = {"step": 1, "mgl_batch": case.G, "sgl_batch": K}[case.kind]
    want, n_terms = ref.sums(Th, X, L, groups=groups, pk=b["pk"])
    assert sq.shape == want.shape
    # (a sum that is exactly zero -- |X|^2 over a 1 x 1 leading block: the diagonal of Theta is V's -- must come back as zero)
    rel = np.abs(sq.astype(np.longdouble) - want) / np.where(want > 0, want, np.finfo(np.float64).tiny)
    bound = ref.sums_bound(n_terms)
    for v, nm in enumerate(("|Om|^2", "|Th-L|^2", "|X|^2", "|r|^2", "|dOm|^2")):
        row = int(np.argmax(rel[:, v] / bound[:, 0]))             # the row closest to its own bound
        _note(case, nm, rel[row, v], bound[row, 0])
    assert np.all(want[:, (0, 1, 3)] > 0)
    assert np.all(rel <= bound), (rel, bound)

    # ---- the same case again from the same start: the same bits ----
    st2, sq2, code2, _, _ = _run(case, b)
    assert code2 == code
    for nm in ("Omega", "Theta", "X") + (("L",) if latent else ()):
        assert np.array_equal(st[nm], st2[nm]), nm
    assert np.array_equal(sq, sq2)


def test_every_dispatch_code_was_asserted():
    """Ends the module: the codes asserted above cover every code the Theta-step launchers can report.  (The case table
    covers them by construction; when only part of the cases was selected, that is all that can be said.)"""
    assert {c.code for c in tsr.CASES if c.code is not None} == tsr.ALL_CODES
    if len(_SEEN) == sum(c.code is not None for c in tsr.CASES):
        assert set(_SEEN.values()) == tsr.ALL_CODES, tsr.ALL_CODES - set(_SEEN.values())
    for name, w in _WORST.items():
        print(name, {k: f"{d:.2e}/{bd:.2e}" for k, (d, bd) in w.items()})
