"""Parity at the REAL dispatch of every BASELINE.json configuration: the kernels, tile shapes,
concurrent-part split and speculation that run at the full sizes are the ones checked here, against the CPU oracle
on the same seeded inputs (a few iterations -- the oracle's eigh dominates the cost) and through size-independent
properties (exact symmetry, positive definiteness, norm identities) for what the oracle does not re-compute.

  headline  GGL K=32, p=500            two concurrent parts, direct-to-LDS 64x64 kernel with 3 DMA stages (variant 17),
                                       speculative Omega-step, per-element Theta kernel <32>
  C3        GGL K=20, p=200            single launch sequence, 32x32 direct-to-LDS product kernel (variant 20)
  C4        FGL K=50, p=500, latent    TD=8 Condat tile, two-part sign iteration of the L-step
  C2        SGL p=1000, 20-point grid  batched lambda path, 64x64 DMA kernel over several rounds of tiles
  C5 slab   GGL K=32, p=1000           per-GPU slab of C5 at 8 GPUs: unsplit launch sequence above 2048 tile pairs
  C5 whole  GGL K=256, p=1000          the whole stack on one GPU: Theta kernel with the K-column over 16 waves of 16
The headline and C4 are additionally solved to convergence on both sides (the oracle's solve is observed along the way, so
the fixed-length comparison and the converged one cost its iterations once).
Reference loop bodies: solver/admm_solver.py:172-246, solver/single_admm_solver.py:157-214.
"""
import contextlib
import io

import numpy as np
import pytest

from oracle import ggl_oracle as orc

pytestmark = pytest.mark.gpu


def quiet(fn, *a, **k):
    with contextlib.redirect_stdout(io.StringIO()):
        return fn(*a, **k)


@contextlib.contextmanager
def oracle_threads(n=16):
    """LAPACK's eigh on p <= 1000 gets slower beyond a few threads (the GPU box has 128 cores)."""
    try:
        from threadpoolctl import threadpool_limits
    except Exception:  # noqa: BLE001
        yield
        return
    with threadpool_limits(limits=n):
        yield


@pytest.fixture()
def stats(monkeypatch):
    """ns_stats of every engine a solver call creates, captured when it is closed."""
    from gglasso_amd import solver
    seen = []
    real_close = solver.HipEngine.close

    def closing(self):
        if getattr(self, "h", None):
            seen.append({**self.ns_stats(), **{"rank_" + k: v for k, v in self.rank_stats().items()},
                         **{"dispatch_" + k: v for k, v in self.last_dispatch().items()},
                         **{"pipe_" + k: v for k, v in self.pipeline_stats().items()}})
        real_close(self)

    monkeypatch.setattr(solver.HipEngine, "close", closing)
    return seen


def _problem(reg, K, p, seed):
    from gglasso_amd import synth
    S, _ = synth.make_problem(reg, K, p, N=2 * p, seed=seed)
    return S, np.repeat(np.eye(p)[None], K, axis=0)


def _oracle_run(S, reg, l1, l2, Om0, checkpoints, tol, latent=False, mu1=None, max_iter=1000):
    """The oracle's ADMM_MGL (oracle/ggl_oracle.py through the test-only engine and the product's own host loop) observed
    along ONE solve: the state after each of ``checkpoints`` iterations (tol = rtol = 1e-20 up to there, which is what a
    fixed-length run does) and then the solve continued to tol = rtol = ``tol``.  Returns ([states], converged state,
    status, total iterations).  The oracle's eigh is the expensive side of these tests; this way a converged full-size solve
    costs its own iterations once.
    NOTE what this pins: the ARITHMETIC of every iteration is the oracle's (NumPy eigh + the C prox twins), the LOOP CONTROL
    around it (rho rule, stopping rule, status strings) is the product's own ``solver._run_admm`` -- so status / iteration
    count agreement here is product loop against product loop on different arithmetic.  The loop control itself is pinned
    against the real reference by fixtures G8 / G9 (tests/test_oracle_golden.py, tests/test_gpu_admm.py) and, where a test
    calls ``orc.ADMM_MGL`` / ``orc.ADMM_SGL`` directly (the third leg of the headline test, C2 converged, the odd-p and
    slab tests), by the oracle's own restatement of admm_solver.py:172-281."""
    from gglasso_amd import solver
    from oracle_engine import OracleEngine
    K, p, _ = S.shape
    eng = OracleEngine(S, Om0, Om0, np.zeros_like(S))
    nk = np.ones(K)
    rho, done, states = 1.0, 0, []
    with oracle_threads():
        for it in checkpoints:
            _, rho = quiet(solver._run_admm, eng, reg, K, p, l1, l2, latent, mu1, nk, rho, 1e-20, 1e-20, 'boyd', True, it - done,
                           False, False, "Multiple")
            done = it
            states.append({k: v.copy() for k, v in eng.state().items()})
        info, rho = quiet(solver._run_admm, eng, reg, K, p, l1, l2, latent, mu1, nk, rho, tol, tol, 'boyd', True,
                          max_iter - done, False, True, "Multiple")
    return states, eng.state(), info['status'], done + len(info['residual'])


def _check_state(out, ref, names, tol):
    for nm in names:
        err = float(np.abs(out[nm] - ref[nm]).max())
        assert err <= tol * max(1.0, float(np.abs(ref[nm]).max())), (nm, err)


def test_headline_dispatch_ggl_K32_p500(stats):
    """bench.py's workload along one oracle solve: 6 iterations with the rho rule from the identity start against the oracle at
    1e-9, the CONVERGED solve (tol = rtol = 1e-10, default Omega-step tolerance) at |Theta - oracle|_F <= 1e-8 with the oracle's
    status and iteration count (north_star: Theta within 1e-8 Frobenius), then 3 iterations at fixed rho
    (every iteration after the first speculative)."""
    from gglasso_amd import solver
    S, Om0 = _problem("GGL", 32, 500, 1239)
    (ref6,), ref, ref_status, ref_iters = _oracle_run(S, "GGL", 0.05, 0.01, Om0, [6], 1e-10)
    out, info = quiet(solver.ADMM_MGL, S, 0.05, 0.01, "GGL", Om0, max_iter=6, tol=1e-20, rtol=1e-20)
    _check_state(out, ref6, ("Omega", "Theta", "X"), 1e-9)
    assert np.array_equal(out["Theta"], out["Theta"].transpose(0, 2, 1))
    assert np.array_equal(out["Omega"], out["Omega"].transpose(0, 2, 1))
    st = stats[-1]
    assert st["last_parts"] == 2 and st["last_variant"] == 17, st          # fork/join two-part chains on variant 17
    assert st["stable_calls"] == 0 and st["eigh_fallbacks"] == 0, st
    assert st["dispatch_theta_kernel"] == 408, st                          # per-element kernel, K-column over four waves
    out, info = quiet(solver.ADMM_MGL, S, 0.05, 0.01, "GGL", Om0, tol=1e-10, rtol=1e-10, measure=True)
    assert info["status"] == ref_status == "optimal"
    assert len(info["residual"]) == ref_iters, (len(info["residual"]), ref_iters)
    assert np.linalg.norm(out["Theta"] - ref["Theta"]) <= 1e-8
    assert np.abs(out["Theta"] - ref["Theta"]).max() <= 1e-10
    kw = dict(max_iter=3, tol=1e-20, rtol=1e-20, update_rho=False, rho=2.0)
    with oracle_threads():
        ref, _ = orc.ADMM_MGL(S, 0.05, 0.01, "GGL", Om0, **kw)
    out, info = quiet(solver.ADMM_MGL, S, 0.05, 0.01, "GGL", Om0, **kw)
    _check_state(out, ref, ("Omega", "Theta", "X"), 1e-9)
    st = stats[-1]
    assert st["spec_calls"] >= 1, st            # fixed rho: the iterations after the first run speculatively
    assert st["last_parts"] == 2 and st["last_variant"] == 17, st


def test_headline_dispatch_exact_omega_step(stats, monkeypatch):
    """The headline at its real dispatch with the Omega-step iterated to fp64 resolution (GGL_OPT_NS_TOL = 0): the
    two-part chains then run the 8-product schedule (two degree-nine steps) and the iterates agree with the oracle's
    eigendecomposition to 2e-12."""
    from gglasso_amd import solver
    monkeypatch.setitem(solver.ENGINE_OPTIONS, "ns_tol", 0.0)
    S, Om0 = _problem("GGL", 32, 500, 1239)
    kw = dict(max_iter=4, tol=1e-20, rtol=1e-20, update_rho=False, rho=2.0)
    with oracle_threads():
        ref, _ = orc.ADMM_MGL(S, 0.05, 0.01, "GGL", Om0, **kw)
    out, info = quiet(solver.ADMM_MGL, S, 0.05, 0.01, "GGL", Om0, **kw)
    _check_state(out, ref, ("Omega", "Theta", "X"), 2e-12)
    st = stats[-1]
    assert st["last_parts"] == 2 and st["last_variant"] == 17, st
    assert st["spec_calls"] >= 1 and st["stable_calls"] == 0, st
    # every Omega-step (incl. a pre-launched chain that was dropped) ran 8 symmetric products of the stack
    assert st["units"] == 8 * st["calls"], st


def test_c3_dispatch_ggl_K20_p200(stats):
    """C3 at its real dispatch along one oracle solve: 12 iterations with the rho rule against the oracle at 1e-9, then the
    CONVERGED solve (tol = rtol = 1e-9): the oracle's status and iteration count, |Theta - oracle|_F <= 1e-8 (VERDICT r5 item 5;
    north_star: Theta within 1e-8 Frobenius)."""
    from gglasso_amd import solver
    S, Om0 = _problem("GGL", 20, 200, 1236)
    (ref12,), ref, ref_status, ref_iters = _oracle_run(S, "GGL", 0.05, 0.01, Om0, [12], 1e-9)
    out, _ = quiet(solver.ADMM_MGL, S, 0.05, 0.01, "GGL", Om0, max_iter=12, tol=1e-20, rtol=1e-20)
    _check_state(out, ref12, ("Omega", "Theta", "X"), 1e-9)
    st = stats[-1]
    assert st["last_parts"] == 1 and st["last_variant"] == 20, st
    assert st["spec_calls"] >= 1, st
    out, info = quiet(solver.ADMM_MGL, S, 0.05, 0.01, "GGL", Om0, tol=1e-9, rtol=1e-9, measure=True)
    assert info["status"] == ref_status == "optimal"
    assert len(info["residual"]) == ref_iters, (len(info["residual"]), ref_iters)
    assert np.linalg.norm(out["Theta"] - ref["Theta"]) <= 1e-8
    assert np.array_equal(out["Theta"], out["Theta"].transpose(0, 2, 1))


@pytest.mark.parametrize("reg,K,p,latent,parts,variant", [("GGL", 32, 501, False, 2, 17), ("GGL", 20, 201, False, 1, 20),
                                                          ("FGL", 5, 333, True, 1, 20), ("GGL", 3, 999, False, 1, 20)])
def test_odd_p_runs_on_the_dma_product_kernel(stats, reg, K, p, latent, parts, variant):
    """Odd p (the reference is indifferent to the parity of p, solver/admm_solver.py:180-187): the same
    direct-to-LDS product kernel, split and speculation as the even neighbour -- rounds 1-5 sent every odd p to the
    register-staged kernel (25-37 % slower per product).  Eight iterations with the rho rule against the oracle at 1e-9, exact
    symmetry, and -- process-wide switch ggl_set_odd_dl(0) -- within 1e-10 of the register-staged route's iterates."""
    from gglasso_amd import solver, _lib
    S, Om0 = _problem(reg, K, p, 1300 + p)
    mu1 = 0.5 * np.ones(K) if latent else None
    kw = dict(max_iter=8, tol=1e-20, rtol=1e-20, latent=latent, mu1=mu1)
    with oracle_threads():
        ref, _ = quiet(orc.ADMM_MGL, S, 0.05, 0.01, reg, Om0, **kw)
    names = ("Omega", "Theta", "X") + (("L",) if latent else ())
    out, _ = quiet(solver.ADMM_MGL, S, 0.05, 0.01, reg, Om0, **kw)
    _check_state(out, ref, names, 1e-9)
    for nm in ("Omega", "Theta"):
        assert np.array_equal(out[nm], out[nm].transpose(0, 2, 1)), nm
    st = stats[-1]
    assert st["last_parts"] == parts and st["last_variant"] == variant, st
    assert st["stable_calls"] == 0 and st["eigh_fallbacks"] == 0, st
    if not latent:
        assert st["spec_calls"] >= 1, st
    lib = _lib.load()
    try:
        lib.ggl_set_odd_dl(0)
        old, _ = quiet(solver.ADMM_MGL, S, 0.05, 0.01, reg, Om0, **kw)
    finally:
        lib.ggl_set_odd_dl(1)
    assert stats[-1]["last_variant"] in (0, 9), stats[-1]
    for nm in names:
        assert np.abs(out[nm] - old[nm]).max() <= 1e-10 * max(1.0, np.abs(old[nm]).max()), nm


def test_c4_dispatch_fgl_K50_p500_latent(stats):
    """FGL with latent variables at full size along one oracle solve: 8 iterations from the identity start
    against the oracle at 1e-9 -- iterations 3, 4 and 6 have an instance whose eigenvalue sits within 1e-5 |C| of the threshold
    (profiles/r3_c4_lstep_threshold_gaps.txt), so the two-tier L-step's CONTINUATION (compact sub-batch, rank_ns_plan_continue,
    trace check) must have run -- and the converged solve (tol = rtol = 1e-9): the oracle's status and iteration count,
    |Theta - oracle|_F <= 1e-8, and numpy.linalg.matrix_rank of every returned L_k (rebuilt by ggl_finalize_L) equal to the
    oracle's.  TD=8 Condat tiles (K > 32), sign iteration in two concurrent parts."""
    from gglasso_amd import solver
    K = 50
    S, Om0 = _problem("FGL", K, 500, 1237)
    mu1 = 0.5 * np.ones(K)
    (ref8,), ref, ref_status, ref_iters = _oracle_run(S, "FGL", 0.05, 0.01, Om0, [8], 1e-9, latent=True, mu1=mu1)
    out, _ = quiet(solver.ADMM_MGL, S, 0.05, 0.01, "FGL", Om0, max_iter=8, tol=1e-20, rtol=1e-20, latent=True, mu1=mu1)
    _check_state(out, ref8, ("Omega", "Theta", "L", "X"), 1e-9)
    for nm in ("Omega", "Theta", "L"):
        assert np.array_equal(out[nm], out[nm].transpose(0, 2, 1)), nm
    st = stats[-1]
    assert st["rank_calls"] == 8 and st["last_parts"] == 2 and st["last_variant"] == 17, st
    assert st["rank_continued_calls"] >= 1 and st["rank_continued_instances"] >= 1, st
    assert st["rank_eigh_fallbacks"] == 0, st
    assert st["dispatch_theta_kernel"] == 3128 and st["dispatch_finalize_calls"] == 1, st      # FGL per element, 128 per workgroup
    out, info = quiet(solver.ADMM_MGL, S, 0.05, 0.01, "FGL", Om0, tol=1e-9, rtol=1e-9, latent=True, mu1=mu1, measure=True)
    assert info["status"] == ref_status == "optimal"
    assert len(info["residual"]) == ref_iters, (len(info["residual"]), ref_iters)
    assert np.linalg.norm(out["Theta"] - ref["Theta"]) <= 1e-8
    assert np.abs(out["L"] - ref["L"]).max() <= 1e-9
    with oracle_threads():
        assert [np.linalg.matrix_rank(out["L"][k]) for k in range(K)] == [np.linalg.matrix_rank(ref["L"][k]) for k in range(K)]


def test_c2_dispatch_sgl_p1000_grid20():
    """The 20-point lambda1 grid of a p=1000 SGL problem as one batch, 2 iterations: three grid points against the
    oracle's ADMM_SGL, all twenty through properties (exact symmetry, finite dual, Omega positive definite)."""
    from gglasso_amd import synth
    from gglasso_amd.batch import ADMM_SGL_batch
    p = 1000
    S, _ = synth.make_problem("GGL", 1, p, N=2 * p, seed=1235)
    S = S[0]
    lams = np.logspace(0, -2, 20)
    res = ADMM_SGL_batch(S, lams, max_iter=2, tol=1e-20, rtol=1e-20)
    assert len(res) == 20
    for k in (0, 9, 19):
        with oracle_threads():
            ref, _ = orc.ADMM_SGL(S, lams[k], np.eye(p), max_iter=2, tol=1e-20, rtol=1e-20)
        sol, info = res[k]
        assert info["status"] == "max iterations reached" and info["iterations"] == 2
        _check_state(sol, ref, ("Omega", "Theta", "X"), 1e-9)
    for k, (sol, info) in enumerate(res):
        assert np.array_equal(sol["Omega"], sol["Omega"].T), k
        assert np.array_equal(sol["Theta"], sol["Theta"].T), k
        assert np.isfinite(sol["X"]).all()
        # Omega = phiplus(...) is positive definite whatever lambda1 (single_admm_solver.py:164-166)
        with oracle_threads():
            assert np.linalg.eigvalsh(sol["Omega"]).min() > 0, k


def test_c2_converged_grid_with_group_schedules_and_compaction():
    """C2 whole and CONVERGED: the 20-point lambda1 grid of the p = 1000 problem as one batch to
    tol = rtol = 1e-8 -- the instances run as contiguous groups with their own Newton-Schulz schedules (GGL_OPT_GROUP_SCHED),
    finished points leave through compaction, the loop runs in C -- against the oracle's ADMM_SGL from the same start
    (Omega_0 = X_0 = I, helper/model_selection.py:595-596) on three points: the best-conditioned one (it finishes first and
    leaves early), one from the middle and the worst-conditioned one: status, iteration count, |Theta - oracle|_F <= 1e-8."""
    from gglasso_amd import synth
    from gglasso_amd.batch import ADMM_SGL_batch
    p = 1000
    S, _ = synth.make_problem("GGL", 1, p, N=2 * p, seed=1235)
    S = S[0]
    lams = np.logspace(0, -2, 20)
    eye = np.eye(p)
    res = ADMM_SGL_batch(S, lams, Omega_0=eye, X_0=eye, tol=1e-8, rtol=1e-8)
    its = [info["iterations"] for _, info in res]
    assert all(info["status"] == "optimal" for _, info in res), [info["status"] for _, info in res]
    assert max(r[1]["carried"] for r in res) > min(r[1]["carried"] for r in res)          # points did leave early
    for k in (int(np.argmin(its)), 10, 19):
        with oracle_threads():
            ref, rinfo = quiet(orc.ADMM_SGL, S, lams[k], eye, X_0=eye, tol=1e-8, rtol=1e-8, measure=True)
        sol, info = res[k]
        assert rinfo["status"] == "optimal" and info["iterations"] == len(rinfo["residual"]), (k, info, len(rinfo["residual"]))
        assert np.linalg.norm(sol["Theta"] - ref["Theta"]) <= 1e-8, (k, float(np.linalg.norm(sol["Theta"] - ref["Theta"])))
        assert np.array_equal(sol["Theta"], sol["Theta"].T)


def test_c5_slab_dispatch_ggl_K32_p1000(stats):
    """Per-GPU slab of C5 (K=256, p=1000 over 8 GPUs): 4352 tile pairs, unsplit launch sequence on the double-buffered
    64x64 DMA kernel; iteration 2 speculates.  Whole state against the oracle."""
    from gglasso_amd import solver
    S, Om0 = _problem("GGL", 32, 1000, 1238)
    # (round 6: seven iterations WITH the rho rule from rho_0 = 4 -- the residual balancing halves rho twice on the way
    # (4, 4, 2, 2, 2, 1, 1), so the run covers rho changes, dropped pre-launched chains and the speculative steps between them)
    hist = []
    kw = dict(max_iter=7, tol=1e-20, rtol=1e-20, rho=4.0)
    with oracle_threads():
        ref, _ = quiet(orc.ADMM_MGL, S, 0.05, 0.01, "GGL", Om0, history=hist, **kw)
    assert len({h[4] for h in hist}) >= 2, [h[4] for h in hist]           # rho did change along the way
    out, _ = quiet(solver.ADMM_MGL, S, 0.05, 0.01, "GGL", Om0, **kw)
    _check_state(out, ref, ("Omega", "Theta", "X"), 1e-9)
    assert np.array_equal(out["Theta"], out["Theta"].transpose(0, 2, 1))
    st = stats[-1]
    assert st["last_parts"] == 1 and st["last_variant"] == 16, st
    assert st["spec_calls"] >= 1, st          # the iterations between the rho changes ran speculatively


def test_c5_whole_ggl_K256_p1000(stats):
    """C5 WHOLE on one GPU (solver/admm_solver.py:172-246 at K = 256, p = 1000): 2 iterations, all of
    Omega / Theta / X against the oracle at 1e-9, on the Theta kernel that spreads the K-column over 16 waves of 16 values
    (k_theta_ggl_cols<16,16,1>, the only one for 128 < K <= 256) and the double-buffered 64x64 DMA product kernel."""
    from gglasso_amd import solver
    S, Om0 = _problem("GGL", 256, 1000, 1240)
    kw = dict(max_iter=2, tol=1e-20, rtol=1e-20)
    with oracle_threads():
        ref, _ = orc.ADMM_MGL(S, 0.05, 0.01, "GGL", Om0, **kw)
    out, _ = quiet(solver.ADMM_MGL, S, 0.05, 0.01, "GGL", Om0, **kw)
    _check_state(out, ref, ("Omega", "Theta", "X"), 1e-9)
    assert np.array_equal(out["Theta"], out["Theta"].transpose(0, 2, 1))
    st = stats[-1]
    assert st["last_parts"] == 1 and st["last_variant"] == 16, st
    assert st["dispatch_theta_kernel"] == 1616, st
    assert st["stable_calls"] == 0 and st["eigh_fallbacks"] == 0, st


@pytest.mark.parametrize("K,p,latent,code", [(256, 64, False, 10416), (100, 21, False, 10216), (130, 50, True, 10416),
                                             (64, 64, False, 808), (256, 200, False, 1616)])
def test_many_instances_of_a_small_matrix(stats, K, p, latent, code):
    """GGL with K > 64 and fewer than 256 workgroups of 128 elements (BASELINE's K = 256, p = 64 among them): the Theta-step
    takes 16 elements per workgroup (k_theta_ggl_cols, SPLIT = 4: p^2 / 16 workgroups instead of p^2 / 128 on 256 CUs), the Omega-step
    the LDS-resident kernel.  Six iterations of all of Omega / Theta / X (/ L) against the oracle (admm_solver.py:172-246);
    the neighbouring shapes keep their 128-element kernels."""
    from gglasso_amd import solver
    S, Om0 = _problem("GGL", K, p, 1250 + p)
    kw = dict(max_iter=6, tol=1e-20, rtol=1e-20, latent=latent, mu1=(0.6 * np.ones(K) if latent else None))
    with oracle_threads():
        ref, _ = orc.ADMM_MGL(S, 0.05, 0.01, "GGL", Om0, **kw)
    out, _ = quiet(solver.ADMM_MGL, S, 0.05, 0.01, "GGL", Om0, **kw)
    _check_state(out, ref, ("Omega", "Theta", "X") + (("L",) if latent else ()), 1e-9)
    assert np.array_equal(out["Theta"], out["Theta"].transpose(0, 2, 1))
    st = stats[-1]
    assert st["dispatch_theta_kernel"] == code, st
    if p <= 64 and not latent:
        assert st["last_variant"] == 41, st


@pytest.mark.parametrize("K", [4, 8, 16])
def test_headline_slab_dispatch(stats, K):
    """Per-GPU slabs of the headline under K-sharding at 8 / 4 / 2 GPUs (what decides strong scaling): K = 4 and K = 16
    (576 64x64 tile pairs) take the 32x32 direct-to-LDS kernel (variant 20) as one launch sequence, K = 8 the same kernel as
    two concurrent parts of four."""
    from gglasso_amd import solver
    S, Om0 = _problem("GGL", K, 500, 1239)
    kw = dict(max_iter=5, tol=1e-20, rtol=1e-20)
    with oracle_threads():
        ref, _ = orc.ADMM_MGL(S, 0.05, 0.01, "GGL", Om0, **kw)
    out, _ = quiet(solver.ADMM_MGL, S, 0.05, 0.01, "GGL", Om0, **kw)
    _check_state(out, ref, ("Omega", "Theta", "X"), 1e-9)
    st = stats[-1]
    assert (st["last_parts"], st["last_variant"]) == {4: (1, 20), 8: (2, 20), 16: (1, 20)}[K], st
    # two concurrent parts: the part stream was checked to run BESIDE the main stream before the first such step (two HIP
    # streams on one hardware queue serialise silently; -1 = never probed, n > 0 = n fresh streams tried until one did)
    assert (st["pipe_part_streams_tried"] >= 0) == (K == 8), st


def test_large_p_sgl_latent_p1500(stats):
    """A single large matrix (ADMM_SGL, p = 1500, latent; single_admm_solver.py:157-214): the sizes the reference's own
    benchmarks run (p = 1000 .. 5000) -- three iterations against the oracle, through the Newton-Schulz Omega-step, the
    deflating L-step at a basis of 8 x 1500 doubles per instance and ggl_finalize_L with rocSOLVER."""
    from gglasso_amd import solver, synth
    p = 1500
    S, _ = synth.make_problem("GGL", 1, p, N=2 * p, seed=1244)
    kw = dict(max_iter=3, tol=1e-20, rtol=1e-20, latent=True, mu1=0.8)
    with oracle_threads():
        ref, _ = quiet(orc.ADMM_SGL, S[0], 0.05, np.eye(p), **kw)
    out, _ = quiet(solver.ADMM_SGL, S[0], 0.05, np.eye(p), **kw)
    for nm in ("Omega", "Theta", "L", "X"):
        err = float(np.abs(out[nm] - ref[nm]).max())
        assert err <= 1e-9 * max(1.0, float(np.abs(ref[nm]).max())), (nm, err)
    with oracle_threads():
        assert np.linalg.matrix_rank(out["L"]) == np.linalg.matrix_rank(ref["L"])
    st = stats[-1]
    assert st["rank_calls"] == 3 and st["rank_deflated_calls"] >= 1 and st["dispatch_finalize_calls"] == 1, st
