"""glasso_problem on the device against the reference's problem.py (fixture G21, tests/golden/make_golden_problem.py).

Selected parameters and adjacency_ are exact.  Tables and estimators carry the tolerances tests/grid_checks.py applies to
G12 / G13 / G16 (a batched grid starts every point from the identity where the reference warm-starts; both stop at
r <= dim * tol): tables rtol 1e-7 with atol 1e-5 (single) / 1e-4 (multiple), estimators 2e-7 (single) / 5e-7 (multiple)."""
import warnings

import numpy as np
import pytest

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def g(golden):
    return golden("g21_problem")


def quiet(fn, *a, **k):
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        return fn(*a, **k)


def check_tables(g, tag, P, atol, rank):
    st = P.modelselect_stats
    assert np.allclose(st['BIC'][0.1], g[f"{tag}_BIC"], rtol=1e-7, atol=atol), tag
    assert np.allclose(st['AIC'], g[f"{tag}_AIC"], rtol=1e-7, atol=atol), tag
    assert np.array_equal(st['SP'], g[f"{tag}_SP"]), tag
    if rank:
        assert np.array_equal(st['RANK'], g[f"{tag}_RANK"]), tag
    assert float(P.reg_params['lambda1']) == float(g[f"{tag}_sel_lambda1"])
    if f"{tag}_sel_lambda2" in g.files:
        assert float(P.reg_params['lambda2']) == float(g[f"{tag}_sel_lambda2"])
    if f"{tag}_sel_mu1" in g.files:
        assert np.array_equal(np.asarray(P.reg_params['mu1'], dtype=float), g[f"{tag}_sel_mu1"])


def check_estimator(g, tag, P, tol):
    sol = P.solution
    assert np.linalg.norm(sol.precision_ - g[f"{tag}_precision"]) <= tol, tag
    assert np.array_equal(sol.adjacency_, g[f"{tag}_adjacency"]), tag
    if f"{tag}_lowrank" in g.files:
        assert np.linalg.norm(sol.lowrank_ - g[f"{tag}_lowrank"]) <= tol, tag
    else:
        assert sol.lowrank_ is None
    want = float(g[f"{tag}_ebic05"])
    assert abs(sol.calc_ebic(0.5) - want) <= 1e-7 * abs(want) + 1e-4, tag


def case3(g, from_data=False):
    from gglasso_amd import glasso_problem
    kw = dict(reg="GGL", reg_params={'lambda1': float(g["c3_lambda1"]), 'lambda2': float(g["c3_lambda2"])}, do_scaling=True)
    if from_data:
        return quiet(glasso_problem.from_data, [g[f"c3_X_{k}"] for k in range(3)], **kw)
    return quiet(glasso_problem, g["c3_S"], g["c3_N"], **kw)


def test_case1_sgl_scaled(g):
    from gglasso_amd import glasso_problem
    tol = float(g["tol"])
    P = quiet(glasso_problem, g["c1_S"], int(g["c1_N"]), reg_params={'lambda1': float(g["c1_lambda1"])}, do_scaling=True)
    assert np.all(np.abs(P._scale - g["c1_scale"]) == 0)
    quiet(P.solve, tol=tol, rtol=tol)
    check_estimator(g, "c1_solve", P, 2e-7)
    quiet(P.model_selection, modelselect_params={'lambda1_range': g["c1_lambda1_range"]}, gamma=0.1, tol=tol, rtol=tol)
    check_tables(g, "c1_ms", P, 1e-5, rank=False)
    check_estimator(g, "c1_ms", P, 2e-7)


def test_case2_sgl_latent_selection(g):
    from gglasso_amd import glasso_problem
    tol = float(g["tol"])
    P = glasso_problem(g["c2_S"], int(g["c2_N"]), latent=True)
    quiet(P.model_selection, modelselect_params={'lambda1_range': g["c2_lambda1_range"], 'mu1_range': g["c2_mu1_range"]},
          gamma=0.1, tol=tol, rtol=tol)
    check_tables(g, "c2_ms", P, 1e-5, rank=True)
    check_estimator(g, "c2_ms", P, 2e-7)


def test_case3_ggl_scaled_through_one_batch(g, monkeypatch):
    from gglasso_amd import batch, solver
    tol = float(g["tol"])
    P = case3(g)
    quiet(P.solve, tol=tol, rtol=tol)
    check_estimator(g, "c3_solve", P, 5e-7)
    calls = {"batch": 0, "solver": 0}
    real_batch, real_solver = batch.ADMM_MGL_batch, solver.ADMM_MGL

    def counting_batch(*a, **k):
        calls["batch"] += 1
        return real_batch(*a, **k)

    def counting_solver(*a, **k):
        calls["solver"] += 1
        return real_solver(*a, **k)
    monkeypatch.setattr(batch, "ADMM_MGL_batch", counting_batch)
    monkeypatch.setattr(solver, "ADMM_MGL", counting_solver)
    quiet(P.model_selection, modelselect_params={'lambda1_range': g["c3_lambda1_range"], 'lambda2_range': g["c3_lambda2_range"]},
          gamma=0.1, tol=tol, rtol=tol)
    assert calls == {"batch": 1, "solver": 0}                       # the 3 x 2 grid is ONE batched call, not six solves
    check_tables(g, "c3_ms", P, 1e-4, rank=False)
    check_estimator(g, "c3_ms", P, 5e-7)


def test_case3_from_data_selects_the_same(g):
    tol = float(g["tol"])
    P = case3(g, from_data=True)
    assert np.array_equal(P.N, g["c3_N"]) and np.abs(P.solution.sample_covariance_ - g["c3_S"]).max() <= 1e-12
    quiet(P.model_selection, modelselect_params={'lambda1_range': g["c3_lambda1_range"], 'lambda2_range': g["c3_lambda2_range"]},
          gamma=0.1, tol=tol, rtol=tol)
    assert float(P.reg_params['lambda1']) == float(g["c3_ms_sel_lambda1"])
    assert float(P.reg_params['lambda2']) == float(g["c3_ms_sel_lambda2"])
    assert np.array_equal(P.solution.adjacency_, g["c3_ms_adjacency"])
    assert np.array_equal(P.modelselect_stats['SP'], g["c3_ms_SP"])


def test_case4_fgl_latent_two_stages(g):
    from gglasso_amd import glasso_problem
    tol = float(g["tol"])
    P = glasso_problem(g["c4_S"], g["c4_N"], reg="FGL", latent=True)
    quiet(P.model_selection, modelselect_params={'lambda1_range': g["c4_lambda1_range"], 'lambda2_range': g["c4_lambda2_range"],
                                                 'mu1_range': g["c4_mu1_range"]}, gamma=0.1, tol=tol, rtol=tol)
    assert np.array_equal(P._stage1['stats']['ix_mu'], g["c4_ix_mu"])
    check_tables(g, "c4_ms", P, 1e-4, rank=True)
    check_estimator(g, "c4_ms", P, 5e-7)


def test_case5_nonconforming_solve(g):
    from gglasso_amd import glasso_problem
    tol = float(g["tol"])
    S = [g[f"c5_S_{k}"] for k in range(3)]
    P = glasso_problem(S, g["c5_N"], reg="GGL", G=g["c5_G"].astype(int),
                       reg_params={'lambda1': float(g["c5_lambda1"]), 'lambda2': float(g["c5_lambda2"])})
    assert not P.conforming and 'update_rho' not in P._default_solver_params()
    quiet(P.solve, tol=tol, rtol=tol)
    for k in range(3):
        assert np.linalg.norm(P.solution.precision_[k] - g[f"c5_solve_precision_{k}"]) <= 5e-7, k
        assert np.array_equal(P.solution.adjacency_[k], g[f"c5_solve_adjacency_{k}"]), k
    want = float(g["c5_solve_ebic05"])
    assert abs(P.solution.calc_ebic(0.5) - want) <= 1e-7 * abs(want) + 1e-4
