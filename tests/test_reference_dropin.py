"""Drop-in check against the REAL reference package, through its recorded seams (fixture G19,
tests/golden/make_golden_dropin.py, tests/seam_calls.py).  The reference's own model-selection drivers and problem class
were run with their own functions at the seams SURVEY.md section 8(b) names, and every call they made there was recorded
with what it returned; here the same calls go to gglasso_amd's functions -- warm starts taken from gglasso_amd's own
earlier returns, as the driver would take them -- and must return what the reference's did.  No GPU here, so the array
work behind gglasso_amd's host loops is done by the test-only oracle engine: what is verified is the boundary (signatures,
kwargs, return dicts, status strings, warm starts), which is exactly what a maintainer's one-line import swap relies on."""
import contextlib
import io

import numpy as np
import pytest

import seam_calls
from conftest import load_golden


@pytest.fixture(scope="module")
def seams():
    g = load_golden("g19_dropin_seams")
    return g, seam_calls.load(g)


@pytest.fixture()
def ours(monkeypatch):
    from gglasso_amd import solver
    from oracle_engine import OracleEngine
    monkeypatch.setattr(solver, "ENGINE", OracleEngine)
    return solver


def quiet(fn, *a, **k):
    with contextlib.redirect_stdout(io.StringIO()):
        return fn(*a, **k)


def functions(ours):
    from gglasso_amd import ext_solver, model_selection as ours_ms
    return {"ADMM_MGL": ours.ADMM_MGL, "ADMM_SGL": ours.ADMM_SGL, "block_SGL": ours.block_SGL,
            "ext_ADMM_MGL": ext_solver.ext_ADMM_MGL, "single_grid_search": ours_ms.single_grid_search,
            "grid_search": ours_ms.grid_search, "K_single_grid": ours_ms.K_single_grid}


def replay(seams, name, ours, known=None):
    g, meta = seams
    return quiet(seam_calls.replay, meta[name], functions(ours), g, known)


def assert_like(got, ref, tol, where):
    """`got` carries everything `ref` (the reference's return) does: same keys (more allowed), same strings / integers,
    arrays and floats within tol * max(1, |ref|_max).  An array the fixture does not store (seam_calls.NOT_STORED) is only
    required to be there."""
    if isinstance(ref, dict):
        assert isinstance(got, dict), where
        for k, v in ref.items():
            assert k in got, (where, k)
            assert_like(got[k], v, tol, f"{where}[{k!r}]")
    elif isinstance(ref, (tuple, list)):
        assert len(got) == len(ref), where
        for j, (a, b) in enumerate(zip(got, ref)):
            assert_like(a, b, tol, f"{where}[{j}]")
    elif isinstance(ref, str) and ref == seam_calls.OMITTED:
        assert isinstance(got, np.ndarray), where
    elif isinstance(ref, np.ndarray):
        got = np.asarray(got)
        assert got.shape == ref.shape, (where, got.shape, ref.shape)
        if ref.dtype.kind == "f":
            scale = max(1.0, float(np.nanmax(np.abs(ref)))) if np.isfinite(ref).any() else 1.0
            assert np.array_equal(np.isnan(got), np.isnan(ref)), where
            ok = ~np.isnan(ref)
            assert np.abs(got[ok] - ref[ok]).max(initial=0.0) <= tol * scale, (where, np.abs(got[ok] - ref[ok]).max())
        else:
            assert np.array_equal(got, ref), where
    elif isinstance(ref, float):
        assert abs(float(got) - ref) <= tol * max(1.0, abs(ref)) or (np.isnan(ref) and np.isnan(got)), (where, got, ref)
    else:
        assert got == ref, (where, got, ref)


def test_seam1_grid_search_takes_our_solver(seams, ours):
    """helper/model_selection.py:55,222 -- grid_search(solver, ...) calls solver(**kwargs), warm-started from the previous
    point (:224): every call of the reference's walk, answered by ours."""
    calls = replay(seams, "seam1_grid", ours)
    assert len(calls) == 6
    for j, (_, got, ref) in enumerate(calls):
        assert_like(got, ref, 1e-7, f"call {j}")
        assert got[1]['status'] == ref[1]['status']


def test_seam2_glasso_problem_with_patched_solvers(seams, ours):
    """problem.py:10-11 imports ADMM_MGL / ADMM_SGL / block_SGL by name; swapping them is the whole integration.  GGL / FGL
    with and without latent variables, then the single problem: non-latent through block_SGL (problem.py:443-450), latent
    through ADMM_SGL (:430-440)."""
    calls = replay(seams, "seam2_problem", ours)
    assert [c[0] for c in calls] == ["ADMM_MGL"] * 4 + ["block_SGL", "ADMM_SGL"]
    for j, (name, got, ref) in enumerate(calls):
        assert_like(got, ref, 1e-8, f"call {j} ({name})")
        if name != "block_SGL":
            assert got[1]['status'] == ref[1]['status'] == 'optimal'


def test_seam2_glasso_problem_on_drawn_configurations(seams, ours):
    """The real glasso_problem class (problem.py) on sixty drawn configurations -- single / GGL / FGL, K = 2 .. 5, p = 6 .. 24,
    latent on / off, do_scaling on / off (the class scales S to correlations before the solver and the solution back after
    it, problem.py:239-262), drawn reg_params: every solver call it made, answered by ours -- same status, same Theta (and
    L)."""
    calls = replay(seams, "seam2_drawn", ours, known=seam_calls.drawn_known())
    assert len(calls) == 60
    for j, (name, got, ref) in enumerate(calls):
        # (the non-latent single problem goes through block_SGL, which returns no info: problem.py:443-450)
        assert_like(got, ref, 1e-8, f"trial {j} ({name})")


def test_seam2_model_selection_single(seams, ours):
    """single_grid_search (model_selection.py:505) drives block_SGL / ADMM_SGL imported at :13, warm-started along the
    lambda path (:632): every point of the path, answered by ours."""
    calls = replay(seams, "seam2_single", ours)
    assert [c[0] for c in calls] == ["block_SGL"] * 5
    for j, (_, got, ref) in enumerate(calls):
        assert_like(got, ref, 1e-7, f"point {j}")


def assert_selection_like(stats, rstats, gamma):
    """The model-selection tables problem.py reads (BEST, and the tables it stores)."""
    assert np.allclose(stats['BIC'][gamma], rstats['BIC'][gamma], rtol=1e-7)
    assert np.array_equal(stats['SP'], rstats['SP'])
    assert np.array_equal(stats['RANK'], rstats['RANK'], equal_nan=True)
    assert stats['BEST'] == rstats['BEST']


def test_seam3a_glasso_problem_model_selection_with_the_batched_grid(seams, ours):
    """problem.py:14 imports single_grid_search by name and model_selection() calls it at :606; gglasso_amd's
    single_grid_search (the whole grid as one batch) must return the selected point, the tables and the estimate of the
    reference's sequential walk, with and without latent variables."""
    calls = replay(seams, "seam3a", ours)
    assert len(calls) == 2
    for got, ref in ((c[1], c[2]) for c in calls):
        assert_like(got[0], ref[0], 1e-6, "best solution")
        assert_like(got[2], ref[2], 1e-6, "low rank")
        assert_selection_like(got[3], ref[3], 0.3)


def test_seam2_ext_admm_nonconforming_through_glasso_problem(seams, ours):
    """problem.py:12,468 -- a dict S with a bookkeeping array G makes glasso_problem.solve() call ext_ADMM_MGL; swapping
    the name for gglasso_amd.ext_ADMM_MGL (instances padded into one stack) must give the reference's solution, with and
    without latent variables (reference tests/test_problem.py:117-138)."""
    calls = replay(seams, "seam2_ext", ours)
    assert len(calls) == 2
    for j, (_, got, ref) in enumerate(calls):
        assert got[1]['status'] == ref[1]['status']
        assert_like(got[0], ref[0], 1e-8, f"call {j}")


def test_seam3b_glasso_problem_model_selection_mgl_with_the_batched_grid(seams, ours):
    """problem.py:14,626-654: model_selection() of a multiple-graph problem calls K_single_grid (latent, stage one) and
    grid_search(solver=ADMM_MGL, ...); gglasso_amd's ADMM_MGL, grid_search and K_single_grid (every grid a batch) must
    select the same (lambda1, lambda2) and return the same tables and estimate as the reference's sequential walks."""
    calls = replay(seams, "seam3b", ours)
    assert [c[0] for c in calls] == ["grid_search", "K_single_grid", "grid_search"]
    for name, got, ref in calls:
        if name == "grid_search":
            assert_selection_like(got[0], ref[0], 0.1)
            assert tuple(got[1]) == tuple(ref[1])
            assert_like(got[2], ref[2], 1e-6, "selected estimate")
        else:
            # stage one (problem.py:633-647): the estimates and the per-instance mu1 choice ix_mu handed to grid_search
            assert_like(got[:2], ref[:2], 1e-6, "K_single_grid estimates")
            assert np.array_equal(got[2]['ix_mu'], ref[2]['ix_mu'])


def test_seam1_reference_grid_search_rank_table_above_the_jacobi_limit(seams, ours):
    """the REFERENCE's grid_search (helper/model_selection.py:55-298) applies numpy.linalg.matrix_rank to
    the sol['L'] our solver hands it (:254).  Answering its calls at p = 160 (the walk over fixture G18's grid), our solver
    must give the RANK table and the sparsity the reference computed with its own solver (G18).  (Array work by the oracle
    engine here; tests/test_gpu_latent_rank.py runs the same walk on the HIP engine, where the returned L is the rebuilt
    one.)"""
    from gglasso_amd.model_selection import mean_sparsity
    g = load_golden("g18_latent_rank_large_p")
    calls = replay(seams, "seam1_rank", ours, known={"mgl_S": g["mgl_S"]})
    _, meta = seams
    K = g["mgl_S"].shape[0]
    assert len(calls) == g["grid_l1"].size * g["grid_l2"].size
    for c, (_, got, _) in zip(meta["seam1_rank"], calls):
        l1 = float(c["kwargs"]["__d"][[k for k, _ in c["kwargs"]["__d"]].index("lambda1")][1]["__f"])
        l2 = float(c["kwargs"]["__d"][[k for k, _ in c["kwargs"]["__d"]].index("lambda2")][1]["__f"])
        # the grid is meshgrid(l1, l2) (model_selection.py:47): lambda2 over the rows, lambda1 over the columns
        i, j = int(np.argmin(np.abs(g["grid_l2"] - l2))), int(np.argmin(np.abs(g["grid_l1"] - l1)))
        sol = got[0]
        assert [np.linalg.matrix_rank(sol['L'][k]) for k in range(K)] == list(g["grid_RANK"][:, i, j]), (i, j)
        assert np.isclose(mean_sparsity(sol['Theta']), g["grid_SP"][i, j]), (i, j)
        if (i, j) == tuple(int(v) for v in g["grid_ix"]):
            assert [np.linalg.matrix_rank(sol['L'][k]) for k in range(K)] == list(g["grid_best_rank"])
