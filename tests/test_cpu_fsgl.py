"""Functional Single Graphical Lasso without a GPU: the G20 fixtures (reference: solver/functional_sgl_admm.py,
solver/ggl_helper.py:45-66, helper/utils.py:69-107) against an independent NumPy statement of the operators, and the host
loop of ``gglasso_amd.ADMM_FSGL`` over a test-only engine."""
import contextlib
import io
import warnings

import numpy as np
import pytest

import fsgl_fixtures as fx
from oracle import ggl_oracle as orc
from oracle_engine import OracleEngine


class FsglOracleEngine(OracleEngine):
    """OracleEngine with the FSGL Theta-step (the block shrink in NumPy)."""

    def set_block_size(self, M):
        self.M = int(M or 0)

    def step_finish(self, rho, lambda1, lambda2, reg, latent, mu1, groupsq_ready):
        if reg != 'FSGL':
            return super().step_finish(rho, lambda1, lambda2, reg, latent, mu1, groupsq_ready)
        assert self.M > 0
        V = self.Om + self.L + self.X
        self.Th = np.stack([fx.prox_sum_frob_np(V[k], self.M, (1 / rho) * lambda1) for k in range(self.K)])
        if latent:
            self.L = orc.rank_stack(self.Th - self.X - self.Om, np.asarray(mu1) / rho)
        self.X = self.X + self.Om - self.Th + self.L
        return np.array([np.sum(self.Om ** 2), np.sum((self.Th - self.L) ** 2), np.sum(self.X ** 2),
                         np.sum((self.Om - self.Th + self.L) ** 2), np.sum((self.Om - self.Om_prev) ** 2)])


@pytest.fixture()
def solver(monkeypatch):
    from gglasso_amd import solver
    monkeypatch.setattr(solver, "ENGINE", FsglOracleEngine)
    return solver


def quiet(fn, *a, **k):
    buf = io.StringIO()
    with contextlib.redirect_stdout(buf):
        out = fn(*a, **k)
    return out, buf.getvalue()


def test_operator_fixtures_agree_with_the_numpy_formula():
    n_seen, kinds = 0, set()
    for n, X, M, l, Y in fx.operator_cases():
        got = fx.prox_sum_frob_np(X, M, l)
        assert np.abs(got - Y).max() <= 1e-12 * np.abs(X).max(), (n, M)
        p = X.shape[0] // M
        norms = fx.block_norms(X, M)[np.triu_indices(p, 1)]
        kinds.add("above" if l > norms.max() else ("below" if l < norms.min() else "inside"))
        assert np.all(np.abs(norms - l) > 1e-9 * l)
        n_seen += 1
    assert n_seen == 20 and kinds == {"above", "below", "inside"}
    assert {M for _, _, M, _, _ in fx.operator_cases()} == {1, 2, 3, 5, 8, 16, 32, 33, 40}
    assert any(np.abs(X - X.T).max() > 0 for _, X, _, _, _ in fx.operator_cases())


@pytest.mark.parametrize("tag", ["A", "B", "C", "D", "E", "F"])
def test_block_norm_fixtures_agree_with_the_numpy_formula(tag):
    c = fx.case(tag)
    N = fx.block_norms(c["S"], c["M"])
    N = np.triu(N) + np.triu(N, 1).T
    assert np.abs(N - c["frob"]).max() <= 1e-12 * np.abs(c["S"]).max()
    np.fill_diagonal(N, 0.0)
    assert np.abs(N - c["frob_od"]).max() <= 1e-12 * np.abs(c["S"]).max()
    assert abs(N.max() - c["lmax"]) <= 1e-12 * np.abs(c["S"]).max()
    for run in c["runs"]:
        nz = np.count_nonzero(np.triu(fx.block_norms(run["Theta"], c["M"]), 1))
        assert nz == run["nz"] and 0 < nz


@pytest.mark.parametrize("tag", ["A", "B", "F"])
def test_host_loop_reproduces_the_reference(solver, tag):
    c = fx.case(tag)
    pM = c["p"] * c["M"]
    for lam, run in zip(c["lams"], c["runs"]):
        latent = "L" in run
        (sol, info), text = quiet(solver.ADMM_FSGL, c["S"], lam, c["M"], np.eye(pM), tol=1e-9, rtol=1e-9, measure=True,
                                  latent=latent, mu1=run.get("mu1"))
        assert info["status"] == run["status"] == "optimal"
        assert len(info["residual"]) == run["iters"], (len(info["residual"]), run["iters"])
        assert f"ADMM terminated after {run['iters']} iterations with status: optimal." in text
        assert np.linalg.norm(sol["Theta"] - run["Theta"]) <= 1e-8
        np.testing.assert_allclose(info["residual"], run["residual"], rtol=1e-8)
        assert set(info) == {"status", "runtime", "residual"}
        assert set(sol) == ({"Omega", "Theta", "X", "L"} if latent else {"Omega", "Theta", "X"})
        if latent:
            assert np.linalg.matrix_rank(sol["L"]) == run["rankL"]
            assert np.linalg.norm(sol["L"] - run["L"]) <= 1e-8


def test_asserts_keys_and_prints(solver):
    c = fx.case("A")
    S, M = c["S"], c["M"]
    I = np.eye(S.shape[0])
    with pytest.raises(AssertionError):
        solver.ADMM_FSGL(S, 0.1, 7, I)                  # pM % M != 0
    with pytest.raises(AssertionError):
        solver.ADMM_FSGL(S, 0.0, M, I)
    with pytest.raises(AssertionError):
        solver.ADMM_FSGL(S, -1.0, M, I)
    with pytest.raises(AssertionError):
        solver.ADMM_FSGL(S, 0.1, M, I, latent=True)     # latent without mu1
    with pytest.raises(AssertionError):
        solver.ADMM_FSGL(S, 0.1, M, I, latent=True, mu1=0.0)
    with pytest.raises(AssertionError):
        solver.ADMM_FSGL(S, 0.1, M, I, rho=0.0)
    (sol, info), text = quiet(solver.ADMM_FSGL, S, c["lams"][1], M, I, max_iter=3, verbose=True)
    assert set(info) == {"status"} and set(sol) == {"Omega", "Theta", "X"}
    assert info["status"] == "max iterations reached"
    lines = text.splitlines()
    assert lines[0] == f"Derived a Functional SGL problem of dimensionality p={c['p']}."
    assert lines[1] == "------------ADMM Algorithm for Functional Single Graphical Lasso----------------"
    assert lines[2].split() == ["iter", "r_t", "s_t", "eps_pri", "eps_dual", "rho"]
    assert len(lines[3].split()) == 6
    assert lines[-1] == "ADMM terminated after 3 iterations with status: max iterations reached."
    # the final line is printed without verbose as well (functional_sgl_admm.py:205)
    (_, _), text = quiet(solver.ADMM_FSGL, S, c["lams"][1], M, I, max_iter=2)
    assert text == "ADMM terminated after 2 iterations with status: max iterations reached.\n"


def test_exit_warnings_are_warnings_with_the_eigenvalue(solver, monkeypatch):
    """functional_sgl_admm.py:207-226 warns (it does not print) with the eigenvalue in the message."""
    S = np.eye(4)
    with warnings.catch_warnings():
        warnings.simplefilter("error")
        quiet(solver.ADMM_FSGL, S, 0.1, 2, np.eye(4), max_iter=5)
    monkeypatch.setattr(FsglOracleEngine, "exit_checks", lambda self, latent: np.array([2e-5, 0.0, 0.0, -0.5, -1e-3]))
    with pytest.warns(UserWarning) as rec:
        quiet(solver.ADMM_FSGL, S, 0.1, 2, np.eye(4), max_iter=2, latent=True, mu1=0.5)
    msgs = [str(w.message) for w in rec]
    assert "Omega variable is not symmetric, largest deviation is 2e-05." in msgs
    assert "Theta (Theta - L resp.) is not positive definite. Solve to higher accuracy! (min EV is -0.5)" in msgs
    assert "L is not positive semidefinite. Solve to higher accuracy! (min EV is -0.001)" in msgs


def test_package_exports():
    import gglasso_amd
    from gglasso_amd import batch, ops, utils
    assert callable(gglasso_amd.ADMM_FSGL) and "ADMM_FSGL" in gglasso_amd.__all__
    assert callable(batch.ADMM_FSGL_batch) and callable(ops.prox_sum_Frob)
    assert callable(utils.frob_norm_per_block) and callable(utils.lambda_max_fsgl)
    import inspect
    sig = inspect.signature(gglasso_amd.ADMM_FSGL)
    assert list(sig.parameters) == ["S", "lambda1", "M", "Omega_0", "Theta_0", "X_0", "rho", "max_iter", "tol", "rtol",
                                    "update_rho", "verbose", "measure", "latent", "mu1"]
    d = {k: v.default for k, v in sig.parameters.items()}
    assert (d["rho"], d["max_iter"], d["tol"], d["rtol"], d["update_rho"], d["latent"], d["mu1"]) == (1., 1000, 1e-7, 1e-4, True,
                                                                                                   False, None)
