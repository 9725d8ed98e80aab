"""glasso_problem / GGLassoEstimator over the test-only oracle engine: the class's host logic (formulation, messages,
defaults, dispatch, scaling bookkeeping) and sample_covariance's argument handling, without a GPU."""
import os
import sys
import warnings

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import problem_helpers as ph  # noqa: E402


@pytest.fixture()
def host(monkeypatch):
    ph.on_host(monkeypatch)
    from gglasso_amd import problem
    return problem


def spd(p, seed=0, K=None):
    rng = np.random.default_rng(seed)
    if K is None:
        B = rng.standard_normal((p, 3 * p))
        return B @ B.T / (3 * p)
    return np.stack([spd(p, seed + k) for k in range(K)])


def trivial_G(p, K):
    ij = np.array([(i, j) for j in range(p) for i in range(j)])
    return np.stack([np.repeat(ij[:, 0][:, None], K, axis=1), np.repeat(ij[:, 1][:, None], K, axis=1)]).astype(int)


def test_exports():
    import gglasso_amd
    from gglasso_amd.problem import glasso_problem, GGLassoEstimator
    assert gglasso_amd.glasso_problem is glasso_problem and gglasso_amd.GGLassoEstimator is GGLassoEstimator
    assert {"glasso_problem", "GGLassoEstimator"} <= set(gglasso_amd.__all__)


def test_formulation_from_input_kind(host):
    P = host.glasso_problem(spd(5), 50)
    assert (P.multiple, P.conforming, P.K, P.p, P.reg) == (False, True, 1, 5, None)
    P = host.glasso_problem(spd(5, K=3), 50, reg="FGL")
    assert (P.multiple, P.conforming, P.K, P.p, P.reg) == (True, True, 3, 5, "FGL")
    assert np.array_equal(P.N, 50 * np.ones(3))
    Sl = [spd(4, 1), spd(4, 2), spd(4, 3)]
    P = host.glasso_problem(Sl, np.array([10, 20, 30]), G=trivial_G(4, 3))
    assert (P.multiple, P.conforming, P.K) == (True, False, 3) and np.array_equal(P.p, [4, 4, 4])
    assert isinstance(P.S, dict) and sorted(P.S) == [0, 1, 2] and P.reg == "GGL"
    assert isinstance(P.solution, host.GGLassoEstimator) and P.solution.n_features is P.p and P.solution.precision_ is None
    S = spd(5)
    P = host.glasso_problem(S, 50)
    S[0, 0] = 99.0
    assert P.S[0, 0] != 99.0 and P.solution.sample_covariance_[0, 0] != 99.0      # copies


def test_assertion_messages(host):
    gp = host.glasso_problem
    with pytest.raises(AssertionError, match="GGLasso can only handle 2 or 3dim-input"):
        gp(np.zeros((2, 2, 2, 2)), 5)
    with pytest.raises(AssertionError, match=r"Specify covariance data in format\(p,p\)!"):
        gp(np.zeros((3, 4)), 5)
    with pytest.raises(AssertionError, match=r"Specify covariance data in format\(K,p,p\)!"):
        gp(np.zeros((2, 3, 4)), 5)
    A = spd(4)
    A[0, 1] += 1e-3
    with pytest.raises(AssertionError, match="Covariance data is not symmetric."):
        gp(A, 5)
    with pytest.raises(AssertionError, match="Covariance data is not symmetric."):
        gp(np.stack([A, A]), 5)
    with pytest.raises(AssertionError, match="For SGL problems, N needs to be a single number, float or int."):
        gp(spd(4), np.array([5]))
    with pytest.raises(AssertionError, match="only one entry"):
        gp([spd(4)], 5, G=trivial_G(4, 1))
    with pytest.raises(AssertionError, match="the input G has to be specified"):
        gp([spd(4), spd(4, 1)], 5)
    with pytest.raises(AssertionError, match="Covariance data for instance 1 is not symmetric."):
        gp([spd(4), A], 5, G=trivial_G(4, 2))
    with pytest.raises(AssertionError, match="do not match for instance 0"):
        gp([np.zeros((3, 4)), spd(4)], 5, G=trivial_G(4, 2))
    with pytest.raises(TypeError, match="Incorrect input type of S"):
        gp({1, 2}, 5)
    with pytest.raises(AssertionError, match="N must be positive."):
        gp(spd(4), 0)
    with pytest.raises(AssertionError, match="Specify 'GGL' for Group Graphical Lasso or 'FGL'"):
        gp(spd(4, K=2), 5, reg="TV")
    P = gp(spd(4), 5)
    with pytest.raises(AssertionError, match="Regularization parameters need to be set first"):
        P.solve()
    with pytest.raises(AssertionError, match="Currently only the ADMM solver is supported"):
        P.solve(solver="ppdna")
    with pytest.raises(AssertionError, match=r"gamma needs to be chosen as a parameter in \[0,1\]."):
        P.model_selection(gamma=2)
    with pytest.raises(AssertionError, match="Supported evaluation methods are eBIC and AIC."):
        P.model_selection(method="CV")


def test_default_parameter_dicts(host):
    P1 = host.glasso_problem(spd(4), 5)
    assert P1.reg_params == {'lambda1': None, 'mu1': None}
    assert sorted(P1.modelselect_params) == ['lambda1_mask', 'lambda1_range', 'mu1_range']
    assert np.array_equal(P1.modelselect_params['lambda1_range'], np.logspace(0, -3, 10))
    assert P1.modelselect_params['mu1_range'] is None and P1.modelselect_params['lambda1_mask'] is None
    assert P1._default_solver_params() == {'verbose': False, 'measure': False, 'rho': 1., 'max_iter': 1000, 'update_rho': True}
    P3 = host.glasso_problem(spd(4, K=2), 5, latent=True)
    assert P3.reg_params == {'lambda1': None, 'lambda2': None, 'mu1': None}
    assert np.array_equal(P3.modelselect_params['lambda2_range'], np.logspace(-1, -4, 5))
    assert np.array_equal(P3.modelselect_params['mu1_range'], np.logspace(2, -1, 10))
    assert 'lambda1_mask' not in P3.modelselect_params
    assert P3._default_start_point().shape == (2, 4, 4)
    Pn = host.glasso_problem([spd(4), spd(4, 1)], 5, G=trivial_G(4, 2))
    assert 'update_rho' not in Pn._default_solver_params()                 # ext_ADMM_MGL has no such argument
    assert sorted(Pn._default_start_point()) == [0, 1]


def test_set_reg_params_merges_and_repr(host):
    P = host.glasso_problem(spd(4, K=2), 5, reg="FGL", reg_params={'lambda1': 0.3}, latent=True)
    P.set_reg_params({'lambda2': 0.1})
    P.set_reg_params()
    assert P.reg_params == {'lambda1': 0.3, 'lambda2': 0.1, 'mu1': None}
    with pytest.raises(AssertionError):
        P.set_reg_params([('lambda1', 1)])
    assert repr(P) == " \nFUSED GRAPHICAL LASSO PROBLEM WITH LATENT VARIABLES\nRegularization parameters:\n" + str(P.reg_params)
    assert repr(host.glasso_problem(spd(4, K=2), 5)).startswith(" \nGROUP GRAPHICAL LASSO PROBLEM \n")
    assert repr(host.glasso_problem(spd(4), 5)).startswith(" \nSINGLE GRAPHICAL LASSO PROBLEM \n")
    with pytest.warns(UserWarning, match="No grid for model selection is specified"):
        P.set_modelselect_params()
    P.set_modelselect_params({'lambda1_range': np.array([0.5])})
    assert np.array_equal(P.modelselect_params['lambda1_range'], [0.5]) and 'lambda2_range' in P.modelselect_params


def test_do_scaling_warnings_and_scale(host):
    S = spd(5, K=2) * 7.0
    with pytest.warns(UserWarning) as rec:
        P = host.glasso_problem(S, 50, do_scaling=True)
    msgs = [str(w.message) for w in rec]
    assert msgs[0].startswith("NOTE: Input data S is rescaled to correlations")
    assert msgs[1].startswith("The output/solution is rescaled to covariances.")
    # a (K,p,p) stack: the reference's list of np.diag VIEWS is overwritten when it scales S in place, so its _scale is all
    # ones and its solution stays on the correlations' scale; the class reproduces that and keeps the variances beside it
    assert isinstance(P._scale, list) and all(np.array_equal(P._scale[k], np.ones(5)) for k in range(2))
    assert all(np.array_equal(P._variances[k], np.diag(S[k])) for k in range(2))
    assert np.allclose(np.diagonal(P.S, axis1=1, axis2=2), 1.0) and np.array_equal(P.solution.sample_covariance_, S)
    with pytest.warns(UserWarning):
        P1 = host.glasso_problem(S[0], 50, do_scaling=True)
    assert np.array_equal(P1._scale, np.diag(S[0]))


def test_block_sgl_gets_tol_as_rtol(host, monkeypatch):
    from gglasso_amd import solver
    seen = {}

    def fake(**kw):
        seen.update(kw)
        return {'Omega': np.eye(4), 'Theta': np.eye(4), 'X': np.zeros((4, 4))}
    monkeypatch.setattr(solver, "block_SGL", fake)
    P = host.glasso_problem(spd(4), 5, reg_params={'lambda1': 0.2})
    P.solve(tol=3e-6, rtol=9e-3, solver_params={'rho': 2.0}, verbose=False)
    assert seen['tol'] == 3e-6 and seen['rtol'] == 3e-6                    # problem.py:447 of the reference
    assert seen['rho'] == 2.0 and seen['max_iter'] == 1000 and seen['update_rho'] is True and seen['lambda1_mask'] is None
    assert P.solver_info == {} and np.array_equal(P.solution.precision_, np.eye(4))
    assert not P.solution.adjacency_.any() and P.solution.lowrank_ is None


def test_fixture_solves_case1_and_case3(host, golden):
    g = golden("g21_problem")
    tol = float(g["tol"])
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        P = host.glasso_problem(g["c1_S"], int(g["c1_N"]), reg_params={'lambda1': float(g["c1_lambda1"])}, do_scaling=True)
        P.solve(tol=tol, rtol=tol)
    assert np.allclose(P._scale, g["c1_scale"], rtol=1e-15, atol=0)
    assert np.linalg.norm(P.solution.precision_ - g["c1_solve_precision"]) <= 2e-7
    assert np.array_equal(P.solution.adjacency_, g["c1_solve_adjacency"])
    assert abs(P.solution.calc_ebic(0.5) - float(g["c1_solve_ebic05"])) <= 1e-7 * abs(float(g["c1_solve_ebic05"])) + 1e-5
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        P = host.glasso_problem(g["c3_S"], g["c3_N"], reg="GGL", do_scaling=True,
                                reg_params={'lambda1': float(g["c3_lambda1"]), 'lambda2': float(g["c3_lambda2"])})
        P.solve(tol=tol, rtol=tol)
    assert np.allclose(np.stack(P._scale), g["c3_scale"], rtol=0, atol=4 * 2.0 ** -53)     # ones, up to the reference's rounding
    assert np.linalg.norm(P.solution.precision_ - g["c3_solve_precision"]) <= 5e-7
    assert np.array_equal(P.solution.adjacency_, g["c3_solve_adjacency"])
    assert P.solver_info['status'] == 'optimal'


def test_sample_covariance_argument_handling(monkeypatch):
    from gglasso_amd import utils
    calls = []

    def stub(Xs, flags, device=0):
        calls.append(([x.shape for x in Xs], flags))
        assert all(x.flags['C_CONTIGUOUS'] and x.dtype == np.float64 for x in Xs)
        return ph.covariance_call_numpy(Xs, flags)
    monkeypatch.setattr(utils, "_covariance_call", stub)
    rng = np.random.default_rng(0)
    X = rng.standard_normal((3, 4, 9))
    S = utils.sample_covariance(X)
    assert S.shape == (3, 4, 4) and np.allclose(S[1], np.cov(X[1], bias=True)) and calls == [([(4, 9)] * 3, 1)]
    S2 = utils.sample_covariance(np.asfortranarray(X[0]), center=False)
    assert S2.shape == (4, 4) and np.allclose(S2, X[0] @ X[0].T / 9) and calls[-1] == ([(4, 9)], 0)
    calls.clear()
    ragged = {0: rng.standard_normal((4, 5)), 1: rng.standard_normal((6, 7)), 2: rng.standard_normal((4, 8))}
    Sd, var = utils.sample_covariance(ragged, scale=True)
    assert calls == [([(4, 5), (4, 8)], 3), ([(6, 7)], 3)]                  # one call per distinct p_k
    assert sorted(Sd) == [0, 1, 2] and Sd[1].shape == (6, 6) and var[2].shape == (4,)
    assert np.allclose(var[1], np.var(ragged[1], axis=1)) and np.allclose(np.diag(Sd[2]), 1.0)
    Sl = utils.sample_covariance([ragged[0], ragged[1]])
    assert isinstance(Sl, dict) and sorted(Sl) == [0, 1]
    with pytest.raises(AssertionError, match="keys 0,...,K-1"):
        utils.sample_covariance({1: ragged[0], 2: ragged[1]})
    with pytest.raises(AssertionError, match=r"use \(p,N\), \(K,p,N\)"):
        utils.sample_covariance(np.zeros(5))


def test_estimator_ebic_of_instances_of_different_dimension(host, golden):
    """calc_ebic over a dict: the reference's value at the reference's own estimate (fixture case 5)."""
    g = golden("g21_problem")
    S = [g[f"c5_S_{k}"] for k in range(3)]
    P = host.glasso_problem(S, g["c5_N"], G=g["c5_G"].astype(int))
    P.solution._set_solution(Theta={k: g[f"c5_solve_precision_{k}"] for k in range(3)})
    assert all(np.array_equal(P.solution.adjacency_[k], g[f"c5_solve_adjacency_{k}"]) for k in range(3))
    want = float(g["c5_solve_ebic05"])
    assert abs(P.solution.calc_ebic(0.5) - want) <= 1e-12 * abs(want)


def test_engine_set_data_then_steps_as_from_S():
    """HipEngine.set_data / get_S as the oracle engine of these tests has them: S from data, then the same iterates."""
    rng = np.random.default_rng(2)
    X = [rng.standard_normal((6, n)) * 3.0 + 5.0 for n in (9, 20)]
    eye = np.stack([np.eye(6)] * 2)
    eng = ph.DataOracleEngine(eye, eye, eye, 0 * eye)
    eng.set_data(X)
    S = eng.get_S()
    assert np.allclose(S, np.stack([np.cov(x, bias=True) for x in X]), rtol=1e-13, atol=0)
    ref = ph.DataOracleEngine(S, eye, eye, 0 * eye)
    for _ in range(3):
        a, b = eng.step(1.0, 0.1, 0.05, 'GGL', False, None, None), ref.step(1.0, 0.1, 0.05, 'GGL', False, None, None)
        assert np.array_equal(a, b)
    assert all(np.array_equal(u, v) for u, v in zip(eng.state(), ref.state()))
    eng.set_data(np.stack([x[:, :9] for x in X]), N=9, scale=True)
    C, var = eng.get_S()
    assert np.allclose(np.diagonal(C, axis1=1, axis2=2), 1.0) and np.allclose(var[1], np.var(X[1][:, :9], axis=1))
    with pytest.raises(AssertionError):
        eng.set_data(X[:1])


def test_from_data(host):
    rng = np.random.default_rng(1)
    X = rng.standard_normal((3, 5, 40))
    P = host.glasso_problem.from_data(X, reg="FGL")
    assert P.multiple and P.reg == "FGL" and np.array_equal(P.N, [40, 40, 40])
    assert np.allclose(P.S[2], np.cov(X[2], bias=True))
    P1 = host.glasso_problem.from_data(X[0], latent=True)
    assert not P1.multiple and P1.N == 40 and P1.latent
    with pytest.raises(TypeError):
        host.glasso_problem.from_data(X, "FGL")                             # keyword-only
