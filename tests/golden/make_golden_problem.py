"""Generates the G21 fixture (the ``glasso_problem`` front end) from the REAL reference package: problem.py with its
solvers and model-selection drivers.

    python tests/golden/make_golden_problem.py

Writes g21_problem.npz: for every case the observations X, the reference's S = numpy.cov(X, bias=True), N, the grids, the
regularization parameters after selection, precision_, lowrank_, adjacency_, the BIC / AIC / SP / RANK tables and
calc_ebic(0.5).  Arrays and short tag strings only.

Cases (all p = 20 or smaller):
  c1  SGL, do_scaling: solve at lambda1 = 0.1; model_selection over 4 lambda1
  c2  SGL latent: model_selection over 3 x 2 (lambda1 x mu1)
  c3  GGL, K = 3, do_scaling: solve; model_selection over a 3 x 2 grid
  c4  FGL latent, K = 3: model_selection, both stages
  c5  GGL over instances of dimension 8, 10, 12 with G from create_group_array: solve
"""
import os
import sys
import warnings

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import make_golden as mg  # noqa: E402

mg._import_reference()
from gglasso.problem import glasso_problem  # noqa: E402
from gglasso.helper.ext_admm_helper import construct_indexer, create_group_array  # noqa: E402

# both sides stop at r <= dim * TOL; the latent cases amplify that distance ~25x, 1e-11 keeps them inside the estimator bounds
TOL = 1e-11


def sparse_precision(rng, p, latent=0):
    A = np.triu((rng.random((p, p)) < 2.5 / p) * rng.uniform(0.25, 0.45, (p, p)) * rng.choice([-1.0, 1.0], (p, p)), 1)
    Th = A + A.T
    Th += (0.6 - np.linalg.eigvalsh(Th).min()) * np.eye(p)
    if latent:
        B = 0.35 * rng.standard_normal((p, latent))
        Th = Th - B @ B.T
        Th += max(0.0, 0.4 - np.linalg.eigvalsh(Th).min()) * np.eye(p)
    return Th


def draw(rng, Th, N, spread):
    """(p,N) observations of N(mean, Th^-1 scaled): variables of different variance and non-zero mean."""
    p = Th.shape[0]
    Sig = np.linalg.inv(Th)
    sd = rng.uniform(1.0, spread, p)
    Sig = Sig * np.outer(sd, sd)
    Z = np.linalg.cholesky(0.5 * (Sig + Sig.T)) @ rng.standard_normal((p, N))
    return Z + rng.uniform(-2.0, 2.0, (p, 1))


def tables(out, tag, P, gamma):
    st = P.modelselect_stats
    out[f"{tag}_BIC"] = np.asarray(st['BIC'][gamma], dtype=float)
    out[f"{tag}_AIC"] = np.asarray(st['AIC'], dtype=float)
    out[f"{tag}_SP"] = np.asarray(st['SP'], dtype=float)
    if 'RANK' in st and st['RANK'] is not None:
        out[f"{tag}_RANK"] = np.asarray(st['RANK'], dtype=float)
    out[f"{tag}_sel_lambda1"] = np.array(float(P.reg_params['lambda1']))
    if P.reg_params.get('lambda2') is not None:
        out[f"{tag}_sel_lambda2"] = np.array(float(P.reg_params['lambda2']))
    if P.reg_params.get('mu1') is not None:
        out[f"{tag}_sel_mu1"] = np.asarray(P.reg_params['mu1'], dtype=float)


def estimator(out, tag, P):
    sol = P.solution
    if isinstance(sol.precision_, dict):
        for k in sol.precision_:
            out[f"{tag}_precision_{k}"] = sol.precision_[k]
            out[f"{tag}_adjacency_{k}"] = sol.adjacency_[k]
    else:
        out[f"{tag}_precision"] = sol.precision_
        out[f"{tag}_adjacency"] = sol.adjacency_
    if sol.lowrank_ is not None:
        out[f"{tag}_lowrank"] = sol.lowrank_
    out[f"{tag}_ebic05"] = np.array(float(sol.calc_ebic(0.5)))


def main():
    warnings.simplefilter("ignore")
    rng = np.random.default_rng(20241018)
    out = {"gamma": np.array(0.1), "tol": np.array(TOL)}
    p, K = 20, 3

    # c1: SGL, do_scaling
    X = draw(rng, sparse_precision(rng, p), 200, 3.0)
    S = np.cov(X, bias=True)
    out.update(c1_X=X, c1_S=S, c1_N=np.array(200), c1_tag=np.array("SGL do_scaling"), c1_lambda1=np.array(0.1),
               c1_lambda1_range=np.array([0.5, 0.25, 0.12, 0.06]))
    P = glasso_problem(S, 200, reg_params={'lambda1': 0.1}, latent=False, do_scaling=True)
    mg.quiet(P.solve, tol=TOL, rtol=TOL)
    out["c1_scale"] = np.asarray(P._scale)
    estimator(out, "c1_solve", P)
    mg.quiet(P.model_selection, modelselect_params={'lambda1_range': out["c1_lambda1_range"]}, method='eBIC', gamma=0.1,
             tol=TOL, rtol=TOL)
    tables(out, "c1_ms", P, 0.1)
    estimator(out, "c1_ms", P)

    # c2: SGL latent
    X = draw(rng, sparse_precision(rng, p, latent=2), 300, 1.0)
    S = np.cov(X, bias=True)
    out.update(c2_X=X, c2_S=S, c2_N=np.array(300), c2_tag=np.array("SGL latent"),
               c2_lambda1_range=np.array([0.3, 0.15, 0.08]), c2_mu1_range=np.array([1.5, 0.6]))
    P = glasso_problem(S, 300, latent=True)
    mg.quiet(P.model_selection, modelselect_params={'lambda1_range': out["c2_lambda1_range"], 'mu1_range': out["c2_mu1_range"]},
             method='eBIC', gamma=0.1, tol=TOL, rtol=TOL)
    tables(out, "c2_ms", P, 0.1)
    estimator(out, "c2_ms", P)

    # c3: GGL, K = 3, do_scaling
    Th = sparse_precision(rng, p)
    Nk = np.array([150, 200, 250])
    X = [draw(rng, Th + 0.05 * k * np.eye(p), int(Nk[k]), 2.0) for k in range(K)]
    S = np.stack([np.cov(x, bias=True) for x in X])
    for k in range(K):
        out[f"c3_X_{k}"] = X[k]
    out.update(c3_S=S, c3_N=Nk, c3_tag=np.array("GGL do_scaling"), c3_lambda1=np.array(0.1), c3_lambda2=np.array(0.05),
               c3_lambda1_range=np.array([0.3, 0.15, 0.08]), c3_lambda2_range=np.array([0.1, 0.03]))
    P = glasso_problem(S, Nk, reg="GGL", reg_params={'lambda1': 0.1, 'lambda2': 0.05}, do_scaling=True)
    mg.quiet(P.solve, tol=TOL, rtol=TOL)
    out["c3_scale"] = np.stack(P._scale)
    estimator(out, "c3_solve", P)
    mg.quiet(P.model_selection, modelselect_params={'lambda1_range': out["c3_lambda1_range"],
                                                    'lambda2_range': out["c3_lambda2_range"]},
             method='eBIC', gamma=0.1, tol=TOL, rtol=TOL)
    tables(out, "c3_ms", P, 0.1)
    estimator(out, "c3_ms", P)

    # c4: FGL latent, K = 3
    Th = sparse_precision(rng, p, latent=2)
    Nk = np.array([300, 300, 300])
    X = np.stack([draw(rng, Th, 300, 1.0) for k in range(K)])
    S = np.stack([np.cov(x, bias=True) for x in X])
    out.update(c4_X=X, c4_S=S, c4_N=Nk, c4_tag=np.array("FGL latent"), c4_lambda1_range=np.array([0.3, 0.15, 0.08]),
               c4_lambda2_range=np.array([0.1, 0.03]), c4_mu1_range=np.array([1.5, 0.6]))
    P = glasso_problem(S, Nk, reg="FGL", latent=True)
    mg.quiet(P.model_selection, modelselect_params={'lambda1_range': out["c4_lambda1_range"],
                                                    'lambda2_range': out["c4_lambda2_range"],
                                                    'mu1_range': out["c4_mu1_range"]},
             method='eBIC', gamma=0.1, tol=TOL, rtol=TOL)
    tables(out, "c4_ms", P, 0.1)
    estimator(out, "c4_ms", P)
    out["c4_ix_mu"] = np.asarray(P._stage1_stats['ix_mu'])

    # c5: GGL over instances of different dimension
    import pandas as pd
    Th = sparse_precision(rng, 12)
    var_ix = [np.arange(0, 8), np.arange(2, 12), np.arange(0, 12)]
    Nk = np.array([120, 150, 180])
    frames, X = [], []
    for k in range(K):
        sub = np.linalg.inv(np.linalg.inv(Th)[np.ix_(var_ix[k], var_ix[k])])
        x = draw(rng, sub, int(Nk[k]), 1.0)
        X.append(x)
        frames.append(pd.DataFrame(x, index=var_ix[k]))
    ix_exist, ix_location = construct_indexer(frames)
    G = mg.quiet(create_group_array, ix_exist, ix_location)
    S = [np.cov(x, bias=True) for x in X]
    for k in range(K):
        out[f"c5_X_{k}"] = X[k]
        out[f"c5_S_{k}"] = S[k]
    out.update(c5_N=Nk, c5_G=G.astype(np.int64), c5_tag=np.array("GGL non-conforming"), c5_lambda1=np.array(0.1),
               c5_lambda2=np.array(0.05))
    P = glasso_problem(S, Nk, reg="GGL", reg_params={'lambda1': 0.1, 'lambda2': 0.05}, G=G)
    mg.quiet(P.solve, tol=TOL, rtol=TOL)
    estimator(out, "c5_solve", P)

    mg.save("g21_problem", **out)


if __name__ == "__main__":
    main()
