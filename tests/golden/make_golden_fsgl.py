"""Generates the G20 fixtures (Functional Single Graphical Lasso) from the REAL reference package: solver/functional_sgl_admm.py,
solver/ggl_helper.py:45-66 (prox_sum_Frob), helper/utils.py:69-107 (frob_norm_per_block, lambda_max_fsgl).

    python tests/golden/make_golden_fsgl.py

Writes g20_fsgl.npz (cases A and its trajectory, tables, tags), g20_fsgl_ops.npz (operator inputs / outputs) and one file per
larger case (g20_fsgl_B.npz ... g20_fsgl_F.npz, g20_fsgl_Ftraj_<stack>.npz): arrays and short tags only, every file under
1 MB.  Symmetric matrices are stored as their packed upper triangle (tests/fsgl_fixtures.py unpacks them).

A case is REFUSED when r_t or s_t lies within a relative 1e-6 of its threshold at the stopping iteration or the one before,
an operator input when a block norm lies within a relative 1e-9 of l: no test outcome hangs on rounding.
"""
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import make_golden as mg  # noqa: E402

_, _, ggl_helper, _, _, utils = mg._import_reference()
from gglasso.solver import functional_sgl_admm as fsgl  # noqa: E402

LIMIT = 1_000_000


def make_S(p, M, N, latent=False, seed=7):
    rng = np.random.default_rng(seed)
    pM = p * M
    adj = np.triu(rng.random((p, p)) < 3.0 / p, 1)
    Th = np.zeros((pM, pM))
    for i, j in zip(*np.nonzero(adj)):
        Th[i * M:(i + 1) * M, j * M:(j + 1) * M] = 0.3 * rng.standard_normal((M, M))
    Th = Th + Th.T
    Th += (0.5 - np.linalg.eigvalsh(Th).min()) * np.eye(pM)
    if latent:
        Bh = 0.25 * rng.standard_normal((pM, 3))
        Th = Th - Bh @ Bh.T
        mn = np.linalg.eigvalsh(Th).min()
        if mn < 0.3:
            Th += (0.3 - mn) * np.eye(pM)
    Sigma = np.linalg.inv(Th)
    Sigma = 0.5 * (Sigma + Sigma.T)
    X = rng.multivariate_normal(np.zeros(pM), Sigma, size=N, method="cholesky")
    return np.cov(X.T, bias=True)


def solve_recorded(S, lam, M, latent, mu1, tol, rtol, max_iter=1000):
    """The reference's ADMM_FSGL itself, with the four numbers of its stopping test (r_t, s_t, e_pri, e_dual) recorded at every
    iteration: the solver does not return them, and the margin check below needs them."""
    rows, orig = [], fsgl.ADMM_stopping_criterion

    def recording(*a, **k):
        out = orig(*a, **k)
        rows.append(out)
        return out

    fsgl.ADMM_stopping_criterion = recording
    try:
        sol, info = mg.quiet(fsgl.ADMM_FSGL, S, lam, M, np.eye(S.shape[0]), tol=tol, rtol=rtol, measure=True, latent=latent,
                             mu1=mu1, max_iter=max_iter)
    finally:
        fsgl.ADMM_stopping_criterion = orig
    return sol, info, np.array(rows)


def triu(A):
    return np.ascontiguousarray(A[np.triu_indices(A.shape[-1])])


def solve_case(tag, p, M, N, lams, latent=False, mu1=None, out=None):
    S = make_S(p, M, N, latent)
    pM = p * M
    out[f"{tag}_pM"] = np.array([p, M, N])
    out[f"{tag}_S"] = triu(S)
    out[f"{tag}_lams"] = np.array(lams)
    out[f"{tag}_frob"] = utils.frob_norm_per_block(S, M)
    out[f"{tag}_frob_od"] = utils.frob_norm_per_block(S, M, off_diag=True)
    lmax = utils.lambda_max_fsgl(S, M)
    out[f"{tag}_lmax"] = np.array(lmax)
    for i, f in enumerate(lams):
        lam = f * lmax
        sol, info, rows = solve_recorded(S, lam, M, latent, mu1, 1e-9, 1e-9)
        assert len(rows) == len(info['residual']) and np.array_equal(info['residual'], rows[:, :2].max(axis=1)), tag
        for row in rows[-2:]:
            r, s, ep, ed = row
            assert abs(r - ep) > 1e-6 * ep and abs(s - ed) > 1e-6 * ed, f"{tag}: stopping test within 1e-6 of its threshold"
        B = sol['Theta'].reshape(p, M, p, M)
        nz = np.count_nonzero(np.triu(np.sqrt((B ** 2).sum(axis=(1, 3))), 1))
        print(f"{tag} lam {f} lmax: {info['status']} after {len(rows)} its; {nz} of {p * (p - 1) // 2} blocks non-zero"
              + (f"; rank L {np.linalg.matrix_rank(sol['L'])}, eig {np.linalg.eigvalsh(sol['L'])[-3:]}" if latent else ""))
        out[f"{tag}_Theta{i}"] = triu(sol['Theta'])
        out[f"{tag}_iters{i}"] = np.array(len(rows))
        out[f"{tag}_status{i}"] = np.array(info['status'])
        out[f"{tag}_residual{i}"] = info['residual']
        out[f"{tag}_nz{i}"] = np.array(nz)
        if latent:
            out[f"{tag}_L{i}"] = triu(sol['L'])
            out[f"{tag}_rankL{i}"] = np.array(np.linalg.matrix_rank(sol['L']))
            out[f"{tag}_mu1"] = np.array(mu1)
    return S, lmax


def trajectory(S, lam, M, latent, mu1):
    """Iterates 1..8 at tol = rtol = 1e-20: the reference solver stopped after 1, 2, ... 8 iterations."""
    sols = [solve_recorded(S, lam, M, latent, mu1, 1e-20, 1e-20, max_iter=it)[0] for it in range(1, 9)]
    return {nm: np.stack([triu(sl[nm] if nm in sl else np.zeros_like(S)) for sl in sols]) for nm in ("Theta", "Omega", "X", "L")}


def op_fixtures():
    rng = np.random.default_rng(7)
    out, n = {}, 0
    #          M, p, kind        kinds: 0 threshold inside the block norms, 1 above all, 2 below all; asym: lower != upper
    plan = [(1, 17, 0), (2, 13, 0), (3, 11, 0), (5, 8, 0), (8, 6, 0), (16, 4, 0), (32, 3, 0), (33, 3, 0), (40, 2, 0),
            (5, 13, 1), (5, 13, 2), (33, 2, 1), (40, 2, 2), (1, 40, 1), (2, 33, 2), (3, 23, 0), (8, 9, 0), (16, 5, 0),
            (32, 2, 0), (5, 7, 0)]
    for n, (M, p, kind) in enumerate(plan):
        pM = M * p
        A = rng.standard_normal((pM, pM))
        X = A + A.T
        if n % 2 == 1:
            X = X + np.tril(0.1 * rng.standard_normal((pM, pM)), -1)      # the lower triangle differs from the upper
        norms = np.sqrt((X.reshape(p, M, p, M) ** 2).sum(axis=(1, 3)))[np.triu_indices(p, 1)]
        l = {0: float(np.median(norms)) * 1.0001 if len(norms) > 1 else 0.5 * norms[0], 1: 1.5 * norms.max(),
             2: 0.5 * norms.min()}[kind]
        assert np.all(np.abs(norms - l) > 1e-9 * l), "a block norm within 1e-9 of the threshold"
        out[f"op{n}_X"], out[f"op{n}_Y"] = X, ggl_helper.prox_sum_Frob(X, M, l)
        out[f"op{n}_Ml"] = np.array([M, l])
    out["n_ops"] = np.array(len(plan))
    return out


OUT = HERE       # --out DIR: write somewhere else (to compare a regeneration with the committed files)


def save(name, arrays):
    path = os.path.join(OUT, name + ".npz")
    np.savez_compressed(path, **arrays)
    size = os.path.getsize(path)
    print(f"wrote {name}.npz: {size} bytes")
    assert size < LIMIT, f"{name}.npz is {size} bytes"


def main():
    main_out = {}
    S, lmax = solve_case("A", 12, 5, 600, (0.1, 0.3), out=main_out)
    for nm, A in trajectory(S, 0.1 * lmax, 5, False, None).items():
        main_out[f"A_traj_{nm}"] = A
    save("g20_fsgl", main_out)
    save("g20_fsgl_ops", op_fixtures())
    for tag, p, M, N, lams in (("B", 30, 5, 1500, (0.1, 0.3)), ("C", 67, 3, 2000, (0.1, 0.3)), ("D", 40, 8, 3000, (0.3,)),
                               ("E", 4, 33, 3000, (0.1, 0.3))):
        o = {}
        solve_case(tag, p, M, N, lams, out=o)
        save(f"g20_fsgl_{tag}", o)
    o = {}
    S, lmax = solve_case("F", 30, 5, 1500, (0.1,), latent=True, mu1=0.3, out=o)
    save("g20_fsgl_F", o)
    for nm, A in trajectory(S, 0.1 * lmax, 5, True, 0.3).items():
        save(f"g20_fsgl_Ftraj_{nm}", {f"F_traj_{nm}": A})


if __name__ == "__main__":
    if "--out" in sys.argv:
        OUT = sys.argv[sys.argv.index("--out") + 1]
        os.makedirs(OUT, exist_ok=True)
    main()
