"""Shared by the FSGL tests: loading the G20 fixtures (tests/golden/make_golden_fsgl.py; symmetric matrices are stored as
their packed upper triangle) and an independent NumPy statement of the operators."""
import numpy as np

from conftest import load_golden


def unpack(t):
    """(…, n(n+1)/2) packed upper triangle -> (…, n, n) symmetric."""
    t = np.asarray(t)
    n = int(round((np.sqrt(8 * t.shape[-1] + 1) - 1) / 2))
    A = np.zeros(t.shape[:-1] + (n, n))
    iu = np.triu_indices(n)
    A[..., iu[0], iu[1]] = t
    A[..., iu[1], iu[0]] = t
    return A


def case(tag):
    """dict of one solved case: p, M, S, lmax, lams (absolute), and per lambda Theta / iters / status / residual (/ L, rankL)."""
    g = load_golden("g20_fsgl" if tag == "A" else f"g20_fsgl_{tag}")
    p, M, _ = (int(v) for v in g[f"{tag}_pM"])
    lmax = float(g[f"{tag}_lmax"])
    out = dict(p=p, M=M, S=unpack(g[f"{tag}_S"]), lmax=lmax, lams=[float(f) * lmax for f in g[f"{tag}_lams"]],
               frob=g[f"{tag}_frob"], frob_od=g[f"{tag}_frob_od"], runs=[])
    for i in range(len(out["lams"])):
        run = dict(Theta=unpack(g[f"{tag}_Theta{i}"]), iters=int(g[f"{tag}_iters{i}"]), status=str(g[f"{tag}_status{i}"]),
                   residual=g[f"{tag}_residual{i}"], nz=int(g[f"{tag}_nz{i}"]))
        if f"{tag}_L{i}" in g.files:
            run.update(L=unpack(g[f"{tag}_L{i}"]), rankL=int(g[f"{tag}_rankL{i}"]), mu1=float(g[f"{tag}_mu1"]))
        out["runs"].append(run)
    return out


def trajectory(tag):
    """{'Theta','Omega','X'[,'L']}: (8,pM,pM) iterates of the first 8 iterations at tol = rtol = 1e-20."""
    if tag == "A":
        g = load_golden("g20_fsgl")
        return {nm: unpack(g[f"A_traj_{nm}"]) for nm in ("Theta", "Omega", "X")}
    return {nm: unpack(load_golden(f"g20_fsgl_{tag}traj_{nm}")[f"{tag}_traj_{nm}"]) for nm in ("Theta", "Omega", "X", "L")}


def operator_cases():
    g = load_golden("g20_fsgl_ops")
    for n in range(int(g["n_ops"])):
        M, l = g[f"op{n}_Ml"]
        yield n, g[f"op{n}_X"], int(M), float(l), g[f"op{n}_Y"]


def block_norms(X, M):
    """(p,p) Frobenius norms of the M x M blocks: reshape to (p,M,p,M), norms over axes 1 and 3."""
    p = X.shape[0] // M
    return np.sqrt((X.reshape(p, M, p, M) ** 2).sum(axis=(1, 3)))


def prox_sum_frob_np(X, M, l):
    """prox of l * sum_{I != J} |X_IJ|_F, vectorised: the upper blocks decide, the lower ones are their transposes, the
    diagonal blocks pass through."""
    p = X.shape[0] // M
    B = X.reshape(p, M, p, M)
    a = np.maximum(block_norms(X, M), l)
    up = np.triu(np.ones((p, p), dtype=bool), 1)
    U = np.where(up[:, None, :, None], B * ((a - l) / a)[:, None, :, None], 0.0).reshape(p * M, p * M)
    D = np.where(np.eye(p, dtype=bool)[:, None, :, None], B, 0.0).reshape(p * M, p * M)
    return U + U.T + D
