#!/usr/bin/env python3
"""
G22: the KKT stopping criterion of the REAL reference on a state that is NOT an ADMM iterate, generated like make_golden.py by
importing the reference in the build container.  G9 / G10 pin one GGL and one SGL value, both non-latent and both on an iterate,
where two of the four terms vanish by construction; here every term is of order 1e-2 .. 1e-1.

  state    K = 3, p = 12: three iterations of the reference's latent ADMM_MGL from the identity, then independent symmetric
           Gaussian noise of standard deviation 0.03 on Omega, Theta, L and X (X is the UNscaled dual the function takes)
  mgl_*    kkt_stopping_criterion (solver/admm_solver.py:333-371) for GGL and FGL, latent (the state's L, unequal mu1) and not
           latent (L = 0), unequal nk
  sgl_*    kkt_stopping_criterion (solver/single_admm_solver.py:293-320) on instance 0: plain, with an array lambda1
           (lambda1 * lambda1_mask), latent
  *_terms  the four terms behind each value, formed here with the reference's own operators (ggl_helper.py: prox_p,
           prox_od_1norm, phiplus, prox_rank_norm) exactly as the function forms them; their maximum IS the function's value
           (asserted).  The maximum alone cannot tell GGL from FGL or a scalar from an array lambda1 when term 1 is not the
           largest; the terms can.

    python tests/golden/make_golden_kkt.py
"""
import numpy as np

import make_golden as mg


def terms_mgl(gh, Om, Th, L, X, S, l1, l2, nk, reg, latent, mu1):
    nrm = np.linalg.norm
    K = S.shape[0]
    D, Q = np.linalg.eigh(Om - nk * S - X)
    t = [nrm(Th - gh.prox_p(Th + X, l1=l1, l2=l2, reg=reg)) / (1 + nrm(Th)), nrm(Th - Om - L) / (1 + nrm(Th)),
         nrm(Om - np.stack([gh.phiplus(beta=nk[k, 0, 0], D=D[k], Q=Q[k]) for k in range(K)])) / (1 + nrm(Om)), 0.0]
    if latent:
        D, Q = np.linalg.eigh(L - X)
        t[3] = nrm(L - np.stack([gh.prox_rank_norm(L[k] - X[k], beta=mu1[k], D=D[k], Q=Q[k]) for k in range(K)])) / (1 + nrm(L))
    return np.array(t)


def terms_sgl(gh, Om, Th, L, X, S, l1, latent, mu1):
    nrm = np.linalg.norm
    D, Q = np.linalg.eigh(Om - S - X)
    t = [nrm(Th - gh.prox_od_1norm(Th + X, l=l1)) / (1 + nrm(Th)), nrm(Om - Th + L) / (1 + nrm(Th)),
         nrm(Om - gh.phiplus(beta=1, D=D, Q=Q)) / (1 + nrm(Om)), 0.0]
    if latent:
        D, Q = np.linalg.eigh(L - X)
        t[3] = nrm(L - gh.prox_rank_norm(A=L - X, beta=mu1, D=D, Q=Q)) / (1 + nrm(L))
    return np.array(t)


def main():
    admm, sadmm, gh, fh, dg, utils = mg._import_reference()
    rng = np.random.default_rng(20261018)
    K, p = 3, 12
    A = rng.standard_normal((K, p, 4 * p))
    S = A @ A.transpose(0, 2, 1) / (4 * p)
    S = 0.5 * (S + S.transpose(0, 2, 1))
    l1, l2 = 0.05, 0.02
    nk = (1.0 + 0.25 * np.arange(K)).reshape(K, 1, 1)
    mu1 = 0.1 + 0.05 * np.arange(K)
    Om0 = np.stack([np.eye(p)] * K)
    sol, _ = mg.quiet(admm.ADMM_MGL, S, l1, l2, 'GGL', Om0, max_iter=3, tol=1e-20, rtol=1e-20, update_rho=False, latent=True,
                      mu1=mu1)

    def noisy(M):
        E = 0.03 * rng.standard_normal((K, p, p))
        return 0.5 * (M + M.transpose(0, 2, 1)) + (E + E.transpose(0, 2, 1)) / np.sqrt(2.0)

    Om, Th, L, X = (noisy(sol[nm]) for nm in ('Omega', 'Theta', 'L', 'X'))
    mask = rng.uniform(0.5, 1.5, (p, p))
    mask = l1 * 0.5 * (mask + mask.T)
    out = dict(S=S, Omega=Om, Theta=Th, L=L, X=X, nk=nk, mu1=mu1, params=np.array([l1, l2]), sgl_lambda1_array=mask)
    Z = np.zeros((K, p, p))
    for reg in ('GGL', 'FGL'):
        out[f"mgl_{reg}_nol"] = np.array(admm.kkt_stopping_criterion(Om, Th, Z, X, S, l1, l2, nk, reg))
        out[f"mgl_{reg}_lat"] = np.array(admm.kkt_stopping_criterion(Om, Th, L, X, S, l1, l2, nk, reg, latent=True, mu1=mu1))
    z = np.zeros((p, p))
    out["sgl_plain"] = np.array(sadmm.kkt_stopping_criterion(Om[0], Th[0], z, X[0], S[0], l1))
    out["sgl_array"] = np.array(sadmm.kkt_stopping_criterion(Om[0], Th[0], z, X[0], S[0], mask))
    out["sgl_lat"] = np.array(sadmm.kkt_stopping_criterion(Om[0], Th[0], L[0], X[0], S[0], l1, latent=True, mu1=0.15))
    for reg in ('GGL', 'FGL'):
        out[f"mgl_{reg}_nol_terms"] = terms_mgl(gh, Om, Th, Z, X, S, l1, l2, nk, reg, False, None)
        out[f"mgl_{reg}_lat_terms"] = terms_mgl(gh, Om, Th, L, X, S, l1, l2, nk, reg, True, mu1)
    out["sgl_plain_terms"] = terms_sgl(gh, Om[0], Th[0], z, X[0], S[0], l1, False, None)
    out["sgl_array_terms"] = terms_sgl(gh, Om[0], Th[0], z, X[0], S[0], mask, False, None)
    out["sgl_lat_terms"] = terms_sgl(gh, Om[0], Th[0], L[0], X[0], S[0], l1, True, 0.15)
    for k in [k for k in out if k.endswith("_terms")]:
        assert out[k].max() == float(out[k[:-6]]), k
        print(k, out[k])
    for k in sorted(out):
        if out[k].ndim == 0:
            print(k, float(out[k]))
    mg.save("g22_kkt_terms", **out)


if __name__ == "__main__":
    main()
