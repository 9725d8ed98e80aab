#!/usr/bin/env python3
"""
G19: the seams of the drop-in check (tests/test_reference_dropin.py), generated like make_golden.py by importing the REAL
reference in the build container.  Each scenario runs one of the reference's drivers with the reference's own function at
the seam SURVEY.md section 8(b) names, wrapped by tests/seam_calls.Recorder: every call the driver makes there is kept with
its arguments (warm starts as references to earlier returns) and the reference's return.  The test replays the calls
through gglasso_amd's functions, which is what the one-line import swap of a maintainer amounts to.

  seam1_grid        grid_search(solver=ADMM_MGL) (helper/model_selection.py:55,222): the ADMM_MGL calls
  seam2_problem     glasso_problem.solve() (problem.py:10-11), GGL / FGL x latent, and the single problem (block_SGL /
                    ADMM_SGL): the solver calls
  seam2_drawn       glasso_problem.solve() on sixty drawn configurations: the solver calls
  seam2_single      single_grid_search (model_selection.py:505) with use_block: the block_SGL / ADMM_SGL calls
  seam2_ext         glasso_problem.solve() with a dict S and G (problem.py:12,468): the ext_ADMM_MGL calls
  seam3a            glasso_problem.model_selection() of a single problem (problem.py:606): the single_grid_search calls
  seam3b            glasso_problem.model_selection() of a GGL problem (problem.py:626-654): the K_single_grid / grid_search
                    calls
  seam1_rank        grid_search(solver=ADMM_MGL) on G18's latent p = 160 problem: the ADMM_MGL calls, S by reference to
                    G18, no returns (the test checks G18's RANK / SP tables)

    python tests/golden/make_golden_dropin.py
"""
import os
import sys

import numpy as np

import make_golden as mg

sys.path.insert(0, os.path.dirname(mg.HERE))                         # tests/: seam_calls
sys.path.insert(0, os.path.dirname(os.path.dirname(mg.HERE)))        # the repository: gglasso_amd
import seam_calls  # noqa: E402


def main():
    mg._import_reference()
    import gglasso.problem as problem
    import gglasso.helper.model_selection as ms
    import gglasso.helper.data_generation as dg
    import gglasso.helper.ext_admm_helper as eh
    import pandas as pd
    arrays, meta = {}, {}
    quiet = mg.quiet

    # seam1_grid
    rec = seam_calls.Recorder()
    K, p, N = 3, 20, 200
    Sig, _ = dg.group_power_network(p, K=K, M=2, seed=7)
    S, _ = dg.sample_covariance_matrix(Sig, N, seed=7)
    quiet(ms.grid_search, rec.wrap("ADMM_MGL", problem.ADMM_MGL), S, np.array([N] * K), p, 'GGL', np.logspace(-1, -2, 3),
          np.logspace(-1, -2, 2), method='eBIC', gamma=0.3, tol=1e-8, rtol=1e-8)
    rec.save("seam1_grid", arrays, meta)

    def record_solvers(rec):
        for mod in (problem, ms):
            for name in ("ADMM_MGL", "ADMM_SGL", "block_SGL"):
                if hasattr(mod, name):
                    setattr(mod, name, rec.wrap(name, getattr(mod, name)))

    originals = {(mod, name): getattr(mod, name) for mod in (problem, ms)
                 for name in ("ADMM_MGL", "ADMM_SGL", "block_SGL", "ext_ADMM_MGL", "single_grid_search", "grid_search",
                              "K_single_grid") if hasattr(mod, name)}

    def restore():
        for (mod, name), fn in originals.items():
            setattr(mod, name, fn)

    # seam2_problem
    rec = seam_calls.Recorder()
    record_solvers(rec)
    K, p, N = 3, 20, 300
    Sig, _ = dg.time_varying_power_network(p, K=K, M=4, seed=9)
    S, _ = dg.sample_covariance_matrix(Sig, N, seed=9)
    for reg in ('GGL', 'FGL'):
        for latent in (False, True):
            P = problem.glasso_problem(S, N, reg=reg, reg_params={'lambda1': 0.05, 'lambda2': 0.02, 'mu1': 0.3},
                                       latent=latent, do_scaling=False)
            quiet(P.solve, tol=1e-9, rtol=1e-9)
    for latent in (False, True):
        P = problem.glasso_problem(S[0], N, reg=None, reg_params={'lambda1': 0.1, 'mu1': 0.4}, latent=latent,
                                   do_scaling=False)
        quiet(P.solve, tol=1e-9, rtol=1e-9)
    rec.save("seam2_problem", arrays, meta)
    restore()

    # seam2_drawn: sixty drawn configurations (single / GGL / FGL, K = 2 .. 5, p = 6 .. 24, latent, do_scaling); S from
    # gglasso_amd.synth, which the test draws again: stored by name where the solver received it unchanged or as correlations
    rec = seam_calls.Recorder(known=seam_calls.drawn_known())
    record_solvers(rec)
    for c in seam_calls.drawn_configurations():
        P = problem.glasso_problem(c["S"], c["N"], reg=c["reg"], reg_params=dict(c["params"]), latent=c["latent"],
                                   do_scaling=c["scaling"])
        quiet(P.solve, tol=1e-9, rtol=1e-9)
    rec.save("seam2_drawn", arrays, meta)
    restore()

    # seam2_single
    rec = seam_calls.Recorder()
    record_solvers(rec)
    p, N = 20, 200
    Sig, _ = dg.generate_precision_matrix(p=p, M=2, style='erdos', prob=0.2, seed=11)
    S, _ = dg.sample_covariance_matrix(Sig, N, seed=11)
    quiet(ms.single_grid_search, S, np.logspace(0, -2, 5), N, method='eBIC', gamma=0.3, latent=False, use_block=True,
          tol=1e-8, rtol=1e-8)
    rec.save("seam2_single", arrays, meta)
    restore()

    # seam2_ext (reference tests/test_problem.py:117-138)
    rec = seam_calls.Recorder()
    problem.ext_ADMM_MGL = rec.wrap("ext_ADMM_MGL", problem.ext_ADMM_MGL)
    rng = np.random.default_rng(5)
    K, N = 4, 200
    all_obs, S = {}, {}
    for k in range(K):
        X = rng.random((5 + k, N))
        all_obs[k] = pd.DataFrame(X)
        S[k] = np.cov(X, bias=True)
    ix_exist, ix_location = eh.construct_indexer(list(all_obs.values()))
    G = quiet(eh.create_group_array, ix_exist, ix_location, 2)
    for latent in (False, True):
        P = problem.glasso_problem(S={k: v.copy() for k, v in S.items()}, N=N, reg="GGL", latent=latent, G=G,
                                   reg_params={'lambda1': 0.01, 'lambda2': 0.001, 'mu1': 0.05}, do_scaling=True)
        quiet(P.solve, tol=1e-9, rtol=1e-9)
    rec.save("seam2_ext", arrays, meta)
    restore()

    # seam3a
    rec = seam_calls.Recorder()
    problem.single_grid_search = rec.wrap("single_grid_search", problem.single_grid_search)
    p, N = 20, 200
    Sig, _ = dg.generate_precision_matrix(p=p, M=2, style='erdos', prob=0.2, seed=13)
    S, _ = dg.sample_covariance_matrix(Sig, N, seed=13)
    for latent in (False, True):
        P = problem.glasso_problem(S, N, reg=None, latent=latent, do_scaling=False)
        P.set_modelselect_params({'lambda1_range': np.logspace(0, -2, 5), 'mu1_range': np.array([1.0, 0.4])})
        quiet(P.model_selection, method='eBIC', gamma=0.3, tol=1e-9, rtol=1e-9)
    rec.save("seam3a", arrays, meta)
    restore()

    # seam3b
    rec = seam_calls.Recorder()
    for name in ("grid_search", "K_single_grid"):
        setattr(problem, name, rec.wrap(name, getattr(problem, name)))
    K, p, N = 3, 16, 200
    Sig, _ = dg.group_power_network(p, K=K, M=2, seed=17)
    S, _ = dg.sample_covariance_matrix(Sig, N, seed=17)
    for latent in (False, True):
        P = problem.glasso_problem(S.copy(), N, reg='GGL', latent=latent, do_scaling=False)
        P.set_modelselect_params({'lambda1_range': np.logspace(-0.5, -1.5, 3), 'lambda2_range': np.array([0.1, 0.02]),
                                  'mu1_range': np.array([1.0, 0.4])})
        quiet(P.model_selection, method='eBIC', gamma=0.1, tol=1e-9, rtol=1e-9)
    rec.save("seam3b", arrays, meta)
    restore()

    # seam1_rank: G18's latent grid (make_golden_rank.py), S by reference
    g = np.load(os.path.join(mg.HERE, "g18_latent_rank_large_p.npz"))
    rec = seam_calls.Recorder(known={"mgl_S": g["mgl_S"]}, keep_returns=False)
    S = g["mgl_S"]
    quiet(ms.grid_search, rec.wrap("ADMM_MGL", problem.ADMM_MGL), S, g["grid_N"], S.shape[1], "GGL", g["grid_l1"],
          l2=g["grid_l2"], method='eBIC', gamma=0.3, latent=True, mu_range=g["grid_mu_range"], ix_mu=g["grid_ix_mu"],
          tol=1e-10, rtol=1e-10)
    rec.save("seam1_rank", arrays, meta)

    mg.save("g19_dropin_seams", __meta__=seam_calls.dump_meta(meta), **arrays)
    for name, calls in meta.items():
        print(f"  {name}: {len(calls)} calls")


if __name__ == "__main__":
    main()
