"""One SHA-1 per array the GGL Theta-step leaves behind, for "same bits before and after" checks of a change to the GGL kernels
of ``csrc/theta_pair.hip``: run it from two checkouts, each with its own built library, and compare the listings byte for byte
(profiles/theta_one_body.txt).

    python tools/theta_identity.py > listing.txt

* every GGL case of tests/theta_step_ref.py ``CASES`` (``HipEngine.step`` and ``mgl_batch_step``; every GGL dispatch code, latent
  and batched routes included): one iteration from the case's start, then Omega, Theta, X, L and the sums it returned;
* ``ops.prox_p(V, l1, l2, 'GGL')`` (no dual, no C) at (K, p) = (9,17), (33,15), (65,11), (129,181);
* the K-sharded route, whose Theta kernels take the all-reduced group sums: ``ADMM_MGL_sharded`` with ``RcclComm()`` at world
  size 1, three iterations, at (K, p) = (9,17), (33,15), (65,11): the state and the residual history.
A line is ``route case key dtype shape sha1``; the step lines carry the dispatch code in the route."""
import contextlib
import hashlib
import io
import os
import socket
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))


def show(route, case, out):
    for key in sorted(out):
        a = np.ascontiguousarray(out[key])
        print(route, case, key, a.dtype, "x".join(str(n) for n in a.shape) or "-", hashlib.sha1(a.tobytes()).hexdigest(), flush=True)


def step_case(c):
    import theta_step_ref as tsr
    from gglasso_amd import solver
    b = tsr.build_case(c)
    eng = solver.HipEngine(b["S"], b["Omega_0"], b["Theta_0"], b["X_0"], b["L_0"], options=c.opts)
    try:
        if c.kind == "step":
            eng.hint_last_step()
            sq = eng.step(float(b["rho"]), float(b["lambda1"]), float(b["lambda2"]), c.reg, c.latent, b["mu1"], np.ones(c.K)).copy()
        else:
            sq = eng.mgl_batch_step(c.G, b["rho"], b["lambda1"], b["lambda2"], c.reg, c.latent, b["mu1"], None)
        st = eng.state()
        code = eng.last_dispatch()["theta_kernel"]
    finally:
        eng.close()
    if not c.latent:
        del st["L"]
    show(f"{c.kind}:{code}", c.name, {**st, "sums": sq})


def main():
    import torch.distributed as dist
    import theta_step_ref as tsr
    from gglasso_amd import ops, synth
    from gglasso_amd.dist import ADMM_MGL_sharded, RcclComm

    for c in tsr.CASES:
        if c.reg == "GGL":
            step_case(c)

    for K, p in ((9, 17), (33, 15), (65, 11), (129, 181)):
        V = tsr.sym(np.random.default_rng(900 + K).standard_normal((K, p, p)))
        show("prox_p", f"K{K}-p{p}", {"out": ops.prox_p(V, 0.3, 0.2 * np.sqrt(K), "GGL")})

    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    port = s.getsockname()[1]
    s.close()
    dist.init_process_group("gloo", init_method=f"tcp://127.0.0.1:{port}", rank=0, world_size=1)
    try:
        for K, p in ((9, 17), (33, 15), (65, 11)):
            S, _ = synth.make_problem("GGL", K, p, seed=700 + K)
            Om0 = np.repeat(np.eye(p)[None], K, axis=0)
            with contextlib.redirect_stdout(io.StringIO()):
                sol, info = ADMM_MGL_sharded(S, 0.05, 0.02, "GGL", Om0, K, RcclComm(), max_iter=3, tol=1e-20, rtol=1e-20)
            show("sharded", f"K{K}-p{p}", {**{nm: sol[nm] for nm in ("Omega", "Theta", "X")},
                                           "residual": np.asarray(info.get("residual", []), dtype=np.float64)})
    finally:
        dist.destroy_process_group()


if __name__ == "__main__":
    main()
