"""The skeptic matrix sin(pi/2 tau-b) from data: the int8 matrix-core kernel against a scipy loop on the host and against a
torch route on the same GPU, at the size of profiles/kendall_skeptic.txt.

    python tools/bench_kendall.py [--shape p,N,B] [--calls 5] [--part single,subsets] [--scipy-vars 50] [--kernel-only]

Two workloads, one JSON line each (whole-call times from the observations on the host to the matrices on the host; the routes
of a workload alternate, --calls rounds after one warm-up round, reported as median, min and max):

* single    one matrix of all N observations.
* subsets   the B subsample matrices of StARS (``model_selection.stars_subsamples``: b = int(10 sqrt(N))).

Routes:

* device    ``utils.skeptic_correlation``: dense ranks on the host, one upload, k_kendall_counts + k_kendall_skeptic.
* torch     the sign matrix Z materialised on the GPU in chunks of a-samples (float32) and multiplied with ``torch.matmul``;
            partial sums are exact in float32 (a chunk holds fewer than 2^24 pairs) and accumulated in float64.
* scipy     ``scipy.stats.kendalltau`` over the pairs of the first --scipy-vars variables of ONE subset on the host; the
            figure for all p (p - 1) / 2 pairs of all B subsets is SCALED from it by the number of calls
            (``scipy_scaled_ms``), not measured.

``--kernel-only`` makes --calls device calls of each workload and nothing else, for a run under ``rocprofv3 --kernel-trace
--stats``.  From the kernel's time there, the line ``model`` of the JSON gives what the two pipes need at least for the work
the kernel issues: matrix core, 16 cycles per v_mfma_i32_16x16x64_i8 (MI355X: the cycles of the bf16 form of the same M x N);
VALU, 4 cycles per wave instruction, 2.75 instructions per generated sign (subtract, v_med3_i32, 3/4 v_perm/v_or)."""
import argparse
import json
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from tools.bench_stars import alternate_ms, make_problem      # noqa: E402

SIMDS, CLOCK = 256 * 4, 2.4e9          # MI355X: 256 CUs of 4 SIMDs, peak engine clock


def kernel_model(p, n, B):
    """Least time of the matrix cores and of the VALU for the instructions k_kendall_counts issues (tile 64, one k = 64 step
    per a-sample and block of 64 b-samples; a diagonal tile pair builds one operand only)."""
    nT, nb = (p + 63) // 64, (n + 63) // 64
    steps = sum(min(bb * 64 + 63, n - 1) for bb in range(nb))                  # (a, b-block) steps of one tile pair
    off, diag = nT * (nT - 1) // 2, nT
    mfma = B * steps * (off + diag) * 16
    valu_instr = B * steps * (off * 8 + diag * 4) * 16 * 2.75                 # wave instructions
    return {"mfma": mfma, "mfma_pipe_ms": 1e3 * mfma * 16 / (SIMDS * CLOCK),
            "valu_sign_ms": 1e3 * valu_instr * 4 / (SIMDS * CLOCK)}


def torch_skeptic(X, idx=None, chunk_elems=1 << 26):
    """The torch yardstick: (B,p,p) skeptic matrices of the column subsets (idx None: all columns)."""
    import torch
    dev = torch.device("cuda")
    Xd = torch.from_numpy(X).to(dev)
    subsets = [Xd] if idx is None else [Xd[:, torch.from_numpy(idx[r].astype(np.int64)).to(dev)] for r in range(idx.shape[0])]
    out = []
    for Xr in subsets:
        p, n = Xr.shape
        G = torch.zeros((p, p), dtype=torch.float64, device=dev)
        rows = max(1, min(n - 1, chunk_elems // (p * n), (1 << 24) // n))
        ar = torch.arange(n, device=dev)
        for a0 in range(0, n - 1, rows):
            a = torch.arange(a0, min(n - 1, a0 + rows), device=dev)
            Z = torch.sign(Xr[:, a, None] - Xr[:, None, :]).to(torch.float32)
            Z = (Z * (ar[None, :] > a[:, None]).to(torch.float32)[None]).reshape(p, -1)
            G += (Z @ Z.T).to(torch.float64)
        d = torch.sqrt(torch.diagonal(G))
        S = torch.sin(np.pi / 2 * G / (d[:, None] * d[None, :]))
        S.fill_diagonal_(1.0)
        out.append(S)
    return torch.stack(out).cpu().numpy()


def scipy_slice(X, nvars, idx=None):
    from scipy.stats import kendalltau
    Xr = X if idx is None else X[:, idx[0]]
    for i in range(nvars):
        for j in range(i + 1, nvars):
            kendalltau(Xr[i], Xr[j], variant='b')


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--shape", default="500,2000,20", help="p,N,B")
    ap.add_argument("--calls", type=int, default=5)
    ap.add_argument("--part", default="single,subsets")
    ap.add_argument("--scipy-vars", type=int, default=50)
    ap.add_argument("--kernel-only", action="store_true", help="only device calls (for a profiler run)")
    args = ap.parse_args()
    from gglasso_amd import model_selection as ms, utils
    p, N, B = (int(v) for v in args.shape.split(","))
    # counts-like data: the chain-graph observations pushed through exp and rounded, so there are ties
    X = np.round(np.exp(make_problem(p, N)) * 4.0) / 4.0
    idx = ms.stars_subsamples(N, B)
    b = idx.shape[1]
    work = {"single": (None, N, 1), "subsets": (idx, b, B)}
    for part in args.part.split(","):
        sub, n, nB = work[part]
        shape = {"part": part, "p": p, "N": N, "B": nB, "b": n, "calls": args.calls}
        if args.kernel_only:
            for _ in range(args.calls):
                utils.skeptic_correlation(X, sub)
            print(json.dumps({**shape, "kernel_only": True, "model": kernel_model(p, n, nB)}), flush=True)
            continue
        S_dev = utils.skeptic_correlation(X, sub)
        S_t = torch_skeptic(X, sub)
        nv = min(args.scipy_vars, p)
        scale = nB * (p * (p - 1) / 2) / max(1, nv * (nv - 1) / 2)
        dev_ms, torch_ms, scipy_ms = alternate_ms([lambda: utils.skeptic_correlation(X, sub), lambda: torch_skeptic(X, sub),
                                                   lambda: scipy_slice(X, nv, sub)], args.calls)
        print(json.dumps({**shape, "device_ms": dev_ms, "torch_ms": torch_ms, "scipy_slice_vars": nv, "scipy_slice_ms": scipy_ms,
                          "scipy_scaled_ms": {k: v * scale for k, v in scipy_ms.items()},
                          "max_abs_device_minus_torch": float(np.abs(S_dev.reshape(S_t.shape) - S_t).max()),
                          "model": kernel_model(p, n, nB)}), flush=True)


if __name__ == "__main__":
    main()
