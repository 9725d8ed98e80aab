"""Debiased graphical lasso (``ggl_debias``): the device route against the numpy twin, and the kernel k_debias against the
full product it replaces, at the sizes of profiles/debiased_inference.txt -- which this tool writes.

    python tools/bench_debias.py [--shapes 1,500;32,500] [--calls 5] [--iters 200] [--out profiles/debiased_inference.txt]

Per shape (K,p), one JSON line each and one block of the text file:

* whole calls, from Theta and S on the host to T and SE on the host, host clock around calls that end in a device
  synchronise: ``utils.debiased_precision`` (device) and ``utils.host_debiased_precision`` (host) ALTERNATE, --calls rounds
  after one warm-up round, reported as median (min - max).
* kernels (``ggl_dev_debias_bench``: HIP events around --iters back-to-back launches on random device data, after three
  warm-up launches): the full product M Theta by ``launch_gemm_right`` -- the only route to that product without k_debias --
  and k_debias (upper tile pairs, both epilogues) with the automatic and both forced tile shapes; --calls rounds, in each of
  which the routes follow one another, median (min - max) of the rounds' averages.

Registers, LDS and waves per SIMD of the two instantiations are read from the compiler's resource report
(``hipcc -Rpass-analysis=kernel-resource-usage`` on csrc/debias.hip with the flags of the build) where hipcc is at hand."""
import argparse
import json
import os
import re
import subprocess
import sys
import tempfile

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from tools.bench_stars import alternate_ms      # noqa: E402


def fmt(t, unit="ms", scale=1.0):
    return f"{t['median'] * scale:.3g} {unit} ({t['min'] * scale:.3g} - {t['max'] * scale:.3g})"


def spread(v):
    return {"median": float(np.median(v)), "min": float(min(v)), "max": float(max(v))}


def resource_report():
    """{instantiation: {'VGPRs', 'SGPRs', 'LDS', 'Occupancy', 'Scratch'}} of k_debias, or None."""
    from gglasso_amd import build
    try:
        with tempfile.TemporaryDirectory() as tmp:
            cmd = [build.HIPCC] + build.FLAGS + ["-Rpass-analysis=kernel-resource-usage", "-c",
                                                 os.path.join(build.CSRC, "debias.hip"), "-o", os.path.join(tmp, "debias.o")]
            text = subprocess.run(cmd, check=True, capture_output=True, text=True, timeout=300).stderr
    except (OSError, subprocess.SubprocessError):
        return None
    out, name = {}, None
    keys = {"VGPRs": r" VGPRs: (\d+)", "SGPRs": r"TotalSGPRs: (\d+)", "LDS": r"LDS Size \[bytes/block\]: (\d+)",
            "Occupancy": r"Occupancy \[waves/SIMD\]: (\d+)", "Scratch": r"ScratchSize \[bytes/lane\]: (\d+)"}
    for line in text.splitlines():
        m = re.search(r"Function Name: \S*k_debiasILi(\d+)ELi(\d+)", line)
        if m:
            name = f"k_debias<{m.group(1)},{m.group(2)}>"
            out[name] = {}
        for key, pat in keys.items():
            m = re.search(pat, line)
            if m and name:
                out[name][key] = int(m.group(1))
    return out or None


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--shapes", default="1,500;32,500", help="K,p;K,p;...")
    ap.add_argument("--calls", type=int, default=5)
    ap.add_argument("--iters", type=int, default=200)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "debiased_inference.txt"))
    args = ap.parse_args()
    from gglasso_amd import _lib, utils
    lib = _lib.load()
    _lib.require_gpu()
    lines = ["Debiased graphical lasso (ggl_debias, csrc/debias.hip) on one MI355X.  Written by tools/bench_debias.py "
             f"--calls {args.calls} --iters {args.iters}:",
             "whole calls from Theta and S on the host to T and SE on the host, the two routes ALTERNATING; kernel times by HIP "
             "events around",
             f"{args.iters} back-to-back launches, the routes following one another in each round; all as median (min - max) of "
             f"{args.calls} rounds.",
             "One run, on the code as it stands.  No target ratio was set in advance.", ""]
    for shape in args.shapes.split(";"):
        K, p = (int(v) for v in shape.split(","))
        rng = np.random.default_rng(0)
        Th = np.empty((K, p, p))
        Sm = np.empty((K, p, p))
        for k in range(K):
            A = np.triu(rng.uniform(-1, 1, (p, p)) * (rng.random((p, p)) < 0.05), 1)
            Th[k] = A + A.T + np.diag(np.abs(A + A.T).sum(axis=1) + 1.0)
            X = rng.standard_normal((p, 2 * p))
            Sm[k] = np.cov(X, bias=True)
        n = np.full(K, 2.0 * p)
        got = {}

        def device():
            got["dev"] = utils.debiased_precision(Th, Sm, n)

        def host():
            got["host"] = utils.host_debiased_precision(Th, Sm, n)

        dev_ms, host_ms = alternate_ms([device, host], args.calls)
        diff = float(np.abs(got["dev"][0] - got["host"][0]).max())
        kern = {}
        for tile in (0, 32, 64):
            rounds = np.zeros((args.calls, 2))
            for r in range(args.calls):
                _lib.check(lib.ggl_dev_debias_bench(K, p, tile, args.iters, _lib.ptr(rounds[r])))
            kern[tile] = (spread(rounds[:, 0]), spread(rounds[:, 1]))
        T64 = (p + 63) // 64
        auto = 64 if K * T64 * (T64 + 1) // 2 >= 256 else 32
        flop_full, flop_sym = 2.0 * K * p ** 3, 2.0 * K * p ** 3 * 0.5 * (1 + 1.0 / p)
        print(json.dumps({"K": K, "p": p, "device_ms": dev_ms, "host_ms": host_ms, "max_abs_device_minus_host": diff,
                          "auto_tile": auto, "gemm_right_ms": kern[0][0],
                          "k_debias_ms": {str(t): kern[t][1] for t in kern}}), flush=True)
        g, d = kern[0][0], kern[0][1]
        lines += [f"K = {K}, p = {p}   (automatic tile: {auto} x {auto})",
                  f"   whole call   device  utils.debiased_precision        {fmt(dev_ms)}",
                  f"                host    utils.host_debiased_precision   {fmt(host_ms)}      max |device - host| of T: {diff:.2e}",
                  f"   kernels      launch_gemm_right, full M Theta         {fmt(g, 'us', 1e3)}    "
                  f"{flop_full / (g['median'] * 1e-3) / 1e12:.2f} TF/s",
                  f"                k_debias, automatic tile                {fmt(d, 'us', 1e3)}    "
                  f"{flop_sym / (d['median'] * 1e-3) / 1e12:.2f} TF/s of useful flops (i <= j), "
                  f"the full product takes {g['median'] / d['median']:.2f} x as long",
                  f"                k_debias, forced 32 x 32                {fmt(kern[32][1], 'us', 1e3)}",
                  f"                k_debias, forced 64 x 64                {fmt(kern[64][1], 'us', 1e3)}", ""]
    res = resource_report()
    if res:
        lines.append("Compiler's resource report (hipcc -Rpass-analysis=kernel-resource-usage, the flags of the build):")
        for name, r in res.items():
            lines.append(f"   {name}: {r.get('VGPRs')} VGPRs, {r.get('SGPRs')} SGPRs, {r.get('Scratch')} bytes of scratch, "
                         f"{r.get('LDS')} bytes of LDS per workgroup of 256, {r.get('Occupancy')} waves per SIMD")
    else:
        lines.append("Compiler's resource report: hipcc was not at hand.")
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        f.write("\n".join(lines) + "\n")
    print(f"wrote {args.out}")


if __name__ == "__main__":
    main()
