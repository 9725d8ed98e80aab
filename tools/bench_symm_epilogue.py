#!/usr/bin/env python3
"""The three epilogues of the direct-to-LDS product kernel (dev tool, libggl_hip_dev.so): isolated launches with the register
epilogue (ggl_dev_set_symm_epilogue(0), the product's: off-diagonal tiles and their mirrors written from the accumulator
registers), the staged one (2: the batched epilogue with the LDS tile, the product's before) and the serial one (1), the epilogue
operands present (ggl_dev_symm_bench_ops), and the no-epilogue ablation as the ceiling.  The share of (staged - ceiling) that the
register path recovers is the number to quote.  (The 64x64 two-stage kernel, variant 16, has no register path -- 96 VGPRs at five
workgroups per CU -- so its first two columns time the same code.)"""
import os, sys
import numpy as np
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from gglasso_amd import _lib
from gglasso_amd._lib import ptr
lib = _lib.load_dev()
def t(K, p, v, ops, iters=200):
    ms = np.zeros(1); _lib.check(lib.ggl_dev_symm_bench_ops(K, p, v, iters, ops, ptr(ms))); return ms[0] * 1e3
names = {0: "none", 1: "E", 3: "E+E2", 7: "E+E2+C2"}
print("us per launch, median of 5 alternating rounds of 200 launches; ceiling = ABL 4 (no epilogue)")
print(f"{'shape':>10s} {'var':>4s} {'operands':>9s} {'register':>9s} {'staged':>9s} {'serial':>9s} {'no-epi':>9s} {'gain %':>7s} {'staged cost':>12s} {'recovered %':>12s}")
for (K, p) in ((32, 500), (16, 500), (8, 500), (4, 500), (20, 200), (8, 1000)):
    for v, abl in ((17, 32), (16, None), (20, 36)):
        for ops in ((0, 1, 3, 7) if v == 17 else (3,)):
            if (K, p) not in ((32, 500), (16, 500), (8, 1000)) and ops != 3:
                continue
            r, g, s, c = [], [], [], []
            for rnd in range(5):
                lib.ggl_dev_set_symm_epilogue(1); s.append(t(K, p, v, ops))
                lib.ggl_dev_set_symm_epilogue(2); g.append(t(K, p, v, ops))
                lib.ggl_dev_set_symm_epilogue(0); r.append(t(K, p, v, ops))
                if abl: c.append(t(K, p, abl, ops))
            r, g, s = np.median(r), np.median(g), np.median(s)
            c = np.median(c) if abl else float("nan")
            rec = 100.0 * (g - r) / (g - c) if abl else float("nan")
            print(f"({K:3d},{p:4d}) {v:4d} {names[ops]:>9s} {r:9.1f} {g:9.1f} {s:9.1f} {c:9.1f} {100.0 * (g - r) / g:7.1f} {g - c:12.1f} {rec:12.1f}", flush=True)
