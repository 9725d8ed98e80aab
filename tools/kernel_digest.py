"""Per-kernel digest of a HIP unit's gfx950 machine code, for "same code before and after" checks of a refactor.

    python tools/kernel_digest.py [--dev] [--root TREE] unit.hip ... > digest.tsv
    python tools/kernel_digest.py --diff before.tsv after.tsv

Compiles each unit of TREE/gglasso_amd/csrc with build.py's flags plus --cuda-device-only -S (and -DGGL_DEV with --dev) and
prints one line per kernel: unit, demangled symbol, VGPRs, SGPRs, LDS bytes, private bytes, SHA-1 of the instruction text
(comments, directives and blank lines stripped).  --diff prints every symbol of either file as same / DIFFERENT / removed /
added / moved (same digest, other unit) and exits 1 if any kernel differs."""
import hashlib
import os
import re
import subprocess
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
from gglasso_amd.build import FLAGS, HIPCC  # noqa: E402

RES = (".amdhsa_next_free_vgpr", ".amdhsa_next_free_sgpr", ".amdhsa_group_segment_fixed_size",
       ".amdhsa_private_segment_fixed_size")


def digest(root, unit, dev):
    src = os.path.join(root, "gglasso_amd", "csrc", unit)
    cmd = [HIPCC] + FLAGS + (["-DGGL_DEV"] if dev else []) + ["--cuda-device-only", "-S", src, "-o", "-"]
    asm = subprocess.run(cmd, check=True, capture_output=True, text=True).stdout
    kernels = set(re.findall(r"^\s*\.amdhsa_kernel\s+(\S+)", asm, re.M))
    text, res, cur, desc = {}, {}, None, None       # cur: kernel whose body is being read, desc: ... whose descriptor
    for line in asm.splitlines():
        s = line.split(";")[0].strip()
        # local labels carry the function's index in the unit, which shifts when another kernel leaves it
        s = re.sub(r"\.L([A-Za-z]+)\d+_", r".L\1_", s)
        m = re.match(r"([^.\s]\S*):$", s)
        if m:
            cur = m.group(1) if m.group(1) in kernels else None
        elif s.startswith(".amdhsa_kernel"):
            desc = s.split()[1]
            res[desc] = {}
        elif s.startswith(RES):
            key, val = s.split()
            res[desc][key] = val
        elif s.startswith((".section", ".Lfunc_end")):
            cur = None
        elif cur and s and (not s.startswith(".") or s.endswith(":")):
            text.setdefault(cur, []).append(re.sub(r"\s+", " ", s))
    names = subprocess.run(["c++filt"] + sorted(kernels), check=True, capture_output=True,
                           text=True).stdout.split("\n") if kernels else []
    rows = []
    for sym, name in zip(sorted(kernels), names):
        name = re.sub(r"^void ", "", name)
        name = re.sub(r"\(.*$", "", name).replace(" ", "")
        h = hashlib.sha1("\n".join(text.get(sym, [])).encode()).hexdigest()[:16]
        rows.append((unit, name) + tuple(res[sym].get(k, "?") for k in RES) + (h,))
    return rows


def load(path):
    out = {}
    for line in open(path):
        f = line.rstrip("\n").split("\t")
        if len(f) == 7:
            out[f[1]] = f
    return out


def diff(a, b):
    A, B = load(a), load(b)
    bad = 0
    print("symbol\tVGPRs\tLDS bytes\tverdict")
    for name in sorted(set(A) | set(B)):
        x, y = A.get(name), B.get(name)
        if x and y:
            same = x[2:] == y[2:]
            verdict = ("same" if x[0] == y[0] else f"moved to {y[0]}, same") if same else "DIFFERENT"
            bad += not same
        else:
            verdict = "removed" if x else "added"
        r = x or y
        print(f"{name}\t{r[2]}\t{r[4]}\t{verdict}")
    return 1 if bad else 0


if __name__ == "__main__":
    args = sys.argv[1:]
    if args and args[0] == "--diff":
        sys.exit(diff(args[1], args[2]))
    dev = "--dev" in args
    root = os.path.dirname(HERE)
    if "--root" in args:
        root = args[args.index("--root") + 1]
    units = [a for a in args if a.endswith(".hip")]
    for u in units:
        for row in digest(root, u, dev):
            print("\t".join(row))
