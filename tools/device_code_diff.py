#!/usr/bin/env python3
"""Prove that two checkouts compile to the same device code: `python tools/device_code_diff.py A B [--only NAME.hip ...]`.

For every entry of build.SOURCES (of checkout B) both trees are compiled for the device only, with build.FLAGS, and three parts of
the two code objects are compared byte for byte: the sorted FUNC / OBJECT symbols, the contents of .text and .rodata, and the notes
(kernel metadata: register counts, LDS, arguments).  Whole files are not compared: they carry the source path and differ between
two compiles of differently edited host code even when these parts are equal.  One line per source; exit status 1 on any difference.
Make the second checkout with `git worktree add <dir> <commit>`.
"""
from __future__ import annotations

import argparse
import importlib.util
import os
import subprocess
import sys
import tempfile
from concurrent.futures import ThreadPoolExecutor


def _load_build(tree):
    spec = importlib.util.spec_from_file_location("_gamer_build", os.path.join(tree, "gamer_amd", "build.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def _llvm(hipcc, tool):
    rocm = os.path.dirname(os.path.dirname(os.path.realpath(hipcc)))
    for d in (os.path.join(rocm, "llvm", "bin"), os.path.join(rocm, "lib", "llvm", "bin"), "/opt/rocm/llvm/bin"):
        if os.path.exists(os.path.join(d, tool)):
            return os.path.join(d, tool)
    raise SystemExit(f"{tool} not found under the ROCm install of {hipcc}")


def _run(cmd):
    r = subprocess.run(cmd, capture_output=True)
    if r.returncode != 0:
        raise RuntimeError(f"{' '.join(cmd)}\n{r.stderr.decode(errors='replace')}")
    return r.stdout


def _parts(tree, build, src, out, readelf, objcopy):
    """(symbols, .text, .rodata, notes) of the device code object of one source of one tree."""
    _run([build._hipcc(), *build.FLAGS, "--cuda-device-only", "--no-gpu-bundle-output", "-c",
          os.path.join(tree, "gamer_amd", "csrc", src), "-o", out])
    syms = []
    for line in _run([readelf, "-s", "-W", out]).decode().splitlines():
        f = line.split()                                    # Num: Value Size Type Bind Vis Ndx Name
        # (__hip_cuid_<hash> names the compilation unit - a hash of the source's path, different in any two checkouts - and holds no code)
        if len(f) == 8 and f[3] in ("FUNC", "OBJECT") and not f[7].startswith("__hip_cuid_"):
            syms.append((f[7], f[3], f[2], f[4], f[6]))
    sections = []
    for sec in (".text", ".rodata"):
        _run([objcopy, "-O", "binary", f"--only-section={sec}", out, out + sec])
        sections.append(open(out + sec, "rb").read() if os.path.exists(out + sec) else b"")
    return sorted(syms), sections[0], sections[1], _run([readelf, "--notes", out])


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("a")
    ap.add_argument("b")
    ap.add_argument("--only", nargs="*", help="compare these sources only")
    args = ap.parse_args()
    trees = [os.path.abspath(args.a), os.path.abspath(args.b)]
    build = _load_build(trees[1])
    sources = [s for s in build.SOURCES if not args.only or s in args.only]
    for s in [s for s in sources if not os.path.exists(os.path.join(trees[0], "gamer_amd", "csrc", s))]:
        print(f"{s:22s} not in {args.a}: a new source, nothing to compare")
        sources.remove(s)
    readelf, objcopy = _llvm(build._hipcc(), "llvm-readelf"), _llvm(build._hipcc(), "llvm-objcopy")
    with tempfile.TemporaryDirectory() as tmp, ThreadPoolExecutor(max_workers=min(16, os.cpu_count() or 1)) as ex:
        jobs = {(src, i): ex.submit(_parts, trees[i], build, src, os.path.join(tmp, f"{i}_{src}.co"), readelf, objcopy)
                for src in sorted(sources, key=lambda s: -os.path.getsize(os.path.join(trees[1], "gamer_amd", "csrc", s)))
                for i in (0, 1)}
        bad = 0
        for src in sources:
            a, b = jobs[src, 0].result(), jobs[src, 1].result()
            diff = [name for name, x, y in zip(("symbols", ".text", ".rodata", "notes"), a, b) if x != y]
            if "symbols" in diff:
                diff[0] += " (" + ", ".join(sorted({s[0] for s in set(a[0]) ^ set(b[0])})[:4]) + " ...)"
            bad += bool(diff)
            print(f"{src:22s} {len(a[0]):4d} symbols  .text {len(a[1]):8d}  .rodata {len(a[2]):6d}  "
                  + ("identical" if not diff else "DIFFERENT: " + "; ".join(diff)), flush=True)
    print(f"{len(sources) - bad} of {len(sources)} sources identical in symbols, .text, .rodata and notes")
    return 1 if bad else 0


if __name__ == "__main__":
    sys.exit(main())
