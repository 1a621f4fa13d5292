#!/usr/bin/env python3
"""Which kernels of two source trees compile to different machine code (no GPU needed):

    python tools/kernel_isa_diff.py <tree A> <tree B> [--work DIR] [--jobs N] [--out FILE]

For every source in SOURCES (the conv3 and training sources, and the per-instance passes that share instance_rows.h)
of both trees: hipcc with tree B's Makefile flags plus --offload-device-only -S, in the builds release, -DSK_BF16 (the twin-built sources only), -DSK_TUNING and
-DSK_TUNING -DSK_TIMING.  The assembly is split per function symbol (instruction stream + its .amdhsa_kernel resource
block); the __hip_cuid_* symbol, comments and the function index inside local labels are ignored.  One line per kernel:
identical, or DIFFERENT with the number of differing lines.  Exit status 1 if any differs.  An up-to-date .s file in
--work is reused, so the parent tree compiles once.
"""
import argparse
import difflib
import os
import re
import subprocess
import sys
import tempfile
from concurrent.futures import ThreadPoolExecutor

SOURCES = ["conv3d.hip", "conv3d_up.hip", "unet_misc.hip", "train.hip",
           # the per-instance passes that share instance_rows.h
           "instance_stats.hip", "instance_mesh.hip", "instance_mesh_emit.hip", "instance_intensity.hip",
           "surface_distance.hip", "contacts.hip", "edt.hip", "nearest_label.hip"]
TWINS = {"conv3d.hip", "unet_misc.hip", "train.hip"}
BUILDS = [("release", []), ("bf16", ["-DSK_BF16"]), ("tuning", ["-DSK_TUNING"]), ("timing", ["-DSK_TUNING", "-DSK_TIMING"])]
HIPCC = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")


def makefile_flags(tree):
    text = open(os.path.join(tree, "skoots_amd/csrc/Makefile")).read()
    arch = re.search(r"^ARCH\s*\?=\s*(\S+)", text, re.M).group(1)
    flags = re.search(r"^FLAGS\s*:=\s*(.*)$", text, re.M).group(1)
    return flags.replace("$(ARCH)", arch).replace("$(EXTRA)", "").split()


def newest(tree):
    return max(os.path.getmtime(os.path.join(d, f)) for sub in ("skoots_amd/csrc", "include")
               for d, _, fs in os.walk(os.path.join(tree, sub)) for f in fs if f.endswith((".hip", ".h", ".inc", ".cpp")))


def compile_s(tree, src, extra, flags, out):
    if os.path.exists(out) and os.path.getmtime(out) > newest(tree):
        return out
    os.makedirs(os.path.dirname(out), exist_ok=True)
    r = subprocess.run([HIPCC] + flags + extra + ["--offload-device-only", "-S", src, "-o", out],
                       cwd=os.path.join(tree, "skoots_amd/csrc"), capture_output=True, text=True)
    if r.returncode:
        sys.stderr.write(r.stderr[-4000:])
        raise SystemExit("hipcc failed: %s %s in %s" % (src, " ".join(extra), tree))
    return out


def functions(path):
    """symbol -> normalised lines, from its .type directive to the next function's (or the metadata)"""
    out, cur = {}, None
    for line in open(path):
        m = re.match(r"\s*\.type\s+(\S+),@function", line)
        if m:
            cur = out.setdefault(m.group(1), [])
        elif re.match(r"\s*\.(amdgpu_metadata|type\s+\S+,@object)", line):
            cur = None
        if cur is None or "__hip_cuid_" in line or re.match(r"\s*\.(section|globl|weak|protected|hidden)\b", line):
            continue   # (the directives in front of the NEXT function follow the emission order, which is the host code's)
        line = re.sub(r"\s*;.*", "", line.rstrip())
        line = re.sub(r"\.L(BB|func_begin|func_end|tmp|JTI)\d+", r".L\1", line)
        if line.strip():
            cur.append(line)
    return out


def demangle(names):
    r = subprocess.run(["c++filt"], input="\n".join(names), capture_output=True, text=True)
    clean = lambda n: re.sub(r"\(.*", "", n.replace("(anonymous namespace)::", "").replace("void ", ""))
    return dict(zip(names, (clean(n) for n in r.stdout.split("\n"))))


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("a")
    ap.add_argument("b")
    ap.add_argument("--work", default=None)
    ap.add_argument("--jobs", type=int, default=min(8, os.cpu_count() or 1))
    ap.add_argument("--out", default=None)
    ap.add_argument("--sources", default=",".join(SOURCES))
    ap.add_argument("--builds", default=",".join(n for n, _ in BUILDS))
    args = ap.parse_args()
    work = args.work or tempfile.mkdtemp(prefix="isa_diff_")
    flags = makefile_flags(args.b)
    jobs = [(src, name, extra) for src in args.sources.split(",") for name, extra in BUILDS
            if name in args.builds.split(",") and (name != "bf16" or src in TWINS)]
    with ThreadPoolExecutor(args.jobs) as ex:
        futs = {(side, src, name): ex.submit(compile_s, os.path.abspath(tree), src, extra, flags,
                                             os.path.join(work, side, name, src.replace(".hip", ".s")))
                for src, name, extra in jobs for side, tree in (("a", args.a), ("b", args.b))}
        paths = {k: f.result() for k, f in futs.items()}
    lines, ndiff, ntotal = [], 0, 0
    for src, name, _ in jobs:
        fa, fb = functions(paths["a", src, name]), functions(paths["b", src, name])
        names = demangle(sorted(set(fa) | set(fb)))
        for sym in sorted(names, key=lambda s: names[s]):
            ntotal += 1
            if sym not in fa or sym not in fb:
                verdict = "ONLY IN " + ("A" if sym in fa else "B")
            elif fa[sym] == fb[sym]:
                verdict = "identical"
            else:
                n = sum(1 for d in difflib.unified_diff(fa[sym], fb[sym], n=0, lineterm="") if d[:1] in "+-" and d[:3] not in ("+++", "---"))
                verdict = "DIFFERENT (%d of %d lines)" % (n, len(fa[sym]))
            ndiff += verdict != "identical"
            lines.append("%-14s %-8s %-90s %s" % (src, name, names[sym][:90], verdict))
    lines.append("%d functions in %d builds, %d not identical" % (ntotal, len(jobs), ndiff))
    text = "\n".join(lines) + "\n"
    sys.stdout.write(text)
    if args.out:
        open(args.out, "w").write(text)
    return 1 if ndiff else 0


if __name__ == "__main__":
    sys.exit(main())
