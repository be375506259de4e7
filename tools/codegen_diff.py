#!/usr/bin/env python3
"""Compare the generated device code of two trees, kernel by kernel (no GPU needed).

    python tools/codegen_diff.py <tree A> <tree B> [--jobs 8] [--keep DIR [--reuse]] [--show]

Every neuralnet-tracker-traincode_amd/csrc/*.hip of either tree is compiled device-side only with the flags of that tree's Makefile
(FLAGS, plus the per-file FLAGS_<name>):   hipcc <flags> --cuda-device-only -S FILE -o OUT.s
From the assembly each kernel (every .amdhsa_kernel symbol) is cut out - from its label to .Lfunc_end: the body and the kernel descriptor -
and normalised: __hip_cuid_ lines dropped, local labels (.LBBn_m, .Ltmpn, .Lfunc_endn and the BBn_m of the loop comments, all of which
count the functions in front of the kernel) renumbered in order of appearance, the blanks between a block label and its loop comment (padded
to a fixed column, so they count the digits of the function number) reduced to one.  Kernels are paired by demangled name and compared as text.
The method of profiles/gemm_family_cleanup_codegen.txt, fp32_storage_params_codegen.txt, exp_switches_codegen.txt and
compile_switches_codegen.txt.
"""
import argparse
import concurrent.futures
import os
import re
import subprocess
import sys
import tempfile

CSRC = os.path.join("neuralnet-tracker-traincode_amd", "csrc")
HIPCC = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
CXXFILT = os.environ.get("CXXFILT", "c++filt")


def makefile_flags(csrc):
    """FLAGS and the per-file FLAGS_<name> of csrc/Makefile (ARCH substituted; -Wall and the like are harmless here)."""
    text = open(os.path.join(csrc, "Makefile")).read()
    arch = re.search(r"^ARCH\s*\?=\s*(\S+)", text, re.M).group(1)
    flags = re.search(r"^FLAGS\s*\?=\s*(.+)$", text, re.M).group(1).replace("$(ARCH)", arch).split()
    per_file = {m.group(1): m.group(2).split() for m in re.finditer(r"^FLAGS_(\w+)\s*:=\s*(.+)$", text, re.M)}
    return flags, per_file


def compile_s(args):
    src, flags, out, reuse = args
    if reuse and os.path.exists(out):
        return out
    subprocess.run([HIPCC, *flags, "--cuda-device-only", "-S", src, "-o", out], check=True, stdout=subprocess.DEVNULL, stderr=subprocess.DEVNULL)
    return out


LABEL = re.compile(r"\.LBB\d+_\d+|\.Ltmp\d+|\.Lfunc_end\d+|\.Lfunc_begin\d+|\bBB\d+_\d+")

LABEL_PAD = re.compile(r"^(\.LBB\d+_\d+:) +;")


def normalise(lines):
    seen = {}

    def sub(m):
        t = m.group(0)
        kind = re.match(r"\.?[A-Za-z_]+", t).group(0)
        if t not in seen:
            seen[t] = f"{kind}#{sum(1 for k in seen if k.startswith(kind))}"
        return seen[t]

    # (a block label's loop comment is padded to a fixed column, so its blanks count the digits of the function number too)
    return [LABEL.sub(sub, LABEL_PAD.sub(r"\1 ;", ln.rstrip())) for ln in lines if "__hip_cuid_" not in ln]


def kernels_of(path):
    """{mangled name: normalised text of body + descriptor}"""
    lines = open(path).read().split("\n")
    names = [ln.split()[1] for ln in lines if ln.lstrip().startswith(".amdhsa_kernel ")]
    start = {m.group(1): i for i, ln in enumerate(lines) if (m := re.match(r"([A-Za-z_$][\w$.]*):", ln))}
    out = {}
    for n in names:
        i = start[n]
        j = next(k for k in range(i, len(lines)) if lines[k].startswith(".Lfunc_end"))  # (the descriptor sits in front of it)
        out[n] = "\n".join(normalise(lines[i : j + 1]))
    return out


def demangle(names):
    if not names:
        return {}
    res = subprocess.run([CXXFILT], input="\n".join(names) + "\n", capture_output=True, text=True, check=True).stdout.split("\n")
    return dict(zip(names, res))


def tree_kernels(tree, work, jobs, reuse):
    csrc = os.path.join(tree, CSRC)
    flags, per_file = makefile_flags(csrc)
    srcs = sorted(f for f in os.listdir(csrc) if f.endswith(".hip"))
    os.makedirs(work, exist_ok=True)
    tasks = [(os.path.join(csrc, f), flags + per_file.get(f[:-4], []), os.path.join(work, f[:-4] + ".s"), reuse) for f in srcs]
    with concurrent.futures.ThreadPoolExecutor(jobs) as ex:
        list(ex.map(compile_s, tasks))
    res = {}
    for f, (_, _, s, _) in zip(srcs, tasks):
        k = kernels_of(s)
        d = demangle(list(k))
        res[f] = {d[m]: body for m, body in k.items()}
    return res


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("tree_a")
    ap.add_argument("tree_b")
    ap.add_argument("--jobs", type=int, default=8)
    ap.add_argument("--keep", help="directory for the .s files (default: a temporary one)")
    ap.add_argument("--reuse", action="store_true", help="with --keep: take the .s files that are already there as they are")
    ap.add_argument("--show", action="store_true", help="print a unified diff of every kernel that differs")
    a = ap.parse_args()
    with tempfile.TemporaryDirectory() as tmp:
        work = a.keep or tmp
        ka = tree_kernels(a.tree_a, os.path.join(work, "a"), a.jobs, a.reuse)
        kb = tree_kernels(a.tree_b, os.path.join(work, "b"), a.jobs, a.reuse)
    print(f"A = {a.tree_a}\nB = {a.tree_b}\n")
    print(f"{'file':<22}{'A':>5}{'B':>5}{'compared':>10}{'differing':>11}")
    tot = [0, 0, 0, 0]
    notes = []
    for f in sorted(set(ka) | set(kb)):
        xa, xb = ka.get(f, {}), kb.get(f, {})
        both = sorted(set(xa) & set(xb))
        diff = [n for n in both if xa[n] != xb[n]]
        print(f"{f:<22}{len(xa):>5}{len(xb):>5}{len(both):>10}{len(diff):>11}")
        for i, v in enumerate((len(xa), len(xb), len(both), len(diff))):
            tot[i] += v
        notes += [f"  {f}: differs: {n}" for n in diff]
        notes += [f"  {f}: in A only: {n}" for n in sorted(set(xa) - set(xb))]
        notes += [f"  {f}: in B only: {n}" for n in sorted(set(xb) - set(xa))]
        if a.show:
            import difflib

            for n in diff:
                sys.stdout.write("\n".join(difflib.unified_diff(xa[n].split("\n"), xb[n].split("\n"), "A:" + n, "B:" + n, lineterm="", n=2)) + "\n")
    print(f"{'total':<22}{tot[0]:>5}{tot[1]:>5}{tot[2]:>10}{tot[3]:>11}\n")
    print("\n".join(notes) if notes else "  no kernel differs, none added or removed")


if __name__ == "__main__":
    main()
