#!/usr/bin/env python3
"""Did a host-side change leave the device code alone?

Compiles the device side of csrc/*.hip files to gfx950 assembly twice -- at a base revision (git archive into a temporary directory) and in
the working tree -- with the flags of csrc/Makefile plus `--cuda-device-only -S`, and compares kernel by kernel: the instruction stream, the
.amdhsa_kernel descriptor block and the kernel's metadata entry (register, spill, LDS, scratch and kernarg figures).  Needs hipcc, no GPU.

    tools/device_asm_diff.py --base HEAD~1 igemm.hip igemm_f16x2.hip
    tools/device_asm_diff.py --base main --rename 'h2_reduce_slabs_kernel=cs_reduce_slabs_kernel<0>' igemm_f16x2.hip

--rename OLD=NEW (kernel names as the summary prints them, repeatable) compares base kernel OLD with head kernel NEW: their bodies must
match once the symbol is substituted.  Several OLD may map to one NEW; a pair that a file does not have is ignored there.  Without file
arguments: every .hip file that differs from the base (a file that only includes a changed one has to be named).  Exit status 0 = every
kernel equal and none added or lost.

Normalised away, and nothing else: lines naming the per-compilation __hip_cuid_ symbol; the function index inside local labels (.LBB<n>_<m>,
BB<n>_<m> in loop comments, .Lfunc_end<n>: it counts the functions of the translation unit, so it shifts when a kernel moves) and the
blanks that pad a label to the comment column; the order in which the kernels appear in the file.
"""
import argparse
import concurrent.futures
import functools
import os
import re
import subprocess
import sys
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = "miccai2021_cataract_semantic_segmentation_amd/csrc"
FIGURES = (".vgpr_count", ".agpr_count", ".sgpr_count", ".vgpr_spill_count", ".sgpr_spill_count", ".group_segment_fixed_size",
           ".private_segment_fixed_size", ".kernarg_segment_size")


def makefile_flags(tree):
    text = open(os.path.join(tree, CSRC, "Makefile")).read()
    flags = re.search(r"^FLAGS := (.*)$", text, re.M).group(1)
    arch = re.search(r"^ARCH \?= (\S+)", text, re.M).group(1)
    flags = flags.replace("$(ARCH)", arch).replace("$(ROOT)", os.path.join(tree, CSRC))
    return [f for f in flags.split() if f != "-fPIC"]


def compile_asm(tree, name, out):
    cmd = ["hipcc"] + makefile_flags(tree) + ["--cuda-device-only", "-S", "-Wno-unused-command-line-argument", os.path.join(tree, CSRC, name), "-o", out]
    subprocess.run(cmd, check=True)
    return out


def kernel_symbols(text):
    return re.findall(r"^\s*\.amdhsa_kernel (\S+)", text, re.M)


def kernels_of(path, renames=(), head_symbols=()):
    """{symbol: (body, descriptor, metadata entry, figures)} of one assembly file"""
    text = open(path).read()
    by_name = {short(sym): sym for sym in head_symbols}
    for sym in kernel_symbols(text):
        new = dict(renames).get(short(sym))
        if new in by_name:
            text = text.replace(sym, by_name[new])
    lines = [l for l in text.splitlines() if "__hip_cuid_" not in l]
    text = "\n".join(lines)
    text = re.sub(r"(?<![A-Za-z0-9_])(\.L)?BB\d+_", r"\1BB_", text)
    text = re.sub(r"\.Lfunc_(begin|end)\d+", r".Lfunc_\1", text)
    text = re.sub(r"^(\.LBB_\d+:)[ \t]+", r"\1 ", text, flags=re.M)      # (the comment column moves with the width of the label)
    desc = {m.group(1): m.group(0) for m in re.finditer(r"^\s*\.amdhsa_kernel (\S+)\n.*?^\s*\.end_amdhsa_kernel", text, re.M | re.S)}
    meta = {}
    for entry in re.split(r"^  - (?=\.\w+:)", text[text.find("amdhsa.kernels:"):], flags=re.M)[1:]:
        entry = entry.split("amdhsa.target:")[0]
        m = re.search(r"^\s*\.name:\s+(\S+)", entry, re.M)
        if m:
            meta[m.group(1)] = entry
    out = {}
    for sym in desc:
        m = re.search(r"^%s:.*?^\.Lfunc_end:" % re.escape(sym), text, re.M | re.S)
        figures = {k: int(v) for k, v in re.findall(r"^\s*(\.\w+):\s+(\d+)\s*$", meta.get(sym, ""), re.M) if k in FIGURES}
        out[sym] = (m.group(0) if m else None, desc[sym], meta.get(sym), figures)
    return out


@functools.lru_cache(None)
def short(sym):
    try:
        name = subprocess.run(["c++filt", "-p", sym], capture_output=True, text=True, check=True).stdout.strip()
        return re.sub(r"^void ", "", name.replace("(anonymous namespace)::", ""))
    except (OSError, subprocess.CalledProcessError):
        return sym


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("--base", default="HEAD", help="revision to compare the working tree against (default HEAD)")
    ap.add_argument("--rename", action="append", default=[], metavar="OLD=NEW")
    ap.add_argument("--jobs", type=int, default=8)
    ap.add_argument("files", nargs="*", help="file names under csrc/")
    args = ap.parse_args()
    renames = [tuple(r.split("=", 1)) for r in args.rename]
    files = args.files
    if not files:
        changed = subprocess.run(["git", "-C", ROOT, "diff", "--name-only", args.base, "--", CSRC], capture_output=True, text=True, check=True).stdout
        files = [os.path.basename(f) for f in changed.split() if f.endswith(".hip")]
    if not files:
        print("no .hip file differs from", args.base)
        return 0
    bad = 0
    with tempfile.TemporaryDirectory() as tmp:
        base = os.path.join(tmp, "base")
        os.makedirs(base)
        archive = subprocess.Popen(["git", "-C", ROOT, "archive", args.base, CSRC, "include"], stdout=subprocess.PIPE)
        subprocess.run(["tar", "-x", "-C", base], stdin=archive.stdout, check=True)
        if archive.wait() != 0:
            sys.exit("git archive %s failed" % args.base)
        with concurrent.futures.ThreadPoolExecutor(args.jobs) as pool:
            jobs = {(f, side): pool.submit(compile_asm, tree, f, os.path.join(tmp, "%s.%s.s" % (f, side)))
                    for f in files for side, tree in (("base", base), ("head", ROOT))}
            asm = {k: j.result() for k, j in jobs.items()}
        for f in files:
            new = kernels_of(asm[(f, "head")])
            old = kernels_of(asm[(f, "base")], renames, list(new))
            print("%s: %d kernels at %s, %d in the working tree" % (f, len(old), args.base, len(new)))
            for sym in sorted(set(old) | set(new)):
                if sym not in new or sym not in old:
                    bad += 1
                    print("  %-9s %s" % ("LOST" if sym in old else "ADDED", short(sym)))
                    continue
                same = old[sym][0] is not None and old[sym][:3] == new[sym][:3]
                bad += not same
                fig = new[sym][3]
                print("  %-9s %s  vgpr %d agpr %d sgpr %d spills %d+%d lds %d scratch %d kernarg %d" % (
                    "equal" if same else "NOT EQUAL", short(sym), *[fig.get(k, -1) for k in FIGURES]))
                if not same and old[sym][3] != fig:
                    print("            base:", old[sym][3])
    print("device code unchanged" if not bad else "%d kernels differ" % bad)
    return 1 if bad else 0


if __name__ == "__main__":
    sys.exit(main())
