#!/usr/bin/env python3
"""Kernel by kernel comparison of the machine code two trees of this project compile to (CPU: hipcc cross-compiles).

    python tools/isa_diff.py OLD_TREE NEW_TREE [--jobs N] [--keep DIR]

Every source of ``_backend.SOURCES`` of each tree is compiled to assembly with the flags of ``build_library()`` (the tree's
own SOURCE_FLAGS included).  For every kernel symbol the tool compares
  * the instruction list: comments stripped, the function index in ``.LBB<f>_<n>`` labels dropped (it counts the functions in
    front of the kernel in its translation unit, so it moves when a kernel changes files); the block labels are entries of the
    list, so a moved branch target shows too;
  * ``.vgpr_count``, ``.agpr_count``, ``.sgpr_count``, the LDS size and the private-segment size of the metadata.
One line per kernel that differs or is missing on one side (or is emitted by more than one unit), then the count of those
that agree; exit status 1 on any difference.  A plain diff: it looks for no particular instruction.  The parsing is
tools/isa_hazards.py's.  What it is for: a change that is meant to leave the hot kernels alone (a moved family, a new likelihood
map) can say "hot kernels unchanged" and show it -- the register allocation of the hand-laid fp64 kernels has been seen to
depend on what else their translation unit holds (kernel inventory).
"""
import argparse
import importlib.util
import os
import re
import subprocess
import sys
import tempfile
from concurrent.futures import ThreadPoolExecutor

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import isa_hazards  # noqa: E402

FIELDS = ("vgpr_count", "agpr_count", "sgpr_count", "group_segment_fixed_size", "private_segment_fixed_size")
LABEL = re.compile(r"\.LBB\d+_(\d+)")


def backend_of(tree):
    """The tree's own t-svgp_amd/_backend.py as a module (SOURCES, SOURCE_FLAGS): imports nothing but the standard library."""
    spec = importlib.util.spec_from_file_location("_backend_" + str(abs(hash(tree))), os.path.join(tree, "t-svgp_amd", "_backend.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def compile_tree(tree, outdir, pool):
    """{source base name: future of the assembly path}."""
    be = backend_of(tree)
    hipcc = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
    os.makedirs(outdir, exist_ok=True)
    jobs = {}
    for src in be.SOURCES:
        base = os.path.basename(src)
        out = os.path.join(outdir, base + ".s")
        cmd = [hipcc, "-O3", "--offload-arch=gfx950", "-std=c++17", "-fPIC", "-I", os.path.join(tree, "include"), "-I", be.CSRC,
               *be.SOURCE_FLAGS.get(base, []), "-S", "--cuda-device-only", src, "-o", out]

        newest = max(os.path.getmtime(p) for p in [src] + be.HEADERS)

        def run(cmd=cmd, out=out, newest=newest):
            if not os.path.exists(out) or os.path.getmtime(out) < newest:  # (--keep: reused while newer than source and headers)
                res = subprocess.run(cmd, capture_output=True, text=True)
                if res.returncode != 0:
                    sys.exit(f"hipcc failed on {cmd[-3]}:\n{res.stderr}")
            return out
        jobs[base] = pool.submit(run)
    return jobs


def kernels_of(jobs):
    """{kernel symbol: [(unit, instruction list, metadata fields)]} over the units of one tree."""
    out = {}
    for base, fut in jobs.items():
        text = open(fut.result()).read()
        for name, meta in isa_hazards.kernel_metadata(text).items():
            ins = []
            for label, block in isa_hazards._blocks_of(text, name, whole=True):
                ins.append(LABEL.sub(r".LBB_\1", label) + ":")
                ins += [LABEL.sub(r".LBB_\1", t) for t in block]
            out.setdefault(name, []).append((base, ins, tuple(meta.get(f) for f in FIELDS)))
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("old_tree")
    ap.add_argument("new_tree")
    ap.add_argument("--jobs", type=int, default=min(8, os.cpu_count() or 1), help="compilations side by side")
    ap.add_argument("--keep", default=None, help="keep the assembly under this directory; a file there is reused while it is newer than its source and the headers")
    args = ap.parse_args()
    with tempfile.TemporaryDirectory() as tmp, ThreadPoolExecutor(args.jobs) as pool:
        root = args.keep or tmp
        old_jobs = compile_tree(os.path.abspath(args.old_tree), os.path.join(root, "old"), pool)
        new_jobs = compile_tree(os.path.abspath(args.new_tree), os.path.join(root, "new"), pool)
        old, new = kernels_of(old_jobs), kernels_of(new_jobs)
    same = bad = 0
    for name in sorted(set(old) | set(new)):
        o, n = old.get(name, []), new.get(name, [])
        where = f"{'+'.join(u for u, _, _ in o) or '-'} -> {'+'.join(u for u, _, _ in n) or '-'}"
        if len(o) != 1 or len(n) != 1:
            what = "missing in NEW" if not n else "missing in OLD" if not o else "in more than one unit"
        elif o[0][1:] == n[0][1:]:
            same += 1
            continue
        else:
            (_, oi, om), (_, ni, nm) = o[0], n[0]
            parts = [f"{f} {a} -> {b}" for f, a, b in zip(FIELDS, om, nm) if a != b]
            if oi != ni:
                first = next((i for i, (a, b) in enumerate(zip(oi, ni)) if a != b), min(len(oi), len(ni)))
                parts.append(f"{len(oi)} -> {len(ni)} instructions, first difference at {first}")
            what = "; ".join(parts)
        bad += 1
        print(f"DIFF {name} [{where}]: {what}")
    print(f"{same} kernel(s) agree instruction for instruction and in registers / LDS / private segment; {bad} differ or are missing "
          f"({len(old)} kernel symbols in OLD, {len(new)} in NEW)")
    sys.exit(1 if bad else 0)


if __name__ == "__main__":
    main()
