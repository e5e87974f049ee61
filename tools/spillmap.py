#!/usr/bin/env python3
"""Where do the register spills of a kernel fall?  Per basic block: MFMA count, scratch ops, loop depth.
usage: spillmap.py <mangled-kernel-name-substring>            every source of _backend.SOURCES compiled to assembly with its
                                                              SOURCE_FLAGS (tools/isa_diff.py's compile), each unit that holds a match
       spillmap.py <file.s> <mangled-kernel-name-substring>   an assembly file at hand"""
import os, re, sys, tempfile
from concurrent.futures import ThreadPoolExecutor


def report(lines, key):
    start = next((i for i, l in enumerate(lines) if l.startswith("_Z") and key in l and l.rstrip().endswith(":") or (key in l and re.match(r"^_Z\S+:", l))), None)
    if start is None:
        return False
    end = next(i for i in range(start, len(lines)) if ".amdhsa_kernel" in lines[i])
    blk, stats, order = "entry", {"entry": dict(mfma=0, scr=0, depth="")}, ["entry"]
    for l in lines[start:end]:
        m = re.match(r"^(\.LBB\d+_\d+):", l)
        if m:
            blk = m.group(1); stats[blk] = dict(mfma=0, scr=0, depth=""); order.append(blk); continue
        if "v_mfma" in l: stats[blk]["mfma"] += 1
        if "scratch_" in l: stats[blk]["scr"] += 1
        m = re.search(r"Depth[= ](\d)", l)
        if m: stats[blk]["depth"] = m.group(1)
    for b in order:
        st = stats[b]
        if st["mfma"] or st["scr"]: print(f"{b:12s} mfma={st['mfma']:4d} scratch={st['scr']:4d} depth={st['depth']}")
    return True


if len(sys.argv) > 2:
    if not report(open(sys.argv[1]).read().split("\n"), sys.argv[2]):
        sys.exit(f"no kernel matching {sys.argv[2]} in {sys.argv[1]}")
else:
    sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
    from isa_diff import compile_tree  # noqa: E402
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    with tempfile.TemporaryDirectory() as tmp, ThreadPoolExecutor(min(8, os.cpu_count() or 1)) as pool:
        found = False
        for unit, fut in compile_tree(root, tmp, pool).items():
            lines = open(fut.result()).read().split("\n")
            if any(sys.argv[1] in l and re.match(r"^_Z\S+:", l) for l in lines):
                print(f"# {unit}")
                found |= report(lines, sys.argv[1])
    if not found:
        sys.exit(f"no kernel matching {sys.argv[1]} in any unit")
