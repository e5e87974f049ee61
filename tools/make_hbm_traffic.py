#!/usr/bin/env python3
"""profiles/hbm_traffic.json from the PMC passes of the build that ran (rocprofv3 --pmc FETCH_SIZE / WRITE_SIZE in separate
passes: tools/pmc_passes.sh):   python tools/make_hbm_traffic.py <pmc dir> <workload> [--source <text>]

Bytes per launch of each C-ABI kernel = (2 * FETCH_SIZE + WRITE_SIZE) * 1024, means per dispatch, summed over the device kernels
of one C-ABI launch.  FETCH_SIZE is doubled as MI355X_MICROARCH.md (HBM section) prescribes for wide coalesced streaming reads
on gfx950 -- register loads and LDS-DMA alike; both counters are in KiB.  FETCH_SIZE counts what leaves the L2, Infinity Cache
hits included, so the figure bounds the HBM bytes from above.  bench.py reads the file for `roofline.traffic`."""
import collections
import csv
import glob
import json
import os
import re
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
# device kernels (anonymous namespace) behind each C-ABI launch of the E-step
LAUNCH = {
    "tsvgp_moments": [r"^panel1_kernel(<(double|float), 1(, \d, \d)?>)?$", r"^panel_kernel<(double|float), 1, \d, (true|false)>$"],
    "tsvgp_site_accum": [r"^syrk1f?_kernel(_cw)?$", r"^syrk_kernel<", r"^syrk_reduce_kernel<"],
    "tsvgp_trmm": [r"^panel1_kernel<(double|float), 0(, \d, \d)?>$", r"^panel_kernel<(double|float), 0, "],
    "tsvgp_se_fill": [r"^se_fill_kernel<"],
    "tsvgp_moments_mean_only": [r"^mean_lik_kernel<"],
}


def main():
    pmc_dir, workload = sys.argv[1], sys.argv[2]
    source = sys.argv[sys.argv.index("--source") + 1] if "--source" in sys.argv else pmc_dir
    per = collections.defaultdict(lambda: collections.defaultdict(list))
    for f in glob.glob(pmc_dir + "/**/*counter_collection.csv", recursive=True):
        for r in csv.DictReader(open(f)):
            if r["Counter_Name"] not in ("FETCH_SIZE", "WRITE_SIZE") or "anonymous namespace" not in r["Kernel_Name"]:
                continue
            full = r["Kernel_Name"].replace("(anonymous namespace)::", "")
            m = re.match(r"(?:void )?([\w:]+(?:<.*>)?)\(", full)
            per[m.group(1) if m else full][r["Counter_Name"]].append(float(r["Counter_Value"]))
    out = {}
    detail = {}
    for launch, pats in LAUNCH.items():
        total, parts = 0.0, {}
        for name, d in per.items():
            if not any(re.search(p, name) for p in pats):
                continue
            # the K(Z, Z) fill of the prelude is the same device kernel as the K(X, Z) fill: keep the large dispatches only
            f, w = d.get("FETCH_SIZE", []), d.get("WRITE_SIZE", [])
            if launch == "tsvgp_se_fill" and w:
                big = max(w)
                keep = [i for i, x in enumerate(w) if x > 0.5 * big]
                w = [w[i] for i in keep]
                f = f[:len(w)] if len(f) != len(d["WRITE_SIZE"]) else [f[i] for i in keep]
            if not f or not w:
                continue
            b = (2.0 * sum(f) / len(f) + sum(w) / len(w)) * 1024.0
            parts[name] = int(b)
            total += b
        if parts:
            out[launch] = int(total)
            detail[launch] = parts
    path = os.path.join(ROOT, "profiles", "hbm_traffic.json")
    try:
        cur = json.load(open(path))
    except Exception:
        cur = {}
    cur[workload] = out
    cur.setdefault("_sources", {})[workload] = {"pmc": source, "device_kernels": detail}
    cur["_note"] = ("bytes per launch: (2 * FETCH_SIZE + WRITE_SIZE) * 1024, means per dispatch from separate rocprofv3 --pmc passes of "
                    "the build that ran (tools/pmc_passes.sh -> tools/make_hbm_traffic.py); FETCH doubled on gfx950 per "
                    "MI355X_MICROARCH.md; requests that leave the L2 (Infinity Cache hits included): an upper bound of the HBM bytes")
    json.dump(cur, open(path, "w"), indent=1, sort_keys=True)
    print(json.dumps(out, indent=1))


if __name__ == "__main__":
    main()
