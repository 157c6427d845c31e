#!/usr/bin/env python
"""Per-kernel resource table of csrc/sem_volume.hip: compiles the unit with
-Rpass-analysis=kernel-resource-usage (no GPU needed) and writes
profiles/volume/kernel_resources.csv, one row per kernel instantiation.
Exits 1 when any instantiation spills or uses scratch memory.

Usage:  python tools/volume_resources.py
"""
import csv
import os
import re
import subprocess
import sys
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from spectralelementmethod_amd import _build  # noqa: E402

MODES = ("gradient", "recover", "norms", "detj")
FIELDS = (("TotalSGPRs", "sgprs"), ("VGPRs", "vgprs"), ("AGPRs", "agprs"),
          ("ScratchSize [bytes/lane]", "scratch_bytes_per_lane"),
          ("Occupancy [waves/SIMD]", "occupancy_waves_per_simd"), ("SGPRs Spill", "sgpr_spill"),
          ("VGPRs Spill", "vgpr_spill"), ("LDS Size [bytes/block]", "lds_bytes_per_block"))


def kernel_name(mangled):
    m = re.search(r"k_vol_elemILi(\d+)ELi(\d+)ELi(\d+)E", mangled)
    if m:
        nd, n, mode = (int(g) for g in m.groups())
        return "k_vol_elem", nd, n, MODES[mode]
    m = re.search(r"\d+(k_vol_[a-z]+)E", mangled)
    return (m.group(1) if m else mangled), "", "", ""


def main():
    with tempfile.TemporaryDirectory() as tmp:
        cmd = [_build.hipcc(), "--offload-arch=" + _build.ARCH, "-O3", "-fPIC", "-std=c++17",
               "-Rpass-analysis=kernel-resource-usage", "-c",
               os.path.join(_build.CSRC, "sem_volume.hip"), "-o", os.path.join(tmp, "v.o")]
        log = subprocess.run(cmd, check=True, capture_output=True, text=True).stderr
    rows, cur = [], None
    for line in log.splitlines():
        m = re.search(r"remark:\s+(.*?): (\S+) \[-Rpass-analysis", line)
        if not m:
            continue
        key, val = m.groups()
        if key == "Function Name":
            kern, nd, n, mode = kernel_name(val)
            cur = dict(kernel=kern, ndim=nd, n=n, mode=mode)
            rows.append(cur)
        else:
            for k, col in FIELDS:
                if key == k:
                    cur[col] = int(val)
    rows.sort(key=lambda r: (r["kernel"] != "k_vol_elem", r["kernel"], r["ndim"] or 0,
                             r["n"] or 0, r["mode"]))
    out = os.path.join(ROOT, "profiles", "volume", "kernel_resources.csv")
    os.makedirs(os.path.dirname(out), exist_ok=True)
    cols = ["kernel", "ndim", "n", "mode"] + [c for _, c in FIELDS]
    with open(out, "w", newline="") as f:
        wr = csv.DictWriter(f, fieldnames=cols)
        wr.writeheader()
        wr.writerows(rows)
    bad = [r for r in rows if r["scratch_bytes_per_lane"] or r["sgpr_spill"] or r["vgpr_spill"]]
    print("%d kernels, max VGPRs %d, max LDS %d B, min occupancy %d waves/SIMD, %d spill"
          % (len(rows), max(r["vgprs"] for r in rows), max(r["lds_bytes_per_block"] for r in rows),
             min(r["occupancy_waves_per_simd"] for r in rows), len(bad)))
    for r in bad:
        print("  spills:", r)
    return 1 if bad else 0


if __name__ == "__main__":
    sys.exit(main())
