#!/usr/bin/env python
"""Per-layer launch times of the limb GEMM from a rocprofv3 --kernel-trace CSV: the dispatches of gemm_x3_kernel grouped
by (instantiation, grid), since the two ConvT forwards (and the two input gradients) of a posterior step share a kernel
name and differ in their workgroup count.  usage: python tools/layer_times.py run_kernel_trace.csv [PATTERN]"""
import csv
import re
import statistics
import sys

pat = sys.argv[2] if len(sys.argv) > 2 else "gemm_x3_kernel"
groups = {}
for r in csv.DictReader(open(sys.argv[1])):
    if not re.search(pat, r["Kernel_Name"]):
        continue
    wg = int(r["Grid_Size_X"]) * int(r["Grid_Size_Y"]) * int(r["Grid_Size_Z"]) // max(1, int(r["Workgroup_Size_X"]))
    m = re.search(r"<[^>]*>", r["Kernel_Name"])
    key = (m.group(0) if m else r["Kernel_Name"][:40], wg)
    groups.setdefault(key, []).append((int(r["End_Timestamp"]) - int(r["Start_Timestamp"])) / 1e3)
print("# columns: instantiation, workgroups, launches, min / median / mean / max us")
for (name, wg), d in sorted(groups.items(), key=lambda kv: -sum(kv[1])):
    print("%-28s %5d WG %5d  %8.1f %8.1f %8.1f %8.1f" % (name, wg, len(d), min(d), statistics.median(d),
                                                        statistics.fmean(d), max(d)))
