#!/usr/bin/env python3
"""Kernel launches and kernel time per toy Q update from rocprofv3 kernel traces of tools/toyq_profile.py.

usage: python tools/toyq_launches.py TRACE_ROOT OUT.json

TRACE_ROOT holds four `rocprofv3 --kernel-trace -f csv -d TRACE_ROOT/<path>_<N> -- python tools/toyq_profile.py --leg
q_update_trace --path <path> --updates <N>` outputs, <path> in {libdamc, stock} and <N> in {4, 10}.  Per update = (the
10-update trace - the 4-update trace) / 6, so start-up kernels cancel.  OUT.json is what toyq_profile.py --leg q_update
--launches merges into profiles/toyq/toyq_qupdate.json.
"""
import csv
import glob
import json
import sys


def trace(root, tag):
    """(kernel count, summed kernel duration in ms) of one trace directory."""
    files = glob.glob("%s/%s/**/*kernel_trace.csv" % (root, tag), recursive=True)
    if not files:
        sys.exit("no kernel trace under %s/%s" % (root, tag))
    n, busy = 0, 0.0
    for f in files:
        with open(f) as fh:
            for r in csv.DictReader(fh):
                n += 1
                busy += (float(r["End_Timestamp"]) - float(r["Start_Timestamp"])) / 1e6
    return n, busy


def main():
    root, out = sys.argv[1], sys.argv[2]
    res = {}
    for path, key in (("libdamc", "libdamc"), ("stock", "stock_torch")):
        (n4, b4), (n10, b10) = trace(root, path + "_4"), trace(root, path + "_10")
        res[key] = (n10 - n4) / 6.0
        res[key + "_kernel_ms_per_update"] = (b10 - b4) / 6.0
        res[path + "_trace_kernels"] = {"4_updates": n4, "10_updates": n10}
    res["method"] = ("rocprofv3 --kernel-trace of tools/toyq_profile.py --leg q_update_trace at 4 and at 10 updates; "
                     "(difference) / 6")
    with open(out, "w") as f:
        json.dump(res, f, indent=1)
    print(json.dumps(res))


if __name__ == "__main__":
    main()
