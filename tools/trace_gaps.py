"""Idle time on the stream around one kernel class's launches, from a rocprofv3 --kernel-trace CSV: for every
training step (the dispatches between two k_adam launches) that holds launches of a kernel matching the regex, the
gap from the previous dispatch's end to the first one's start ("before"), between consecutive ones ("between",
summed) and from the last one's end to the next dispatch's start ("after"), with the launches' own time; averaged
over the steps that have the most common launch count (the headline workload's steps).

usage: trace_gaps.py run_kernel_trace.csv [kernel-name regex, default k_mlp_bwd16]
"""
import collections
import csv
import re
import sys

rows = sorted(csv.DictReader(open(sys.argv[1])), key=lambda r: int(r["Start_Timestamp"]))
pat = re.compile(sys.argv[2] if len(sys.argv) > 2 else "k_mlp_bwd16")
adam = [i for i, r in enumerate(rows) if "k_adam" in r["Kernel_Name"]]
steps = []
for s, e in zip(adam[:-1], adam[1:]):
    hit = [i for i in range(s + 1, e) if pat.search(rows[i]["Kernel_Name"])]
    if not hit or hit[0] == 0 or hit[-1] + 1 >= len(rows):
        continue
    st = lambda i: int(rows[i]["Start_Timestamp"])
    en = lambda i: int(rows[i]["End_Timestamp"])
    steps.append({
        "launches": len(hit),
        "grids": tuple(int(rows[i]["Grid_Size_X"]) for i in hit),
        "before": st(hit[0]) - en(hit[0] - 1),
        "between": sum(st(b) - en(b - 1) for b in hit[1:]),
        "after": st(hit[-1] + 1) - en(hit[-1]),
        "kernels": sum(en(i) - st(i) for i in hit),
        "span": en(hit[-1]) - st(hit[0]),
    })
if not steps:
    sys.exit("no step holds a launch of that kernel")
key = collections.Counter((s["launches"], s["grids"]) for s in steps).most_common(1)[0][0]
sel = [s for s in steps if (s["launches"], s["grids"]) == key]
print(f"{len(sel)} steps with {key[0]} launch(es) per step, grid sizes {key[1]} (threads)")
for k in ("before", "between", "after", "kernels", "span"):
    v = [s[k] / 1000 for s in sel]
    print(f"  {k:8s} avg {sum(v) / len(v):9.2f} us   min {min(v):9.2f}   max {max(v):9.2f}")
