"""List the idle intervals of the last solve in a rocprofv3 kernel trace (csv) as JSON: every gap between kernels longer than
--min-us with the kernels on either side, the busy and idle totals, and the launch count per kernel name.

A solve begins with a launch of nd_maxabs2_kernel (the first kernel of a factorisation): the solve listed is the last one that
another follows, from its first kernel to its last; the idle time up to the next solve's first kernel is given beside it.

usage: idle_gaps.py KERNEL_TRACE.csv [--min-us 20] [--out FILE.json]
"""
import argparse
import csv
import json
from collections import Counter


def short(name):
    name = name.replace("(anonymous namespace)::", "").replace("void ", "")
    return name.split("(")[0].split("<")[0]


ap = argparse.ArgumentParser()
ap.add_argument("trace")
ap.add_argument("--min-us", type=float, default=20.0)
ap.add_argument("--out", default="")
args = ap.parse_args()
rows = []
with open(args.trace) as f:
    for r in csv.DictReader(f):
        rows.append((int(r["Start_Timestamp"]), int(r["End_Timestamp"]), short(r["Kernel_Name"])))
rows.sort()
heads = [i for i, r in enumerate(rows) if r[2] == "nd_maxabs2_kernel"]
if len(heads) < 2:
    raise SystemExit("the trace holds fewer than two factorisations: run at least two solves")
between_us = 1e-3 * (rows[heads[-1]][0] - max(r[1] for r in rows[heads[-2]:heads[-1]]))
rows = rows[heads[-2]:heads[-1]]
t0 = rows[0][0]
cur_end, cur_name, busy = rows[0][0], rows[0][2], 0
gaps, small = [], 0
for s, e, name in rows:
    if s > cur_end:
        if s - cur_end >= args.min_us * 1e3:
            gaps.append({"at_ms": round(1e-6 * (cur_end - t0), 3), "us": round(1e-3 * (s - cur_end), 1), "after": cur_name, "before": name})
        else:
            small += s - cur_end
        busy += e - s
        cur_end, cur_name = e, name
    elif e > cur_end:
        busy += e - cur_end
        cur_end, cur_name = e, name
window = cur_end - t0
out = {"window_ms": round(1e-6 * window, 3), "busy_ms": round(1e-6 * busy, 3), "idle_ms": round(1e-6 * (window - busy), 3),
       "idle_in_listed_gaps_ms": round(1e-3 * sum(g["us"] for g in gaps), 3), "idle_in_shorter_gaps_ms": round(1e-6 * small, 3),
       "idle_until_next_solve_us": round(between_us, 1), "min_gap_us": args.min_us, "kernels": len(rows), "gaps": gaps, "launches": dict(sorted(Counter(r[2] for r in rows).items()))}
text = json.dumps(out, indent=1)
if args.out:
    with open(args.out, "w") as f:
        f.write(text + "\n")
print(text)
