"""Summarise a rocprofv3 kernel trace (rocpd SQLite output) of tools/bench_track.py: per-kernel stats (the --stats table) and, per
Track call, the device span from its first to its last kernel (gaps between dependent launches included).  bench_track.py runs, per
volume (the map, then the instance), --reps calls without HIP events and --reps with them (its device-time pass): the four groups
are reported apart.
Usage: python tools/track_trace_summary.py track_results.db stats.csv calls.json"""
import csv
import json
import sqlite3
import sys
from collections import defaultdict

db = sqlite3.connect(sys.argv[1])
rows = list(db.execute("select name, start, end, duration, grid_x, workgroup_x, vgpr_count, scratch_size, lds_size from kernels order by start"))
stats = defaultdict(list)
for name, s, e, d, *_ in rows:
    stats[name].append(d)
total = sum(sum(v) for v in stats.values())
with open(sys.argv[2], "w", newline="") as f:
    w = csv.writer(f, quoting=csv.QUOTE_NONNUMERIC)
    w.writerow(["Name", "Calls", "TotalDurationNs", "AverageNs", "Percentage", "MinNs", "MaxNs"])
    for name, v in sorted(stats.items(), key=lambda kv: -sum(kv[1])):
        w.writerow([name, len(v), sum(v), sum(v) / len(v), round(100.0 * sum(v) / total, 2), min(v), max(v)])
# Track calls: a k_track_pyramid opens a call; the call's kernels are the track kernels up to the next pyramid
calls, cur = [], None
for name, s, e, d, gx, wx, vg, sc, lds in rows:
    short = name.split("(")[0].replace("void ", "")
    if "k_track_" not in short:
        continue
    if "k_track_pyramid" in short:
        cur = {"kernels": []}
        calls.append(cur)
    if cur is not None:
        cur["kernels"].append((short, s, e, d, gx // max(wx, 1)))
out = []
for c in calls:
    ks = c["kernels"]
    span = (ks[-1][2] - ks[0][1]) / 1e3
    busy = sum(k[3] for k in ks) / 1e3
    out.append(dict(launches=len(ks), span_us=round(span, 2), kernel_us=round(busy, 2),
                    first_grid=ks[1][4] if len(ks) > 1 else None))
q = len(out) // 4
groups = {"map": out[:q], "map_with_hip_events": out[q:2 * q], "instance": out[2 * q:3 * q], "instance_with_hip_events": out[3 * q:]}


def agg(lst):
    sp = sorted(x["span_us"] for x in lst)
    kb = sorted(x["kernel_us"] for x in lst)
    return dict(n=len(lst), launches=lst[0]["launches"] if lst else None, span_us_median=sp[len(sp) // 2], span_us_min=sp[0],
                kernel_us_median=kb[len(kb) // 2])


summary = {k: agg(v) for k, v in groups.items()}
print(json.dumps(summary))
with open(sys.argv[3], "w") as f:
    json.dump(dict(summary, per_call=out), f, indent=1)
