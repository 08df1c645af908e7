#!/usr/bin/env python3
"""Summarise a rocprofv3 rocpd database (kernel-trace) with one row per (kernel instance, grid in workgroups): the launches
of one kernel at different pyramid levels or segment plans stay apart, which scripts/rocpd_stats.py's per-kernel table merges.
   python scripts/rocpd_stats_by_grid.py x_results.db [kernel_name_regex] [launches_to_skip_per_row]"""
import re
import sqlite3
import sys

db = sqlite3.connect(sys.argv[1])
want = re.compile(sys.argv[2] if len(sys.argv) > 2 else r"k_[a-z0-9_]+")
skip = int(sys.argv[3]) if len(sys.argv) > 3 else 0
rows = db.execute("select name, grid_x, grid_y, grid_z, workgroup_x, end - start from kernels order by start").fetchall()
by = {}
for name, gx, gy, gz, wx, dur in rows:
    if not want.search(name):
        continue
    m = re.search(r"(k_[a-z0-9_]+(<[^>]*>)?)", name)
    if not m:
        continue
    by.setdefault((m.group(1), "%dx%dx%d" % (gx // max(wx, 1), gy, gz)), []).append(dur / 1e3)
print("%-34s %-14s %5s %11s %9s %9s %9s" % ("instance", "grid", "n", "total_us", "avg", "min", "max"))
for (name, grid), d in sorted(by.items()):
    d = d[skip:]
    if d:
        print("%-34s %-14s %5d %11.1f %9.2f %9.2f %9.2f" % (name, grid, len(d), sum(d), sum(d) / len(d), min(d), max(d)))
# per-step sums of kernel families (a step = the launches between two Histogram launches): what a row's min and max cannot
# give, the spread of a SUM over the steps
marks = [i for i, r in enumerate(rows) if "k_hist" in r[0]]
if len(marks) >= 3:
    for fam in ("k_polyexp", "k_flow_iter3"):
        sums = []
        for a, b in zip([0] + marks, marks + [len(rows)]):
            s = sum(r[5] for r in rows[a:b] if fam in r[0]) / 1e3
            if s > 0:
                sums.append(s)
        if sums:
            print("-- %s: sum per step over %d steps (us): mean %.1f min %.1f max %.1f | %s" % (
                fam, len(sums), sum(sums) / len(sums), min(sums), max(sums), " ".join("%.0f" % s for s in sums)))
