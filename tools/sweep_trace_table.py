"""The last bit-parallel sweep of a rocprofv3 kernel trace as a table (tools/sweep_route_trace.sh):
python tools/sweep_trace_table.py <..._kernel_trace.csv>
Every kernel, fill and copy from the last batch_seed_kernel to the label pass with its start, its duration and the gap to
its predecessor's end, then the sums: kernel time, the gaps in front of a level's first kernel (the host turning the
level round: what follows a batch_totals_kernel, a batch_tail_kernel or the seed) and all other gaps."""
import csv
import sys

rows = list(csv.DictReader(open(sys.argv[1])))
if rows and "start_ns" in rows[0]:                            # the reduced form kept under profiles/ (kernel, start_ns, duration_ns)
    rows = [{"Kernel_Name": r["kernel"], "Start_Timestamp": r["start_ns"], "End_Timestamp": str(int(r["start_ns"]) + int(r["duration_ns"]))}
            for r in rows]
rows.sort(key=lambda r: int(r["Start_Timestamp"]))
name = lambda r: r["Kernel_Name"].split("(")[0].replace("grb::", "").replace("void ", "")
first = max(i for i, r in enumerate(rows) if "batch_seed" in r["Kernel_Name"])
# the fills in front of the seed (counters, seen, tail state) belong to the sweep: go back while the gap stays short
while first > 0 and "batch_" not in rows[first - 1]["Kernel_Name"] and \
        int(rows[first]["Start_Timestamp"]) - int(rows[first - 1]["End_Timestamp"]) < 20000:
    first -= 1
last = max(i for i, r in enumerate(rows) if "batch_labels" in r["Kernel_Name"])
t0 = int(rows[first]["Start_Timestamp"])
busy = level_gaps = other_gaps = 0.0
launches = 0
prev_end, level_start = None, True
print("%-44s %10s %9s %9s" % ("kernel", "start us", "dur us", "gap us"))
for r in rows[first:last + 1]:
    s, e = int(r["Start_Timestamp"]), int(r["End_Timestamp"])
    gap = 0.0 if prev_end is None else max(0.0, (s - prev_end) / 1e3)
    nm = name(r)
    print("%-44s %10.1f %9.1f %9.1f%s" % (nm[:44], (s - t0) / 1e3, (e - s) / 1e3, gap, "  <- level" if level_start and prev_end else ""))
    busy += (e - s) / 1e3
    launches += 1
    if prev_end is not None:
        if level_start:
            level_gaps += gap
        else:
            other_gaps += gap
    level_start = "batch_totals" in nm or "batch_tail" in nm
    prev_end = e if prev_end is None else max(prev_end, e)
span = (int(rows[last]["End_Timestamp"]) - t0) / 1e3
print("launches %d  span %.1f us  kernel time %.1f us  gaps before a level's first kernel %.1f us  other gaps %.1f us"
      % (launches, span, busy, level_gaps, other_gaps))
