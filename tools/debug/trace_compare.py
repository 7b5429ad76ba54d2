"""Two rocprofv3 kernel-stats CSVs (tools/debug/trace_libs.sh writes them: t_kernel_stats.csv per library) side by side: calls and
average duration of every kernel whose name matches the pattern, and the difference summed over a step's calls.
usage: python tools/debug/trace_compare.py old_kernel_stats.csv new_kernel_stats.csv 'substring|substring' [steps traced]"""
import csv
import re
import sys

old, new, pat = sys.argv[1:4]
steps = int(sys.argv[4]) if len(sys.argv) > 4 else 52        # bench.py --steps 30 --warmup 5 replays the captured step 52 times
load = lambda f: {r["Name"]: (int(r["Calls"]), float(r["AverageNs"]) / 1e3) for r in csv.DictReader(open(f)) if re.search(pat, r["Name"])}
a, b = load(old), load(new)
total = 0.0
for name in sorted(set(a) | set(b)):
    ca, ta = a.get(name, (0, 0.0))
    cb, tb = b.get(name, (0, 0.0))
    per_step = (cb * tb - ca * ta) / steps
    total += per_step
    print("%-88s calls %5d / %5d  avg %7.2f -> %7.2f us  (%+6.2f us per step)" % (re.sub(r"\(anonymous namespace\)::|void ", "", name)[:88], ca, cb, ta, tb, per_step))
print("sum over the matched kernels: %+.1f us per step (%d steps traced)" % (total, steps))
