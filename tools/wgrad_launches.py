"""Per-dispatch times of the trunk GEMM launches in a rocprofv3 kernel trace of serialised eager steps
(tools/shard_prof.py).  The critic's, the actor's and the input layer's weight grads share one kernel symbol
(and, at MT50 W = 2048, one grid size), so the launches of a symbol are told apart by their place in the step:
one row per (symbol, grid size, k-th launch of that pair in the step), mean / min / max over the steps.
usage: wgrad_launches.py <kernel_trace.csv> [symbol substring, default gemm_x3p_kernel]"""
import collections
import csv
import statistics
import sys

want = sys.argv[2] if len(sys.argv) > 2 else "gemm_x3p_kernel"
rows = sorted(csv.DictReader(open(sys.argv[1])), key=lambda r: int(r["Start_Timestamp"]))
starts = [int(r["Start_Timestamp"]) for r in rows if "replay_indices" in r["Kernel_Name"]]
a, b = starts[2], starts[-1]  # skip warm-up steps
nsteps = len(starts) - 3
gcol = next(c for c in rows[0] if c.startswith("Grid_Size"))
groups = collections.defaultdict(list)
step, seen = -1, collections.Counter()
for r in rows:
    s = int(r["Start_Timestamp"])
    if not a <= s < b:
        continue
    if "replay_indices" in r["Kernel_Name"]:
        step, seen = step + 1, collections.Counter()
    if want in r["Kernel_Name"]:
        k = r["Kernel_Name"].replace("mtsac::", "").replace("x3pk::", "").split("(")[0][:96]
        groups[(k, int(r[gcol]), seen[(k, r[gcol])])].append((int(r["End_Timestamp"]) - s) / 1e3)
        seen[(k, r[gcol])] += 1
print(f"{nsteps} steps; per (symbol, {gcol}, k-th such launch of the step): mean / min / max us")
for (k, g, i), v in sorted(groups.items()):
    print(f"{statistics.mean(v):8.1f} {min(v):8.1f} {max(v):8.1f}  n {len(v):3d}  launch {i}  grid {g:8d}  {k}")
