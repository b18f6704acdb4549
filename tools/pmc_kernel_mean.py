#!/usr/bin/env python3
"""Mean of a rocprofv3 counter over the last 150 launches of one kernel (profiles/r16_pmc_summary.txt).  The counter run, one
counter per run and no tracing beside it:

    rocprofv3 --pmc FETCH_SIZE --output-format csv -d OUT -- python3 bench.py --steps 20 --warmup 5 --no-cpu-baseline --no-stress --no-large-pool --no-host-fed
    python tools/pmc_kernel_mean.py OUT [kernel name part, default k_act_mid_rows]
"""
import csv
import glob
import sys

d = sys.argv[1]
kernel = sys.argv[2] if len(sys.argv) > 2 else "k_act_mid_rows"
vals = []
for f in glob.glob(d + "/**/*counter_collection.csv", recursive=True):
    for r in csv.DictReader(open(f)):
        if kernel in r.get("Kernel_Name", ""):
            vals.append((r["Counter_Name"], float(r["Counter_Value"])))
if not vals:
    sys.exit(f"{d}: no launch of {kernel}")
name = vals[0][0]
v = [x for n, x in vals if n == name][-150:]
print(f"{name} of {kernel}, mean of the last {len(v)} launches: {sum(v) / len(v):.1f} (as rocprofv3 reports it, KB)")
