#!/usr/bin/env python3
"""The compiler's per-kernel figures of two builds side by side (profiles/r16_resources.txt): which kernels changed, which are new.

    python tools/resources_diff.py PARENT/bithtm_amd/libbithtm_hip.resources.json bithtm_amd/libbithtm_hip.resources.json [name part ...]
"""
import json
import sys

par, new = json.load(open(sys.argv[1])), json.load(open(sys.argv[2]))
print("changed:", [k for k in par if par[k] != new.get(k)], " new:", sorted(k for k in new if k not in par))
for k in sorted(new):
    if any(s in k for s in sys.argv[3:]):
        print(k, "\n   parent:", par.get(k), "\n   now:   ", new[k])
