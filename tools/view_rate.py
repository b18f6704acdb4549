"""What inference views buy, as one JSON line: B streams stepped with learning=False over ONE learned model at the bench shape
(65 536 columns x 32 cells, bench.py's large_pool: 350 patterns, a learned pool of ~0.65 M segments), for each B in --sizes:

  shared          ModelGroup.views(parent, B).run(...) with BITHTM_SHARED_SCAN=1: the shared scan (kgrp_scan_shared: the store
                  read once per step for each chunk of M members)
  per_member      the same group with BITHTM_SHARED_SCAN=0 (the default): one scan per member (kgrp_scan)
  copies          B full copies (load_state_dict of the parent), learning=False, in a ModelGroup: every copy owns its weights
and, per B, the scan launch's device time per step (htm_profile of an eager run: "group:tm_scan_shared" against the per-member
"group:tm_scan*"), with the device bytes of one view and of one copy (htm_device_bytes).  Aggregate rates are B x steps / s of
the timed call, wrapped in synchronisations; every member cycles through its own noisy copy of the pattern bank.

    python tools/view_rate.py [--sizes 1,2,4,8,16] [--steps 200] [--only shared|per_member] [--out profiles/r09_view_rate.json]
--only: one form of the views' scan alone and nothing else timed (for a counter pass: rocprofv3 --pmc FETCH_SIZE -- python
tools/view_rate.py --sizes 8 --steps 20 --only shared).
"""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np  # noqa: E402

import bithtm_amd as B  # noqa: E402
from bench import LARGE_POOL, build_htm, make_inputs  # noqa: E402


def log(*a):
    print(*a, file=sys.stderr, flush=True)


def timed(group, inputs, steps):
    for m in group.models:
        m.engine.sync()
    t0 = time.perf_counter()
    group.run(inputs, steps, learning=False)
    for m in group.models:
        m.engine.sync()
    return time.perf_counter() - t0


def scan_us(group, inputs, steps):
    """Device time per step of the group's scan launch (and of the whole step), from an eager profiled run."""
    e = group.models[0].engine
    e.profile(True)
    group.run(inputs, steps, learning=False, use_graph=False)
    prof = e.profile_read()
    e.profile(False)
    scan = {n: ms for n, (ms, cnt) in prof.items() if "scan" in n}
    return {n: round(1e3 * ms / steps, 2) for n, ms in scan.items()}, round(1e3 * sum(ms for ms, _ in prof.values()) / steps, 2)


def views_group(parent, n, shared):
    os.environ["BITHTM_SHARED_SCAN"] = "1" if shared else "0"      # (read when each view is made)
    try:
        return B.ModelGroup.views(parent, n)
    finally:
        os.environ.pop("BITHTM_SHARED_SCAN", None)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sizes", default="1,2,4,8,16")
    ap.add_argument("--steps", type=int, default=200)
    ap.add_argument("--only", choices=("shared", "per_member"))
    ap.add_argument("--out")
    args = ap.parse_args()
    sizes = [int(s) for s in args.sizes.split(",")]
    w = dict(LARGE_POOL)
    noisy, perm = make_inputs(w)
    parent = build_htm(w, perm, 0)
    bank = parent.engine.upload_bank(noisy)
    parent.engine.run(bank, noisy.shape[0], 10 * w["patterns"], learning=True)     # the learned state, as bench.py's large_pool
    segments = parent.engine.check_capacity().segments
    log(f"parent: {segments} segments")
    rng = np.random.RandomState(1)
    streams = np.stack([noisy[rng.permutation(len(noisy))[:64]] for _ in range(max(sizes))])
    out = dict(tool="view_rate", shape="65536 columns x 32 cells, 1000 -> 1024 inputs", patterns=w["patterns"], segments=int(segments),
               steps=args.steps, sizes={})
    forms = ("shared", "per_member") if args.only is None else (args.only,)
    copies = []
    if args.only is None:
        st = parent.state_dict()
        for i in range(max(sizes)):
            c = build_htm(w, perm, 0)
            c.load_state_dict(st)
            c.reset()
            copies.append(c)
        del st
    for n in sizes:
        row = {}
        inputs = streams[:n]
        for form in forms:
            g = views_group(parent, n, form == "shared")
            g.run(inputs, 70, learning=False)                     # (untimed: graphs captured)
            dt = timed(g, inputs, args.steps)
            row[form] = dict(timesteps_per_s=round(n * args.steps / dt, 1))
            if args.only is None:
                row[form]["scan_us_per_step"], row[form]["step_us"] = scan_us(g, inputs, 20)
            if form == "shared":
                row["view_bytes"] = g.models[0].engine.device_bytes()
            del g
        if copies:
            g = B.ModelGroup(copies[:n])
            g.run(inputs, 70, learning=False)
            dt = timed(g, inputs, args.steps)
            row["copies"] = dict(timesteps_per_s=round(n * args.steps / dt, 1))
            row["copies"]["scan_us_per_step"], row["copies"]["step_us"] = scan_us(g, inputs, 20)
            row["copy_bytes"] = copies[0].engine.device_bytes()
            del g
        log(n, row)
        out["sizes"][str(n)] = row
    print(json.dumps(out))
    if args.out:
        with open(args.out, "w") as f:
            json.dump(out, f, indent=1)


if __name__ == "__main__":
    main()
