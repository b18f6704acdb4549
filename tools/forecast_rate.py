"""Closed-loop forecast rates at the bench shape (65 536 columns x 32 cells, bench.py's headline workload, learned), as one JSON
line.  An inference view of the learned model, given a few context steps, rolls forward on its own encoded votes:

  host     the loop forecast() replaces, on calls that exist without it -- per step predicted_input() (a launch and a
           synchronising copy), encode on the host (NumPy), process(x, learning=False) (an upload and the step's launches)
  device   view.forecast(steps): the loop on the device (htm_set_run_feedback), rows read back once per call
  group    ModelGroup.views(parent, B).forecast(steps) for each B of --group: B streams, one launch sequence per step

Each leg is timed --repeats times between synchronisations after an untimed call (graphs captured); the line holds the median
rate and the lowest and highest (the run-to-run spread), in forecast steps per second (the group's: B x steps).  The host leg
uses nothing this tool's commit added, so the same file runs beside an older checkout with --legs host.

    python tools/forecast_rate.py [--steps 256] [--repeats 5] [--min-votes 1] [--max-bits 20] [--group 4,16] [--legs host,device,group]
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
from bench import WORKLOAD, build_htm, make_inputs  # noqa: E402


def log(*a):
    print(*a, file=sys.stderr, flush=True)


def encode(votes, min_votes, max_bits):
    x = votes >= min_votes
    if max_bits and x.sum() > max_bits:
        keep = np.lexsort((np.arange(votes.size), -votes.astype(np.int64)))[:max_bits]
        x = np.zeros(votes.size, bool)
        x[keep] = True
    return x


def host_loop(view, steps, min_votes, max_bits):
    bits = 0
    for _ in range(steps):
        x = encode(view.predicted_input(), min_votes, max_bits)
        view.process(x, learning=False)
        bits += int(x.sum())
    return bits


def rates(fn, sync, steps, repeats):
    """fn() timed `repeats` times after one untimed call: (median, lowest, highest) steps per second."""
    fn()
    out = []
    for _ in range(repeats):
        sync()
        t0 = time.perf_counter()
        fn()
        sync()
        out.append(steps / (time.perf_counter() - t0))
    out.sort()
    return dict(steps_per_s=round(out[len(out) // 2], 1), lowest=round(out[0], 1), highest=round(out[-1], 1))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=256)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--min-votes", type=int, default=1)
    ap.add_argument("--max-bits", type=int, default=20)
    ap.add_argument("--group", default="4,16")
    ap.add_argument("--legs", default="host,device,group")
    ap.add_argument("--train", type=int, default=1000)
    ap.add_argument("--out")
    args = ap.parse_args()
    legs = args.legs.split(",")
    w = dict(WORKLOAD)
    noisy, perm = make_inputs(w)
    parent = build_htm(w, perm, 0)
    parent.run(noisy, args.train)
    segments = parent.engine.check_capacity().segments
    log(f"parent: {args.train} learning steps, {segments} segments")
    context = noisy[:w["patterns"]]
    mv, mb = args.min_votes, args.max_bits
    out = dict(tool="forecast_rate", shape="65536 columns x 32 cells, 1024 inputs", segments=int(segments), steps=args.steps,
               repeats=args.repeats, min_votes=mv, max_bits=mb)

    def fresh_view():
        v = parent.inference_view()
        v.run(context, 8)
        return v

    if "host" in legs:
        v = fresh_view()
        bits = host_loop(v, 16, mv, mb)
        out["host"] = rates(lambda: host_loop(v, args.steps, mv, mb), v.engine.sync, args.steps, args.repeats)
        out["host"]["bits_per_row_first_16"] = round(bits / 16, 1)
        log("host", out["host"])
        del v
    if "device" in legs:
        v = fresh_view()
        rows = v.forecast(16, mv, mb)
        out["device"] = rates(lambda: v.forecast(args.steps, mv, mb), v.engine.sync, args.steps, args.repeats)
        out["device"]["bits_per_row_first_16"] = round(float(rows.sum()) / 16, 1)
        out["device"]["plan"] = v.engine.run_plan(args.steps)
        v.engine.profile(True)
        v.forecast(16, mv, mb, use_graph=False)
        prof = v.engine.profile_read()
        v.engine.profile(False)
        out["device"]["launches_per_step"] = round(sum(n for _, n in prof.values()) / 16, 2)
        out["device"]["kernel_us_per_step"] = {name: round(1e3 * ms / 16, 2) for name, (ms, _) in sorted(prof.items())}
        log("device", out["device"])
        del v
    if "group" in legs:
        out["group"] = {}
        for n in [int(s) for s in args.group.split(",") if s]:
            g = B.ModelGroup.views(parent, n)
            streams = np.stack([np.roll(context, i, axis=0) for i in range(n)])
            g.run(streams, 8)
            sync = lambda: [m.engine.sync() for m in g.models]      # noqa: E731
            out["group"][str(n)] = rates(lambda: g.forecast(args.steps, mv, mb), sync, n * args.steps, args.repeats)
            log("group", n, out["group"][str(n)])
            del g
    print(json.dumps(out))
    if args.out:
        with open(args.out, "w") as f:
            json.dump(out, f, indent=1)


if __name__ == "__main__":
    main()
