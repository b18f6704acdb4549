"""What a region stack costs, as one JSON object: RegionStack.run at 1 000 -> 65 536 x 32 -> 8 192 x 32, stride 1 and stride 4,
over calls of --steps steps with graph replay after a warm-up, and on the same build and the same learned state its three parts
alone:

  level0          level 0 alone, recorded with "active_column" (Engine.run_into: what the stack's first launch sequence does)
  level1          level 1 alone over the bank the stack's last chunk packed (steps / stride steps)
  pack            the htm_pack_columns launch of one chunk alone
Every figure is the median of --repeats calls wrapped in synchronisations, with the spread (max - min) beside it; the expectation
is stack = level0 + level1 + pack plus one chunk boundary per level per chunk.  Level 1's float64 permanences are 8 192 x 65 536
x 8 bytes = 4.3 GB of device memory (and as much host memory while the model is built); level 0's are 0.5 GB.

    python tools/stack_rate.py [--steps 2000] [--repeats 3] [--strides 1,4] [--out profiles/r10_stack_rate.json]
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


def log(*a):
    print(*a, file=sys.stderr, flush=True)


def timed(sync, fn, repeats):
    """Seconds of fn() between two synchronisations: (median, max - min) over `repeats` calls."""
    out = []
    for _ in range(repeats):
        sync()
        t0 = time.perf_counter()
        fn()
        sync()
        out.append(time.perf_counter() - t0)
    return float(np.median(out)), float(max(out) - min(out))


def measure(stride, steps, repeats, patterns=50):
    rng = np.random.RandomState(0)
    inputs = rng.rand(patterns, 1000) < 0.1
    stack = B.RegionStack(1000, [(65536, 32), (8192, 32)], strides=[stride], seed=0)
    lower, upper = (m.engine for m in stack.levels)
    sync = lower.sync                               # (one stream)
    for _ in range(2):                              # untimed: graphs captured, the default-sized pools grown
        stack.run(inputs, steps)
    lower, upper = (m.engine for m in stack.levels)
    row = dict(stride=stride, steps=steps, chunk_steps=stack.chunk_steps, chunks_per_call=len(stack.last_run_chunks))
    dt, spread = timed(sync, lambda: stack.run(inputs, steps), repeats)
    row["stack"] = dict(seconds=round(dt, 5), spread=round(spread, 5), level0_steps_per_s=round(steps / dt, 1))
    chunk = stack.last_run_chunks[-1][0]
    lists = stack._bufs[(0, "active_column")][0]
    bank1 = stack._bufs[(1, "bank")][0]
    bank0 = stack.levels[0]._bank[1]
    k0, rows = stack.levels[0].active_columns, chunk // stride

    def level0():
        done = 0
        while done < steps:
            n = min(chunk, steps - done)
            lower.run_into(bank0, patterns, n, {"active_column": lists})
            done += n

    def level1():
        done = 0
        while done < steps:
            n = min(chunk, steps - done) // stride
            upper.run_into(bank1, n, n, {})
            done += n * stride

    def pack():
        done = 0
        while done < steps:
            n = min(chunk, steps - done) // stride
            upper.pack_columns(lists, k0, n, stride, bank1, n, upper.steps % n)
            done += n * stride

    for name, fn in (("level0", level0), ("level1", level1), ("pack", pack)):
        fn()                                        # (untimed: its own graphs)
        dt, spread = timed(sync, fn, repeats)
        row[name] = dict(seconds=round(dt, 5), spread=round(spread, 5))
    row["parts_sum_seconds"] = round(sum(row[n]["seconds"] for n in ("level0", "level1", "pack")), 5)
    row["segments"] = [int(m.engine.check_capacity().segments) for m in stack.levels]
    log(row)
    return row


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=2000)
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--strides", default="1,4")
    ap.add_argument("--out")
    args = ap.parse_args()
    out = dict(tool="stack_rate", shape="1000 -> 65536 x 32 -> 8192 x 32", runs=[measure(int(s), args.steps, args.repeats)
                                                                                for s in args.strides.split(",")])
    print(json.dumps(out))
    if args.out:
        with open(args.out, "w") as f:
            json.dump(out, f, indent=1)


if __name__ == "__main__":
    main()
