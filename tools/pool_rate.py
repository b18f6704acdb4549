"""What a pooling link costs, as one JSON object: RegionStack.run at 1 000 -> 65 536 x 32 -> 8 192 x 32 with a PoolingLink (the
defaults: active_weight 1, predicted_weight 8, decay 1, ceiling 16, union_bits 2 x 1 311) against the plain link, stride 1 and
stride 4, over calls of --steps steps with graph replay after a warm-up.  Per stride, on one device in one process:

  plain, pooled   seconds per call, the median of --repeats calls wrapped in synchronisations with the lowest and the highest, the
                  two stacks taking turns and the one that comes first alternating.  The upper levels see different rows, so the
                  two differ by more than the link: `level0` below is the part that is the same work.
  level0          the pooled stack's level 0 alone, recorded with what the link reads (active_column and column_prediction), and
                  the plain stack's (active_column)
  launches        device time of the link's launches of one call (htm_profile: the kernels' own begin and end stamps): pool_pack,
                  pool_scan and pool_select, and the plain link's pack_columns
  process         the stepwise stack.process() loop over --process-steps steps of the pooled stack: the host alternative
And, with --parent DIR (a checkout of the parent commit with its library built), bench.py's headline (--steps 2000 --warmup 200)
alone (no CPU baseline, no further legs) from this tree and from DIR in turns, --bench-runs runs each, as medians.

    python tools/pool_rate.py [--steps 2000] [--repeats 5] [--strides 1,4] [--parent DIR] [--out profiles/r23_pool_rate.json]
"""
import argparse
import json
import os
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np  # noqa: E402

import bithtm_amd as B  # noqa: E402


def log(*a):
    print(*a, file=sys.stderr, flush=True)


def spread(ts):
    return dict(median=round(float(np.median(ts)), 5), low=round(float(min(ts)), 5), high=round(float(max(ts)), 5))


def once(sync, fn):
    sync()
    t0 = time.perf_counter()
    fn()
    sync()
    return time.perf_counter() - t0


def link_launches(stack, inputs, steps):
    """Device milliseconds and launch counts of the link's launches over one call."""
    upper = stack.levels[1].engine
    upper.profile(True)
    stack.run(inputs, steps)
    upper.sync()
    prof = upper.profile_read(256)
    upper.profile(False)
    return {name: dict(ms=round(ms, 4), launches=int(n)) for name, (ms, n) in prof.items() if name.startswith(("pool_", "pack_columns"))}


def measure(stride, steps, repeats, process_steps, patterns=50):
    rng = np.random.RandomState(0)
    inputs = rng.rand(patterns, 1000) < 0.1
    stacks = {"plain": B.RegionStack(1000, [(65536, 32), (8192, 32)], links=[stride], seed=0),
              "pooled": B.RegionStack(1000, [(65536, 32), (8192, 32)], links=[B.PoolingLink(stride)], seed=0)}
    sync = stacks["plain"].levels[0].engine.sync
    for s in stacks.values():
        for _ in range(2):                          # untimed: graphs captured, the default-sized pools grown
            s.run(inputs, steps)
    row = dict(stride=stride, steps=steps, union_bits=stacks["pooled"].links[0].union_bits, chunk_steps=stacks["pooled"].chunk_steps)
    times = {name: [] for name in stacks}
    for r in range(repeats):
        for name in (("plain", "pooled") if r % 2 == 0 else ("pooled", "plain")):
            s = stacks[name]
            times[name].append(once(lambda: [m.engine.sync() for m in s.levels], lambda: s.run(inputs, steps)))
    for name in stacks:
        row[name] = dict(seconds=spread(times[name]), level0_steps_per_s=round(steps / float(np.median(times[name])), 1))
    row["pooled_over_plain"] = round(float(np.median(times["pooled"]) / np.median(times["plain"])), 4)
    # level 0 alone, recording what each link reads
    for name, fields in (("plain", ("active_column",)), ("pooled", ("active_column", "column_prediction"))):
        s = stacks[name]
        lower = s.levels[0].engine
        bufs = {f: s._bufs[(0, f)][0] for f in fields}
        bank0 = s.levels[0]._bank[1]
        chunk = s.last_run_chunks[-1][0]

        def level0():
            done = 0
            while done < steps:
                n = min(chunk, steps - done)
                lower.run_into(bank0, patterns, n, bufs)
                done += n
        level0()
        row[name]["level0_seconds"] = spread([once(lower.sync, level0) for _ in range(repeats)])
    row["launches"] = {name: link_launches(s, inputs, steps) for name, s in stacks.items()}
    pooled = stacks["pooled"]
    n = process_steps // stride * stride
    t = once(lambda: [m.engine.sync() for m in pooled.levels], lambda: [pooled.process(inputs[i % patterns]) for i in range(n)])
    row["process"] = dict(steps=n, seconds=round(t, 4), steps_per_s=round(n / t, 1))
    row["segments"] = {name: [int(m.engine.check_capacity().segments) for m in s.levels] for name, s in stacks.items()}
    log(row)
    return row


def headline(tree):
    r = subprocess.run([sys.executable, "bench.py", "--gpus", "1", "--steps", "2000", "--warmup", "200", "--no-cpu-baseline", "--no-stress", "--no-large-pool",
                        "--no-host-fed"], cwd=tree, capture_output=True, text=True, timeout=600)
    if r.returncode != 0:
        raise RuntimeError(f"bench.py in {tree} failed:\n{(r.stdout + r.stderr)[-2000:]}")
    res = json.loads(r.stdout.strip().splitlines()[-1])
    return res


def bench_ab(parent, runs):
    out = {"this": [], "parent": []}
    for r in range(runs):
        for name, tree in ((("this", ROOT), ("parent", parent)) if r % 2 == 0 else (("parent", parent), ("this", ROOT))):
            res = headline(tree)
            value = res.get("value", res.get("timesteps_per_s"))
            out[name].append(value)
            log(name, value)
    return dict(runs=out, median={k: float(np.median(v)) for k, v in out.items()}, unit="bench.py's headline value")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=2000)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--strides", default="1,4")
    ap.add_argument("--process-steps", type=int, default=200)
    ap.add_argument("--parent")
    ap.add_argument("--bench-runs", type=int, default=3)
    ap.add_argument("--out")
    args = ap.parse_args()
    out = dict(tool="pool_rate", shape="1000 -> 65536 x 32 -> 8192 x 32",
               runs=[measure(int(s), args.steps, args.repeats, args.process_steps) for s in args.strides.split(",") if s])
    if args.parent:
        out["bench"] = bench_ab(os.path.abspath(args.parent), args.bench_runs)
    print(json.dumps(out))
    if args.out:
        with open(args.out, "w") as f:
            json.dump(out, f, indent=1)


if __name__ == "__main__":
    main()
