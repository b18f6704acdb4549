"""Live-tick rates of model groups at the reference shape (1 000 inputs -> 2 048 columns x 32 cells, two scalar fields, learned
members), as one JSON line (and, with --out, a file: profiles/r14_tick_rate.json).

Per group size B (default 1, 8, 64, 256), alternating in one process, --repeats times round:
  tick_graph    group.tick(values, encoder=enc)                  host wall time per tick over --ticks ticks (BITHTM_EAGER_BELOW = 0,
  tick_eager    group.tick(values, encoder=enc, use_graph=False)   so use_graph alone decides how the step is launched)
  run_1         group.run(values[:, None, :], 1, encoder=enc, record=("counters", "predicted_value")) -- the batched call of one step:
                B banks uploaded and encoded, B records read
  process       enc.encode(values) on the host, group.process, group.predicted_value -- the host-fed tick: per member a read-back,
                a capacity check, and two launches with a read-back for the prediction
The last two are what the library offered for the same result before the tick; they run over fewer ticks at large B (the count is
in the output).  device_us is the time of the tick's launches by HIP events (htm_profile on the first member, whose handle the
group's launches are counted on; profiled launches are eager), per tick over --profiled ticks, with the launch count.

Each leg runs after an untimed tick of its kind; times are the median of the rounds with the lowest and the highest.

    python tools/tick_rate.py [--sizes 1,8,64,256] [--ticks 200] [--repeats 3] [--out profiles/r14_tick_rate.json]
"""
import argparse
import json
import os
import sys
import time

os.environ["BITHTM_EAGER_BELOW"] = "0"
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np  # noqa: E402

import bithtm_amd as B  # noqa: E402

SHAPE = dict(input_dim=1000, column_dim=2048, cell_dim=32)
RECORD = ("counters", "predicted_value")


def log(*a):
    print(*a, file=sys.stderr, flush=True)


def encoder():
    return B.ScalarEncoder([B.ScalarField(0.0, 100.0, 500, 21), B.ScalarField(0.0, 7.0, 500, 25, periodic=True)], input_dim=1000)


def stream(n, rows, seed, period=10):
    """float64 [rows, n, 2]: per member a sequence of `period` value pairs, repeated, with a little noise on the first field."""
    rng = np.random.RandomState(seed)
    base = np.stack([100.0 * rng.rand(n, period), 7.0 * rng.rand(n, period)], axis=-1)
    v = base[:, np.arange(rows) % period].transpose(1, 0, 2).copy()
    v[:, :, 0] += rng.randn(rows, n)
    return v


def spread(times, ticks):
    us = sorted(1e6 * t / ticks for t in times)
    return dict(us_per_tick=round(us[len(us) // 2], 1), lowest=round(us[0], 1), highest=round(us[-1], 1), ticks=ticks)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sizes", default="1,8,64,256")
    ap.add_argument("--ticks", type=int, default=200)
    ap.add_argument("--profiled", type=int, default=50)
    ap.add_argument("--train", type=int, default=200)
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--out")
    args = ap.parse_args()
    enc = encoder()
    out = dict(tool="tick_rate", shape="1000 inputs -> 2048 columns x 32 cells, 2 fields", ticks=args.ticks, sizes={})
    for n in [int(x) for x in args.sizes.split(",")]:
        group = B.ModelGroup.create(n, seeds=range(n), **SHAPE)
        values = stream(n, args.train + args.ticks, 7 + n)
        group.run(np.ascontiguousarray(values[:args.train].transpose(1, 0, 2)), args.train, encoder=enc)
        live = values[args.train:]
        sync = group.models[0].engine.sync
        few = max(20, args.ticks // max(1, n // 16))       # (the older paths cost milliseconds per member)

        def tick(use_graph):
            return lambda v: group.tick(v, encoder=enc, use_graph=use_graph)

        def run_1(v):
            group.run(v[:, None, :], 1, encoder=enc, record=RECORD)

        def process(v):
            group.process(enc.encode(v))
            group.predicted_value(enc)

        legs = dict(tick_graph=(tick(True), args.ticks), tick_eager=(tick(False), args.ticks), run_1=(run_1, few), process=(process, few))
        times = {name: [] for name in legs}
        for _ in range(args.repeats):
            for name, (fn, ticks) in legs.items():
                fn(live[0])
                sync()
                t0 = time.perf_counter()
                for t in range(ticks):
                    fn(live[t % len(live)])
                sync()
                times[name].append(time.perf_counter() - t0)
        res = {name: spread(times[name], legs[name][1]) for name in legs}
        eng = group.models[0].engine
        group.tick(live[0], encoder=enc)
        eng.profile(True)
        for t in range(args.profiled):
            group.tick(live[t % len(live)], encoder=enc)
        prof = eng.profile_read()
        eng.profile(False)
        res["device_us"] = round(1e3 * sum(ms for ms, _ in prof.values()) / args.profiled, 1)
        res["launches_per_tick"] = sum(c for _, c in prof.values()) / args.profiled
        res["device_us_by_launch"] = {name: round(1e3 * ms / args.profiled, 2) for name, (ms, _) in sorted(prof.items())}
        segs = [int(m.engine.info().segments) for m in group.models[:4]]
        res["segments_of_the_first_members"] = segs
        out["sizes"][str(n)] = res
        log(n, {k: v for k, v in res.items() if k != "device_us_by_launch"})
        del group
    print(json.dumps(out))
    if args.out:
        with open(args.out, "w") as fh:
            json.dump(out, fh, indent=1)


if __name__ == "__main__":
    main()
