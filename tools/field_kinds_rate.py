"""What the field kinds cost on the device, as one JSON line (and, with --out, a file:
profiles/r17_field_kinds_rate.json).  The baseline is the linear kernels of the same build -- k_bank_encode, k_decode_votes,
klive_finish, which a table of linear fields launches exactly as the parent commit does -- and the legs alternate in one process.

  One row of 1 000 inputs holds two fields of 500 bits and width 21 side by side: "linear" has two linear fields (the older
  kernels), "mixed" a linear field and a hashed field of 1 000 buckets over the same bits and width (the twins).

  kernels  at the bench shape (65 536 columns x 32 cells, input_dim 1 000): Engine.bank_encode of a --rows-row bank and
           Engine.decode_votes of --rows vote rows, per table; device time per launch from the engine's profile events
           (htm_profile), --launches launches a round, --repeats rounds, the table that comes first alternating; and the host
           wall time of the same launches between two synchronisations
  tick     a group of --members members at tools/tick_rate.py's shape (1 000 inputs -> 2 048 columns x 32 cells), trained over
           --train rows: host wall time per group.tick(values, encoder=) with either table over --ticks ticks, the legs taking
           turns every 20 ticks inside a round and the first turn alternating, and the device time of the encode and finish
           launches of a tick (htm_profile)

Every figure is the median of the rounds with the lowest and the highest.

    python tools/field_kinds_rate.py [--rows 1000] [--launches 50] [--members 64] [--ticks 200] [--train 200] [--repeats 5]
                                     [--out profiles/r17_field_kinds_rate.json]
"""
import argparse
import json
import os
import sys
import time

os.environ["BITHTM_EAGER_BELOW"] = "0"
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))
import numpy as np  # noqa: E402

import bithtm_amd as B  # noqa: E402
from bench import WORKLOAD, build_htm, make_inputs  # noqa: E402
from tick_rate import SHAPE, log  # noqa: E402

SLICE = 20                                  # ticks a leg takes before the other leg's turn


def tables():
    linear = B.ScalarEncoder([B.ScalarField(0.0, 100.0, 500, 21), B.ScalarField(0.0, 100.0, 500, 21)], input_dim=1000)
    mixed = B.ScalarEncoder([B.ScalarField(0.0, 100.0, 500, 21), B.HashedField(0.0, 100.0, 500, 21, buckets=1000, seed=1)], input_dim=1000)
    return {"linear": linear, "mixed": mixed}


def median(values, digits=2):
    v = sorted(values)
    return dict(median=round(v[len(v) // 2], digits), lowest=round(v[0], digits), highest=round(v[-1], digits))


def stream(n, rows, seed, period=10):
    """float64 [rows, n, 2]: per member a sequence of `period` value pairs in [0, 100), repeated, with a little noise."""
    rng = np.random.RandomState(seed)
    base = 100.0 * rng.rand(n, period, 2)
    return base[:, np.arange(rows) % period].transpose(1, 0, 2) + 0.3 * rng.randn(rows, n, 2)


def kernels(args, out):
    w = dict(WORKLOAD, input_dim=1000)
    _, perm = make_inputs(w)
    eng = build_htm(w, perm, 0).engine
    encs = tables()
    rng = np.random.RandomState(1)
    values = rng.uniform(-5.0, 105.0, (args.rows, 2))
    votes = rng.randint(0, 40, (args.rows, 1000)).astype(np.int32)
    d_values, d_bank = eng.upload_values(values), eng.zero_bank(args.rows)
    d_votes, d_out = eng.device_buffer(votes.nbytes, votes), eng.device_buffer(args.rows * 2 * 2 * 4)
    calls = {"bank_encode": lambda enc: eng.bank_encode(enc, d_values, args.rows, d_bank, args.rows),
             "decode_votes": lambda enc: eng.decode_votes(enc, d_votes, args.rows, d_out)}
    # (that both tables compute their definition here, before anything is timed)
    for name, enc in encs.items():
        calls["bank_encode"](enc)
        assert np.array_equal(eng.read_bank(d_bank, args.rows), enc.encode(values)), name
    res = {}
    for what, call in calls.items():
        device = {name: [] for name in encs}
        wall = {name: [] for name in encs}
        for r in range(args.repeats + 1):           # (round 0 is the warm-up)
            for name in (list(encs) if r % 2 == 0 else list(encs)[::-1]):
                eng.sync()
                t0 = time.perf_counter()
                for _ in range(args.launches):
                    call(encs[name])
                eng.sync()
                t1 = time.perf_counter()
                eng.profile(True)
                for _ in range(args.launches):
                    call(encs[name])
                prof = eng.profile_read()
                eng.profile(False)
                if r:
                    wall[name].append(1e6 * (t1 - t0) / args.launches)
                    device[name].append(1e3 * prof[what][0] / prof[what][1])
        res[what] = {name: dict(device_us_per_launch=median(device[name]), wall_us_per_launch=median(wall[name])) for name in encs}
        log(what, res[what])
    out["kernels"] = dict(shape="65536 columns x 32 cells, 1000 inputs", rows=args.rows, launches_per_round=args.launches, **res)


def ticks(args, out):
    n = args.members
    encs = tables()
    group = B.ModelGroup.create(n, seeds=range(n), **SHAPE)
    values = stream(n, args.train + args.ticks, 7 + n)
    group.run(np.ascontiguousarray(values[:args.train].transpose(1, 0, 2)), args.train, encoder=encs["mixed"])
    live = values[args.train:]
    sync = group.models[0].engine.sync
    times = {name: [] for name in encs}
    for enc in encs.values():
        group.tick(live[0], encoder=enc)
        group.tick(live[1], encoder=enc)
    for r in range(args.repeats):
        spent, at = {name: 0.0 for name in encs}, 0
        for piece in range(-(-args.ticks // SLICE)):
            count = min(SLICE, args.ticks - piece * SLICE)
            for name in (list(encs) if (piece + r) % 2 == 0 else list(encs)[::-1]):
                sync()
                t0 = time.perf_counter()
                for t in range(at, at + count):
                    group.tick(live[t % len(live)], encoder=encs[name])
                sync()
                spent[name] += time.perf_counter() - t0
            at += count
        for name in encs:
            times[name].append(1e6 * spent[name] / args.ticks)
    res = {name: dict(wall_us_per_tick=median(times[name], 1)) for name in encs}
    eng = group.models[0].engine
    for name, enc in encs.items():
        eng.profile(True)
        for t in range(40):
            group.tick(live[t % len(live)], encoder=enc)
        prof = eng.profile_read()
        eng.profile(False)
        res[name]["launches_per_tick"] = sum(c for _, c in prof.values()) / 40
        res[name]["encode_launch_us"] = round(1e3 * prof["live:encode"][0] / prof["live:encode"][1], 2)
        res[name]["finish_launch_us"] = round(1e3 * prof["live:finish"][0] / prof["live:finish"][1], 2)
    out["tick"] = dict(shape="1000 inputs -> 2048 columns x 32 cells", members=n, ticks=args.ticks, **res)
    log("tick", out["tick"])


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", type=int, default=1000)
    ap.add_argument("--launches", type=int, default=50)
    ap.add_argument("--members", type=int, default=64)
    ap.add_argument("--ticks", type=int, default=200)
    ap.add_argument("--train", type=int, default=200)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--out")
    args = ap.parse_args()
    out = dict(tool="field_kinds_rate", table="two fields of 500 bits, width 21: linear + linear against linear + hashed (1000 buckets)")
    kernels(args, out)
    ticks(args, out)
    print(json.dumps(out))
    if args.out:
        with open(args.out, "w") as fh:
            json.dump(out, fh, indent=1)
            fh.write("\n")


if __name__ == "__main__":
    main()
