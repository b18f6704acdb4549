"""What a coordinate field costs on the device, as one JSON line (and, with --out, a file:
profiles/r22_coordinate_rate.json).

  One row of 1 000 inputs holds one field of 1 000 bits and width 21: "coordinate" is a CoordinateField of max_radius 127
  (kcoord_bank), "hashed" a hashed field of 1 000 buckets over the same bits and width (kenc_bank: the cost floor -- the same
  21 hashed positions ORed into the row, without a select).

  bank   at the bench shape (65 536 columns x 32 cells, input_dim 1 000): a --rows-row bank from values at each radius of
         --radii.  Device time per launch from the engine's profile events (htm_profile), --launches launches a round, --repeats
         rounds, the legs alternating; the host wall time of the same launches between two synchronisations; and the yardstick --
         encoder.encode in NumPy plus Engine.upload_bank, the only way to such a bank without the device encode -- once per
         radius (where a bank has more than 5 million candidates, --host-rows rows of it, scaled to --rows)
  tick   a group of --members members at tools/tick_rate.py's shape (1 000 inputs -> 2 048 columns x 32 cells), trained over
         --train rows: launches per tick and the device time of the encode and finish launches of a tick with either table
         (the coordinate table at radius --tick-radius), and the host wall time per tick, the legs taking turns every 20 ticks

Every figure is the median of the rounds with the lowest and the highest.

    python tools/coordinate_rate.py [--rows 1000] [--radii 2 8 32 127] [--launches 20] [--members 64] [--ticks 200] [--train 200]
                                    [--repeats 5] [--out profiles/r22_coordinate_rate.json]
"""
import argparse
import ctypes as C
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
from field_kinds_rate import SLICE, median  # noqa: E402
from tick_rate import SHAPE, log  # noqa: E402


def tables():
    return {"coordinate": B.ScalarEncoder([B.CoordinateField(1000, 21, 127, seed=1)], input_dim=1000),
            "hashed": B.ScalarEncoder([B.HashedField(0.0, 100.0, 1000, 21, buckets=1000, seed=1)], input_dim=1000)}


def positions(rows, radius, seed):
    """float64 [rows, 3]: random centres within +-10 000 cells and the radius."""
    rng = np.random.RandomState(seed)
    return np.concatenate([rng.uniform(-1e4, 1e4, (rows, 2)), np.full((rows, 1), float(radius))], axis=1)


def bank(args, out):
    w = dict(WORKLOAD, input_dim=1000)
    _, perm = make_inputs(w)
    eng = build_htm(w, perm, 0).engine
    encs = tables()
    d_bank = eng.zero_bank(args.rows)
    scalar = np.random.RandomState(1).uniform(-5.0, 105.0, (args.rows, 1))
    legs = {f"coordinate r={r}": (encs["coordinate"], positions(args.rows, r, r)) for r in args.radii}
    legs["hashed"] = (encs["hashed"], scalar)
    device_values = {name: eng.upload_values(v) for name, (_, v) in legs.items()}
    call = lambda name: eng.bank_encode(legs[name][0], device_values[name], args.rows, d_bank, args.rows)
    host = {}
    for name, (enc, v) in legs.items():             # (every leg computes its definition here, before anything is timed; the yardstick)
        candidates = 1 if name == "hashed" else (2 * int(name.split("=")[1]) + 1) ** 2
        n = args.rows if candidates * args.rows <= 5000000 else min(args.rows, args.host_rows)
        t0 = time.perf_counter()
        rows = enc.encode(v[:n])
        t1 = time.perf_counter()
        ptr = eng.upload_bank(rows)
        eng.sync()
        t2 = time.perf_counter()
        call(name)
        assert np.array_equal(eng.read_bank(d_bank, args.rows)[:n], rows), name
        scale = args.rows / n
        host[name] = dict(rows_timed=n, encode_ms=round(1e3 * (t1 - t0) * scale, 2), upload_ms=round(1e3 * (t2 - t1) * scale, 3),
                          total_ms=round(1e3 * (t2 - t0) * scale, 2))
        del ptr
    device, wall = {name: [] for name in legs}, {name: [] for name in legs}
    for r in range(args.repeats + 1):               # (round 0 is the warm-up)
        for name in (list(legs) if r % 2 == 0 else list(legs)[::-1]):
            eng.sync()
            t0 = time.perf_counter()
            for _ in range(args.launches):
                call(name)
            eng.sync()
            t1 = time.perf_counter()
            eng.profile(True)
            for _ in range(args.launches):
                call(name)
            prof = eng.profile_read()
            eng.profile(False)
            if r:
                wall[name].append(1e6 * (t1 - t0) / args.launches)
                device[name].append(1e3 * prof["bank_encode"][0] / prof["bank_encode"][1])
    res = {name: dict(device_us_per_launch=median(device[name]), wall_us_per_launch=median(wall[name]), numpy_encode_and_upload=host[name]) for name in legs}
    for name in res:
        log("bank", name, res[name])
    out["bank"] = dict(shape="65536 columns x 32 cells, 1000 inputs", rows=args.rows, launches_per_round=args.launches, **res)
    for ptr in device_values.values():
        eng.lib.hipFree(C.c_void_p(ptr))


def stream(enc, n, rows, seed, radius, period=10):
    """float64 [rows, n, columns]: per member a loop of `period` rows, repeated."""
    rng = np.random.RandomState(seed)
    if len(enc) == 3:
        base = np.concatenate([rng.uniform(-500, 500, (n, period, 2)), np.full((n, period, 1), float(radius))], axis=2)
    else:
        base = 100.0 * rng.rand(n, period, 1)
    return np.ascontiguousarray(base[:, np.arange(rows) % period].transpose(1, 0, 2))


def ticks(args, out):
    n = args.members
    encs = tables()
    group = B.ModelGroup.create(n, seeds=range(n), **SHAPE)
    values = {name: stream(enc, n, args.train + args.ticks, 7 + n, args.tick_radius) for name, enc in encs.items()}
    group.run(np.ascontiguousarray(values["coordinate"][:args.train].transpose(1, 0, 2)), args.train, encoder=encs["coordinate"])
    live = {name: v[args.train:] for name, v in values.items()}
    sync = group.models[0].engine.sync
    times = {name: [] for name in encs}
    for name, enc in encs.items():
        group.tick(live[name][0], encoder=enc)
        group.tick(live[name][1], encoder=enc)
    for r in range(args.repeats):
        spent, at = {name: 0.0 for name in encs}, 0
        for piece in range(-(-args.ticks // SLICE)):
            count = min(SLICE, args.ticks - piece * SLICE)
            for name in (list(encs) if (piece + r) % 2 == 0 else list(encs)[::-1]):
                sync()
                t0 = time.perf_counter()
                for t in range(at, at + count):
                    group.tick(live[name][t % args.ticks], encoder=encs[name])
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
            group.tick(live[name][t % args.ticks], encoder=enc)
        prof = eng.profile_read()
        eng.profile(False)
        res[name]["launches_per_tick"] = sum(c for _, c in prof.values()) / 40
        res[name]["encode_launch_us"] = round(1e3 * prof["live:encode"][0] / prof["live:encode"][1], 2)
        res[name]["finish_launch_us"] = round(1e3 * prof["live:finish"][0] / prof["live:finish"][1], 2)
    out["tick"] = dict(shape="1000 inputs -> 2048 columns x 32 cells", members=n, ticks=args.ticks, radius=args.tick_radius, **res)
    log("tick", out["tick"])


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", type=int, default=1000)
    ap.add_argument("--radii", type=int, nargs="+", default=[2, 8, 32, 127])
    ap.add_argument("--host-rows", type=int, default=50)
    ap.add_argument("--launches", type=int, default=20)
    ap.add_argument("--members", type=int, default=64)
    ap.add_argument("--ticks", type=int, default=200)
    ap.add_argument("--train", type=int, default=200)
    ap.add_argument("--tick-radius", type=int, default=8)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--out")
    args = ap.parse_args()
    out = dict(tool="coordinate_rate", table="one field of 1000 bits, width 21: a coordinate field (max_radius 127) against a hashed field (1000 buckets)")
    bank(args, out)
    ticks(args, out)
    print(json.dumps(out))
    if args.out:
        with open(args.out, "w") as fh:
            json.dump(out, fh, indent=1)
            fh.write("\n")


if __name__ == "__main__":
    main()
