"""What the anomaly likelihood costs on the device, at tools/tick_rate.py's shape (1 000 inputs -> 2 048
columns x 32 cells, two scalar fields, learned members), as one JSON line (and, with --out, a file:
profiles/r15_likelihood_rate.json).

  ticks    per group size B (default 1, 8, 64, 256), alternating in one process, --repeats rounds: host wall time per
           group.tick(values, encoder=enc) with and without likelihood= over --ticks ticks, the median of the rounds with the
           lowest and the highest (inside a round the two legs take turns every 20 ticks); and the tick's launch count with and without (htm_profile) -- expected: one launch more,
           whatever B is
  run      group.run(values, --steps steps, encoder=enc, likelihood=lk) against the same run with record=True followed by the
           NumPy definition (bithtm_amd/likelihood.py) looped over the read-back counters, per B, behind two untimed runs, the
           leg that comes first alternating
  update   AnomalyLikelihood.update_counts alone at (0, 1, 16384, 64, 1) -- an estimate at every step, the widest averaging
           window, the worst case -- and at NuPIC's defaults, --steps steps of B streams; the time includes the upload of the
           records and the read-back

    python tools/likelihood_rate.py [--sizes 1,8,64,256] [--ticks 200] [--steps 1000] [--repeats 3] [--out profiles/r15_likelihood_rate.json]
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
from bithtm_amd.likelihood import define  # noqa: E402
from tick_rate import SHAPE, encoder, log, spread, stream  # noqa: E402

SLICE = 20                                  # ticks a leg takes before the other leg's turn
P_EVERY = dict(learning_period=0, estimation_samples=1, history=16384, averaging_window=64, reestimation_period=1)


def median(times):
    ms = sorted(1e3 * t for t in times)
    return dict(ms=round(ms[len(ms) // 2], 3), lowest=round(ms[0], 3), highest=round(ms[-1], 3))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sizes", default="1,8,64,256")
    ap.add_argument("--ticks", type=int, default=200)
    ap.add_argument("--steps", type=int, default=1000)
    ap.add_argument("--train", type=int, default=200)
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--out")
    args = ap.parse_args()
    enc = encoder()
    out = dict(tool="likelihood_rate", shape="1000 inputs -> 2048 columns x 32 cells, 2 fields", ticks=args.ticks, steps=args.steps, sizes={})
    for n in [int(x) for x in args.sizes.split(",")]:
        group = B.ModelGroup.create(n, seeds=range(n), **SHAPE)
        values = stream(n, args.train + max(args.ticks, args.steps), 7 + n)
        banked = np.ascontiguousarray(values.transpose(1, 0, 2))
        group.run(banked[:, :args.train], args.train, encoder=enc)
        live = values[args.train:]
        sync = group.models[0].engine.sync
        lk = B.AnomalyLikelihood(n)
        legs = dict(tick=lambda v: group.tick(v, encoder=enc), tick_scored=lambda v: group.tick(v, encoder=enc, likelihood=lk))
        # (the members keep learning, so a tick costs a little more the later it comes: the two legs take turns every SLICE ticks
        # inside a round, and the turn that comes first alternates)
        times = {name: [] for name in legs}
        for fn in legs.values():
            fn(live[0])
        for _ in range(args.repeats):
            spent, at = {name: 0.0 for name in legs}, 0
            for piece in range(-(-args.ticks // SLICE)):
                count = min(SLICE, args.ticks - piece * SLICE)
                for name in (list(legs) if piece % 2 == 0 else list(legs)[::-1]):
                    sync()
                    t0 = time.perf_counter()
                    for t in range(at, at + count):
                        legs[name](live[t % len(live)])
                    sync()
                    spent[name] += time.perf_counter() - t0
                at += count
            for name in legs:
                times[name].append(spent[name])
        res = {name: spread(times[name], args.ticks) for name in legs}
        eng = group.models[0].engine
        for name, fn in legs.items():
            fn(live[0])
            eng.profile(True)
            for t in range(20):
                fn(live[t % len(live)])
            prof = eng.profile_read()
            eng.profile(False)
            res[name]["launches_per_tick"] = sum(c for _, c in prof.values()) / 20
            res[name]["device_us"] = round(1e3 * sum(ms for ms, _ in prof.values()) / 20, 1)
            if "live:likelihood" in prof:
                res[name]["likelihood_launch_us"] = round(1e3 * prof["live:likelihood"][0] / 20, 2)
        # the batched run: scored on the device against the definition looped on the host
        rows = banked[:, args.train:args.train + args.steps]
        scored, looped = [], []
        run_lk = B.AnomalyLikelihood(n)

        def run_scored():
            sync()
            t0 = time.perf_counter()
            group.run(rows, args.steps, encoder=enc, likelihood=run_lk)
            scored.append(time.perf_counter() - t0)

        def run_looped():
            sync()
            t0 = time.perf_counter()
            recs = group.run(rows, args.steps, encoder=enc, record=True)
            t1 = time.perf_counter()
            for r in recs:
                define(r.active_columns, r.bursting_columns)
            looped.append((time.perf_counter() - t0, time.perf_counter() - t1))
        for _ in range(2):                          # untimed: the bank's upload, the object's buffers, the pools' growth to this stream
            group.run(rows, args.steps, encoder=enc, likelihood=run_lk)
        for r in range(args.repeats):               # (the leg that comes first alternates)
            for leg in ((run_scored, run_looped) if r % 2 == 0 else (run_looped, run_scored)):
                leg()
        res["run_scored"] = median(scored)
        res["run_then_numpy"] = median([a for a, _ in looped])
        res["numpy_loop_alone"] = median([b for _, b in looped])
        # update_counts alone
        rng = np.random.RandomState(n)
        active = np.full((n, args.steps), 40, dtype=np.int64)
        bursting = rng.binomial(40, 0.1, (n, args.steps)).astype(np.int64)
        for label, params in (("update_every_step", P_EVERY), ("update_defaults", {})):
            alone = B.AnomalyLikelihood(n, **params).bind(group.models[0])
            alone.update_counts(active[:, :1], bursting[:, :1])
            ts = []
            for _ in range(args.repeats):
                alone.reset()
                sync()
                t0 = time.perf_counter()
                alone.update_counts(active, bursting)
                ts.append(time.perf_counter() - t0)
            res[label] = median(ts)
        out["sizes"][str(n)] = res
        log(n, res)
        del group
    print(json.dumps(out))
    if args.out:
        with open(args.out, "w") as fh:
            json.dump(out, fh, indent=1)


if __name__ == "__main__":
    main()
