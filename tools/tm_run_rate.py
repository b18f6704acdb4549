"""What a batched stand-alone Temporal Memory run buys, as one JSON line: a TemporalMemory of 65 536 columns x 32 cells fed 50
rows of 1 311 random distinct columns, from a learned state (--learn steps of the sequence first), stepped

  host     by the stepwise loop, process(SimpleNamespace(active_column=row)) once per step (htm_tm_step: a host sort, a copy
           and a stream synchronisation in every call), --host-steps steps per repetition
  device   by run(lists, 2000) (htm_tm_run: graph replay, the lists resident in device memory), 2 000 steps per repetition

each leg five repetitions after an untimed call; reported per leg: the median rate in timesteps/s with the lowest and the
highest, and the kernel launches per step (htm_profile of a short eager stretch, under which the learning role and the scan
are two launches; unprofiled calls fuse them into one).  Both legs start from the same learned state
(learned with the stepwise loop, which every version of the library has) and keep learning while they are timed.

    python tools/tm_run_rate.py [--legs host,device] [--learn 500] [--host-steps 200] [--out profiles/r10_tm_run_rate.json]
--legs host runs on a library without TemporalMemory.run too.
"""
import argparse
import json
import os
import sys
import time
from types import SimpleNamespace

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np  # noqa: E402

import bithtm_amd as B  # noqa: E402

C, K, N, ROWS, REPS, RUN_STEPS = 65536, 32, 1311, 50, 5, 2000


def log(*a):
    print(*a, file=sys.stderr, flush=True)


def stepwise(tm, lists, steps):
    for _ in range(steps):
        tm.process(SimpleNamespace(active_column=lists[tm._engine.steps % ROWS]))


def learned(lists, steps):
    tm = B.TemporalMemory(C, K, seed=0)
    tm.process(SimpleNamespace(active_column=lists[0]))
    stepwise(tm, lists, steps - 1)
    return tm


def launches_per_step(tm, step, steps=20):
    eng = tm._engine
    eng.profile(True)
    step(steps)
    prof = eng.profile_read()
    eng.profile(False)
    return round(sum(cnt for _, cnt in prof.values()) / steps, 2), sorted(prof)


def leg(tm, step, steps):
    step(steps)                                     # untimed: graphs captured, buffers allocated
    rates = []
    for _ in range(REPS):
        tm._engine.sync()
        t0 = time.perf_counter()
        step(steps)
        tm._engine.sync()
        rates.append(steps / (time.perf_counter() - t0))
    rates.sort()
    return dict(steps_per_repetition=steps, repetitions=REPS, timesteps_per_s=dict(median=round(rates[REPS // 2], 1), lowest=round(rates[0], 1),
                                                                                    highest=round(rates[-1], 1)),
                us_per_step=round(1e6 / rates[REPS // 2], 2))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--legs", default="host,device")
    ap.add_argument("--learn", type=int, default=500)
    ap.add_argument("--host-steps", type=int, default=200)
    ap.add_argument("--out")
    args = ap.parse_args()
    legs = args.legs.split(",")
    rng = np.random.RandomState(0)
    lists = np.stack([rng.choice(C, N, replace=False) for _ in range(ROWS)]).astype(np.int32)
    out = dict(tool="tm_run_rate", shape=f"{C} columns x {K} cells, {N} columns per row, {ROWS} rows", learn_steps=args.learn, legs={})
    for name in legs:
        tm = learned(lists, args.learn)
        if name == "host":
            step, steps = (lambda n: stepwise(tm, lists, n)), args.host_steps
        elif name == "device":
            step, steps = (lambda n: tm.run(lists, n)), RUN_STEPS
        else:
            raise SystemExit(f"--legs: host and / or device, got {name!r}")
        row = leg(tm, step, steps)
        row["launches_per_step"], row["launches"] = launches_per_step(tm, (lambda n: tm.run(lists, n, use_graph=False)) if name == "device" else step)
        row["segments"] = int(tm._engine.check_capacity().segments)
        log(name, row)
        out["legs"][name] = row
        del tm
    if "host" in out["legs"] and "device" in out["legs"]:
        h, d = out["legs"]["host"]["timesteps_per_s"], out["legs"]["device"]["timesteps_per_s"]
        out["speedup"] = dict(median=round(d["median"] / h["median"], 1), least=round(d["lowest"] / h["highest"], 1))
    print(json.dumps(out))
    if args.out:
        with open(args.out, "w") as f:
            json.dump(out, f, indent=1)


if __name__ == "__main__":
    main()
