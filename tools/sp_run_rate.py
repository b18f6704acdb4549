"""What a batched stand-alone Spatial Pooler run buys, as one JSON line: a SpatialPooler of input_dim 1 000, 65 536 columns and
1 311 active columns fed 50 rows at density 0.1, stepped -- one object, one process --

  stepwise           by the loop `for x in inputs: sp.process(x)` (htm_sp_step: a host-to-device copy of the input and the
                     step's launches in every call), --host-steps steps per repetition; learning and frozen, and ("observed")
                     reading every step's State -- the only way that loop has to see a winner list: three read-backs a step,
                     two of them column_dim long --, --observed-steps steps per repetition
  run                by sp.run(inputs, --run-steps) (htm_sp_run: graph replay, the bank resident in device memory), learning and
                     frozen (learning=False), unrecorded and with all three record fields (read back once per call, inside the
                     timed window)

The legs take turns inside every repetition (the same code, the same device state, the same neighbours on the machine), each
repetition after an untimed round of all legs (graphs captured, buffers allocated); a leg's window ends in a synchronisation.
Reported per leg: the median rate in timesteps/s over the repetitions with the lowest and the highest, and the kernel launches
per step (htm_profile of a short eager stretch).

    python tools/sp_run_rate.py [--reps 5] [--run-steps 8000] [--host-steps 1000] [--observed-steps 200] [--out profiles/r11_sp_run_rate.json]
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

I, C, K_ACTIVE, ROWS, DENSITY = 1000, 65536, 1311, 50, 0.1
ALL = ("active_column", "active_overlap", "active_boosted")


def log(*a):
    print(*a, file=sys.stderr, flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--run-steps", type=int, default=8000)
    ap.add_argument("--host-steps", type=int, default=1000)
    ap.add_argument("--observed-steps", type=int, default=200)
    ap.add_argument("--out")
    args = ap.parse_args()
    np.random.seed(0)
    sp = B.SpatialPooler(I, C, K_ACTIVE)
    inputs = np.random.RandomState(1).rand(ROWS, I) < DENSITY

    def stepwise(n, learning=True):
        for _ in range(n):
            sp.process(inputs[sp._engine.steps % ROWS], learning=learning)

    def observed(n):
        for _ in range(n):
            st = sp.process(inputs[sp._engine.steps % ROWS])
            st.active_column, st.overlaps, st.boosted_overlaps

    sp.process(inputs[0])                           # (creates the engine)
    legs = {
        "stepwise_observed": (observed, args.observed_steps),
        "stepwise": (lambda n: stepwise(n), args.host_steps),
        "stepwise_frozen": (lambda n: stepwise(n, learning=False), args.host_steps),
        "run": (lambda n: sp.run(inputs, n), args.run_steps),
        "run_recorded": (lambda n: sp.run(inputs, n, record=ALL), args.run_steps),
        "run_frozen": (lambda n: sp.run(inputs, n, learning=False), args.run_steps),
        "run_frozen_recorded": (lambda n: sp.run(inputs, n, learning=False, record=ALL), args.run_steps),
    }
    eng = sp._engine
    rates = {name: [] for name in legs}
    for rep in range(-1, args.reps):                # (repetition -1: the untimed round)
        for name, (step, steps) in legs.items():
            eng.sync()
            t0 = time.perf_counter()
            step(steps)
            eng.sync()
            dt = time.perf_counter() - t0
            if rep >= 0:
                rates[name].append(steps / dt)
        log("repetition", rep, {name: round(r[-1], 1) for name, r in rates.items() if r})
    out = dict(tool="sp_run_rate", shape=f"input_dim {I}, {C} columns, {K_ACTIVE} active columns, {ROWS} rows at density {DENSITY}",
               repetitions=args.reps, legs={})
    for name, (step, steps) in legs.items():
        r = sorted(rates[name])
        eng.profile(True)
        (step if name.startswith("stepwise") else
         (lambda n, name=name: sp.run(inputs, n, learning="frozen" not in name, use_graph=False, record=ALL if "recorded" in name else None)))(20)
        prof = eng.profile_read()
        eng.profile(False)
        out["legs"][name] = dict(steps_per_repetition=steps,
                                 timesteps_per_s=dict(median=round(r[len(r) // 2], 1), lowest=round(r[0], 1), highest=round(r[-1], 1)),
                                 us_per_step=round(1e6 / r[len(r) // 2], 2),
                                 launches_per_step=round(sum(cnt for _, cnt in prof.values()) / 20, 2),
                                 launches=sorted(n for n, (_, cnt) in prof.items() if cnt))
    for run, base in (("run", "stepwise"), ("run_recorded", "stepwise"), ("run_recorded", "stepwise_observed"), ("run_frozen", "stepwise_frozen"), ("run_frozen_recorded", "stepwise_frozen")):
        a, b = out["legs"][run]["timesteps_per_s"], out["legs"][base]["timesteps_per_s"]
        out.setdefault("speedup_over_stepwise", {})[run if base != "stepwise_observed" else run + "_over_observed"] = dict(median=round(a["median"] / b["median"], 2), least=round(a["lowest"] / b["highest"], 2))
    print(json.dumps(out))
    if args.out:
        with open(args.out, "w") as f:
            json.dump(out, f, indent=1)


if __name__ == "__main__":
    main()
