"""What predicted-input decoding costs, as one JSON line:

  bench      timesteps/s at the bench shape (bench.py WORKLOAD: 65 536 columns x 32 cells, 50 patterns x 20 noisy copies, SP and TM
             learning, learned by bench.py's untimed pre-training), 2 000-step calls in graph replay: undecoded, and with every
             step's votes (run(record=("predicted_input",)) / htm_set_run_predicted_input), alternated in one process (each
             call: prepare, sync, then run + sync, timed end to end)
  example    the same at the reference's example shape (example.py: 1 000 inputs -> 2 048 columns x 32 cells)
  host_fed   microseconds of one predicted_input() (one launch and a synchronising copy) after a process() at the bench shape

    python tools/predicted_input_rate.py [--reps 5] [--steps 2000] [--out FILE]
"""
import argparse
import json
import os
import statistics
import sys
import time

sys.path.insert(0, os.getcwd())
import numpy as np

import bench
import bithtm_amd as B


def rates(htm, noisy, steps, reps, pretrain):
    eng = htm.engine
    bank = eng.upload_bank(noisy)
    n_bank = noisy.shape[0]
    for _ in range(pretrain):                                  # (the learned state)
        eng.run(bank, n_bank, n_bank)
    eng.sync()
    votes = eng._record_buffer("predicted_input", steps * eng.input_dim)
    out = {"none": [], "predicted_input": []}
    for r in range(reps + 1):                                  # (round 0 warms every graph; not reported)
        for name in out:
            eng.set_run_predicted_input(votes if name == "predicted_input" else None)
            try:
                eng.prepare(bank, n_bank, steps)
                eng.sync()
                t0 = time.perf_counter()
                eng.run(bank, n_bank, steps)
                eng.sync()
                dt = time.perf_counter() - t0
            finally:
                eng.set_run_predicted_input(None)
            if r:
                out[name].append(steps / dt)
    med = {name: statistics.median(v) for name, v in out.items()}
    return dict(bank_rows=n_bank, steps_per_call=steps, reps=reps, hip_graph=True, segments=eng.info().segments,
                plan=eng.run_plan(steps), timesteps_per_s={k: round(v) for k, v in med.items()},
                all_reps={k: [round(x) for x in v] for k, v in out.items()},
                overhead_pct=round(100 * (1 - med["predicted_input"] / med["none"]), 2),
                overhead_us_per_step=round(1e6 / med["predicted_input"] - 1e6 / med["none"], 2),
                predicted_columns_last=int(htm.temporal_memory.last_state.cell_prediction.any(axis=1).sum()))


def bench_shape(steps, reps):
    w = bench.WORKLOAD
    noisy, perm = bench.make_inputs(w)
    htm = bench.build_htm(w, perm, 0)
    res = rates(htm, noisy, steps, reps, pretrain=10)
    res["shape"] = "65536 x 32, bench WORKLOAD, learned"
    return res, htm, noisy


def example_shape(steps, reps, seed=0):
    I, Cn, K, patterns = 1000, 2048, 32, 50
    rng = np.random.RandomState(seed)
    base = rng.rand(patterns, I) < 0.02
    noisy = np.concatenate([base ^ (rng.rand(patterns, I) < 0.005) for _ in range(4)])
    np.random.seed(seed)
    htm = B.HierarchicalTemporalMemory(I, Cn, K, seed=seed)
    res = rates(htm, noisy, steps, reps, pretrain=10)
    res["shape"] = "1000 -> 2048 x 32 (example.py), learned"
    return res


def host_fed(htm, noisy, steps=50):
    for t in range(5):
        htm.process(noisy[t])
        htm.predicted_input()
    times = []
    for t in range(steps):
        htm.process(noisy[t % len(noisy)])
        htm.engine.sync()
        t0 = time.perf_counter()
        htm.predicted_input()
        times.append(time.perf_counter() - t0)
    return dict(steps=steps, us_per_call_median=round(1e6 * statistics.median(times), 1))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=2000)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    res, htm, noisy = bench_shape(args.steps, args.reps)
    line = json.dumps(dict(tool="predicted_input_rate", bench=res, host_fed=host_fed(htm, noisy),
                           example=example_shape(args.steps, args.reps)))
    print(line)
    if args.out:
        with open(args.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
