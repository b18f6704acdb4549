"""What a per-step record costs (htm_run_recorded; HierarchicalTemporalMemory.run(record=...)), as one JSON line:

  run        timesteps/s at the bench shape (bench.py WORKLOAD: 65 536 columns x 32 cells, 50 patterns x 20 noisy copies, learned
             by bench.py's untimed pre-training), 2 000-step calls in graph replay, unrecorded / counters only / all three fields
             alternated in one process (each call: prepare, sync, then run + sync + the record's read-back, timed end to end)
  example    bithtm_amd/example.py at 2 048 and 65 536 columns: --batched_report (one recorded run() per epoch, the per-step
             lines printed from the record) next to the default stepwise loop (process() and two States read per step)

    python tools/record_overhead.py [--reps 5] [--steps 2000] [--variants unrecorded,counters] [--no-example]

Under rocprofv3 (which crashes inside hipGraph replay here, as bench.py notes) the calls launch eagerly: the kernel
trace of such a run gives each launch's duration and the gaps between them, the rate JSON of a run without the profiler
gives the rates.
"""
import argparse
import io
import json
import os
import statistics
import sys
import time

sys.path.insert(0, os.getcwd())
import numpy as np

import bench
from bithtm_amd import example as E
from bithtm_amd import HierarchicalTemporalMemory

VARIANTS = (("unrecorded", None), ("counters", ("counters",)), ("all", ("counters", "active_column", "column_prediction")))


def run_rates(steps, reps, variants, use_graph):
    w = bench.WORKLOAD
    noisy, perm = bench.make_inputs(w)
    htm = bench.build_htm(w, perm, 0)
    eng = htm.engine
    bank = eng.upload_bank(noisy)
    n_bank = noisy.shape[0]
    for a in range(0, 10 * w["patterns"], w["patterns"]):       # bench.py's untimed pre-training: the learned state
        eng.run(bank, n_bank, w["patterns"], use_graph=use_graph)
    eng.sync()
    chosen = [(name, fields) for name, fields in VARIANTS if name in variants]
    rates = {name: [] for name, _ in chosen}
    for r in range(reps + 1):                                  # (round 0 warms every graph and buffer; not reported)
        for name, fields in chosen:
            eng.prepare(bank, n_bank, steps, use_graph=use_graph, record=fields is not None)
            eng.sync()
            t0 = time.perf_counter()
            eng.run(bank, n_bank, steps, use_graph=use_graph, record=fields)
            eng.sync()
            dt = time.perf_counter() - t0
            if r:
                rates[name].append(steps / dt)
    med = {name: statistics.median(v) for name, v in rates.items()}
    out = dict(shape="65536 x 32, bench WORKLOAD, learned", steps_per_call=steps, reps=reps, hip_graph=use_graph,
               segments=eng.info().segments, timesteps_per_s={name: round(v) for name, v in med.items()},
               all_reps={name: [round(x) for x in v] for name, v in rates.items()})
    for name in ("counters", "all"):
        if name in med and "unrecorded" in med:
            out[f"overhead_{name}_pct"] = round(100 * (1 - med[name] / med["unrecorded"]), 2)
            out[f"overhead_{name}_us_per_step"] = round(1e6 / med[name] - 1e6 / med["unrecorded"], 2)
    return out


def example_rates(cols, epochs_batched=6, epochs_stepwise=1):
    out = {}
    for mode in ("batched_report", "stepwise"):
        epochs = epochs_batched if mode == "batched_report" else epochs_stepwise
        argv = ["--epochs", str(epochs), "--column_dim", str(cols)]
        opts = E.parse(argv)
        np.random.seed(0)
        bank = np.random.rand(opts.input_patterns, opts.input_dim) < opts.input_density
        htm = HierarchicalTemporalMemory(opts.input_dim, opts.column_dim, opts.cell_dim)
        fn = E.run_batched_report if mode == "batched_report" else E.run_stepwise
        fn(htm, bank, E.parse(["--epochs", "1", "--column_dim", str(cols)]), io.StringIO())    # warm (graphs, buffers)
        t0 = time.perf_counter()
        fn(htm, bank, opts, io.StringIO())
        dt = time.perf_counter() - t0
        out[mode] = round(epochs * opts.input_patterns / dt)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=2000)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--variants", default=",".join(name for name, _ in VARIANTS))
    ap.add_argument("--no-example", action="store_true")
    args = ap.parse_args()
    use_graph = "ROCP_TOOL_LIBRARIES" not in os.environ
    res = dict(tool="record_overhead", run=run_rates(args.steps, args.reps, args.variants.split(","), use_graph))
    if not args.no_example:
        res["example"] = {str(c): example_rates(c) for c in (2048, 65536)}
    print(json.dumps(res))


if __name__ == "__main__":
    main()
