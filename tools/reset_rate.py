"""What sequence resets cost, as one JSON line:

  run        timesteps/s at the bench shape (bench.py WORKLOAD: 65 536 columns x 32 cells, 50 patterns x 20 noisy copies, learned
             by bench.py's untimed pre-training), 2 000-step calls in graph replay: no reset bits, and resets before every 10th
             and every 100th bank row (run(resets=) / htm_set_run_resets), alternated in one process (each call: prepare, sync,
             then run + sync, timed end to end)
  host_fed   a stand-alone TemporalMemory of the same shape fed 1 311 random columns per step: process() alone, reset() +
             process() (htm_reset: one launch on the device), and process(prev_state=get_empty_state()) by the host import it
             replaces (htm_import_begin / htm_write / htm_import_commit of the empty state) -- microseconds per step

    python tools/reset_rate.py [--reps 5] [--steps 2000] [--host-steps 60]
"""
import argparse
import json
import os
import statistics
import sys
import time
from types import SimpleNamespace

sys.path.insert(0, os.getcwd())
import numpy as np

import bench
import bithtm_amd as B

EVERY = (("none", 0), ("every_100", 100), ("every_10", 10))


def run_rates(steps, reps):
    w = bench.WORKLOAD
    noisy, perm = bench.make_inputs(w)
    htm = bench.build_htm(w, perm, 0)
    eng = htm.engine
    bank = eng.upload_bank(noisy)
    n_bank = noisy.shape[0]
    for a in range(0, 10 * w["patterns"], w["patterns"]):       # bench.py's untimed pre-training: the learned state
        eng.run(bank, n_bank, w["patterns"])
    eng.sync()
    bits = {name: None if every == 0 else eng.upload_resets(np.arange(n_bank) % every == 0) for name, every in EVERY}
    rates = {name: [] for name, _ in EVERY}
    for r in range(reps + 1):                                  # (round 0 warms every graph; not reported)
        for name, _ in EVERY:
            eng.prepare(bank, n_bank, steps, resets=bits[name])
            eng.sync()
            t0 = time.perf_counter()
            eng.run(bank, n_bank, steps, resets=bits[name])
            eng.sync()
            dt = time.perf_counter() - t0
            if r:
                rates[name].append(steps / dt)
    med = {name: statistics.median(v) for name, v in rates.items()}
    out = dict(shape="65536 x 32, bench WORKLOAD, learned", bank_rows=n_bank, steps_per_call=steps, reps=reps, hip_graph=True,
               segments=eng.info().segments, timesteps_per_s={name: round(v) for name, v in med.items()},
               all_reps={name: [round(x) for x in v] for name, v in rates.items()})
    for name, _ in EVERY[1:]:
        out[f"overhead_{name}_pct"] = round(100 * (1 - med[name] / med["none"]), 2)
        out[f"overhead_{name}_us_per_step"] = round(1e6 / med[name] - 1e6 / med["none"], 2)
    return out


def host_fed(steps, C=65536, K=32, k=1311):
    rng = np.random.RandomState(0)
    seqs = [SimpleNamespace(active_column=np.sort(rng.choice(C, k, replace=False))) for _ in range(20)]
    out = {}
    for mode in ("process", "reset+process", "prev_state_import"):
        tm = B.TemporalMemory(C, K, seed=1)
        for t in range(40):                                    # (a learned state: predictions, matching segments)
            tm.process(seqs[t % 20])
        tm._engine.sync()
        t0 = time.perf_counter()
        for t in range(steps):
            sp = seqs[t % 20]
            if mode == "process":
                st = tm.process(sp)
            elif mode == "reset+process":
                tm.reset()
                st = tm.process(sp)
            else:
                st = tm.process(sp, prev_state=_empty_not_by_identity(tm))
        tm._engine.sync()
        del st
        out[mode] = round(1e6 * (time.perf_counter() - t0) / steps, 1)
    return dict(shape=f"{C} x {K}, {k} active columns, stand-alone TemporalMemory", steps=steps, us_per_step=out)


def _empty_not_by_identity(tm):
    """get_empty_state() in a form process() cannot recognise as empty (a predicted cell it never reads), so that it takes
    the host import -- what process(prev_state=get_empty_state()) cost before htm_reset."""
    st = tm.get_empty_state()
    pred = np.zeros((tm.column_dim, tm.cell_dim), bool)
    pred[0, 0] = True
    st._cache["cell_prediction"] = pred
    return st


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=2000)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--host-steps", type=int, default=60)
    args = ap.parse_args()
    res = dict(tool="reset_rate", run=run_rates(args.steps, args.reps), host_fed=host_fed(args.host_steps))
    print(json.dumps(res))


if __name__ == "__main__":
    main()
