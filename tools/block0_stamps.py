#!/usr/bin/env python3
"""Where block 0 of the batched run's first launch (k_first_handover, csrc/htm_handover.h) spends its time, at the bench workload.

Needs a diagnostic build of the library, given by BITHTM_LIBRARY (the product library has no stamps):

    BITHTM_EXTRA_FLAGS=-DBITHTM_HANDOVER_STAMPS python -m bithtm_amd.build --force     # or hipcc ... -o another.so
    BITHTM_LIBRARY=$PWD/bithtm_amd/another.so python tools/block0_stamps.py [pairs]

Per traced steady-state step (two per pair, as tools/step_spans.py), in us from the launch's first block: block 0 before its wait
for the activation, after it, with the column lists in and the list of winners without a segment built, (only where winners ask
for a segment: the needed 1 024-blocks picked, their rows ranked, the end); how many winners asked and how many 1 024-blocks
were needed; when the last activation block ended, when block 0 ended, when its lists were stored.  Columns of a path the step
did not take hold an earlier step's stamps (large negative numbers).  profiles/r22_block0_stamps.txt."""
import os
import sys

import numpy as np

os.environ["BITHTM_TRACE"] = "1"
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import bench  # noqa: E402

WARMUP = 1500
w = dict(bench.WORKLOAD)
noisy, perm = bench.make_inputs(w)
k = round(w["column_dim"] * 0.02)
n_act = (k * 32 + 255) // 256
print("us from launch start: before wait | after wait | lists in | picked | seg loads in (ranked) | end ; n_un n_need ; last act block end")
for u in range(int(sys.argv[1]) if len(sys.argv) > 1 else 12):
    steps = 35 + 2 * u
    os.environ["BITHTM_TRACE_UNTIL"] = str(WARMUP + steps - 2)
    htm = bench.build_htm(w, perm, 0)
    eng = htm.engine
    bank = eng.upload_bank(noisy)
    eng.run(bank, noisy.shape[0], WARMUP, learning=True)
    eng.run(bank, noisy.shape[0], steps, learning=True, use_graph=True, pipeline=True)
    eng.sync()
    t = eng.trace_read()
    for parity in (0, 1):
        tt = t[parity * 4]
        blocks = np.nonzero(tt[:, 0] > 0)[0]
        if not len(blocks):
            continue
        first = tt[blocks, 0].min()
        act_end = (tt[:n_act, 1].max() - first) / 100
        s = t[parity * 4 + 3].reshape(-1)[:9]
        st = [(int(x) - first) / 100 if x else float("nan") for x in s[:6]]
        print("  " + " ".join(f"{x:6.2f}" for x in st) + f" ; {int(s[6]):4d} {int(s[7]):3d} ; {act_end:5.2f}  block0 end {(tt[n_act + 256, 1] - first) / 100:5.2f}  lists stored {(int(s[8]) - first) / 100:6.2f}")
    del htm, eng
