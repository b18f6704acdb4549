#!/usr/bin/env python3
"""steps/s of htm.run at the bench shape over a bank of 50 % dense inputs: every byte of an input row is non-zero, so the
two-launch schedule's overlap reads every byte plane of the mask -- its worst case (profiles/r16_dense_inputs.txt).

    python tools/dense_rate.py          # run it in the tree to be measured (a parent checkout with its own build for the other figure)
"""
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import bench  # noqa: E402

w = dict(bench.WORKLOAD)
noisy, perm = bench.make_inputs(w)
dense = np.random.RandomState(5).rand(*noisy.shape) < 0.5
htm = bench.build_htm(w, perm, 0)
eng = htm.engine
bank = eng.upload_bank(dense)
eng.run(bank, dense.shape[0], 500, learning=True)
eng.sync()
rates = []
for rep in range(5):
    t0 = time.perf_counter()
    eng.run(bank, dense.shape[0], 2000, learning=True, use_graph=True)
    eng.sync()
    rates.append(2000 / (time.perf_counter() - t0))
print(f"dense 50 % inputs, I = {w['input_dim']}: htm.run median {np.median(rates):.0f} steps/s (min {min(rates):.0f}, max {max(rates):.0f}); segments {eng.info().segments}")
