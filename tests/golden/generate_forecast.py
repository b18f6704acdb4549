#!/usr/bin/env python3
"""Records tests/golden/forecast.npz from the UNMODIFIED reference, for tests/test_forecast_cpu.py and tests/test_hip_forecast.py.

Needs a checkout of the reference (cokwa/bitHTM):   BITHTM_REFERENCE=<checkout> python tests/golden/generate_forecast.py

The reference under keyed_rand (tests/refdiff.py), as generate_predicted_input.py runs it: 8 patterns trained for 40 epochs, two
context steps with learning off, then for each (min_votes, max_bits) of forecast_fixture.CASES, from a copy of that state, 20
closed-loop steps in the reference's own terms:

    pp = htm.spatial_pooler.proximal_projection
    votes = (pp.permanence[tm_state.cell_prediction.any(axis=1)] >= pp.permanence_threshold).sum(axis=0)
    x = encode(votes, min_votes, max_bits);  htm.process(x, learning=False)

The oracle runs beside it and is checked field by field every step.  Kept per case: the packed x of every step, a digest of the
votes of the state every step leaves, and every step's active columns.
"""

import copy
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

import refdiff  # noqa: E402
from forecast_fixture import CASES, RUN, encode, pack_rows, training_inputs, votes_of  # noqa: E402
from oracle.ref_hooks import import_reference  # noqa: E402


def main():
    ref = import_reference()
    cfg = RUN
    seed, I, C, K, k, steps = (cfg[f] for f in ("seed", "input_dim", "column_dim", "cell_dim", "active_columns", "steps"))
    np.random.seed(seed)
    perm0 = ref.projections.DenseProjection(I, C).permanence          # what build_pair's reference will draw
    ref_htm, ora = refdiff.build_pair(ref, seed, I, C, K, active_columns=k)
    bank, n_train, n_all = training_inputs(cfg)
    rows, digests, cols, seed_digests = [], [], [], []
    with refdiff.keyed_rand(seed, K) as patch:
        for t in range(n_all):
            patch.step = t
            ora_sp, ora_tm = ora.step(bank[t % len(bank)], learning=t < n_train)
            ref_sp, ref_tm = ref_htm.process(bank[t % len(bank)], learning=t < n_train)
            refdiff.compare_step(t, ref_sp, ref_tm, ora_sp, ora_tm, K)
        for min_votes, max_bits in CASES:
            r_htm, o, r_tm = copy.deepcopy(ref_htm), copy.deepcopy(ora), ref_tm
            pp = r_htm.spatial_pooler.proximal_projection
            votes = votes_of(pp.permanence, pp.permanence_threshold, r_tm.cell_prediction)
            seed_digests.append(refdiff.digest(votes))
            xs, ds, cs = [], [], []
            for t in range(n_all, n_all + steps):
                patch.step = t
                x = encode(votes, min_votes, max_bits)
                o_sp, o_tm = o.step(x, learning=False)
                r_sp, r_tm = r_htm.process(x, learning=False)
                refdiff.compare_step(t, r_sp, r_tm, o_sp, o_tm, K)
                votes = votes_of(pp.permanence, pp.permanence_threshold, r_tm.cell_prediction)
                xs.append(x)
                ds.append(refdiff.digest(votes))
                cs.append(np.sort(r_sp.active_column))
            xs = np.asarray(xs, bool)
            print(f"(min_votes, max_bits) = ({min_votes}, {max_bits}): bits per row {xs.sum(axis=1).tolist()}")
            for p in range(steps):                  # how far each row is from the learned sequence
                want = bank[(n_all + p) % len(bank)]
                if not np.array_equal(xs[p] & want, xs[p]) or (max_bits == 0 and not np.array_equal(xs[p], want)):
                    print(f"  step {p}: {int((xs[p] & ~want).sum())} stray bits, {int((want & ~xs[p]).sum())} missing")
            rows.append(pack_rows(xs))
            digests.append(ds)
            cols.append(cs)
    bits = [forecast.sum(axis=1) for forecast in (np.unpackbits(r, axis=1) for r in rows)]
    assert bits[0].min() > 0 and bits[1].min() > 0, "the sustained cases must keep non-empty rows"
    assert bits[2].min() == 0, "the third case must reach an all-zero row"
    path = os.path.join(HERE, "forecast.npz")
    np.savez_compressed(
        path, **{f: np.asarray(v) for f, v in cfg.items()}, cases=np.asarray(CASES, dtype=np.int32), rows=np.asarray(rows, dtype=np.uint8),
        votes_digest=np.asarray(digests, dtype=np.uint64), seed_votes_digest=np.asarray(seed_digests, dtype=np.uint64),
        active_column=np.asarray(cols, dtype=np.int32), permanence_digest=np.uint64(refdiff.digest(perm0)))
    print(f"wrote {path}: {os.path.getsize(path)} bytes")


if __name__ == "__main__":
    main()
