#!/usr/bin/env python3
"""Records tests/golden/predicted_input.npz from the UNMODIFIED reference, for tests/test_predicted_input_cpu.py and
tests/test_hip_predicted_input.py.

Needs a checkout of the reference (cokwa/bitHTM):   BITHTM_REFERENCE=<checkout> python tests/golden/generate_predicted_input.py

A lock-step run as generate_lockstep_reset.py records it (tests/refdiff.py, the reference under keyed_rand), with learning off on
some steps and a few sequence resets in the reference's own idiom (`tm.last_state = tm.get_empty_state()`).  After every step
the reference's predicted-input votes are taken from its own objects:

    pp = htm.spatial_pooler.proximal_projection
    votes_t = (pp.permanence[tm_state.cell_prediction.any(axis=1)] >= pp.permanence_threshold).sum(axis=0)

The oracle runs beside it and is checked field by field every step, and the identity votes_t . x_{t+1} = sum of step t+1's
overlaps over the columns step t predicts is checked where step t+1 follows without a reset.  What is kept: a digest of every
step's votes and their sum, the reset steps, the learning flags and the initial permanences' digest.
"""

import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

import refdiff  # noqa: E402
from oracle.ref_hooks import import_reference  # noqa: E402

RUN = dict(seed=41, input_dim=300, column_dim=1024, cell_dim=8, active_columns=64, patterns=8, density=0.06, noise=0.0, steps=150)
RESETS = [1, 37, 60, 61, 96, 120]
LEARNING_OFF = sorted(set(range(70, 90)) | {120, 121})


def votes_of(permanence, threshold, cell_prediction):
    return (permanence[np.asarray(cell_prediction).any(axis=1)] >= threshold).sum(axis=0).astype(np.int32)


def main():
    ref = import_reference()
    cfg = RUN
    seed, I, C, K, k, steps = (cfg[f] for f in ("seed", "input_dim", "column_dim", "cell_dim", "active_columns", "steps"))
    np.random.seed(seed)
    perm0 = ref.projections.DenseProjection(I, C).permanence          # what build_pair's reference will draw
    ref_htm, ora = refdiff.build_pair(ref, seed, I, C, K, active_columns=k)
    bank, rng = refdiff.make_inputs(seed + 1, cfg["patterns"], I, cfg["density"])
    tm = ref_htm.temporal_memory
    pp = ref_htm.spatial_pooler.proximal_projection
    digests, totals, learning = [], [], []
    prev_votes = None
    with refdiff.keyed_rand(seed, K) as patch:
        for t in range(steps):
            x = bank[refdiff.pattern_index(t, cfg["patterns"], 0.0, rng)] ^ (rng.rand(I) < cfg["noise"])
            learn = t not in LEARNING_OFF
            patch.step = t
            if t in RESETS:
                tm.last_state = tm.get_empty_state()
                empty = tm.get_empty_state()
                ora_sp = ora.spatial_pooler.step(x, learning=learn)
                ora_tm = ora.temporal_memory.step(ora_sp.active_column, learning=learn, prev_state=empty)
            else:
                ora_sp, ora_tm = ora.step(x, learning=learn)
            prev_pred = ref_htm.temporal_memory.last_state.cell_prediction.any(axis=1) if t else np.zeros(C, bool)
            ref_sp, ref_tm = ref_htm.process(x, learning=learn)
            refdiff.compare_step(t, ref_sp, ref_tm, ora_sp, ora_tm, K)
            if prev_votes is not None and t not in RESETS:
                assert int(prev_votes @ x.astype(np.int64)) == int(ref_sp.overlaps[prev_pred].sum()), t
            votes = votes_of(pp.permanence, pp.permanence_threshold, ref_tm.cell_prediction)
            assert np.array_equal(votes, votes_of(ora.spatial_pooler.permanence, ora.spatial_pooler.params.permanence_threshold,
                                                  ora_tm.cell_prediction)), t
            digests.append(refdiff.digest(votes))
            totals.append(int(votes.sum()))
            learning.append(learn)
            prev_votes = votes.astype(np.int64)
    assert sum(1 for v in totals if v) > steps // 2, "too few steps with predictions to pin anything"
    path = os.path.join(HERE, "predicted_input.npz")
    np.savez_compressed(
        path, **{k: np.asarray(v) for k, v in cfg.items()}, resets=np.array(RESETS, dtype=np.int32),
        learning=np.array(learning, dtype=np.bool_), votes_digest=np.array(digests, dtype=np.uint64),
        votes_total=np.array(totals, dtype=np.int64), permanence_digest=np.uint64(refdiff.digest(perm0)))
    print(f"wrote {path}: {steps} steps, {sum(1 for v in totals if v)} with predictions, {os.path.getsize(path)} bytes")


if __name__ == "__main__":
    main()
