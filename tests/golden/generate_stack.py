#!/usr/bin/env python3
"""Records tests/golden/stack_two_level.npz from the UNMODIFIED reference, for tests/test_region_stack_cpu.py and
tests/test_hip_region_stack.py.

Needs a checkout of the reference (cokwa/bitHTM):   BITHTM_REFERENCE=<checkout> python tests/golden/generate_stack.py

A region stack in reference terms: two reference HierarchicalTemporalMemory objects, the upper one's
input_dim the lower one's column_dim.  The lower one steps on every input; after every `stride` of its steps the upper one
steps on the bool vector with a bit for every column in sp_state.active_column of any step of that window.  Level l draws with
seed + l: np.random.rand is replaced by the keyed generator (oracle.ref_hooks.keyed_rand), whose seed, cell_dim and step are
switched to the level's before each level's process().  Sequence resets, in the reference's idiom
`tm.last_state = tm.get_empty_state()`, hit BOTH levels before the step they precede and stand on window boundaries; a stretch
of steps runs with learning off.  Two oracle models run beside the two reference models and are compared field by field every
step (tests/refdiff.py: compare_step).  One file holds two runs, stride 1 (prefix s1_) and stride 3 (s3_).

What is kept is the reference's side, per level and step: digests of active_column, cell_prediction and the flat winner cells,
the segment count, the digest of the upper level's input row; and level 0's active-column lists themselves (the input of
htm_pack_columns' NumPy statement).
"""

import os
import sys
from types import SimpleNamespace

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

import refdiff  # noqa: E402
from oracle.ref_hooks import import_reference  # noqa: E402

CFG = dict(seed=41, input_dim=300, patterns=8, density=0.1, steps=240,
           column_dim=(1024, 256), cell_dim=(8, 8), active_columns=(64, 32))
# (the upper level's k: a distal segment fires on 15 connected synapses to the winner cells of the step before, one winner
# per predicted column -- with k = 16 a single column the upper Spatial Pooler exchanges silences the prediction, and the
# reference alone then predicts in 0.19 of the stride-3 run's later steps; with k = 32 in 0.72, stride 1 in 0.85)
STRIDES = (1, 3)
RESETS = (48, 96, 99, 168)                      # level-0 steps a reset precedes: multiples of every stride recorded
LEARNING_OFF = (120, 144)                       # level-0 steps [a, b) with learning off (a, b multiples of every stride)


def predicted_share(prediction_any, stride, patterns):
    """Share of the top level's steps after the first two passes through the patterns that have a predicted column."""
    later = np.asarray(prediction_any)[-(-2 * patterns // stride):]
    return float(later.mean()) if later.size else 0.0


def record_run(ref, stride):
    seed, I, steps = CFG["seed"], CFG["input_dim"], CFG["steps"]
    C, K, k = CFG["column_dim"], CFG["cell_dim"], CFG["active_columns"]
    dims = (I, C[0])
    pairs = [refdiff.build_pair(ref, seed + l, dims[l], C[l], K[l], active_columns=k[l]) for l in range(2)]
    perm_digest = [refdiff.digest(ora.spatial_pooler.permanence) for _, ora in pairs]
    bank, _ = refdiff.make_inputs(seed + 100, CFG["patterns"], I, CFG["density"])
    out = {l: dict(active_column=[], cell_prediction=[], winner_cell=[], segments=[], predicted=[]) for l in range(2)}
    lists, upper_rows = [], []
    window = np.zeros(C[0], dtype=np.bool_)
    pending_reset = False                       # a reset the upper level still has to take (before its next step)

    def step(l, t, x, learn, reset, patch):
        ref_htm, ora = pairs[l]
        patch.seed, patch.cell_dim, patch.step = seed + l, K[l], t
        if reset:
            tm = ref_htm.temporal_memory
            tm.last_state = tm.get_empty_state()
            ora_sp = ora.spatial_pooler.step(x, learning=learn)
            ora_tm = ora.temporal_memory.step(ora_sp.active_column, learning=learn, prev_state=SimpleNamespace(
                cell_prediction=np.zeros((C[l], K[l]), bool), cell_activation=np.zeros((C[l], K[l]), bool), winner_cell=None,
                distal_state=None))
        else:
            ora_sp, ora_tm = ora.step(x, learning=learn)
        ref_sp, ref_tm = ref_htm.process(x, learning=learn)
        refdiff.compare_step(t, ref_sp, ref_tm, ora_sp, ora_tm, K[l])
        o = out[l]
        o["active_column"].append(refdiff.digest(ref_sp.active_column))
        o["cell_prediction"].append(refdiff.digest(ref_tm.cell_prediction))
        o["winner_cell"].append(refdiff.digest(ref_tm.winner_cell[0] * K[l] + ref_tm.winner_cell[1]))
        o["segments"].append(len(ref_tm.distal_state.segment_potential))
        o["predicted"].append(bool(ref_tm.cell_prediction.any()))
        return ref_sp

    with refdiff.keyed_rand(seed, K[0]) as patch:
        for t in range(steps):
            learn = not LEARNING_OFF[0] <= t < LEARNING_OFF[1]
            reset = t in RESETS
            pending_reset |= reset
            sp0 = step(0, t, bank[t % CFG["patterns"]], learn, reset, patch)
            lists.append(np.asarray(sp0.active_column))
            window[sp0.active_column] = True
            if (t + 1) % stride == 0:
                upper_rows.append(refdiff.digest(window))
                step(1, t // stride, window.copy(), learn, pending_reset, patch)
                pending_reset = False
                window[:] = False
    for l, (ref_htm, ora) in enumerate(pairs):
        refdiff.compare_store(steps, ref_htm, ora)
    share = predicted_share(out[1]["predicted"], stride, CFG["patterns"])
    assert share > 0.5, f"stride {stride}: only {share:.2f} of the top level's later steps predict a column"
    rec = {"permanence_digest": np.array(perm_digest, dtype=np.uint64), "upper_input_digest": np.array(upper_rows, dtype=np.uint64),
           "l0_lists": np.array(lists, dtype=np.uint16)}
    for l in range(2):
        for f in ("active_column", "cell_prediction", "winner_cell"):
            rec[f"l{l}_{f}_digest"] = np.array(out[l][f], dtype=np.uint64)
        rec[f"l{l}_segments"] = np.array(out[l]["segments"], dtype=np.int32)
        rec[f"l{l}_predicted"] = np.array(out[l]["predicted"], dtype=np.bool_)
    return rec, share


def main():
    ref = import_reference()
    z = {k: np.asarray(v) for k, v in CFG.items()}
    z.update(strides=np.array(STRIDES, dtype=np.int32), resets=np.array(RESETS, dtype=np.int32),
             learning_off=np.array(LEARNING_OFF, dtype=np.int32))
    for s in STRIDES:
        rec, share = record_run(ref, s)
        z.update({f"s{s}_{k}": v for k, v in rec.items()})
        print(f"stride {s}: {CFG['steps']} steps, segments {rec['l0_segments'][-1]} / {rec['l1_segments'][-1]}, "
              f"top level predicts in {share:.2f} of its later steps")
    path = os.path.join(HERE, "stack_two_level.npz")
    np.savez_compressed(path, **z)
    print(f"wrote {path}: {os.path.getsize(path)} bytes")


if __name__ == "__main__":
    main()
