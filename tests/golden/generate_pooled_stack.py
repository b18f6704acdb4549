#!/usr/bin/env python3
"""Records tests/golden/stack_pooled.npz from the UNMODIFIED reference, for tests/test_pooling_cpu.py and
tests/test_hip_pooling.py.

Needs a checkout of the reference (cokwa/bitHTM):   BITHTM_REFERENCE=<checkout> python tests/golden/generate_pooled_stack.py

The two reference models of tests/golden/generate_stack.py (300 -> 1 024 x 8, k = 64 -> 256 x 8, k = 32; level l draws with
seed + l through the keyed generator), chained through a pooling link (bithtm_amd/pooling.py is the
definition) where generate_stack.py chains them through the OR: after each of the lower model's steps the link takes the step's
sp_state.active_column and tm_state.cell_prediction.any(axis=1), and after every `stride` of them the upper model steps on the
link's row.  Sequence resets hit both levels and the link before the step they precede and stand on window boundaries; a stretch
of steps runs with learning off (the link goes on: it is dynamics, not weights).  Two oracle models run beside the two reference
models and are compared field by field every step.  One file holds two runs, stride 1 (prefix s1_) and stride 3 (s3_).

What is kept is the reference's side, per level and step: digests of active_column, cell_prediction and the flat winner cells,
the segment count, the digest of the upper level's input row and its bit count; and the link's final persistence.
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
from bithtm_amd.pooling import PoolingLink, PoolingState  # noqa: E402
from oracle.ref_hooks import import_reference  # noqa: E402

CFG = dict(seed=41, input_dim=300, patterns=8, density=0.1, steps=240,
           column_dim=(1024, 256), cell_dim=(8, 8), active_columns=(64, 32))
LINK = dict(active_weight=1, predicted_weight=8, decay=1, ceiling=16, union_bits=96)
STRIDES = (1, 3)
RESETS = (48, 96, 99, 168)                      # level-0 steps a reset precedes: multiples of every stride recorded
LEARNING_OFF = (120, 144)                       # level-0 steps [a, b) with learning off (a, b multiples of every stride)


def record_run(ref, stride):
    seed, I, steps = CFG["seed"], CFG["input_dim"], CFG["steps"]
    C, K, k = CFG["column_dim"], CFG["cell_dim"], CFG["active_columns"]
    dims = (I, C[0])
    pairs = [refdiff.build_pair(ref, seed + l, dims[l], C[l], K[l], active_columns=k[l]) for l in range(2)]
    perm_digest = [refdiff.digest(ora.spatial_pooler.permanence) for _, ora in pairs]
    bank, _ = refdiff.make_inputs(seed + 100, CFG["patterns"], I, CFG["density"])
    out = {l: dict(active_column=[], cell_prediction=[], winner_cell=[], segments=[], predicted=[]) for l in range(2)}
    upper_rows, upper_bits = [], []
    link = PoolingState(PoolingLink(stride=stride, **LINK).resolved(C[0], k[0]), C[0])
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
        return ref_sp, ref_tm

    with refdiff.keyed_rand(seed, K[0]) as patch:
        for t in range(steps):
            learn = not LEARNING_OFF[0] <= t < LEARNING_OFF[1]
            reset = t in RESETS
            pending_reset |= reset
            if reset:
                link.reset()
            sp0, tm0 = step(0, t, bank[t % CFG["patterns"]], learn, reset, patch)
            link.step(np.asarray(sp0.active_column), np.asarray(tm0.cell_prediction).any(axis=1))
            if (t + 1) % stride == 0:
                row = link.row()
                upper_rows.append(refdiff.digest(row))
                upper_bits.append(int(row.sum()))
                step(1, t // stride, row, learn, pending_reset, patch)
                pending_reset = False
    for l, (ref_htm, ora) in enumerate(pairs):
        refdiff.compare_store(steps, ref_htm, ora)
    rec = {"permanence_digest": np.array(perm_digest, dtype=np.uint64), "upper_input_digest": np.array(upper_rows, dtype=np.uint64),
           "upper_input_bits": np.array(upper_bits, dtype=np.int32), "link_persistence": link.persistence.copy(), "link_prev": link.prev.copy()}
    for l in range(2):
        for f in ("active_column", "cell_prediction", "winner_cell"):
            rec[f"l{l}_{f}_digest"] = np.array(out[l][f], dtype=np.uint64)
        rec[f"l{l}_segments"] = np.array(out[l]["segments"], dtype=np.int32)
        rec[f"l{l}_predicted"] = np.array(out[l]["predicted"], dtype=np.bool_)
    return rec


def main():
    ref = import_reference()
    z = {k: np.asarray(v) for k, v in CFG.items()}
    z.update(strides=np.array(STRIDES, dtype=np.int32), resets=np.array(RESETS, dtype=np.int32),
             learning_off=np.array(LEARNING_OFF, dtype=np.int32),
             link=np.array([LINK[n] for n in PoolingLink.PARAMETERS[1:]], dtype=np.int64))
    for s in STRIDES:
        rec = record_run(ref, s)
        z.update({f"s{s}_{k}": v for k, v in rec.items()})
        later = rec["l1_predicted"][-(-2 * CFG["patterns"] // s):]
        print(f"stride {s}: {CFG['steps']} steps, segments {rec['l0_segments'][-1]} / {rec['l1_segments'][-1]}, upper rows of "
              f"{rec['upper_input_bits'].min()}..{rec['upper_input_bits'].max()} bits, top level predicts in {later.mean():.2f} of its later steps")
    path = os.path.join(HERE, "stack_pooled.npz")
    np.savez_compressed(path, **z)
    print(f"wrote {path}: {os.path.getsize(path)} bytes")


if __name__ == "__main__":
    main()
