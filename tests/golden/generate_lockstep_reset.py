#!/usr/bin/env python3
"""Records tests/golden/lockstep_reset.npz from the UNMODIFIED reference, for tests/test_sequence_reset_cpu.py.

Needs a checkout of the reference (cokwa/bitHTM):   BITHTM_REFERENCE=<checkout> python tests/golden/generate_lockstep_reset.py

A lock-step run as generate_lockstep.py records them (tests/refdiff.py), with sequence resets in the reference's own idiom:
before the steps in RESETS, `tm.last_state = tm.get_empty_state()` (networks.py:57-65, read by process at :92-93) -- a
reset at step 1, two consecutive resets, resets on steps with learning off.  The oracle runs beside it with the empty state
as prev_state and is checked field by field every step while it is recorded.  What is kept is the reference's side: a
digest of every output every step and of its synapse store at the store checks, the reset steps and the learning flags.
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

RUN = dict(seed=36, input_dim=160, column_dim=1024, cell_dim=8, patterns=20, density=0.1, noise=0.02, steps=160, store_every=10)
RESETS = sorted({1, 20, 40, 41, 60, 80, 100, 101, 120, 140} | {t for t in range(160) if t % 17 == 3})
LEARNING_OFF = [t for t in range(160) if t % 17 == 3]       # (each of these also resets)


def main():
    ref = import_reference()
    cfg = RUN
    seed, I, C, K, steps = cfg["seed"], cfg["input_dim"], cfg["column_dim"], cfg["cell_dim"], cfg["steps"]
    np.random.seed(seed)
    perm0 = ref.projections.DenseProjection(I, C).permanence          # what build_pair's reference will draw
    ref_htm, ora = refdiff.build_pair(ref, seed, I, C, K)
    bank, rng = refdiff.make_inputs(seed + 1, cfg["patterns"], I, cfg["density"])
    tm = ref_htm.temporal_memory
    digests, stores, store_steps, learning, names = [], [], [], [], {}
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
            ref_sp, ref_tm = ref_htm.process(x, learning=learn)
            refdiff.compare_step(t, ref_sp, ref_tm, ora_sp, ora_tm, K)
            learning.append(learn)
            fields = refdiff.step_fields(ref_sp, ref_tm)
            names.setdefault("step", list(fields))
            digests.append([refdiff.digest(a) for a in fields.values()])
            if t % cfg["store_every"] == 0 or t == steps - 1:
                refdiff.compare_store(t, ref_htm, ora)
                fields = refdiff.reference_store_fields(ref_htm)
                names.setdefault("store", list(fields))
                store_steps.append(t)
                stores.append([refdiff.digest(a) for a in fields.values()])
    path = os.path.join(HERE, "lockstep_reset.npz")
    np.savez_compressed(
        path, **{k: np.asarray(v) for k, v in cfg.items() if k != "store_every"}, jump=np.float64(0.0), epsilon=np.float64(np.nan),
        resets=np.array(RESETS, dtype=np.int32), learning=np.array(learning, dtype=np.bool_),
        step_field_names=np.array(names["step"]), step_digest=np.array(digests, dtype=np.uint64),
        store_field_names=np.array(names["store"]), store_steps=np.array(store_steps, dtype=np.int32),
        store_digest=np.array(stores, dtype=np.uint64), permanence_digest=np.uint64(refdiff.digest(perm0)),
        segments=np.int64(ora.temporal_memory.S))
    print(f"wrote {path}: {steps} steps, {len(RESETS)} resets, {ora.temporal_memory.S} segments, {os.path.getsize(path)} bytes")


if __name__ == "__main__":
    main()
