#!/usr/bin/env python3
"""Records tests/golden/lockstep_*.npz from the UNMODIFIED reference, for tests/test_oracle_vs_reference.py.

Needs a checkout of the reference (cokwa/bitHTM):   BITHTM_REFERENCE=<checkout> python tests/golden/generate_lockstep.py

Each file is one lock-step run of the reference (through its own `boosting=` / `inhibition=` hooks, with `np.random.rand`
replaced by the keyed generator) beside the oracle, checked field by field every step while it is recorded
(tests/refdiff.py: run_lockstep).  What is kept is the reference's side: a digest of every output it returned, every
step, and of its synapse store at the store checks.  `lockstep_bridge.npz` is recorded with the product's own
replacement, bithtm_amd.reference_bridge.keyed_rand, in place of the test infrastructure's, and also keeps every call the
reference made to it (the caller, the locals that decide the draws, the shape) with a digest of what it returned.
"""

import contextlib
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

import refdiff  # noqa: E402
from oracle.ref_hooks import import_reference  # noqa: E402

RUNS = {
    "small": dict(seed=31, input_dim=200, column_dim=1024, cell_dim=8, patterns=50, density=0.1, noise=0.02, steps=330,
                  store_every=30),
    "wide_epsilon": dict(seed=33, input_dim=160, column_dim=1024, cell_dim=8, patterns=20, density=0.1, noise=0.02,
                         steps=160, store_every=20, jump=0.1, epsilon=0.3),
    "prev_state": dict(seed=34, input_dim=160, column_dim=1024, cell_dim=8, patterns=20, density=0.1, noise=0.02, steps=150,
                       store_every=15, prev_schedule=lambda t: 3 if t > 10 and t % 7 == 0 else None),
    "learning_off_jumps": dict(seed=32, input_dim=160, column_dim=1024, cell_dim=16, patterns=30, density=0.1, noise=0.02,
                               steps=200, store_every=25, jump=0.2, learning_schedule=lambda t: (t % 17) != 3),
}
BRIDGE = dict(seed=35, input_dim=160, column_dim=1024, cell_dim=8, patterns=20, density=0.1, noise=0.02, steps=120,
              store_every=20, jump=0.1)


class LoggedBridge:
    """np.random.rand while the reference runs: hands each call to the product's KeyedRand from a stand-in caller with the
    same name and locals (tests/refdiff.py: call_rand_as) and logs it."""

    def __init__(self, patch):
        self.patch, self.log = patch, []

    @property
    def step(self):
        return self.patch.step

    @step.setter
    def step(self, t):
        self.patch.step = t

    def __call__(self, *shape):
        frame = sys._getframe(1)
        where = frame.f_code.co_name
        if where not in refdiff.RAND_CALLERS:
            return self.patch.fallback(*shape)
        args = refdiff.rand_call_args(where, frame.f_locals)
        np.random.rand = self.patch
        try:
            out = refdiff.call_rand_as(where, args, shape)
        finally:
            np.random.rand = self
        self.log.append((self.patch.step, refdiff.RAND_CALLERS.index(where), tuple(shape), args, refdiff.digest(out)))
        return out


def record_bridge(ref, path):
    from bithtm_amd.reference_bridge import keyed_rand
    loggers = []

    @contextlib.contextmanager
    def logged(seed, cell_dim):
        with keyed_rand(seed, cell_dim) as patch:
            loggers.append(LoggedBridge(patch))
            np.random.rand = loggers[-1]
            yield loggers[-1]

    original, refdiff.keyed_rand = refdiff.keyed_rand, logged
    try:
        stats = refdiff.record_lockstep(ref, path, **BRIDGE)[0]
    finally:
        refdiff.keyed_rand = original
    (logger,) = loggers
    log = logger.log
    args = [a for c in log for a in c[3]]
    z = refdiff.load_lockstep(path)
    z.update(call_step=np.array([c[0] for c in log], dtype=np.int32),
             call_where=np.array([c[1] for c in log], dtype=np.int8),
             call_shape=np.array([c[2] + (0,) * (2 - len(c[2])) for c in log], dtype=np.int64),
             call_shape_len=np.array([len(c[2]) for c in log], dtype=np.int8),
             call_arg_len=np.array([len(a) for a in args], dtype=np.int64),
             call_args=np.concatenate(args).astype(np.int64) if args else np.zeros(0, np.int64),
             call_digest=np.array([c[4] for c in log], dtype=np.uint64))
    np.savez_compressed(path, **z)
    return stats, len(log)


def main():
    ref = import_reference()
    for name, cfg in RUNS.items():
        path = os.path.join(HERE, f"lockstep_{name}.npz")
        stats = refdiff.record_lockstep(ref, path, **cfg)[0]
        print(f"wrote {path}: {cfg['steps']} steps, {stats['segments']} segments, {os.path.getsize(path)} bytes")
    path = os.path.join(HERE, "lockstep_bridge.npz")
    stats, calls = record_bridge(ref, path)
    print(f"wrote {path}: {BRIDGE['steps']} steps, {stats['segments']} segments, {calls} keyed draws, {os.path.getsize(path)} bytes")


if __name__ == "__main__":
    main()
