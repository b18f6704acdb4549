"""Driver of the live tick's launch trace (tests/test_live_tick_cpu.py; tests/host_stub/hip_stub_runtime.cpp with
BITHTM_STUB_TRACE): the engine's host code, built host-only without a sanitizer and loaded through BITHTM_LIBRARY, driven
through ModelGroup.tick / ModelGroup.reset while the stub runtime writes one line per kernel launch and asynchronous copy.

Prints one JSON object:
  "tick"   {"B=<n> enc=<0|1> resets=<0|1>": the trace lines of one eager tick behind a warm-up tick}
  "step"   {"B=<n>": the lines of one recorded, decoding htm_group_step of the same group}
  "reset"  {"B=<n>": the lines of group.reset(mask)}
  "graph"  the lines of the second and third tick of a group that replays graphs (BITHTM_EAGER_BELOW = 0)

Kernels do nothing in the stub: the trace says which launches and copies the host code makes, not what they compute."""
import ctypes as C
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
TRACE = os.environ["BITHTM_STUB_TRACE"]
os.environ["BITHTM_EAGER_BELOW"] = "0"              # use_graph alone decides between graphs and eager launches
import bithtm_amd as B  # noqa: E402
from bithtm_amd.engine import pack_bits  # noqa: E402
from live_tick_cases import MID, encoder_for  # noqa: E402

I, Cn, K, k = MID


def lines():
    with open(TRACE) as f:
        return f.read().splitlines()


def traced(call):
    n = len(lines())
    call()
    return lines()[n:]


def group_of(n):
    return B.ModelGroup.create(n, I, Cn, K, active_columns=k, seeds=range(3, 3 + n))


def inputs(n, enc, seed):
    rng = np.random.RandomState(seed)
    return rng.rand(n, len(enc)) if enc is not None else rng.rand(n, I) < 0.1


def recorded_decoding_step(group, X):
    """htm_group_step with a record and decoding rows on every member: the launches the tick's budget is counted against."""
    words = (I + 31) // 32
    packed = np.ascontiguousarray(np.stack([pack_bits(x, words) for x in X]), dtype=np.uint32)
    group._current()
    recs, _ = group._records(("counters", "predicted_input"), 1)
    try:
        group._check(group.lib.htm_group_step(group._g, packed.ctypes.data_as(C.c_void_p), 1, recs), "htm_group_step")
    finally:
        group._unset_votes()
    for m in group.models:
        m.engine.steps += 1
        m.temporal_memory._new_state(None)


def main():
    out = {"tick": {}, "step": {}, "reset": {}}
    for n in (1, 7):
        mask = np.arange(n) % 3 == 0                # (member 0 is flagged at either size)
        for with_enc in (0, 1):
            enc = encoder_for(MID) if with_enc else None
            for with_resets in (0, 1):
                group = group_of(n)
                group.tick(inputs(n, enc, 1), encoder=enc, use_graph=False)
                resets = mask if with_resets else None
                out["tick"][f"B={n} enc={with_enc} resets={with_resets}"] = traced(
                    lambda: group.tick(inputs(n, enc, 2), encoder=enc, resets=resets, use_graph=False))
        group = group_of(n)
        group.tick(inputs(n, None, 1), use_graph=False)
        out["step"][f"B={n}"] = traced(lambda: recorded_decoding_step(group, inputs(n, None, 3)))
        out["reset"][f"B={n}"] = traced(lambda: group.reset(mask))
    group = group_of(3)
    enc = encoder_for(MID)
    for t in range(2):                              # (one graph per step parity)
        group.tick(inputs(3, enc, t), encoder=enc)
    out["graph"] = [traced(lambda: group.tick(inputs(3, enc, 2 + t), encoder=enc)) for t in range(2)]
    print(json.dumps(out))


if __name__ == "__main__":
    main()
