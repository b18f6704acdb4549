"""Driver of tests/test_winner_list_cpu.py (tests/host_stub/hip_stub_runtime.cpp with BITHTM_STUB_TRACE, as trace_driver.py): which
kernels the engine's host code launches per step -- a batched run() in the two-launch schedule, whose steps begin with
k_first_handover and must end with k_last_handover, and the callers that keep k_learn_scan_emit.  Prints one JSON object:
{pattern: [plain kernel name of every launch line]}."""
import json
import os
import re
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
TRACE = os.environ["BITHTM_STUB_TRACE"]
os.environ["BITHTM_EAGER_BELOW"] = "0"              # use_graph alone decides between graphs and eager launches
import bithtm_amd as B  # noqa: E402

I, C = 100, 512
BANK = np.random.RandomState(1).rand(7, I) < 0.1


def lines():
    with open(TRACE) as f:
        return f.read().splitlines()


def kernel(line):
    m = re.match(r"launch _Z(\d+)", line)
    return line[m.end():m.end() + int(m.group(1))] if m else None


def traced(call):
    n = len(lines())
    call()
    return [k for k in map(kernel, lines()[n:]) if k]


def model(K=8, **env):
    for name in ("BITHTM_LEAN", "BITHTM_SCAN_LARGE"):
        os.environ.pop(name, None)
    os.environ.update(env)
    np.random.seed(K)
    return B.HierarchicalTemporalMemory(I, C, K, seed=K)


def main():
    out = {}
    for name, env in (("run", {}), ("run large", dict(BITHTM_SCAN_LARGE="1")), ("run lean1", dict(BITHTM_LEAN="1")), ("run lean0", dict(BITHTM_LEAN="0"))):
        for K in (8, 40):
            htm = model(K, **env)
            # eager launches (a graph's are captured once); the second call streams on: its first step is a steady one too
            out[f"{name} K={K}"] = traced(lambda: htm.run(BANK, 12, use_graph=False, continuing=True))
            out[f"{name} K={K} more"] = traced(lambda: htm.run(BANK, 5, use_graph=False))
            out[f"{name} K={K} resume"] = traced(lambda: (htm.run(BANK, 6, use_graph=False, continuing=True), htm.run(BANK, 3, use_graph=False, pipeline=False)))
            out[f"{name} K={K} capture"] = traced(lambda: htm.run(BANK, 9, use_graph=True))
            out[f"{name} K={K} learning off"] = traced(lambda: htm.run(BANK, 4, use_graph=False, learning=False))
            out[f"{name} K={K} process"] = traced(lambda: htm.process(BANK[0]))
    group = B.ModelGroup([model() for _ in range(3)])
    inputs = np.random.RandomState(2).rand(3, 7, I) < 0.1
    out["group step"] = traced(lambda: group.process(inputs[:, 0]))
    out["group run"] = traced(lambda: group.run(inputs, 6, use_graph=False))
    print(json.dumps(out))


if __name__ == "__main__":
    main()
