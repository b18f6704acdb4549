"""Driver of the launch trace for stream forks (tests/test_stream_fork_cpu.py; built and run as tests/test_launch_trace_cpu.py
runs trace_driver.py: the engine's host code host-only, no sanitizer, nothing preloaded, over tests/host_stub's runtime with
BITHTM_STUB_TRACE).  Prints one JSON object:
    sync        the trace lines of one InferenceView.sync() (htm_view_sync)
    resync      ... of a second one, after the parent learned and the fork stepped
    after_sync  ... of the fork's first step behind a sync that followed the parent's learning
    lookahead   ... of one lookahead() chunk of `windows` windows
Kernels do nothing in the stub: the trace says which launches and copies the host code makes, not what they compute."""
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
TRACE = os.environ["BITHTM_STUB_TRACE"]
os.environ["BITHTM_EAGER_BELOW"] = "0"
import bithtm_amd as B  # noqa: E402

I, C, K = 100, 512, 8
BANK = np.random.RandomState(1).rand(7, I) < 0.1


def lines():
    with open(TRACE) as f:
        return f.read().splitlines()


def traced(call):
    n = len(lines())
    call()
    return lines()[n:]


def main():
    np.random.seed(K)
    tm = B.TemporalMemory(C, K, distal_projection=B.PredictiveProjection(C * K, segment_capacity=8192), seed=K)
    htm = B.HierarchicalTemporalMemory(I, C, K, temporal_memory=tm)
    htm.run(BANK, 9)
    fork = htm.inference_view()
    out = {"sync": traced(lambda: fork.sync())}
    assert fork.engine.steps == htm.engine.steps == 9
    htm.run(BANK, 4)
    fork.run(BANK, 3)
    out["resync"] = traced(lambda: fork.sync())
    assert fork.engine.steps == 13
    out["after_sync"] = traced(lambda: fork.process(BANK[0]))
    sibling = fork.fork()
    assert sibling.engine.steps == 14 and sibling.sync(fork) is sibling
    windows = 3
    htm.lookahead_chunk = windows
    htm.lookahead(BANK, 2, 2)                        # (the kept fork, its bank and its result buffer are made here)
    out["windows"] = windows
    out["lookahead"] = traced(lambda: htm.lookahead(BANK, 2 * windows, 4, every=2, record=("counters",), resets=np.eye(7, dtype=bool)[2]))
    assert htm.engine.steps == 13 + 2 + 2 * windows
    print(json.dumps(out))


if __name__ == "__main__":
    main()
