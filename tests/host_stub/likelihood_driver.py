"""Driver of the launch traces of the anomaly likelihood (tests/test_likelihood_cpu.py; tests/host_stub/hip_stub_runtime.cpp with
BITHTM_STUB_TRACE), as tests/host_stub/live_tick_driver.py is for the live tick: the engine's host code, built host-only without
a sanitizer and loaded through BITHTM_LIBRARY, driven through ModelGroup.tick and AnomalyLikelihood.update_counts.

Prints one JSON object:
  "tick"    {"B=<n> enc=<0|1> scored=<0|1>": the trace lines of one eager tick behind a warm-up tick of the same kind}
  "update"  {"B=<n> T=<steps>": the lines of update_counts over T steps of n streams}
  "reset"   {"B=<n> mask=<0|1>": the lines of AnomalyLikelihood.reset}

Kernels do nothing in the stub: the trace says which launches and copies the host code makes, not what they compute."""
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
from likelihood_cases import CHUNK, P_SMALL, as_kwargs  # noqa: E402
from live_tick_cases import MID, encoder_for  # noqa: E402

I, Cn, K, k = MID


def lines():
    with open(TRACE) as f:
        return f.read().splitlines()


def traced(call):
    n = len(lines())
    call()
    return lines()[n:]


def inputs(n, enc, seed):
    rng = np.random.RandomState(seed)
    return rng.rand(n, len(enc)) if enc is not None else rng.rand(n, I) < 0.1


def main():
    out = {"tick": {}, "update": {}, "reset": {}}
    for n in (1, 7):
        for with_enc in (0, 1):
            enc = encoder_for(MID) if with_enc else None
            for scored in (0, 1):
                group = B.ModelGroup.create(n, I, Cn, K, active_columns=k, seeds=range(3, 3 + n))
                lk = B.AnomalyLikelihood(n, **as_kwargs(P_SMALL)) if scored else None
                group.tick(inputs(n, enc, 1), encoder=enc, use_graph=False, likelihood=lk)
                out["tick"][f"B={n} enc={with_enc} scored={scored}"] = traced(
                    lambda: group.tick(inputs(n, enc, 2), encoder=enc, use_graph=False, likelihood=lk))
    for n in (1, 3, 130):
        lk = B.AnomalyLikelihood(n, **as_kwargs(P_SMALL))
        lk.update_counts(np.ones((n, 1), np.int64), np.zeros((n, 1), np.int64), device=0)
        for T in (1, CHUNK, CHUNK + 1, 2 * CHUNK + 3):
            out["update"][f"B={n} T={T}"] = traced(lambda: lk.update_counts(np.ones((n, T), np.int64), np.zeros((n, T), np.int64)))
        out["reset"][f"B={n} mask=0"] = traced(lambda: lk.reset())
        out["reset"][f"B={n} mask=1"] = traced(lambda: lk.reset(np.arange(n) % 2 == 0))
    print(json.dumps(out))


if __name__ == "__main__":
    main()
