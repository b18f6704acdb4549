"""Driver of the launch trace (tests/test_launch_trace_cpu.py; tests/host_stub/hip_stub_runtime.cpp with BITHTM_STUB_TRACE): the
engine's host code, built host-only WITHOUT a sanitizer and loaded through BITHTM_LIBRARY, driven through the Python classes
while the stub runtime writes one line per kernel launch, asynchronous memset / copy, capture and graph launch.

    trace_driver.py invariants   prints one JSON object: the launch lines of the call patterns the committed test asserts on
    trace_driver.py full         every batched call pattern in every schedule, host-fed process() loops under each combination
                                 of the step's knobs (inputs below, at and above the width of a launch's arguments), the
                                 stand-alone Spatial Pooler (process, run, phase by phase with plug-in objects) and a
                                 column-sharded group of two ranks in one process, with a `# label` line before each pattern:
                                 the trace file of one build of the engine is compared with another's by diff (a refactor of
                                 the host code must leave it as it was)

Kernels do nothing in the stub, so the device state stays zero: what the trace holds is which launches the host code makes, in
which order, with which grids -- not what they compute."""
import gc
import itertools
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
from bithtm_amd.engine import HtmError  # noqa: E402

I, C = 100, 512
ALL = ("counters", "active_column", "column_prediction")
PIN = ALL + ("predicted_input",)
RESETS = np.array([1, 0, 0, 1, 1, 0, 0], bool)
BANK = np.random.RandomState(1).rand(7, I) < 0.1


def lines():
    with open(TRACE) as f:
        return f.read().splitlines()


def label(text):
    with open(TRACE, "a") as f:
        f.write(f"# {text}\n")


def kernel(line):
    """The plain name of the kernel a `launch` line names (its mangled device name starts _Z<length><name>), else None."""
    m = re.match(r"launch _Z(\d+)", line)
    return line[m.end():m.end() + int(m.group(1))] if m else None


def model(K=8, **env):
    for name in ("BITHTM_LEAN", "BITHTM_SCAN_LARGE"):
        os.environ.pop(name, None)
    os.environ.update(env)
    np.random.seed(K)
    return B.HierarchicalTemporalMemory(I, C, K, seed=K)


def traced(call):
    """The trace lines `call` appends."""
    n = len(lines())
    call()
    return lines()[n:]


def invariants():
    out = {}
    modes = dict(record=PIN, resets=RESETS, use_graph=False)
    # modes do not outlive their call: the same plain run and host-fed step behind a call with every mode and behind a plain one
    tails = []
    for kw in (modes, dict(use_graph=False)):
        htm = model()
        htm.run(BANK, 8, **kw)
        tails.append(traced(lambda: (htm.run(BANK, 6, use_graph=False), htm.process(BANK[0]))))
    out["tail_after_modes"], out["tail_after_plain"] = tails
    # the step the resume fallback runs carries the call's modes, and the call's descriptors are filled once
    for n in (7, 1):
        htm = model()
        htm.run(BANK, 5, continuing=True, use_graph=False)
        ahead = htm.engine.run_plan(5, continuing=True)["pipelined"]
        try:
            htm.process(BANK[0])
            ahead = False
        except HtmError as e:
            ahead = ahead and "ahead" in str(e)
        out[f"fallback_{n}"] = dict(ahead=bool(ahead), kernels=[kernel(x) for x in traced(lambda: htm.run(BANK, n, pipeline=False, **modes))])
    print(json.dumps(out))


def drive_run(htm, kw, use_graph):
    eng = htm.engine
    flags = dict(use_graph=use_graph)
    htm.process(BANK[0])
    htm.run(BANK, 40, **flags, **kw)
    for n in (3, 20, 17):
        htm.run(BANK, n, continuing=True, **flags, **kw)
    htm.run(BANK, 5, **flags, **kw)
    htm.run(BANK, 6, continuing=True, **flags, **kw)
    htm.run(BANK, 9, pipeline=False, **flags, **kw)             # the resume fallback
    htm.run(BANK, 6, continuing=True, **flags, **kw)
    htm.run(BANK, 1, pipeline=False, **flags, **kw)             # ... of one step
    htm.process(BANK[1])
    dev = htm._bank[1]                              # (the device bank run() uploaded and keeps)
    resets = eng.upload_resets(RESETS) if "resets" in kw else None
    for n, pipe, cont in ((40, True, False), (12, True, True), (12, False, False), (1, True, False)):
        args = dict(use_graph=use_graph, pipeline=pipe, continuing=cont)
        label(f"plan {n} {pipe} {cont}: {sorted(eng.run_plan(n, **args).items())}")
        eng.prepare(dev, len(BANK), n, record="record" in kw, resets=resets, **args)
        htm.run(BANK, n, pipeline=pipe, continuing=cont, use_graph=use_graph, **kw)
    htm.run(BANK, 2, **flags, **kw)
    htm.process(BANK[2])


def second_handle(kw, use_graph, lean):
    htm = model(8, BITHTM_LEAN=lean)
    htm.run(BANK, 20, continuing=True, use_graph=use_graph, **kw)
    ahead = htm.engine.run_plan(20, continuing=True)["pipelined"]
    other = model(8, BITHTM_LEAN=lean)              # (a stream of its own: the first model's pipelined schedule is gone)
    other.process(BANK[1])
    assert ahead and not htm.engine.run_plan(17, continuing=True)["pipelined"]
    htm.run(BANK, 17, continuing=True, use_graph=use_graph, **kw)
    htm.run(BANK, 9, use_graph=use_graph, **kw)
    htm.process(BANK[0])
    other.process(BANK[0])


def forecast(use_graph, record):
    htm = model()
    htm.process(BANK[0])
    htm.run(BANK, 10)
    htm.forecast(12, record=record, use_graph=use_graph)
    htm.process(BANK[1])


def tm_run(use_graph, record, resets, K):
    lists = np.stack([np.random.RandomState(r).choice(C, 10, replace=False) for r in range(7)])
    tm = B.TemporalMemory(C, K, seed=3)
    tm.run(lists, 40, use_graph=use_graph, record=record, resets=resets)
    tm.run(lists, 3, use_graph=use_graph, record=record, resets=resets)
    tm.run(lists, 5, use_graph=use_graph)


def group(use_graph, record):
    inputs = np.random.RandomState(2).rand(3, 7, I) < 0.1
    group = B.ModelGroup([model() for _ in range(3)])
    group.process(inputs[:, 0])
    group.run(inputs, 40, use_graph=use_graph, record=record)
    group.run(inputs, 3, use_graph=use_graph, record=record)
    group.process(inputs[:, 1], record=record is not None)
    group.forecast(6, record=record, use_graph=use_graph)
    # feedback on one member only
    group._current()
    banks = group._banks(inputs)
    first = group.models[0].engine
    first.set_run_feedback(banks[0], 7)
    try:
        group._check(group.lib.htm_group_run(group._g, banks, 7, 20, 0, int(use_graph), None), "htm_group_run")
    finally:
        first.set_run_feedback(None)
    for m in group.models:
        m.engine.steps += 20
    group.run(inputs, 4, use_graph=use_graph)
    group.models[1].process(inputs[1, 2])


def stack(use_graph):
    stack = B.RegionStack(I, [(C, 8), (256, 8)], strides=[2])
    stack.process(BANK[0])
    stack.process(BANK[1])
    stack.run(BANK, 40, use_graph=use_graph, record=ALL)
    stack.run(BANK, 6, use_graph=use_graph, record=ALL, resets=np.arange(7) % 4 == 0)    # (flags at multiples of the stride)
    stack.process(BANK[2])


STEP_KNOBS = ("BITHTM_STEP_SPLIT", "BITHTM_DEFER_TAIL", "BITHTM_FUSE_TM", "BITHTM_TAIL_ROWS")


def host_fed(input_dim, K, off):
    """A process() loop (htm_step: one input per call) with the knobs `off` of the step set to 0; then an entry point that lets
    a held-back last launch go, and a step without learning."""
    for name in STEP_KNOBS:
        os.environ.pop(name, None)
    os.environ.update({name: "0" for name in off})
    np.random.seed(K)
    htm = B.HierarchicalTemporalMemory(input_dim, C, K, seed=K)      # (the knobs are read when the handle is created)
    for name in STEP_KNOBS:
        os.environ.pop(name, None)
    bank = np.random.RandomState(3).rand(7, input_dim) < 0.1
    for t in range(6):
        htm.process(bank[t])
    htm.run(bank, 3, use_graph=False)
    htm.process(bank[0], learning=False)
    htm.process(bank[1])


class HostProjection:
    """Plug-in objects with the reference's methods that live on the host: SpatialPooler.process then runs phase by phase."""

    def process(self, input_activation):
        return np.arange(C) % 5

    def update(self, input_activation, active_column):
        pass


class HostBoosting:
    def process(self, overlaps):
        return np.asarray(overlaps, np.float64) * 1.5

    def update(self, active_column):
        pass


class HostInhibition:
    def process(self, boosted):
        return np.sort(np.argsort(-np.asarray(boosted), kind="stable")[:10])


def spatial_pooler(use_graph, record):
    sp = B.SpatialPooler(I, C, 10)
    sp.process(BANK[0])
    sp.run(BANK, 12, use_graph=use_graph, record=record)
    sp.run(BANK, 3, use_graph=use_graph, learning=False)
    sp.process(BANK[1], learning=False)


def sp_phases(**foreign):
    sp = B.SpatialPooler(I, C, 10, **foreign)
    for t in range(3):
        sp.process(BANK[t])
    sp.process(BANK[3], learning=False)


def shard_group(use_graph, pipeline, K):
    from bithtm_amd.distributed import LocalGroup
    group = LocalGroup(2, I, C, K, permanence=np.random.RandomState(5).normal(0.0, 0.1, (C, I)), seed=5)
    group.process(BANK[0])
    group.upload_bank(BANK)
    group.run(6, use_graph=use_graph, pipeline=pipeline)
    group.run(2, stepwise=True)
    group.run(5, learning=False, use_graph=use_graph, pipeline=pipeline)
    group.process(BANK[1])


def full():
    def pattern(text, call, *args, **kw):           # (every pattern's models are gone before the next one's are made)
        label(text)
        call(*args, **kw)
        gc.collect()
    run_modes = {"plain": {}, "record": dict(record=ALL), "resets": dict(resets=RESETS), "record+resets": dict(record=ALL, resets=RESETS),
                 "predicted_input": dict(record=("predicted_input",)), "record+resets+predicted_input": dict(record=PIN, resets=RESETS)}
    for (name, kw), use_graph, lean, large, K in itertools.product(run_modes.items(), (True, False), "012", (None, "1"), (8, 40)):
        env = dict(BITHTM_LEAN=lean, **({"BITHTM_SCAN_LARGE": large} if large else {}))
        pattern(f"htm_run {name} graph={use_graph} lean={lean} scan_large={large} K={K}", lambda: drive_run(model(K, **env), kw, use_graph))
    for (name, kw), use_graph, lean in itertools.product(run_modes.items(), (True, False), "012"):
        pattern(f"second handle {name} graph={use_graph} lean={lean}", second_handle, kw, use_graph, lean)
    for use_graph, record in itertools.product((True, False), (None, ALL, PIN)):
        pattern(f"forecast graph={use_graph} record={record}", forecast, use_graph, record)
    for use_graph, record, resets, K in itertools.product((True, False), (None, ALL), (None, RESETS), (8, 40)):
        pattern(f"tm_run graph={use_graph} record={record} resets={resets is not None} K={K}", tm_run, use_graph, record, resets, K)
    for use_graph, record in itertools.product((True, False), (None, ALL, PIN)):
        pattern(f"group graph={use_graph} record={record}", group, use_graph, record)
    for use_graph in (True, False):
        pattern(f"stack graph={use_graph}", stack, use_graph)
    # host-fed steps: an input that rides in the launch's arguments, one just over their width (2080 bits: 65 packed words), and
    # one exactly at it (2048)
    for n_off in range(len(STEP_KNOBS) + 1):
        for off, input_dim, K in itertools.product(itertools.combinations(STEP_KNOBS, n_off), (I, 2080, 2048), (8, 40)):
            pattern(f"host-fed input_dim={input_dim} K={K} off={','.join(off)}", host_fed, input_dim, K, off)
    for use_graph, record in itertools.product((True, False), (None, ("active_column", "active_overlap", "active_boosted"))):
        pattern(f"spatial pooler graph={use_graph} record={record}", spatial_pooler, use_graph, record)
    for name, foreign in (("proximal_projection", HostProjection), ("boosting", HostBoosting), ("inhibition", HostInhibition)):
        pattern(f"sp phases, host {name}", sp_phases, **{name: foreign()})
    pattern("sp phases, host boosting + inhibition", sp_phases, boosting=HostBoosting(), inhibition=HostInhibition())
    for use_graph, pipeline, K in itertools.product((True, False), (True, False), (8, 32)):       # (a sharded handle: cell_dim <= 32)
        pattern(f"shard group graph={use_graph} pipeline={pipeline} K={K}", shard_group, use_graph, pipeline, K)


if __name__ == "__main__":
    {"invariants": invariants, "full": full}[sys.argv[1]]()
