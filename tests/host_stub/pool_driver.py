"""Driver of the launch traces of pooling links (tests/test_pooling_cpu.py; used as coordinate_driver.py is: the engine's host code
host-only, no sanitizer, nothing preloaded, over tests/host_stub's runtime with BITHTM_STUB_TRACE).

    pool_driver.py plain    prints one JSON object {"<pattern> graph=<bool>": trace lines} of a PLAIN stack's calls: what
                            tests/golden/stack_traces_before.json holds, recorded with this mode on the commit before pooling links
    pool_driver.py all      the same patterns under "plain", the same calls of a stack whose link is a PoolingLink under "pooled",
                            "refused": the trace lines of every refused htm_pool_columns call (none), "codes" their return codes,
                            "accepted" the codes of calls at the limits (all 0) and "accepted_trace" their launches

Kernels do nothing in the stub: the trace says which launches and copies the host code makes, not what they compute."""
import ctypes as C
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
TRACE = os.environ["BITHTM_STUB_TRACE"]
os.environ["BITHTM_EAGER_BELOW"] = "0"
import bithtm_amd as B  # noqa: E402

I, C0, C1 = 100, 512, 256
ALL = ("counters", "active_column", "column_prediction")
BANK = np.random.RandomState(1).rand(8, I) < 0.1
RESETS = np.arange(8) % 4 == 0


def lines():
    with open(TRACE) as f:
        return f.read().splitlines()


def traced(call):
    n = len(lines())
    call()
    return lines()[n:]


def patterns(make, use_graph):
    """The calls of one stack, each traced: a first run, a second of the same length, a recorded run with resets, and a run in
    chunks of 8 steps."""
    out = {}
    stack = make()
    stack.process(BANK[0])
    stack.process(BANK[1])
    out["first run"] = traced(lambda: stack.run(BANK, 40, use_graph=use_graph))
    out["second run"] = traced(lambda: stack.run(BANK, 40, use_graph=use_graph))
    out["recorded run with resets"] = traced(lambda: stack.run(BANK, 8, use_graph=use_graph, record=ALL, resets=RESETS))
    stack.chunk_steps = 8
    out["run in chunks"] = traced(lambda: stack.run(BANK, 24, use_graph=use_graph))
    out["process"] = traced(lambda: (stack.process(BANK[2]), stack.process(BANK[3])))
    return {f"{name} graph={use_graph}": v for name, v in out.items()}


def plain():
    out = {}
    for use_graph in (True, False):
        out.update(patterns(lambda: B.RegionStack(I, [(C0, 8), (C1, 8)], strides=[2]), use_graph))
    return out


def refusals():
    from bithtm_amd import _lib
    stack = B.RegionStack(I, [(C0, 8), (C1, 8)], links=[B.PoolingLink(stride=2)])
    eng = stack.levels[1].engine
    lib, h, void = eng.lib, eng.h, C.c_void_p
    k, n = 10, 4
    W = eng.words
    buf = lambda nbytes: eng.device_buffer(nbytes + 64, np.zeros(nbytes + 64, np.uint8))
    lists, colpred, pers, prev, bits = buf(4 * k * n * 2), buf(4 * 16 * n * 2), buf(C0), buf(64), buf(16)
    bank = buf(4 * W * 8)
    window = 2 * W * 4 + W * 32                     # a window's scratch at stride 2: two bitmap rows and a snapshot row
    scratch = buf(8 * window)

    def link(**kw):
        p = dict(stride=2, active_weight=1, predicted_weight=8, decay=1, ceiling=16, union_bits=64)
        p.update(kw)
        out = _lib.HtmPoolLink()
        out.struct_bytes = kw.get("struct_bytes", C.sizeof(_lib.HtmPoolLink))
        for name in ("stride", "active_weight", "predicted_weight", "decay", "ceiling", "union_bits"):
            setattr(out, name, p[name])
        return out

    def call(handle=h, lk=None, lists=lists, k=k, colpred=colpred, n=n, pers=pers, prev=prev, bits=bits, scratch=scratch, scratch_bytes=8 * window,
             bank=bank, bank_rows=8, first_row=0):
        v = lambda p: void(p) if p else None
        return lambda: lib.htm_pool_columns(handle, lk or link(), v(lists), k, v(colpred), n, v(pers), v(prev), v(bits), v(scratch), scratch_bytes,
                                            v(bank), bank_rows, first_row)
    plain_tm = B.TemporalMemory(64, 4, seed=1)      # a handle without the device's Spatial Pooler
    plain_tm.run(np.arange(8).reshape(2, 4), 2)
    ahead = B.HierarchicalTemporalMemory(C0, 64, 4, seed=2)
    ahead.run(np.zeros((3, C0), bool), 5, continuing=True, use_graph=False)
    is_ahead = ahead.engine.run_plan(5, continuing=True)["pipelined"]
    bad = {"a null handle": call(handle=None), "null lists": call(lists=0), "a null column prediction": call(colpred=0), "a null persistence": call(pers=0),
           "a null prev": call(prev=0), "a null scratch": call(scratch=0), "a null bank": call(bank=0),
           "k 0": call(k=0), "stride 0": call(lk=link(stride=0)), "n_rows -1": call(n=-1), "bank_rows 0": call(bank_rows=0), "first_row -1": call(first_row=-1),
           "first_row at bank_rows": call(first_row=8), "a misaligned bank": call(bank=bank + 4),
           "struct_bytes": call(lk=link(struct_bytes=28)), "active_weight -1": call(lk=link(active_weight=-1)), "active_weight 256": call(lk=link(active_weight=256)),
           "predicted_weight -1": call(lk=link(predicted_weight=-1)), "predicted_weight 256": call(lk=link(predicted_weight=256)),
           "both weights 0": call(lk=link(active_weight=0, predicted_weight=0)), "decay 0": call(lk=link(decay=0)), "decay 256": call(lk=link(decay=256)),
           "ceiling 0": call(lk=link(ceiling=0)), "ceiling 256": call(lk=link(ceiling=256)), "union_bits 0": call(lk=link(union_bits=0)),
           "union_bits above the columns": call(lk=link(union_bits=C0 + 1)),
           "a misaligned persistence": call(pers=pers + 4), "a misaligned prev": call(prev=prev + 2), "a misaligned scratch": call(scratch=scratch + 8),
           "a scratch too small for one window": call(scratch_bytes=window - 1), "a negative scratch": call(scratch_bytes=-1),
           "a handle without the Spatial Pooler": call(handle=plain_tm._engine.h)}
    if is_ahead:
        bad["a handle that is ahead"] = call(handle=ahead.engine.h, lk=link(union_bits=32))
    good = {"one window of scratch": call(scratch_bytes=window), "no rows": call(n=0), "the largest parameters": call(lk=link(active_weight=255, predicted_weight=255, decay=255, ceiling=255, union_bits=C0)),
            "the smallest parameters": call(lk=link(stride=1, active_weight=0, predicted_weight=1, decay=1, ceiling=1, union_bits=1)),
            "no reset bits": call(bits=0), "the last first_row": call(first_row=7)}
    out, codes = {}, {}
    out["refused"] = traced(lambda: codes.update({name: c() for name, c in bad.items()}))
    out["codes"] = codes
    accepted = {}
    out["accepted_trace"] = {}
    for name, c in good.items():
        out["accepted_trace"][name] = traced(lambda: accepted.update({name: c()}))
    out["accepted"] = accepted
    stack.run(BANK, 8)                              # ... and the handle goes on
    return out


def main():
    if sys.argv[1] == "plain":
        print(json.dumps(plain()))
        return
    out = {"plain": plain(), "pooled": {}}
    for use_graph in (True, False):
        out["pooled"].update(patterns(lambda: B.RegionStack(I, [(C0, 8), (C1, 8)], links=[B.PoolingLink(stride=2)]), use_graph))
    out.update(refusals())
    print(json.dumps(out))


if __name__ == "__main__":
    main()
