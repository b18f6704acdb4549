"""Driver of the launch traces of stacks of model groups (tests/test_group_stack_cpu.py; used as pool_driver.py is: the engine's
host code host-only, no sanitizer, nothing preloaded, over tests/host_stub's runtime with BITHTM_STUB_TRACE).

    group_stack_driver.py before   prints one JSON object: "plain" and "pooled", the RegionStack patterns of pool_driver.py, and
                                   "group", a ModelGroup.run -- what tests/golden/group_stack_traces_before.json holds, recorded with
                                   this mode on the commit before stacks of groups (the mode uses nothing younger)
    group_stack_driver.py all      the same under "before"; "stacks": {"<plain|pooled> B=<B>": {pattern: trace lines}} of
                                   GroupStack.run; "refused", "codes", "accepted", "accepted_trace": the two entries' refusals and
                                   calls at the limits; "python": the refusals of the Python layer that came before any library call

In the GroupStack traces the driver writes lines of its own between the runtime's: "py chunk" in front of every chunk's first
level, "py end" behind its last, "py sync" where the host waits for or reads from the device (Engine.sync, Engine.info,
Engine.read_words).  Kernels do nothing in the stub: the trace says which launches and copies the host code makes."""
import ctypes as C
import json
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import pool_driver as pd  # noqa: E402  (puts the repository on the path, reads BITHTM_STUB_TRACE, imports bithtm_amd as B)

B = pd.B
I, C0, C1 = pd.I, pd.C0, pd.C1
ALL = pd.ALL
traced, lines = pd.traced, pd.lines


def before():
    out = {"plain": pd.plain(), "pooled": {}}
    for use_graph in (True, False):
        out["pooled"].update(pd.patterns(lambda: B.RegionStack(I, [(C0, 8), (C1, 8)], links=[B.PoolingLink(stride=2)]), use_graph))
    group = B.ModelGroup.create(3, I, C0, 8)
    inputs = np.stack([pd.BANK] * 3)
    out["group"] = {"first run": traced(lambda: group.run(inputs, 8)), "second run": traced(lambda: group.run(inputs, 8)),
                    "recorded run": traced(lambda: group.run(inputs, 8, record=ALL))}
    return out


def note(text):
    with open(pd.TRACE, "a") as f:
        f.write(text + "\n")


def marked(stack):
    """`stack` with the driver's lines in its traces (see the module's docstring)."""
    from bithtm_amd.engine import Engine
    from bithtm_amd.group import ModelGroup
    if not getattr(Engine, "_driver_marked", False):
        Engine._driver_marked = True
        for name in ("sync", "info", "read_words"):
            def wrap(inner):
                def outer(self, *a, **kw):
                    note("py sync")
                    return inner(self, *a, **kw)
                return outer
            setattr(Engine, name, wrap(getattr(Engine, name)))
        inner_run = ModelGroup.run_into

        def run_into(self, *a, **kw):
            owner = getattr(self, "_driver_stack", None)
            if owner is not None and self is owner.groups[0]:
                note("py chunk")
            inner_run(self, *a, **kw)
            if owner is not None and self is owner.groups[-1]:
                note("py end")
        ModelGroup.run_into = run_into
    for g in stack.groups:
        g._driver_stack = stack
    return stack


def stack_patterns(make, n):
    inputs = np.stack([pd.BANK] * n)
    out = {}
    stack = marked(make(n))
    stack.process(inputs[:, 0])
    stack.process(inputs[:, 1])
    out["first run"] = traced(lambda: stack.run(inputs, 40))
    out["second run"] = traced(lambda: stack.run(inputs, 40))
    out["recorded run"] = traced(lambda: stack.run(inputs, 8, record=ALL))
    stack.chunk_steps = 8
    out["run in chunks"] = traced(lambda: stack.run(inputs, 24))
    out["eager run"] = traced(lambda: stack.run(inputs, 8, use_graph=False))
    return out


def python_refusals():
    """Every refusal of the Python layer, with the trace lines it left (none)."""
    stack = B.GroupStack(2, I, [(C0, 8), (C1, 8)], strides=[2])
    trained = B.RegionStack(I, [(C0, 8), (C1, 8)], strides=[2])
    views = B.GroupStack.views(trained, 2)
    good = np.zeros((2, 4, I), bool)
    calls = {"inputs of two dimensions": lambda: stack.run(good[0], 4), "another member count": lambda: stack.run(good[:1], 4),
             "another input_dim": lambda: stack.run(good[:, :, :-1], 4), "no rows": lambda: stack.run(good[:, :0], 4),
             "resets=": lambda: stack.run(good, 4, resets=np.zeros(4, bool)), "steps that are no multiple": lambda: stack.run(good, 3),
             "negative steps": lambda: stack.run(good, -2), "learning=True on views": lambda: views.run(good, 4, learning=True),
             "process: learning=True on views": lambda: views.process(good[:, 0], learning=True), "process: another shape": lambda: stack.process(good[0, 0]),
             "an unknown record field": lambda: stack.run(good, 4, record=("nothing",)), "predicted_value without an encoder": lambda: stack.run(good, 4, record=("predicted_value",))}
    out = {}

    def attempt(name, call):
        try:
            call()
            out[name] = "accepted"
        except (ValueError, NotImplementedError) as e:
            out[name] = type(e).__name__ + ": " + str(e)
    left = traced(lambda: [attempt(name, call) for name, call in calls.items()])
    stack.process(good[:, 0])                       # in the middle of a window
    attempt("a run in the middle of a window", lambda: stack.run(good, 4))
    attempt("a reset in the middle of a window", lambda: stack.reset())
    return {"refusals": out, "trace": left}


def refusals():
    from bithtm_amd import _lib
    n = 3
    stack = B.GroupStack(n, I, [(C0, 8), (C1, 8)], links=[B.PoolingLink(stride=2)])
    group = stack.groups[1]
    eng = group.models[0].engine
    lib, g, void = eng.lib, group._g, C.c_void_p
    k, rows = 10, 4
    W = eng.words
    buf = lambda nbytes: eng.device_buffer(nbytes + 64, np.zeros(nbytes + 64, np.uint8))
    each = lambda nbytes: [buf(nbytes) for _ in range(n)]
    lists, colpred, pers, prev, bits, banks = each(4 * k * rows * 2), each(4 * 16 * rows * 2), each(C0), each(64), each(16), each(4 * W * 8)
    window = 2 * W * 4 + W * 32                     # a window's scratch at stride 2: two bitmap rows and a snapshot row
    scratch = buf(8 * n * window)

    def link(**kw):
        p = dict(stride=2, active_weight=1, predicted_weight=8, decay=1, ceiling=16, union_bits=64)
        p.update(kw)
        out = _lib.HtmPoolLink()
        out.struct_bytes = kw.get("struct_bytes", C.sizeof(_lib.HtmPoolLink))
        for name in ("stride", "active_weight", "predicted_weight", "decay", "ceiling", "union_bits"):
            setattr(out, name, p[name])
        return out

    def table(ptrs):
        return None if ptrs is None else (void * len(ptrs))(*ptrs)

    def firsts(rows_):
        return None if rows_ is None else (C.c_int32 * len(rows_))(*rows_)

    def hole(ptrs, i=1, value=None):
        out = list(ptrs)
        out[i] = value if value is not None else None
        return out

    def pool(handle=g, lk=None, lists=lists, k=k, colpred=colpred, n_rows=rows, pers=pers, prev=prev, bits=bits, scratch=scratch, scratch_bytes=8 * n * window,
             banks=banks, bank_rows=8, first=(0, 3, 7)):
        return lambda: lib.htm_group_pool_columns(handle, lk or link(), table(lists), k, table(colpred), n_rows, table(pers), table(prev), table(bits),
                                                  void(scratch) if scratch else None, scratch_bytes, table(banks), bank_rows, firsts(first))

    def pack(handle=g, lists=lists, k=k, n_rows=rows, stride=2, banks=banks, bank_rows=8, first=(0, 3, 7)):
        return lambda: lib.htm_group_pack_columns(handle, table(lists), k, n_rows, stride, table(banks), bank_rows, firsts(first))
    # a group with a member on a stream of its own, and one with a member that is ahead
    own = [B.HierarchicalTemporalMemory(C0, C1, 8, seed=s) for s in range(2)]
    mixed = B.ModelGroup(own)
    # (member 0 is the one ahead: the group's stream is its own, so the refusal is for being ahead)
    ahead_models = B.ModelGroup([B.HierarchicalTemporalMemory(C0, 64, 4, seed=s) for s in range(2)])
    ahead_models.models[0].run(np.zeros((3, C0), bool), 5, continuing=True, use_graph=False)
    is_ahead = ahead_models.models[0].engine.run_plan(5, continuing=True)["pipelined"]
    two = lambda ptrs: ptrs[:2]
    bad = {"pool: a null group": pool(handle=None), "pool: null lists": pool(lists=None), "pool: a null entry of the lists": pool(lists=hole(lists)),
           "pool: null column predictions": pool(colpred=None), "pool: a null entry of the column predictions": pool(colpred=hole(colpred, 2)),
           "pool: null persistences": pool(pers=None), "pool: a null entry of the persistences": pool(pers=hole(pers, 0)),
           "pool: null prevs": pool(prev=None), "pool: a null entry of the prevs": pool(prev=hole(prev)), "pool: a null scratch": pool(scratch=0),
           "pool: null banks": pool(banks=None), "pool: a null entry of the banks": pool(banks=hole(banks, 2)), "pool: null first_rows": pool(first=None),
           "pool: k 0": pool(k=0), "pool: stride 0": pool(lk=link(stride=0)), "pool: n_rows -1": pool(n_rows=-1), "pool: bank_rows 0": pool(bank_rows=0),
           "pool: a first_row of -1": pool(first=(0, -1, 0)), "pool: a first_row at bank_rows": pool(first=(0, 0, 8)),
           "pool: a misaligned bank of one member": pool(banks=hole(banks, 1, banks[1] + 4)), "pool: struct_bytes": pool(lk=link(struct_bytes=28)),
           "pool: active_weight 256": pool(lk=link(active_weight=256)), "pool: both weights 0": pool(lk=link(active_weight=0, predicted_weight=0)),
           "pool: decay 0": pool(lk=link(decay=0)), "pool: ceiling 256": pool(lk=link(ceiling=256)), "pool: union_bits 0": pool(lk=link(union_bits=0)),
           "pool: union_bits above the columns": pool(lk=link(union_bits=C0 + 1)),
           "pool: a misaligned persistence of one member": pool(pers=hole(pers, 2, pers[2] + 4)), "pool: a misaligned prev of one member": pool(prev=hole(prev, 0, prev[0] + 8)),
           "pool: a misaligned scratch": pool(scratch=scratch + 8), "pool: a scratch too small for one window of all members": pool(scratch_bytes=n * window - 1),
           "pool: a negative scratch": pool(scratch_bytes=-1),
           "pack: a null group": pack(handle=None), "pack: null lists": pack(lists=None), "pack: a null entry of the lists": pack(lists=hole(lists, 2)),
           "pack: null banks": pack(banks=None), "pack: a null entry of the banks": pack(banks=hole(banks, 0)), "pack: null first_rows": pack(first=None),
           "pack: k 0": pack(k=0), "pack: stride 0": pack(stride=0), "pack: n_rows -1": pack(n_rows=-1), "pack: bank_rows 0": pack(bank_rows=0),
           "pack: a first_row of -1": pack(first=(-1, 0, 0)), "pack: a first_row at bank_rows": pack(first=(0, 8, 0)),
           "pack: a misaligned bank of one member": pack(banks=hole(banks, 2, banks[2] + 8)),
           "state: pool, a member on another stream": pool(handle=mixed._g, lists=two(lists), colpred=two(colpred), pers=two(pers), prev=two(prev), bits=two(bits),
                                                           banks=two(banks), first=(0, 1)),
           "state: pack, a member on another stream": pack(handle=mixed._g, lists=two(lists), banks=two(banks), first=(0, 1))}
    if is_ahead:
        bad["state: pool, a member that is ahead"] = pool(handle=ahead_models._g, lists=two(lists), colpred=two(colpred), pers=two(pers), prev=two(prev), bits=two(bits),
                                                          banks=two(banks), first=(0, 1))
        bad["state: pack, a member that is ahead"] = pack(handle=ahead_models._g, lists=two(lists), banks=two(banks), first=(0, 1))
    good = {"pool: one window of scratch for all members": pool(scratch_bytes=n * window), "pool: no rows": pool(n_rows=0),
            "pool: the largest parameters": pool(lk=link(active_weight=255, predicted_weight=255, decay=255, ceiling=255, union_bits=C0)),
            "pool: no reset bits": pool(bits=None), "pool: reset bits of one member only": pool(bits=[bits[0], None, None]),
            "pool: a scratch of two windows and a byte less than a third": pool(scratch_bytes=3 * n * window - 1),
            "pool: the last first_rows": pool(first=(7, 7, 7)), "pack: one call": pack(), "pack: no rows": pack(n_rows=0), "pack: the last first_rows": pack(first=(7, 7, 7))}
    out, codes = {}, {}
    out["refused"] = traced(lambda: codes.update({name: c() for name, c in bad.items()}))
    out["codes"] = codes
    accepted = {}
    out["accepted_trace"] = {}
    for name, c in good.items():
        out["accepted_trace"][name] = traced(lambda: accepted.update({name: c()}))
    out["accepted"] = accepted
    stack.run(np.stack([pd.BANK] * n), 8)           # ... and the group goes on
    return out


def main():
    if sys.argv[1] == "before":
        print(json.dumps(before()))
        return
    out = {"before": before(), "stacks": {}}
    for n in (1, 3, 7):
        out["stacks"][f"plain B={n}"] = stack_patterns(lambda b: B.GroupStack(b, I, [(C0, 8), (C1, 8)], strides=[2]), n)
        out["stacks"][f"pooled B={n}"] = stack_patterns(lambda b: B.GroupStack(b, I, [(C0, 8), (C1, 8)], links=[B.PoolingLink(stride=2)]), n)
    out["python"] = python_refusals()
    out.update(refusals())
    print(json.dumps(out))


if __name__ == "__main__":
    main()
