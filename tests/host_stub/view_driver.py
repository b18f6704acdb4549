"""Driver of the sanitizer build for inference views (tests/test_inference_view_cpu.py runs it as test_host_sanitizers.py runs
driver.py): a parent and three views over a HIP runtime made of host memory, a group of the views, every refusal, and the
parent destroyed before its views -- the reference counting of the shared weights and the aliasing of the views' descriptors,
which a device run cannot report."""
import ctypes as C
import gc
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
import bithtm_amd as B  # noqa: E402
from bithtm_amd import _lib as L  # noqa: E402
from bithtm_amd.engine import HtmError  # noqa: E402


def refused(fn, exc=HtmError):
    try:
        fn()
    except exc:
        return True
    return False


def main():
    os.environ["BITHTM_SHARED_SCAN"] = "1"           # (the views' groups take the shared scan)
    lib = L.load()
    rng = np.random.RandomState(3)
    for K in (8, 40):
        I, Cn = 100, 512
        parent = B.HierarchicalTemporalMemory(I, Cn, K, seed=K)
        bank = rng.rand(6, I) < 0.1
        for x in bank:
            parent.process(x)
        views = [parent.inference_view() for _ in range(3)]
        pe = parent.engine
        assert all(v.engine.device_bytes() < pe.device_bytes() for v in views)
        for v in views:
            v.process(bank[0])
            v.run(bank, 5)
            v.run(bank, 3, record=("counters", "active_column", "column_prediction", "predicted_input"), resets=np.eye(6, dtype=bool)[0])
            v.reset()
            v.predicted_input()
            v.temporal_memory.last_state.cell_prediction
        parent.process(bank[1])                      # the parent learns between view calls
        parent.run(bank, 4)
        # groups (the stub runtime launches grids of one member only: a group of three is created and refuses, one of one runs)
        group = B.ModelGroup(views)
        assert refused(lambda: group.run(np.stack([bank] * 3), 1, learning=True), ValueError)
        assert lib.htm_group_step(group._g, np.zeros((3, 4), np.uint32).ctypes.data_as(C.c_void_p), 1, None) == -4
        mixed = B.ModelGroup([parent] + views[:2])
        assert refused(lambda: mixed.process(np.stack([bank[0]] * 3), learning=True), ValueError)
        del mixed
        one = B.ModelGroup(views[1:2])
        one.run(bank[None], 4)
        one.run(bank[None], 2, record=("counters", "predicted_input"))
        one.process(bank[2][None])
        # refusals on a view, nothing enqueued
        v = views[0]
        h = v.engine.h
        assert refused(lambda: v.process(bank[0], learning=True), ValueError)
        assert refused(v.state_dict, ValueError) and refused(v.inference_view, ValueError) and refused(v.grow_pool, ValueError)
        assert lib.htm_step(h, np.zeros(4, np.uint32).ctypes.data_as(C.c_void_p), 1) == -4
        assert lib.htm_run(h, C.c_void_p(v.engine.upload_bank(bank)), 6, 2, 1, 1) == -4
        assert lib.htm_write(h, L.F_SEG_NSYN, np.zeros(4, np.int32).ctypes.data_as(C.c_void_p), 4) == -4
        assert lib.htm_write(h, L.F_SEG_PERM, np.zeros(4, np.float32).ctypes.data_as(C.c_void_p), 4) == -4
        assert lib.htm_sp_set_permanence(h, np.zeros((1, I)).ctypes.data_as(C.c_void_p), 0, 1) == -4
        assert lib.htm_populate(h, 0, 8, 1, 8, 0.3, 0.7, 1) == -4
        assert lib.htm_import_begin(h, 0) == -4
        assert lib.htm_sp_phase(h, L.SP_LEARN, None, 0) == -4
        out = C.c_void_p()
        assert lib.htm_create_view(h, C.byref(out)) == -4 and out.value is None
        assert lib.htm_create_view(None, C.byref(out)) == -1 and lib.htm_device_bytes(None) == -1
        # a parent that is ahead refuses its views' calls
        parent.run(bank, 3, continuing=True)
        assert refused(lambda: v.process(bank[0]))
        assert refused(lambda: group.process(np.stack([bank[0]] * 3)))
        parent.run(bank, 1)
        v.process(bank[0])
        # the parent first, then the group, then the views one by one: each keeps the weights alive
        del parent, pe
        gc.collect()
        for v in views:
            v.process(bank[3])
        one.run(bank[None], 2)
        del group, one
        for i in range(len(views)):
            views.pop().process(bank[4]) if views else None
            gc.collect()
    # a view of a model whose pool grew: refused from then on
    parent = B.HierarchicalTemporalMemory(100, 512, 8)
    parent.process(rng.rand(100) < 0.1)
    v = parent.inference_view()
    parent.grow_pool()
    assert refused(lambda: v.process(rng.rand(100) < 0.1), ValueError)
    del v, parent
    gc.collect()
    print("view sanitizer driver: ok")


if __name__ == "__main__":
    main()
