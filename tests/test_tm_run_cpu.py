"""CPU: the host side of batched stand-alone Temporal Memory runs (TemporalMemory.run, Engine.upload_lists, htm_tm_run): the
check of the lists that is made once per bank, the refusals that need no device, and the C declaration against the binding."""

import ctypes as C
import os
import re

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def built():
    import __graft_entry__ as ge
    ge.build()


def test_check_lists_range_distinctness_and_shape(built):
    from bithtm_amd.engine import check_lists
    good = np.array([[5, 0, 999], [7, 8, 9]], dtype=np.int64)
    out = check_lists(good, 1000)
    assert out.dtype == np.int32 and out.flags.c_contiguous and np.array_equal(out, good)      # (the caller's order is kept)
    assert np.array_equal(check_lists(good.tolist(), 1000), good)
    assert np.array_equal(check_lists(good[:, ::-1], 1000), good[:, ::-1].copy())               # (any strides)
    for bad, what in (([[5, 0, 1000], [7, 8, 9]], r"row 0 has a column id outside \[0, 1000\)"),
                      ([[5, 0, 9], [7, -1, 9]], r"row 1 has a column id outside"),
                      ([[5, 0, 9], [7, 9, 9]], "row 1 lists a column twice"),
                      ([[3, 3, 3]], "row 0 lists a column twice"),
                      ([5, 0, 9], "n_rows, n"),
                      (np.zeros((0, 3), np.int32), "n_rows, n"),
                      (np.zeros((3, 0), np.int32), "n_rows, n"),
                      (np.zeros((2, 2, 2), np.int32), "n_rows, n"),
                      ([[0.5, 1.0]], "integer column ids"),
                      ([[True, False]], "integer column ids")):
        with pytest.raises(ValueError, match=what):
            check_lists(bad, 1000)
    with pytest.raises(ValueError, match="only 3 columns"):
        check_lists([[0, 1, 2, 3]], 3)
    assert check_lists([[2, 0, 1]], 3).shape == (1, 3)                                         # (every column: allowed)


def test_run_refuses_on_the_host_before_any_engine_exists(built):
    import bithtm_amd as B
    lists = np.array([[1, 2, 3], [4, 5, 6]])
    tm = B.TemporalMemory(64, 4)
    for kw, what in ((dict(active_columns=[[1, 2, 64]]), "outside"), (dict(active_columns=[[1, 2, 2]]), "twice"),
                     (dict(record=("predicted_input",)), "no proximal mask"), (dict(record=("counters", "predicted_input")), "no proximal mask"),
                     (dict(record=("nonsense",)), "record"), (dict(resets=[True]), "one flag per row"), (dict(steps=-1), "negative")):
        with pytest.raises(ValueError, match=what):
            tm.run(**{**dict(active_columns=lists, steps=4), **kw})
    assert tm._engine is None                                   # nothing was created, let alone enqueued
    with pytest.raises(ValueError, match="cell_dim above 64"):
        B.TemporalMemory(64, 65).run(lists, 4)

    class Projection(B.PredictiveProjection):
        pass
    with pytest.raises(ValueError, match="plug-in distal_projection"):
        B.TemporalMemory(64, 4, distal_projection=Projection(64 * 4)).run(lists, 4)


C_TYPES = {"htm_handle *": C.c_void_p, "const int32_t *": C.c_void_p, "int32_t": C.c_int32}


def test_header_declares_htm_tm_run_as_the_binding_calls_it(built):
    from bithtm_amd import _lib
    header = open(os.path.join(ROOT, "include", "bithtm_hip.h")).read()
    m = re.search(r"^int htm_tm_run\(([^)]*)\);", header, flags=re.M)
    assert m, "include/bithtm_hip.h does not declare htm_tm_run"
    params = [re.sub(r"\s+", " ", p.strip()) for p in m.group(1).split(",")]
    names = [re.search(r"(\w+)$", p).group(1) for p in params]
    types = [p[:-len(n)].strip() for p, n in zip(params, names)]
    assert names == ["h", "device_lists", "n_rows", "n", "n_steps", "learning", "use_graph", "rec"]
    want = [C.POINTER(_lib.HtmRunRecord) if t == "const htm_run_record *" else C_TYPES[t] for t in types]
    restype, argtypes = _lib.EXPORTS["htm_tm_run"]
    assert restype is C.c_int and argtypes == want
    lib = _lib.load()
    assert lib.htm_tm_run.argtypes == want
    assert lib.htm_tm_run(None, None, 1, 1, 1, 1, 1, None) == -1           # a NULL handle: HTM_ERR_ARGUMENT, nothing touched
    assert "128 = htm_tm_run" in header and _lib.ABI_VERSION == 4
