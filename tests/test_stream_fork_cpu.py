"""CPU: stream forks (include/bithtm_hip.h htm_view_sync, htm_bank_rows) -- declared and bound, refusing
NULL without a GPU, the Python surface, the copy kernel's compiler report, and the launches the host code makes for a sync and
for a look-ahead chunk (tests/host_stub/fork_driver.py over the host-only build of tests/test_launch_trace_cpu.py)."""

import ctypes as C
import json
import os
import re
import subprocess
import sys

import numpy as np
import pytest

from test_launch_trace_cpu import _build, needs_hipcc

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FORK_ABI = {"htm_view_sync": 2, "htm_bank_rows": 6}


def test_the_header_declares_the_fork_abi_and_the_binding_matches_it():
    from bithtm_amd import _lib as L
    header = open(os.path.join(ROOT, "include", "bithtm_hip.h")).read()
    for name, n_args in FORK_ABI.items():
        m = re.search(rf"^int {name}\(([^)]*)\);", header, flags=re.M)
        assert m, name
        assert len([p for p in m.group(1).split(",") if p.strip()]) == n_args, name
        restype, argtypes = L.EXPORTS[name]
        assert restype is C.c_int and len(argtypes) == n_args, name
    assert L.EXPORTS["htm_bank_rows"][1][3] is C.c_int64            # (first_step: a step index)
    assert L.ABI_VERSION == 4
    assert "htm_fork.h" in open(os.path.join(ROOT, "bithtm_amd", "csrc", "htm_engine.hip")).read()


def test_fork_calls_refuse_null_without_touching_a_gpu():
    from bithtm_amd import _lib as L
    lib = L.load()
    assert lib.htm_view_sync(None, None) == -1
    assert lib.htm_view_sync(None, C.c_void_p(0)) == -1
    assert lib.htm_bank_rows(None, None, 1, 0, 1, None) == -1


def test_the_python_surface_is_exported():
    import bithtm_amd as B
    from bithtm_amd.engine import Engine
    for cls in (B.HierarchicalTemporalMemory, B.InferenceView):
        assert callable(cls.fork) and callable(cls.lookahead)
    assert callable(B.InferenceView.sync) and callable(Engine.view_sync) and callable(Engine.bank_rows)
    assert B.InferenceView.fork is not B.HierarchicalTemporalMemory.fork
    assert B.HierarchicalTemporalMemory.lookahead_chunk >= 1
    import inspect
    assert inspect.signature(B.ModelGroup.views).parameters["fork"].default is False
    assert inspect.signature(B.InferenceView.lookahead).parameters["learning"].default is False
    assert inspect.signature(B.HierarchicalTemporalMemory.lookahead).parameters["learning"].default is True


def test_argument_errors_need_no_device():
    """lookahead() checks its own arguments before it touches the model's engine."""
    import bithtm_amd as B
    htm = B.HierarchicalTemporalMemory.__new__(B.HierarchicalTemporalMemory)
    for kw in (dict(steps=5, horizon=2, every=2), dict(steps=4, horizon=0), dict(steps=4, horizon=2, every=0), dict(steps=-2, horizon=1, every=2)):
        with pytest.raises(ValueError):
            htm.lookahead(None, **kw)
    with pytest.raises(ValueError):
        B.InferenceView.__new__(B.InferenceView).lookahead(None, 4, 2, learning=True)
    wide = B.HierarchicalTemporalMemory(30, 64, 65)               # (more than 64 cells per column: stepped on the host, no engine)
    for call in (wide.fork, lambda: wide.lookahead(np.zeros((2, 30), bool), 2, 1)):
        with pytest.raises(ValueError):
            call()


def test_the_copy_kernel_has_no_scratch_and_no_lds():
    """k_stream_fork as built: a grid-stride copy out of a table in the kernel's arguments -- no scratch (the table is not
    copied to the stack to be indexed), no LDS, and the 16 VGPRs it had when written (full occupancy)."""
    from bithtm_amd.build import kernel_resources
    res = kernel_resources()
    if res is None:
        pytest.skip("the library in the tree was not built here")
    k = [v for n, v in res.items() if "k_stream_fork" in n]
    assert len(k) == 1, k
    assert k[0]["scratch_bytes_per_lane"] == 0 and k[0]["lds_bytes"] == 0 and k[0]["vgprs"] <= 16 and k[0]["occupancy"] >= 8, k[0]
    rows = [v for n, v in res.items() if "k_bank_rows" in n]
    assert len(rows) == 1 and rows[0]["scratch_bytes_per_lane"] == 0 and rows[0]["lds_bytes"] == 0, rows


@pytest.fixture(scope="module")
def traces(tmp_path_factory):
    tmp = str(tmp_path_factory.mktemp("fork_trace"))
    env = dict(os.environ, BITHTM_LIBRARY=_build(tmp), BITHTM_STUB_TRACE=os.path.join(tmp, "trace.txt"))
    for name in ("LD_PRELOAD", "BITHTM_LEAN", "BITHTM_SCAN_LARGE"):
        env.pop(name, None)
    r = subprocess.run([sys.executable, os.path.join(ROOT, "tests", "host_stub", "fork_driver.py")], env=env, capture_output=True, text=True,
                       timeout=600)
    assert r.returncode == 0, (r.stdout + r.stderr)[-4000:]
    return json.loads(r.stdout.splitlines()[-1])


def _kernels(lines):
    out = []
    for line in lines:
        m = re.match(r"launch _Z(\d+)", line)
        if m:
            out.append(line[m.end():m.end() + int(m.group(1))])
    return out


def _copies(lines):
    return [int(line.split()[1]) for line in lines if line.startswith(("memcpy ", "memset "))]


COUNTER_BLOCK_MAX = 1024                            # (k_stream_fork copies the counter block with one thread per word of its 256)


@needs_hipcc
@pytest.mark.parametrize("which", ["sync", "resync"])
def test_a_sync_is_one_launch_and_no_bulk_copy(traces, which):
    """htm_view_sync, the first and a later one (the parent has learned, the fork has stepped): exactly one kernel launch, no
    graph, and no asynchronous copy or memset larger than the counter block."""
    lines = traces[which]
    assert _kernels(lines) == ["k_stream_fork"], lines
    assert not [line for line in lines if line.startswith(("graph_launch", "capture"))], lines
    assert all(n <= COUNTER_BLOCK_MAX for n in _copies(lines)), lines
    grid = int(re.match(r"launch \S+ grid (\d+) 1 block 256 lds 0", [line for line in lines if line.startswith("launch")][0]).group(1))
    assert 39 <= grid <= 48 * 512                   # (a block group per table entry)


@needs_hipcc
def test_a_synced_view_does_not_take_view_enters_wait(traces):
    """The fork's first step behind a sync that followed the parent's learning: view_enter copies the parent's segment count (4
    bytes) and nothing else before the step's first launch -- no cm_dense_step word from the host, whose copy is waited for."""
    lines = traces["after_sync"]
    first = next(i for i, line in enumerate(lines) if line.startswith("launch"))
    assert lines[:first] == ["memcpy 4"], lines[:first + 1]


@needs_hipcc
def test_a_lookahead_chunk_syncs_once_per_window(traces):
    lines, windows = traces["lookahead"], traces["windows"]
    kernels = _kernels(lines)
    assert kernels.count("k_stream_fork") == windows and kernels.count("k_bank_rows") == windows, kernels
    assert kernels.count("k_encode") >= windows
    # the order inside a window: the model's steps, the sync, the seed row, the fork's steps, the rows
    marks = [k for k in kernels if k in ("k_stream_fork", "k_bank_rows")]
    assert marks == ["k_stream_fork", "k_bank_rows"] * windows, marks
