"""Live ticks of model groups (ModelGroup.tick / ModelGroup.reset; htm_live_tick, htm_live_reset) -- what holds without a GPU:
the C ABI's declarations, binding and result-row layout, the refusals of the C calls and of the Python layer, the compiler's
report for the new kernels, the launches and copies a tick makes (the host code built host-only against
tests/host_stub/hip_stub_runtime.cpp, as tests/test_launch_trace_cpu.py builds it), and the host code under ASan + UBSan as a
stand-alone program (tests/host_stub/live_tick_host.cpp)."""
import ctypes as C
import json
import os
import re
import subprocess
import sys

import numpy as np
import pytest

from live_tick_cases import MID, SMALL, derived, edge_values, encoded_rows, decoded, encoder_for

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CLANG_DIR = "/opt/rocm/lib/llvm"
HEADER = os.path.join(ROOT, "include", "bithtm_hip.h")
needs_hipcc = pytest.mark.skipif(not os.path.exists("/opt/rocm/bin/hipcc"), reason="needs hipcc")


# ---- the C ABI
def _declarations():
    header = open(HEADER).read()
    return {m.group(1): m.group(2) for m in re.finditer(r"\b(htm_live_[a-z_]+)\s*\(([^)]*)\)\s*;", header)}


def test_the_header_declares_the_live_abi_and_the_binding_matches_it():
    from bithtm_amd import _lib as L
    decl = _declarations()
    assert set(decl) == {"htm_live_tick", "htm_live_reset"}
    for name, params in decl.items():
        assert params.split(",")[0].strip() == "htm_group *g", (name, params)
        assert len(L.EXPORTS[name][1]) == len(params.split(",")), name
        assert L.EXPORTS[name][0] is C.c_int
    assert L.ABI_VERSION == 4


def test_the_result_row_is_48_bytes_and_its_mirror_matches_the_header():
    """htm_live_row: the eight htm_step_record counters, an int64 step index, the int32 flags and padding to a multiple of 8 --
    the ctypes mirror against the header's text and, where a compiler is there, against sizeof / offsetof."""
    from bithtm_amd import _lib as L
    from bithtm_amd.engine import RECORD_COUNTERS
    row = L.HtmLiveRow
    assert C.sizeof(row) == 48 and C.sizeof(row) % 8 == 0
    assert [n for n, _ in row._fields_[:8]] == list(RECORD_COUNTERS)
    assert (row.step_index.offset, row.step_index.size) == (32, 8)
    assert (row.capacity_error.offset, row.capacity_error.size) == (40, 4)
    body = re.search(r"typedef struct htm_live_row \{(.*?)\} htm_live_row;", open(HEADER).read(), re.S).group(1)
    assert [re.sub(r"\s+", " ", x.strip()) for x in body.split(";") if x.strip()] == [
        "htm_step_record record", "int64_t step_index", "int32_t capacity_error", "int32_t reserved"]
    dtype = np.dtype(row)
    assert dtype.itemsize == 48 and dtype.fields["step_index"][1] == 32
    clang = os.path.join(CLANG_DIR, "bin", "clang")
    if os.path.exists(clang):
        src = ('#include <stddef.h>\n#include "%s"\n_Static_assert(sizeof(htm_live_row) == 48, "size");\n'
               '_Static_assert(offsetof(htm_live_row, step_index) == 32 && offsetof(htm_live_row, capacity_error) == 40, "layout");\n'
               '_Static_assert(sizeof(htm_step_record) == 32, "record");\n' % HEADER)
        r = subprocess.run([clang, "-x", "c", "-fsyntax-only", "-"], input=src, capture_output=True, text=True)
        assert r.returncode == 0, r.stderr


def test_the_c_calls_refuse_null_arguments_without_a_gpu():
    from bithtm_amd import _lib as L
    lib = L.load()
    rows = (L.HtmLiveRow * 2)()
    x = (C.c_uint32 * 8)()
    assert lib.htm_live_tick(None, None, None, 0, x, None, 1, 1, rows, None, None) == -1
    assert lib.htm_live_tick(None, None, None, 0, None, None, 1, 1, None, None, None) == -1
    assert lib.htm_live_reset(None, None) == -1
    assert lib.htm_live_reset(None, (C.c_uint8 * 2)(1, 1)) == -1


# ---- the Python layer's refusals (before anything reaches the library)
class _Engine:
    """What ModelGroup.tick reads of a member's engine before its first library call."""

    def __init__(self, size):
        self.input_dim, self.column_dim, self.cell_dim, self.active_columns = size
        self.steps, self._live_states = 0, []


def _shell(size, B, views=False):
    """A ModelGroup of B members without a library behind it: enough for the argument checks, which come first."""
    import bithtm_amd as Bm
    from bithtm_amd.group import ModelGroup
    group = ModelGroup.__new__(ModelGroup)
    kind = Bm.InferenceView if views else Bm.HierarchicalTemporalMemory
    group.models = []
    for _ in range(B):
        m = kind.__new__(kind)
        m._engine = _Engine(size)
        group.models.append(m)
    group._g = None
    group._auto_grow = False
    return group


def test_python_refusals_come_before_any_library_call():
    group = _shell(MID, 3)
    assert group.models[0].engine.input_dim == MID[0]
    enc = encoder_for(MID)
    with pytest.raises(ValueError, match=r"values: float64 \[3, 2\]"):
        group.tick(np.zeros((3, 3)), encoder=enc)
    with pytest.raises(ValueError, match=r"values: float64 \[3, 2\]"):
        group.tick(np.zeros((2, 2)), encoder=enc)
    with pytest.raises(ValueError, match=r"values: bool \[3, 300\]"):
        group.tick(np.zeros((3, 299), bool))
    with pytest.raises(ValueError, match=r"values: bool \[3, 300\]"):
        group.tick(np.zeros((1, 3, 300), bool))
    with pytest.raises(ValueError, match=r"resets: bool \[3\]"):
        group.tick(np.zeros((3, 2)), encoder=enc, resets=np.zeros(4, bool))
    with pytest.raises(ValueError, match=r"resets: bool \[3\]"):
        group.tick(np.zeros((3, 300), bool), resets=np.zeros((3, 1), bool))
    with pytest.raises(ValueError, match=r"members: bool \[3\]"):
        group.reset(np.zeros(2, bool))
    with pytest.raises(ValueError, match="input_dim"):
        group.tick(np.zeros((3, 1)), encoder=encoder_for(SMALL))
    with pytest.raises(ValueError, match="learning=False only"):
        _shell(MID, 2, views=True).tick(np.zeros((2, 2)), encoder=enc, learning=True)


def test_group_tick_is_a_run_record_with_the_same_formulas():
    """GroupTick from result rows: the counters by name, RunRecord's derived properties, value_of with NaN for 'nothing'."""
    import bithtm_amd as Bm
    from bithtm_amd import _lib as L
    from bithtm_amd.engine import RECORD_COUNTERS
    rows = np.zeros(3, dtype=L.HtmLiveRow)
    rng = np.random.RandomState(0)
    for name in RECORD_COUNTERS:
        rows[name] = rng.randint(0, 40, 3)
    rows["active_columns"] = [48, 0, 48]
    rows["bursting_columns"] = [48, 0, 5]
    rows["step_index"] = [7, 2 ** 31 + 5, 9]
    rows["capacity_error"] = [0, 3, 0]
    enc = encoder_for(MID)
    pairs = np.array([[[4, 9], [-1, 0]], [[-1, 0], [32, 2]], [[259, 1], [0, 1]]], dtype=np.int32)
    tick = Bm.GroupTick(rows, pairs, None, enc)
    assert isinstance(tick, Bm.RunRecord) and len(tick) == 3
    assert tick.step_index.dtype == np.int64 and tick.step_index.tolist() == [7, 2 ** 31 + 5, 9]
    assert tick.capacity_error.dtype == np.int32 and tick.capacity_error.tolist() == [0, 3, 0]
    for name in RECORD_COUNTERS:
        assert getattr(tick, name).dtype == np.int32 and np.array_equal(getattr(tick, name), rows[name])
    correct, incorrect, score = derived(rows["active_columns"], rows["bursting_columns"], rows["predicted_columns_before"])
    assert np.array_equal(tick.correct_columns, correct) and np.array_equal(tick.incorrect_columns, incorrect)
    assert np.array_equal(tick.anomaly_score, score) and score.tolist() == [1.0, 0.0, 1.0 - 43 / 48]
    assert np.array_equal(tick.predicted_bucket, pairs[:, :, 0]) and np.array_equal(tick.predicted_score, pairs[:, :, 1])
    assert np.array_equal(np.isnan(tick.predicted_value), pairs[:, :, 0] < 0)
    assert np.array_equal(tick.predicted_value, enc.value_of(pairs[:, :, 0]), equal_nan=True)
    assert tick.predicted_input is None and Bm.GroupTick(rows).predicted_value is None


def test_the_cases_edge_values_cover_the_definition():
    """The case table's edge values reach every branch of the definition: missing values, both end buckets, wrapping windows --
    and decode(encode(v)) gives v's bucket back wherever a value is present."""
    for size, layout in ((MID, "default"), (SMALL, "default"), (MID, "sixteen")):
        enc = encoder_for(size, layout)
        v = edge_values(enc)
        b = enc.bucket(v)
        rows = encoded_rows(enc, v)
        assert rows.shape == (len(v), size[0]) and not rows[:, enc.offsets[-1] + enc.fields[-1].bits:].any()
        for j, f in enumerate(enc.fields):
            assert (b[:, j] == -1).any() and (b[:, j] == 0).any() and (b[:, j] == f.buckets - 1).any() or f.periodic
            assert np.array_equal(rows[:, enc.offsets[j]:enc.offsets[j] + f.bits].sum(axis=1), np.where(b[:, j] >= 0, f.width, 0))
        bucket, score, value = decoded(enc, rows.astype(np.int32))
        assert np.array_equal(bucket, b) and np.array_equal(np.isnan(value), b < 0)
    enc = encoder_for(MID)
    assert (enc.fields[0].bits, enc.fields[0].width, enc.fields[0].periodic, enc.offsets[1], enc.fields[1].bits) == (260, 21, True, 260, 37)
    wrap = encoded_rows(enc, np.array([[23.9, 0.0]]))[0, :260]
    assert wrap[0] and wrap[259]                    # (a window that wraps round the periodic field's end)


# ---- the compiler's report
def test_the_new_kernels_have_no_scratch_and_the_masked_reset_keeps_its_waves():
    from bithtm_amd.build import kernel_resources
    res = kernel_resources()
    if res is None:
        pytest.skip("the library in the tree was not built here")
    new = {k: v for k, v in res.items() if re.match(r"_Z\d+klive_", k)}
    assert len(new) == 2 and any("klive_reset" in k for k in new) and any("klive_finish" in k for k in new), sorted(new)
    for name, r in new.items():
        assert r["scratch_bytes_per_lane"] == 0, (name, r)
    solo_names = {re.match(r"_Z\d+(k_[a-z_]+)", k).group(1) for k in res if re.match(r"_Z\d+k_", k)}
    grp_names = {re.match(r"_Z\d+(kgrp_[a-z_]+)", k).group(1) for k in res if re.match(r"_Z\d+kgrp_", k)}
    for k in new:                                   # (the budget tests find kernels with re.search: no name inside another)
        assert not [s for s in solo_names | grp_names if s in k], k
    reset = [v for k, v in res.items() if re.search(r"klive_reset", k)]
    solo = [v for k, v in res.items() if re.search(r"k_tm_reset", k)]
    assert len(reset) == 1 and len(solo) == 1
    assert reset[0]["occupancy"] >= solo[0]["occupancy"], (reset, solo)
    finish = [v for k, v in res.items() if re.search(r"klive_finish", k)][0]
    decode = [v for k, v in res.items() if re.search(r"k_decode_votes", k)]
    assert len(decode) == 1 and finish["lds_bytes"] == decode[0]["lds_bytes"] and finish["occupancy"] >= decode[0]["occupancy"]


# ---- the launch trace
def _host_objects(tmp, extra=()):
    """htm_engine.hip host-only and the stub runtime, as tests/test_launch_trace_cpu.py builds them (`extra`: further flags for
    both) -> (engine object, stub object, the --defsym the link needs for the device image the host object expects)."""
    hipcc = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
    clang = os.path.join(CLANG_DIR, "bin", "clang++")
    flags = ["-std=c++17", "-O1", "-g", "-fPIC", "-fno-omit-frame-pointer"] + list(extra)
    obj, stub = (os.path.join(tmp, n) for n in ("engine_host.o", "hip_stub.o"))
    subprocess.run([hipcc, "--offload-host-only", "-ffp-contract=off", "-w"] + flags + ["-c", os.path.join(ROOT, "bithtm_amd", "csrc", "htm_engine.hip"), "-o", obj],
                   check=True, capture_output=True)
    subprocess.run([clang, "-D__HIP_PLATFORM_AMD__", "-I/opt/rocm/include", "-w"] + flags + ["-c", os.path.join(ROOT, "tests", "host_stub", "hip_stub_runtime.cpp"), "-o", stub],
                   check=True, capture_output=True)
    undefined = subprocess.run(["nm", "-u", obj], check=True, capture_output=True, text=True).stdout
    fatbin = re.search(r"__hip_fatbin_\w+", undefined)       # (the device image the host object expects beside it: there is none)
    return obj, stub, ([f"-Wl,--defsym={fatbin.group(0)}=0"] if fatbin else [])


@pytest.fixture(scope="module")
def traces(tmp_path_factory):
    tmp = str(tmp_path_factory.mktemp("live_tick_trace"))
    obj, stub, defsym = _host_objects(tmp)
    lib = os.path.join(tmp, "libbithtm_host_trace.so")
    subprocess.run([os.path.join(CLANG_DIR, "bin", "clang++"), "-shared", obj, stub, "-ldl", "-o", lib] + defsym, check=True, capture_output=True)
    env = dict(os.environ, BITHTM_LIBRARY=lib, BITHTM_STUB_TRACE=os.path.join(tmp, "trace.txt"))
    for name in ("LD_PRELOAD", "BITHTM_LEAN", "BITHTM_SCAN_LARGE"):
        env.pop(name, None)
    r = subprocess.run([sys.executable, os.path.join(ROOT, "tests", "host_stub", "live_tick_driver.py")], env=env, capture_output=True, text=True,
                       timeout=600)
    assert r.returncode == 0, (r.stdout + r.stderr)[-4000:]
    return json.loads(r.stdout.splitlines()[-1])


def _kernel(line):
    m = re.match(r"launch _Z(\d+)", line)
    return line[m.end():m.end() + int(m.group(1))] if m else None


# the two launches of a tick whose member index is grid x, not y: one block per descriptor (kgrp_rec_clear, as the group's recorded
# calls launch it) and one block per bank row (k_bank_encode, as it is)
MEMBER_IN_X = {"kgrp_rec_clear", "k_bank_encode"}


def _shape(lines):
    """The trace without what may depend on B: kernel names (with grid x, block and LDS) and the kind of every other line."""
    out = []
    for line in lines:
        m = re.match(r"launch (\S+) grid (\d+) (\d+) block (\d+) lds (\d+)", line)
        name = _kernel(line)
        out.append((name, "B" if name in MEMBER_IN_X else m.group(2), m.group(4), m.group(5)) if m else line.split()[0])
    return out


def _grid_y(lines):
    return {_kernel(line): int(re.match(r"launch \S+ grid \d+ (\d+)", line).group(1)) for line in lines if line.startswith("launch ")}


VARIANTS = [(e, r) for e in (0, 1) for r in (0, 1)]


@needs_hipcc
@pytest.mark.parametrize("enc,resets", VARIANTS)
def test_a_tick_makes_the_same_launches_and_two_copies_whatever_b_is(traces, enc, resets):
    one, seven = (traces["tick"][f"B={n} enc={enc} resets={resets}"] for n in (1, 7))
    assert _shape(one) == _shape(seven), (one, seven)
    for n, lines in ((1, one), (7, seven)):
        assert [line.split()[0] for line in lines if not line.startswith("launch ")] == ["memcpy", "memcpy"], lines
        assert lines[0].startswith("memcpy ") and lines[-1].startswith("memcpy "), lines        # (in first, out last)
        gy = _grid_y(lines)
        solo = MEMBER_IN_X
        assert all(y == n for k, y in gy.items() if k not in solo) and len(gy) >= 8, gy
        for line in lines:
            if _kernel(line) in solo:
                assert re.match(r"launch \S+ grid (\d+) 1 ", line).group(1) == str(n), line
    kernels = [_kernel(x) for x in seven if x.startswith("launch ")]
    assert ("klive_reset" in kernels) == bool(resets) and ("k_bank_encode" in kernels) == bool(enc)
    assert kernels[-1] == "klive_finish" and kernels.count("klive_finish") == 1
    if resets:
        assert kernels[0] == "klive_reset" and kernels.index("klive_reset") < kernels.index("kgrp_rec_begin")
    # against a recorded, decoding htm_group_step of the same group: at most three launches more
    step = [_kernel(x) for x in traces["step"]["B=7"] if x.startswith("launch ")]
    assert "kgrp_rec_step" in step and "kgrp_pin_step" in step
    assert len(kernels) <= len(step) + 3, (kernels, step)
    extra = [k for k in kernels if k not in step]
    assert set(extra) <= {"klive_reset", "k_bank_encode", "klive_finish"}, extra
    # the byte counts: the copy in carries the rows or the values with the flags, the copy out the rows and the pairs
    I, words_per_row = MID[0], 12
    for n, lines in ((1, one), (7, seven)):
        copy_in, copy_out = (int(lines[i].split()[1]) for i in (0, -1))
        if enc:
            assert n * 2 * 8 + n * 4 <= copy_in <= n * 2 * 8 + n * 4 + 8 and copy_out == n * 48 + n * 2 * 8
        else:
            assert copy_in == n * words_per_row * 4 + n * 4 and copy_out == n * 48
    assert I == 300


@needs_hipcc
def test_a_group_reset_is_one_launch_over_the_members(traces):
    for n in (1, 7):
        lines = traces["reset"][f"B={n}"]
        launches = [x for x in lines if x.startswith("launch ")]
        assert len(launches) == 1 and _kernel(launches[0]) == "klive_reset", lines
        assert _grid_y(launches) == {"klive_reset": n}
        assert [x for x in lines if not x.startswith("launch ")] == [f"memcpy {4 * n}"], lines
    assert _shape(traces["reset"]["B=1"]) == _shape(traces["reset"]["B=7"])


@needs_hipcc
def test_graph_ticks_replay_cached_graphs_with_the_copies_outside(traces):
    """From the third tick on (one graph per step parity) nothing is captured: a tick is its copy in, the eager launches around
    the step, one graph launch, the finish launch and the copy out."""
    for lines in traces["graph"]:
        kinds = [_kernel(x) or x.split()[0] for x in lines]
        assert "capture" not in kinds and kinds.count("graph_launch") == 1 and kinds.count("memcpy") == 2, lines
        assert kinds[0] == "memcpy" and kinds[-1] == "memcpy" and kinds[-2] == "klive_finish", kinds
        assert kinds.index("k_bank_encode") < kinds.index("graph_launch") < kinds.index("klive_finish")
        assert not [k for k in kinds if k and k.startswith("kgrp_") and k not in ("kgrp_rec_clear", "kgrp_rec_begin", "kgrp_pin_begin")], kinds


# ---- the host code under ASan + UBSan, as a stand-alone program
@needs_hipcc
def test_the_host_code_of_the_live_calls_runs_clean_under_asan_and_ubsan(tmp_path):
    """tests/host_stub/live_tick_host.cpp and htm_engine.hip (host-only), both with -fsanitize=address,undefined, linked against the
    stub runtime into ONE program that is run directly: nothing is preloaded."""
    tmp = str(tmp_path)
    san = ["-fsanitize=address,undefined", "-fno-sanitize-recover=undefined"]
    obj, stub, defsym = _host_objects(tmp, san)
    clang = os.path.join(CLANG_DIR, "bin", "clang++")
    exe = os.path.join(tmp, "live_tick_host")
    subprocess.run([clang, "-std=c++17", "-O1", "-g", "-fno-omit-frame-pointer"] + san +
                   [os.path.join(ROOT, "tests", "host_stub", "live_tick_host.cpp"), obj, stub, "-ldl", "-o", exe] + defsym, check=True, capture_output=True)
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=0", UBSAN_OPTIONS="print_stacktrace=1")
    for name in ("LD_PRELOAD", "BITHTM_STUB_TRACE", "BITHTM_LIBRARY"):
        env.pop(name, None)
    r = subprocess.run([exe], env=env, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0 and r.stdout.strip().endswith("ok"), (r.stdout + r.stderr)[-6000:]
    assert "runtime error" not in r.stderr and "AddressSanitizer" not in r.stderr, r.stderr[-6000:]
