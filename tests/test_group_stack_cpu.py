"""No GPU: stacks of model groups (bithtm_amd.GroupStack, htm_group_pack_columns, htm_group_pool_columns).
The header's text and the binding, every group case of tests/group_stack_cases.py on the paths its members name, the compiler's
report for the three new kernels beside every earlier report, the launch traces of GroupStack.run and the refusals of both entries
and of the Python layer (the host code built host-only against tests/host_stub/hip_stub_runtime.cpp), what the commit before
launched (tests/golden/group_stack_traces_before.json), and the host code under ASan + UBSan as a stand-alone program
(tests/host_stub/group_stack_host.cpp)."""
import json
import os
import re
import subprocess
import sys

import numpy as np
import pytest

import group_stack_cases as gc
import pooling_cases as pc

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "bithtm_hip.h")
CLANG_DIR = "/opt/rocm/lib/llvm"
needs_hipcc = pytest.mark.skipif(not os.path.exists("/opt/rocm/bin/hipcc"), reason="needs hipcc")
GROUPS = gc.groups()


# ---- the cases
@pytest.mark.parametrize("g", GROUPS, ids=[g.name for g in GROUPS])
def test_every_member_reaches_the_path_it_names(g):
    for c, r in zip(g.members, gc.replay(g)):
        assert c.reaches(c, r), c.name
        assert len(r.snapshots) == c.windows
    assert len(g.members) >= 2


def test_the_group_cases_cover_the_list():
    by_name = {g.name: g for g in GROUPS}
    assert sorted(by_name) == sorted(["a short row beside a full one", "a tie at the cut across a trip boundary beside none", "a bad id in one member only",
                                      "reset bits for one member and NULL for another", "different first_rows", "three batches"])
    bad = [r.bad for r in gc.replay(by_name["a bad id in one member only"])]
    assert bad == [False, True, False] and [r.bad for r in gc.replay_pack(by_name["a bad id in one member only"])] == bad
    resets = [c.resets is None for c in by_name["reset bits for one member and NULL for another"].members]
    assert resets == [False, True]
    assert len({c.first_row for c in by_name["different first_rows"].members}) == 3
    three = by_name["three batches"]
    assert three.batch_windows == 3 and three.windows == 9 and len(three.members) == 3
    rows = [np.unpackbits(r.bank.view(np.uint8), axis=1, bitorder="little").sum(axis=1) for r in gc.replay(by_name["a short row beside a full one"])]
    assert rows[0].min() < 290 and rows[1].max() == 290


# ---- the C ABI
def test_header_text_and_the_binding():
    import ctypes
    from bithtm_amd import _lib
    header = open(HEADER).read()
    assert re.search(r"#define BITHTM_ABI_VERSION\s+4\b", header) and _lib.ABI_VERSION == 4
    clean = lambda args: [re.sub(r"\s+", " ", a).strip() for a in args.split(",")]
    bare = re.sub(r"/\*.*?\*/", "", header, flags=re.S)
    pack = re.search(r"\bint htm_group_pack_columns\s*\(([^;]*)\)\s*;", bare, re.S).group(1)
    assert clean(pack) == ["htm_group *dst", "const int32_t *const *device_lists", "int32_t k", "int32_t n_rows", "int32_t stride", "uint32_t *const *device_banks",
                           "int32_t bank_rows", "const int32_t *first_rows"]
    pool = re.search(r"\bint htm_group_pool_columns\s*\(([^;]*)\)\s*;", bare, re.S).group(1)
    assert clean(pool) == ["htm_group *dst", "htm_pool_link link", "const int32_t *const *device_lists", "int32_t k", "const uint32_t *const *device_column_prediction",
                           "int32_t n_rows", "uint8_t *const *device_persistence", "uint32_t *const *device_prev", "const uint32_t *const *device_reset_bits",
                           "void *device_scratch", "int64_t scratch_bytes", "uint32_t *const *device_banks", "int32_t bank_rows", "const int32_t *first_rows"]
    comment = header[header.index("Stacks of model groups (DESIGN.md section 30)"):header.index("int htm_group_pack_columns")]
    for text in ("exactly that of htm_pack_columns", "HOST arrays", "read before the call returns", "ONE table per call", "go by", "no wait", "ONE launch",
                 "three launches whatever B is", "floor(scratch_bytes / (B * (stride + 8) * 4 * words_per_row))", "bit 64", "no other member's", "HTM_ERR_ARGUMENT",
                 "NULL entry", "outside [0, bank_rows)", "too small for one window of all members", "65535 members", "HTM_ERR_STATE", "another stream"):
        assert text in comment, text
    for name, n in (("htm_group_pack_columns", 8), ("htm_group_pool_columns", 14)):
        assert name in _lib.EXPORTS and len(_lib.EXPORTS[name][1]) == n and _lib.EXPORTS[name][0] is ctypes.c_int
    assert _lib.EXPORTS["htm_group_pool_columns"][1][1] is _lib.HtmPoolLink and _lib.EXPORTS["htm_group_pool_columns"][1][10] is ctypes.c_int64
    lib = _lib.load()
    buf = ctypes.create_string_buffer(64)
    p = ctypes.cast(buf, ctypes.c_void_p)
    link = _lib.HtmPoolLink(32, 1, 1, 8, 1, 16, 4, 0)
    assert lib.htm_group_pack_columns(None, p, 1, 1, 1, p, 1, p) == -1             # a NULL group needs no device
    assert lib.htm_group_pool_columns(None, link, p, 1, p, 1, p, p, None, p, 4096, p, 1, p) == -1
    import bithtm_amd
    assert bithtm_amd.GroupStack.__module__ == "bithtm_amd.group_stack"


# ---- the compiler's report
def test_the_new_kernels_report_and_every_earlier_report():
    from bithtm_amd import build
    new, pool, old = build.kernel_resources("htm_group_stack.h"), build.kernel_resources("htm_pool.h"), build.kernel_resources()
    if new is None or pool is None or old is None:
        pytest.skip("the library in the tree was not built here")
    assert list(build.GROUP_STACK_REPORTS) == ["htm_group_stack.h"] and list(build.POOL_REPORTS) == ["htm_pool.h"]
    names = {re.match(r"_Z\d+(kg[a-z]+_[a-z_]+?)PK", k).group(1): v for k, v in new.items()}
    assert sorted(names) == ["kgpool_scan", "kgpool_select", "kgrp_pack_columns"] and len(new) == 3, sorted(new)
    solo = {"kgpool_scan": [v for k, v in pool.items() if "kpool_scan" in k], "kgpool_select": [v for k, v in pool.items() if "kpool_select" in k],
            "kgrp_pack_columns": [v for k, v in old.items() if re.match(r"_Z\d+k_pack_columns", k)]}
    for name, r in names.items():
        assert len(solo[name]) == 1
        twin = solo[name][0]
        print(name, r, "solo:", twin)
        assert r["scratch_bytes_per_lane"] == 0, name                               # no private segment
        assert r["occupancy"] >= twin["occupancy"], name
        assert r["lds_bytes"] == twin["lds_bytes"], name
    # every earlier report function returns what it returned: none of them holds a new kernel, the pooling report holds its two
    whole, coord = build.whole_library_kernel_resources(), build.kernel_resources("htm_coord.h")
    assert not set(new) & (set(whole) | set(coord) | set(pool)) and len(pool) == 2 and len(coord) == 3
    with open(os.path.join(ROOT, "tests", "golden", "kernel_resources_before_likelihood.json")) as f:
        before = json.load(f)
    changed = {k: (before[k], old.get(k)) for k in before if before[k] != old.get(k)}
    assert not changed, changed


# ---- the launch traces and the refusals
@pytest.fixture(scope="module")
def traces(tmp_path_factory):
    from test_launch_trace_cpu import _build
    tmp = str(tmp_path_factory.mktemp("group_stack_trace"))
    env = dict(os.environ, BITHTM_LIBRARY=_build(tmp), BITHTM_STUB_TRACE=os.path.join(tmp, "trace.txt"))
    for name in ("LD_PRELOAD", "BITHTM_LEAN", "BITHTM_SCAN_LARGE", "BITHTM_STACK_CHUNK"):
        env.pop(name, None)
    r = subprocess.run([sys.executable, os.path.join(ROOT, "tests", "host_stub", "group_stack_driver.py"), "all"], env=env, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, (r.stdout + r.stderr)[-4000:]
    return json.loads(r.stdout.splitlines()[-1])


def _kernel(line):
    m = re.match(r"launch _Z(\d+)", line)
    return line[m.end():m.end() + int(m.group(1))] if m else None


def _chunks(lines):
    """The trace lines of each chunk of a GroupStack.run trace (between the driver's "py chunk" and "py end")."""
    out, cur = [], None
    for x in lines:
        if x == "py chunk":
            assert cur is None
            cur = []
        elif x == "py end":
            out.append(cur)
            cur = None
        elif cur is not None:
            cur.append(x)
    assert cur is None
    return out


LINK_KERNELS = {"plain": ["kgrp_pack_columns"], "pooled": ["kgrp_pack_columns", "kgpool_scan", "kgpool_select"]}


@needs_hipcc
def test_what_the_parent_launched_is_launched_still(traces):
    with open(os.path.join(ROOT, "tests", "golden", "group_stack_traces_before.json")) as f:
        before = json.load(f)
    assert sorted(before) == ["group", "plain", "pooled"] and len(before["plain"]) == len(before["pooled"]) == 10 and len(before["group"]) == 3
    for part in before:
        for name in before[part]:
            assert traces["before"][part][name] == before[part][name], (part, name)
    solo = [_kernel(x) for part in before.values() for t in part.values() for x in t]
    assert "k_pack_columns" in solo and "kpool_select" in solo and not [k for k in solo if k and k.startswith(("kgrp_pack", "kgpool"))]


@needs_hipcc
@pytest.mark.parametrize("kind", ["plain", "pooled"])
def test_a_chunk_launches_the_same_kernels_at_every_B(traces, kind):
    """Per pattern: the kernel-name sequence of every chunk is the same at B = 1, 3 and 7 and only grid y differs; one link call
    per chunk with one table copy in front of its launches; no host wait inside a chunk."""
    stacks = traces["stacks"]
    assert sorted(stacks) == sorted(f"{k} B={n}" for k in ("plain", "pooled") for n in (1, 3, 7))
    for pattern in ("first run", "second run", "recorded run", "run in chunks", "eager run"):
        per_B = {n: _chunks(stacks[f"{kind} B={n}"][pattern]) for n in (1, 3, 7)}
        assert len(per_B[1]) == (3 if pattern == "run in chunks" else 1), pattern
        for n, chunks in per_B.items():
            assert len(chunks) == len(per_B[1])
            for i, chunk in enumerate(chunks):
                assert "py sync" not in chunk, (pattern, n)                         # no synchronisation, no read-back inside a chunk
                launches = [x for x in chunk if x.startswith("launch")]
                assert [_kernel(x) for x in launches] == [_kernel(x) for x in per_B[1][i] if x.startswith("launch")], (pattern, n)
                grids = [re.search(r"grid (\d+) (\d+) block (\d+) lds (\d+)$", x).groups() for x in launches]
                ones = [re.search(r"grid (\d+) (\d+) block (\d+) lds (\d+)$", x).groups() for x in per_B[1][i] if x.startswith("launch")]
                # (kgrp_rec_clear, the older one-wave launch in front of a recorded group run, has its members on x)
                clear = [_kernel(x) == "kgrp_rec_clear" for x in launches]
                assert [(a, c, d) for (a, _, c, d), skip in zip(grids, clear) if not skip] == [(a, c, d) for (a, _, c, d), skip in zip(ones, clear) if not skip], (pattern, n)
                assert {int(y) for (_, y, _, _), skip in zip(grids, clear) if not skip} == {n}, (pattern, n)      # every launch of a chunk covers all members
                assert {(x, y) for (x, y, _, _), skip in zip(grids, clear) if skip} <= {(str(n), "1")}
                assert [x for x in chunk if x == "graph_launch"] == [x for x in per_B[1][i] if x == "graph_launch"]
                # the link: its launches in order, once, directly behind ONE copy of n table rows
                ours = [j for j, x in enumerate(chunk) if _kernel(x) in LINK_KERNELS["pooled"]]
                assert [_kernel(chunk[j]) for j in ours] == LINK_KERNELS[kind] and ours == list(range(ours[0], ours[0] + len(ours))), (pattern, n)
                row_bytes = 24 if kind == "plain" else 24 + 104                   # GrpPackRow; with a PoolDev in front of it
                assert chunk[ours[0] - 1] == f"memcpy {n * row_bytes}", (pattern, n, chunk[ours[0] - 1])
                assert sum(x == f"memcpy {n * row_bytes}" for x in chunk) == 1
        # 512 lower columns: 16 words; windows of 2 steps
        windows = {"first run": 20, "second run": 20}.get(pattern, 4)
        chunk = per_B[3][0]
        first = [j for j, x in enumerate(chunk) if _kernel(x) == "kgrp_pack_columns"][0]
        if kind == "plain":
            assert re.search(rf"grid {windows} 3 block 256 lds 64$", chunk[first])
        else:
            pack, scan, select = chunk[first:first + 3]
            assert re.search(rf"grid {2 * windows} 3 block 256 lds 64$", pack) and re.search(r"grid 2 3 block 256 lds 0$", scan)
            assert re.search(rf"grid {windows} 3 block 256 lds 64$", select)


@needs_hipcc
def test_the_second_chunk_of_one_length_captures_no_graph(traces):
    for name, patterns in traces["stacks"].items():
        chunks = _chunks(patterns["run in chunks"])
        assert "capture" not in chunks[1] + chunks[2], name
        assert "capture" not in _chunks(patterns["second run"])[0], name
        assert "capture" in _chunks(patterns["first run"])[0], name
        assert not [x for x in _chunks(patterns["eager run"])[0] if x in ("capture", "graph_launch")], name


@needs_hipcc
def test_every_refusal_of_the_entries_enqueues_nothing(traces):
    codes = traces["codes"]
    assert len(codes) >= 47, sorted(codes)
    assert {k: v for k, v in codes.items() if v != (-4 if k.startswith("state:") else -1)} == {}
    # (a member that is ahead cannot be had here: htm_group_create refuses one, and a member of a group plans no run that leaves it
    # ahead; the entries' check of it is the one every group call makes)
    assert {"state: pool, a member on another stream", "state: pack, a member on another stream"} <= set(codes)
    assert traces["refused"] == []
    assert set(traces["accepted"].values()) == {0} and len(traces["accepted"]) == 10
    shapes = {name: [_kernel(x) or x for x in lines] for name, lines in traces["accepted_trace"].items()}
    three = ["kgrp_pack_columns", "kgpool_scan", "kgpool_select"]
    assert shapes["pool: no rows"] == [] and shapes["pack: no rows"] == []
    assert shapes["pool: one window of scratch for all members"] == ["memcpy 384"] + three * 4      # one table, a batch per window
    assert shapes["pool: a scratch of two windows and a byte less than a third"] == ["memcpy 384"] + three * 2
    assert shapes["pool: reset bits of one member only"] == ["memcpy 384"] + three and shapes["pool: no reset bits"] == ["memcpy 384"] + three
    assert shapes["pack: one call"] == ["memcpy 72", "kgrp_pack_columns"]


@needs_hipcc
def test_the_python_layer_refuses_before_any_library_call(traces):
    got = traces["python"]["refusals"]
    assert traces["python"]["trace"] == []
    assert len(got) == 14 and not [k for k, v in got.items() if v == "accepted"]
    assert got["resets="].startswith("NotImplementedError: sequence resets inside a group run are not available yet")
    for name, text in (("inputs of two dimensions", "inputs: bool [2, n_inputs, 100]"), ("another member count", "inputs: bool [2, n_inputs, 100]"),
                       ("another input_dim", "inputs: bool"), ("no rows", "inputs: bool"), ("steps that are no multiple", "multiples of 2"),
                       ("negative steps", "multiples of 2"), ("learning=True on views", "learning=False only"),
                       ("process: learning=True on views", "learning=False only"), ("process: another shape", "X: bool [2, 100]"),
                       ("a run in the middle of a window", "multiples of 2"), ("a reset in the middle of a window", "middle of a window")):
        assert got[name].startswith("ValueError") and text in got[name], (name, got[name])


def test_the_constructors_refuse_before_anything_touches_a_device(monkeypatch):
    import bithtm_amd.group_stack as module
    from bithtm_amd import GroupStack, PoolingLink

    def touched(*a, **kw):
        raise AssertionError("a refusal came after the stack reached for a device")
    monkeypatch.setattr(module, "SharedStream", touched)
    monkeypatch.setattr(module, "HierarchicalTemporalMemory", touched)
    levels = [(256, 4, 10), (64, 4)]
    for args, kw, match in (((0, 100, levels), {}, "streams"), ((2, 100, levels), dict(seeds=[1]), "seeds"), ((2, 100, levels), dict(strides=[1], links=[1]), "not both"),
                            ((2, 100, levels), dict(links=[0]), "strides"), ((2, 100, levels), dict(links=[PoolingLink(union_bits=257)]), "link 0.*union_bits"),
                            ((2, 0, levels), {}, "input_dim"), ((2, 100, [(256, 65)]), {}, "cell_dim"), ((2, 100, []), {}, "levels")):
        with pytest.raises(ValueError, match=match):
            GroupStack(*args, **kw)
    with pytest.raises(AssertionError):             # (a good shape goes on to the device)
        GroupStack(2, 100, levels, links=[PoolingLink(union_bits=256)])
    with pytest.raises(ValueError, match="at least one"):
        GroupStack.of([])
    with pytest.raises(ValueError, match="not a RegionStack"):
        GroupStack.of([object()])
    with pytest.raises(ValueError, match="a RegionStack"):
        GroupStack.views(object(), 2)


# ---- the host code under ASan + UBSan, as a stand-alone program
@needs_hipcc
def test_the_host_code_runs_clean_under_asan_and_ubsan(tmp_path):
    """tests/host_stub/group_stack_host.cpp and htm_engine.hip (host-only), both with -fsanitize=address,undefined, linked against
    the stub runtime into ONE program that is run directly: nothing is preloaded."""
    from test_likelihood_cpu import _host_objects
    tmp = str(tmp_path)
    san = ["-fsanitize=address,undefined", "-fno-sanitize-recover=undefined"]
    obj, stub, defsym = _host_objects(tmp, san)
    clang = os.path.join(CLANG_DIR, "bin", "clang++")
    exe = os.path.join(tmp, "group_stack_host")
    subprocess.run([clang, "-std=c++17", "-O1", "-g", "-fno-omit-frame-pointer", "-ffp-contract=off"] + san +
                   [os.path.join(ROOT, "tests", "host_stub", "group_stack_host.cpp"), obj, stub, "-ldl", "-o", exe] + defsym, check=True, capture_output=True)
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=0", UBSAN_OPTIONS="print_stacktrace=1")
    for name in ("LD_PRELOAD", "BITHTM_STUB_TRACE", "BITHTM_LIBRARY"):
        env.pop(name, None)
    r = subprocess.run([exe], env=env, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0 and r.stdout.strip().endswith("ok"), (r.stdout + r.stderr)[-6000:]
    assert "runtime error" not in r.stderr and "AddressSanitizer" not in r.stderr, r.stderr[-6000:]
