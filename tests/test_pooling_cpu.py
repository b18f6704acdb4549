"""No GPU: pooling links of region stacks (bithtm_amd/pooling.py, htm_pool_columns).  The definition on a
stream worked by hand, every case of tests/pooling_cases.py on the path it names, the two degenerate settings against the plain
link's NumPy statement, the refusals of PoolingLink and of links=, the header's text and the exported symbol, the compiler's
report for the new kernels, the launch traces of plain and pooled stacks (the host code built host-only against
tests/host_stub/hip_stub_runtime.cpp), the host code under ASan + UBSan as a stand-alone program (tests/host_stub/pool_host.cpp),
the recorded chained reference (tests/golden/stack_pooled.npz) replayed with chained oracles, and the model-level property."""
import json
import os
import re
import subprocess
import sys

import numpy as np
import pytest

import pooling_cases as pc
import stack_fixture as sf
from bithtm_amd.pooling import PoolingLink, PoolingState

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "bithtm_hip.h")
CLANG_DIR = "/opt/rocm/lib/llvm"
needs_hipcc = pytest.mark.skipif(not os.path.exists("/opt/rocm/bin/hipcc"), reason="needs hipcc")
CASES = pc.cases()


# ---- the definition
def test_a_stream_computed_by_hand():
    """Six columns, active_weight 1, predicted_weight 3, decay 1, ceiling 4, union_bits 2."""
    s = PoolingState(PoolingLink(1, active_weight=1, predicted_weight=3, decay=1, ceiling=4, union_bits=2), 6)
    pred = lambda *cols: np.isin(np.arange(6), cols)
    s.step([0, 1], pred(1, 2))                      # nothing was predicted: 1 each
    assert s.persistence.tolist() == [1, 1, 0, 0, 0, 0] and s.row().tolist() == [True, True, False, False, False, False]
    s.step([1, 2], pred(2))                         # decay, then 1 and 2 were predicted: 0 + 3
    assert s.persistence.tolist() == [0, 3, 3, 0, 0, 0] and s.row().tolist() == [False, True, True, False, False, False]
    s.step([2, 5], pred())                          # 2: 2 + 3 -> the ceiling; 5 was not predicted: 1; ties 1 < 5 do not matter yet
    assert s.persistence.tolist() == [0, 2, 4, 0, 0, 1] and s.row().tolist() == [False, True, True, False, False, False]
    s.step([0, 3], pred(0))                         # 1: 1, 2: 3, 5: 0; 0 and 3: 1 each -- the cut falls among 0, 1, 3: the lowest index wins
    assert s.persistence.tolist() == [1, 1, 3, 1, 0, 0] and s.row().tolist() == [True, False, True, False, False, False]
    s.step([0], pred())                             # 0: 0 + 3; the rest decays to 0 but column 2
    assert s.persistence.tolist() == [3, 0, 2, 0, 0, 0] and s.prev.tolist() == [False] * 6
    s.step([], pred())
    s.step([], pred())
    assert s.persistence.tolist() == [1, 0, 0, 0, 0, 0] and s.row().sum() == 1         # fewer positive columns than union_bits: a short row
    s.step([], pred(4))
    assert not s.row().any() and s.prev.tolist() == [False, False, False, False, True, False]
    s.step([4, 9, -1], pred())                      # (ids outside the range count for nothing)
    assert s.persistence.tolist() == [0, 0, 0, 0, 3, 0]
    s.reset()
    assert not s.persistence.any() and not s.prev.any()


@pytest.mark.parametrize("c", CASES, ids=[c.name for c in CASES])
def test_every_case_reaches_the_path_it_names(c):
    r = pc.replay(c)
    assert c.reaches(c, r)
    assert len(r.snapshots) == c.windows == sum(c.calls) and c.lists.shape == (c.windows * c.link.stride, c.k)
    written = {(c.first_row + i) % c.bank_rows for i in range(c.windows)}
    rest = sorted(set(range(c.bank_rows)) - written)
    assert np.array_equal(r.bank[rest], r.before[rest])
    rows = sf.unpack_rows(r.bank, pc.bank_words(c.C) * 32)
    assert not rows[sorted(written), c.C:].any() and (rows[sorted(written)].sum(axis=1) <= c.link.union_bits).all()


def test_the_cases_cover_the_list():
    names = {c.name for c in CASES}
    for name in ("one partial word", "two scan blocks", "the select's later trips", "the bench shape", "ceiling reached and held", "decay >= ceiling: the plain link",
                 "active_weight 0", "predicted_weight 0", "union_bits 1", "union_bits C", "a short row", "ties inside one word", "ties across a word boundary",
                 "ties across a thread's boundary", "ties across a trip's boundary", "ties across a scan block boundary", "a reset at window 0",
                 "a reset at a middle window", "first_row != 0 with bank_rows > n_rows", "three batches, two calls", "an id outside the range"):
        assert name in names, name
    shapes = {(c.C, c.k, c.link.stride, c.windows) for c in CASES}
    assert {(37, 5, 1, 4), (257, 16, 3, 5), (8192 + 37, 64, 2, 3), (65536, 1311, 1, 8)} <= shapes
    kernel = open(os.path.join(ROOT, "bithtm_amd", "csrc", "htm_pool.h")).read()
    assert "#define POOL_THREADS 256" in kernel and "#define POOL_TRIP (POOL_THREADS * 16)" in kernel        # (the geometry the cases aim at)
    assert (pc.SCAN_BLOCK, pc.THREAD, pc.TRIP) == (256, 16, 4096)


def test_the_degenerate_settings_against_the_plain_link():
    """decay >= ceiling with equal weights, union_bits >= k and stride 1: the plain link's row, bit for bit.  active_weight 0:
    only columns that were predicted when they became active."""
    c = next(c for c in CASES if c.name == "decay >= ceiling: the plain link")
    r = pc.replay(c)
    plain = r.before.copy()
    assert not sf.pack_columns(c.lists, c.C, 1, plain, c.first_row)
    assert np.array_equal(r.bank, plain)
    fx = sf.load()
    lists = fx["s1_l0_lists"][:40].astype(np.int64)
    C, k = int(fx["column_dim"][0]), int(fx["active_columns"][0])
    for union_bits, decay, ceiling, w in ((k, 16, 16, 1), (C, 255, 3, 255), (k + 5, 7, 7, 7)):
        link = PoolingLink(1, active_weight=w, predicted_weight=w, decay=decay, ceiling=ceiling, union_bits=union_bits)
        bank, plain = np.zeros((40, C // 32), np.uint32), np.ones((40, C // 32), np.uint32)
        rng = np.random.RandomState(union_bits)
        pc.pool_columns(link, C, lists, rng.rand(40, C) < 0.3, np.zeros(C, np.uint8), np.zeros(C, bool), None, bank, 0)
        sf.pack_columns(lists, C, 1, plain, 0)
        assert np.array_equal(bank, plain)
    c = next(c for c in CASES if c.name == "active_weight 0")
    state = PoolingState(c.link, c.C)
    ever = np.zeros(c.C, bool)
    for s in range(len(c.lists)):
        ever[c.lists[s][state.prev[c.lists[s]]]] = True
        state.step(c.lists[s], c.colpred[s])
        assert not state.persistence[~ever].any()
    assert ever.any() and state.persistence.any()


# ---- refusals
@pytest.mark.parametrize("kw", [dict(stride=0), dict(stride=-1), dict(stride=1.0), dict(active_weight=-1), dict(active_weight=256), dict(predicted_weight=-1),
                                dict(predicted_weight=256), dict(active_weight=0, predicted_weight=0), dict(decay=0), dict(decay=256), dict(ceiling=0),
                                dict(ceiling=256), dict(union_bits=0), dict(union_bits=-4), dict(union_bits="8"), dict(decay=True), dict(ceiling=None)])
def test_pooling_link_refuses(kw):
    with pytest.raises(ValueError, match="PoolingLink"):
        PoolingLink(**kw)


def test_pooling_link_limits_and_the_default_union_bits():
    PoolingLink(1, 0, 255, 255, 255, 1), PoolingLink(10 ** 6, 255, 0, 1, 1, 10 ** 9)
    assert PoolingLink().resolved(1024, 64).union_bits == 128 and PoolingLink().resolved(100, 64).union_bits == 100
    assert PoolingLink(union_bits=100).resolved(100, 2).union_bits == 100
    with pytest.raises(ValueError, match="union_bits"):
        PoolingLink(union_bits=101).resolved(100, 2)
    assert PoolingLink(2) == PoolingLink(2, 1, 8, 1, 16) and PoolingLink(2) != PoolingLink(3) and PoolingLink(2) != 2
    with pytest.raises(ValueError, match="resolved"):
        PoolingState(PoolingLink(), 8)


def test_links_refusals_come_before_anything_touches_a_device(monkeypatch):
    import bithtm_amd.stack as stack_module
    from bithtm_amd import RegionStack

    def touched(*a, **kw):
        raise AssertionError("a refusal came after the stack reached for a device")
    monkeypatch.setattr(stack_module, "SharedStream", touched)
    monkeypatch.setattr(stack_module, "HierarchicalTemporalMemory", touched)
    levels = [(256, 4, 10), (64, 4)]
    for kw, match in ((dict(strides=[1], links=[1]), "not both"), (dict(links=[]), "links"), (dict(links=[1, 2]), "links"), (dict(links=[0]), "strides"),
                      (dict(links=[1.5]), "links"), (dict(links=["1"]), "links"), (dict(links=[True]), "links"), (dict(links=[None]), "links"),
                      (dict(links=[PoolingLink(union_bits=257)]), "link 0.*union_bits"), (dict(strides=[0]), "strides")):
        with pytest.raises(ValueError, match=match):
            RegionStack(100, levels, **kw)
    with pytest.raises(ValueError, match="link 1.*union_bits"):
        RegionStack(100, [(256, 4), (64, 4), (32, 4)], links=[PoolingLink(), PoolingLink(union_bits=65)])
    with pytest.raises(AssertionError):             # (a good link goes on to the device)
        RegionStack(100, levels, links=[PoolingLink(union_bits=256)])


# ---- the C ABI
def test_header_text_and_the_exported_symbol():
    from bithtm_amd import _lib
    header = open(HEADER).read()
    assert re.search(r"#define BITHTM_ABI_VERSION\s+4\b", header) and _lib.ABI_VERSION == 4
    assert re.search(r"int htm_pool_columns\(htm_handle \*dst, htm_pool_link link, const int32_t \*device_lists, int32_t k, const uint32_t \*device_column_prediction,\s*"
                     r"int32_t n_rows, uint8_t \*device_persistence, uint32_t \*device_prev, const uint32_t \*device_reset_bits,\s*"
                     r"void \*device_scratch, int64_t scratch_bytes, uint32_t \*device_bank, int32_t bank_rows, int32_t first_row\);", header)
    comment = header[header.index("Pooling links (DESIGN.md sections 14 and 29"):header.index("#define HTM_POOL_MAX_COLUMNS")]
    for text in ("bithtm_amd/pooling.py", "max(P - decay, 0)", "predicted_weight : active_weight", "to the lower column index", "np.lexsort((arange(C), -P))[:union_bits]",
                 "(first_row + r) % bank_rows", "htm_set_run_resets", "exactly as htm_pack_columns", "(stride + 8) * 4 * words_per_row", "no copy, no wait, no allocation",
                 "bit 64", "keep their contents", "struct_bytes", "both 0", "outside [1, 255]", "outside [1, C]", "16-byte aligned", "too small for one window",
                 "HTM_ERR_STATE"):
        assert text in comment, text
    assert "#define HTM_POOL_MAX_COLUMNS 262144" in header and _lib.POOL_MAX_COLUMNS == 262144 >= 65536
    fields = re.search(r"typedef struct htm_pool_link \{(.*?)\} htm_pool_link;", header, re.S).group(1)
    names = re.findall(r"(\w+)(?:,|;)", re.sub(r"/\*.*?\*/", "", fields))
    assert names == [n for n, _ in _lib.HtmPoolLink._fields_] and PoolingLink.PARAMETERS == tuple(names[1:-1])
    import ctypes
    assert ctypes.sizeof(_lib.HtmPoolLink) == 32
    assert "htm_pool_columns" in _lib.EXPORTS
    lib = _lib.load()
    assert lib.htm_pool_columns is not None
    buf = ctypes.create_string_buffer(64)
    p = ctypes.cast(buf, ctypes.c_void_p)
    link = _lib.HtmPoolLink(32, 1, 1, 8, 1, 16, 4, 0)
    assert lib.htm_pool_columns(None, link, p, 1, p, 1, p, p, None, p, 4096, p, 1, 0) == -1        # a NULL handle needs no device


# ---- the compiler's report
def test_the_new_kernels_have_no_scratch_and_the_older_reports_are_unchanged():
    from bithtm_amd import build
    new, old, whole, coord = build.kernel_resources("htm_pool.h"), build.kernel_resources(), build.whole_library_kernel_resources(), build.kernel_resources("htm_coord.h")
    if new is None or old is None:
        pytest.skip("the library in the tree was not built here")
    assert list(build.POOL_REPORTS) == ["htm_pool.h"] and list(build.COORD_REPORTS) == ["htm_coord.h"]
    names = {re.match(r"_Z\d+(kpool_[a-z]+)", k).group(1): v for k, v in new.items()}
    assert sorted(names) == ["kpool_scan", "kpool_select"] and len(new) == 2, sorted(new)
    pack = [v for k, v in old.items() if re.match(r"_Z\d+k_pack_columns", k)]
    assert len(pack) == 1                           # (the first of the three launches is the plain link's kernel, as it is)
    for name, r in list(names.items()) + [("k_pack_columns", pack[0])]:
        print(name, r)
        assert r["scratch_bytes_per_lane"] == 0 and r["occupancy"] >= 1, (name, r)
    assert names["kpool_scan"]["lds_bytes"] == 0
    # the select's static LDS (a histogram per wave, the scan's and the select's words) and the largest row bitmap launch without
    # asking for more than a launch gets
    assert 4 * 256 * 4 <= names["kpool_select"]["lds_bytes"] <= 4 * 256 * 4 + 64
    from bithtm_amd import _lib
    assert names["kpool_select"]["lds_bytes"] + _lib.POOL_MAX_COLUMNS // 8 <= 64 * 1024
    assert not set(new) & set(whole) and not set(new) & set(coord) and len(coord) == 3
    older = {re.match(r"_Z\d+(k[a-z]*_[a-z_0-9]+)", k).group(1) for k in list(whole) + list(coord) if re.match(r"_Z\d+k[a-z]*_", k)}
    for name in names:                              # (the budget tests find kernels with re.search: no name inside another)
        assert not [s for s in older if s in name or name in s], name
    with open(os.path.join(ROOT, "tests", "golden", "kernel_resources_before_likelihood.json")) as f:
        before = json.load(f)
    changed = {k: (before[k], old.get(k)) for k in before if before[k] != old.get(k)}
    assert not changed, changed


# ---- the launch traces and the refusals
@pytest.fixture(scope="module")
def traces(tmp_path_factory):
    from test_launch_trace_cpu import _build
    tmp = str(tmp_path_factory.mktemp("pool_trace"))
    env = dict(os.environ, BITHTM_LIBRARY=_build(tmp), BITHTM_STUB_TRACE=os.path.join(tmp, "trace.txt"))
    for name in ("LD_PRELOAD", "BITHTM_LEAN", "BITHTM_SCAN_LARGE", "BITHTM_STACK_CHUNK"):
        env.pop(name, None)
    r = subprocess.run([sys.executable, os.path.join(ROOT, "tests", "host_stub", "pool_driver.py"), "all"], env=env, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, (r.stdout + r.stderr)[-4000:]
    return json.loads(r.stdout.splitlines()[-1])


def _kernel(line):
    m = re.match(r"launch _Z(\d+)", line)
    return line[m.end():m.end() + int(m.group(1))] if m else None


@needs_hipcc
def test_a_plain_stack_launches_what_it_launched_before(traces):
    with open(os.path.join(ROOT, "tests", "golden", "stack_traces_before.json")) as f:
        before = json.load(f)
    assert sorted(traces["plain"]) == sorted(before) and len(before) == 10
    for name in before:
        assert traces["plain"][name] == before[name], name
    assert not [x for lines in traces["plain"].values() for x in lines if (_kernel(x) or "").startswith("kpool_")]


@needs_hipcc
def test_a_pooled_link_launches_pack_scan_and_select_where_the_plain_one_launched_pack(traces):
    for name, plain in traces["plain"].items():
        pooled = traces["pooled"][name]
        if name.startswith("process"):
            assert pooled == plain                  # (process() goes through the host: no link launch at all)
            continue
        # the run's own launches follow what the levels record (the lower level of a pooled link records its column prediction
        # too): the links' launches and the graph replays are compared
        ours = ("k_pack_columns", "kpool_scan", "kpool_select")
        a = [_kernel(x) for x in plain if _kernel(x) in ours]
        b = [_kernel(x) for x in pooled if _kernel(x) in ours]
        assert a and set(a) == {"k_pack_columns"} and b == ["k_pack_columns", "kpool_scan", "kpool_select"] * len(a), (name, b)
        assert len(a) == (3 if name.startswith("run in chunks") else 1)
        assert [x for x in plain if x == "graph_launch"] == [x for x in pooled if x == "graph_launch"], name
        assert sum(x.startswith("memcpy") for x in plain) == sum(x.startswith("memcpy") for x in pooled), name        # no copy enqueued by the link
        i = [j for j, x in enumerate(pooled) if _kernel(x) == "k_pack_columns"][0]
        pack, scan, select = pooled[i:i + 3]
        windows, stride, W = (4 if name.startswith(("recorded", "run in chunks")) else 20), 2, 16          # (512 lower columns: 16 words)
        assert re.search(rf"grid {windows * stride} 1 block 256 lds {4 * W}$", pack), pack
        assert re.search(rf"grid {W * 32 // 256} 1 block 256 lds 0$", scan), scan
        assert re.search(rf"grid {windows} 1 block 256 lds {4 * W}$", select), select


@needs_hipcc
def test_every_refusal_enqueues_nothing(traces):
    codes = traces["codes"]
    assert len(codes) >= 32, sorted(codes)
    state = {"a handle without the Spatial Pooler", "a handle that is ahead"}
    assert {k: v for k, v in codes.items() if v != (-4 if k in state else -1)} == {}
    assert traces["refused"] == []
    assert set(traces["accepted"].values()) == {0} and len(traces["accepted"]) == 6
    shapes = {name: [_kernel(x) for x in lines] for name, lines in traces["accepted_trace"].items()}
    assert shapes["no rows"] == [] and shapes["one window of scratch"] == ["k_pack_columns", "kpool_scan", "kpool_select"] * 4
    assert shapes["no reset bits"] == ["k_pack_columns", "kpool_scan", "kpool_select"]


# ---- the host code under ASan + UBSan, as a stand-alone program
@needs_hipcc
def test_the_host_code_runs_clean_under_asan_and_ubsan(tmp_path):
    """tests/host_stub/pool_host.cpp and htm_engine.hip (host-only), both with -fsanitize=address,undefined, linked against the
    stub runtime into ONE program that is run directly: nothing is preloaded."""
    from test_likelihood_cpu import _host_objects
    tmp = str(tmp_path)
    san = ["-fsanitize=address,undefined", "-fno-sanitize-recover=undefined"]
    obj, stub, defsym = _host_objects(tmp, san)
    clang = os.path.join(CLANG_DIR, "bin", "clang++")
    exe = os.path.join(tmp, "pool_host")
    subprocess.run([clang, "-std=c++17", "-O1", "-g", "-fno-omit-frame-pointer", "-ffp-contract=off"] + san +
                   [os.path.join(ROOT, "tests", "host_stub", "pool_host.cpp"), obj, stub, "-ldl", "-o", exe] + defsym, check=True, capture_output=True)
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=0", UBSAN_OPTIONS="print_stacktrace=1")
    for name in ("LD_PRELOAD", "BITHTM_STUB_TRACE", "BITHTM_LIBRARY"):
        env.pop(name, None)
    r = subprocess.run([exe], env=env, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0 and r.stdout.strip().endswith("ok"), (r.stdout + r.stderr)[-6000:]
    assert "runtime error" not in r.stderr and "AddressSanitizer" not in r.stderr, r.stderr[-6000:]


# ---- the recorded chained reference
@pytest.fixture(scope="module")
def fx():
    with np.load(os.path.join(ROOT, "tests", "golden", "stack_pooled.npz")) as z:
        return {k: z[k] for k in z.files}


@pytest.mark.parametrize("stride", [1, 3])
def test_chained_oracles_replay_the_recorded_pooled_stack(fx, stride):
    assert fx["strides"].tolist() == [1, 3] and [int(v) for v in fx["link"]] == [1, 8, 1, 16, 96]
    levels = [(int(C), int(K), int(k)) for C, K, k in zip(fx["column_dim"], fx["cell_dim"], fx["active_columns"])]
    ora = pc.pooled_oracles(int(fx["input_dim"]), levels, [PoolingLink(stride, *[int(v) for v in fx["link"]])], int(fx["seed"]))
    for l, o in enumerate(ora.levels):
        assert sf.refdiff.digest(o.spatial_pooler.permanence) == fx[f"s{stride}_permanence_digest"][l]
    bank = sf.inputs(fx)
    learning, reset = sf.schedule(fx)
    count = [0, 0]
    for t in range(int(fx["steps"])):
        if reset[t]:
            ora.reset()
        for l, st in enumerate(ora.process(bank[t % len(bank)], learning=bool(learning[t]))):
            if st is not None:
                sf.check_step(fx, stride, l, count[l], st[0], st[1], ora.levels[l].temporal_memory.S)
                count[l] += 1
    rows = np.array(ora.upper_inputs)
    assert [sf.refdiff.digest(x) for x in rows] == fx[f"s{stride}_upper_input_digest"].tolist()
    assert rows.sum(axis=1).tolist() == fx[f"s{stride}_upper_input_bits"].tolist() and rows.sum(axis=1).max() == 96
    assert np.array_equal(ora.pool[0].persistence, fx[f"s{stride}_link_persistence"]) and np.array_equal(ora.pool[0].prev, fx[f"s{stride}_link_prev"])
    assert fx[f"s{stride}_l1_predicted"][-(-16 // stride):].mean() > 0.5     # (the upper level learns the pooled rows)


# ---- what the link is for
def test_pooled_rows_stay_put_inside_a_known_sequence_and_differ_between_sequences():
    """The committed stream (pooling_cases.PROPERTY: HTMOracle 300 -> 1024 x 8, k = 64, seed 3; 4 sequences of 8 random patterns of
    density 0.1 from RandomState(7), each shown 30 times in shuffled order with a reset before each; active_weight 1,
    predicted_weight 8, decay 1, ceiling 16, union_bits 160).  Measured in the last epoch over steps 4..7 of each sequence:

        measure                                                     pooled rows    plain active-column rows
        share of a row's bits already in the previous row           0.629          0.031
        mean overlap of two rows of the same sequence, bits         67.9           1.4
        mean overlap of two rows of different sequences, bits       15.5           2.6
        share of a sequence's last row that reappears next time     0.997          (not compared)

    Only the directions are asserted, with margins."""
    f = pc.property_figures()
    print(f)
    assert f["pooled_share"] >= 0.5
    assert f["pooled_same"] >= 2 * f["pooled_different"]
    assert f["plain_share"] < 0.1
