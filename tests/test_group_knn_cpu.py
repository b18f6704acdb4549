"""KNN classifier banks (bithtm_amd/knn.py's KNNBankDefinition, KNNClassifierBank, htm_knns_*) -- what holds without
a GPU: the bank definition against one KNNDefinition per stream on every case of tests/group_knn_cases.py, the path every case names,
the model group's hit rates on the oracle's states, the C ABI's declarations and binding, the refusals, the compiler's report for the
new kernels, the launches of an update, a group run and a tick with a bank (the host code built host-only against
tests/host_stub/hip_stub_runtime.cpp) beside the unchanged traces of the earlier calls, and the host code under ASan + UBSan as a
stand-alone program (tests/host_stub/group_knn_host.cpp), which also evaluates the bank header's arithmetic on the host."""
import ctypes as C
import json
import os
import re
import subprocess
import sys

import numpy as np
import pytest

import group_knn_cases as cases
import knn_cases as one
from group_knn_cases import CASE_IDS
from knn_cases import CHUNK, QUERIES, SLOTS
from test_likelihood_cpu import CLANG_DIR, HEADER, ROOT, _host_objects, _kernel, _launch, needs_hipcc

ABI = {"htm_knns_create": "htm_handle *h", "htm_knns_labels": "htm_knn *knn", "htm_knns_update": "htm_knn *knn", "htm_knns_reset": "htm_knn *knn",
       "htm_knns_export": "htm_knn *knn", "htm_knns_import": "htm_knn *knn", "htm_knns_info": "const htm_knn *knn", "htm_knns_tick": "htm_group *g"}
NEW_KERNELS = ["kgknn_append", "kgknn_distance_global", "kgknn_distance_lds", "kgknn_place", "kgknn_scatter", "kgknn_select"]


# ---- the definition
@pytest.mark.parametrize("name", CASE_IDS)
def test_the_bank_definition_equals_one_definition_per_stream(name):
    from bithtm_amd.knn import KNNDefinition
    c = cases.case(name)
    want, bank = cases.expected(name)
    p, S = c["params"], c["streams"]
    src = cases.source_definition(c)
    solos = [KNNDefinition(p["labels"], p["k"], p["min_overlap"], p["capacity"], *p["shape"]) for _ in range(S)]
    looked_at = range(S) if S <= 16 else (0, 1, S // 2, S - 1)
    for x, (best, votes) in zip(c["calls"], want):
        assert best.shape == x["index"].shape[:2] + (5,) and votes.shape == x["index"].shape[:2] + (p["labels"],) and best.dtype == votes.dtype == np.int32
        for i in looked_at:
            if src is None:
                b, v = solos[i].update(x["index"][i], x["words"][i], x["labels"][i], x["learning"])
            else:                                   # (a frozen stream over the source's store: every slot is seen)
                rows = [src.infer(list(zip(x["index"][i][t].tolist(), (x["words"][i][t].astype(np.int64) & 0xFFFFFFFF).tolist()))) for t in range(x["index"].shape[1])]
                b, v = np.array([r[0] for r in rows], np.int32), np.array([r[1] for r in rows], np.int32)
            assert np.array_equal(best[i], b) and np.array_equal(votes[i], v), (name, i)
    if src is None:
        for i in looked_at:
            a, b = bank.defs[i].store_arrays(), solos[i].store_arrays()
            assert all(np.array_equal(x, y) for x, y in zip(a, b)) and bank.defs[i].total == solos[i].total == bank.total, (name, i)
    else:
        assert bank.count == [0] * S and bank.total == sum(x["index"].shape[1] for x in c["calls"]) and src.count == cases.SLOTS + 5
        with pytest.raises(ValueError, match="learning is refused"):
            bank.update(c["calls"][0]["index"], c["calls"][0]["words"], None, True)
    if c["refused"] is not None:
        r = c["refused"]
        before = [d.store_arrays() for d in bank.defs], bank.total
        fresh = cases.run_definition(c)[1]          # (the cached definition stays as it is)
        with pytest.raises(ValueError, match="stream 1.*capacity"):
            fresh.update(r["index"], r["words"], r["labels"])
        after = [d.store_arrays() for d in fresh.defs], fresh.total
        assert before[1] == after[1] and all(np.array_equal(x, y) for a, b in zip(before[0], after[0]) for x, y in zip(a, b))


def test_every_case_reaches_the_path_it_names():
    counts = {name: cases.expected(name)[1].count for name in CASE_IDS}
    assert counts["counts-0-1-257"] == [0, 1, SLOTS + 1]
    words = cases.table_words(one.SHAPE)
    assert cases.distance_grid(counts["counts-0-1-257"], 24, words) == (2, 3 * 3)          # (the grid of the largest; stream 0's blocks all leave)
    c = cases.case("mixed-store")
    stored = np.stack([x["labels"][:, 0] >= 0 for x in c["calls"]])
    assert all(x["index"].shape[1] == 1 for x in c["calls"]) and (stored.any(1) & ~stored.all(1)).sum() >= 5 and not stored[:, 3].any()
    c = cases.case("chunk-plus-3")
    assert c["calls"][0]["index"].shape[1] == CHUNK + 3 and cases.chunk_of(2, c["params"]["capacity"], words) == CHUNK
    assert counts["capacity"] == [2, 5, 0] and cases.case("capacity")["params"]["capacity"] == 5
    best = cases.expected("ties")[0][1][0]
    assert best[0, 0].tolist() == [1, 1, 5, 0, 0] and best[1, 0].tolist() == [0, 1, 4, 0, 0] and best[2, 0].tolist()[:4] == [2, 2, 6, 0]
    assert cases.expected("ties")[0][1][1][1, 0].tolist() == [1, 0, 0, 0, 1, 0]            # (slot 1, labelled 4, beats slot 2 at the k-th overlap)
    assert (cases.WPC2_SHAPE[1] + 31) // 32 == 2 and cases.case("wpc2")["params"]["shape"] == cases.WPC2_SHAPE
    g = cases.case("global-table")
    gw = cases.table_words(g["params"]["shape"])
    assert g["params"]["shape"] == (12289, 4, 8) and gw * 4 > cases.TABLE_BYTES and g["streams"] == 2 and counts["global-table"] == [33, 8]
    assert (g["calls"][0]["labels"][1] < 0).all()                                          # (stream 1 asks an empty store at first)
    s = cases.case("small-chunk")
    assert cases.chunk_of(s["streams"], s["params"]["capacity"], words) == 32 < CHUNK and s["calls"][0]["index"].shape[1] == 32 + 3
    assert cases.shared_distance_grid(SLOTS + 5, 9, 1, words) == (2, 2) and 9 % QUERIES == 1
    w2048 = cases.table_words(cases.TABLE_2048_SHAPE)
    assert w2048 == 2048 and cases.queries_of(w2048) == 6 and cases.shared_distance_grid(SLOTS + 5, 7, 2, w2048) == (2, 3)


def test_the_twins_of_the_bank_arithmetic():
    assert cases.chunk_of(3, 64, 256) == 64 and cases.chunk_of(1024, 64, 256) == 32 and cases.chunk_of(65535, 64, 256) == 1 and cases.chunk_of(65536, 64, 256) == 0
    assert cases.chunk_of(3, 1 << 20, 256) == 32 and cases.chunk_of(64, 1 << 20, 256) == 2 and cases.chunk_of(129, 1 << 20, 256) == 0
    assert cases.scratch_bytes(2, 64, 300, 14000) == 2 * 64 * (600 + 56000) and cases.scratch_bytes(2, 64, 300, 256) == 2 * 64 * 600
    assert cases.chunk_of(100, 8, 12289) == 32                                             # (the tables alone: 100 x 64 x 49 156 bytes are past 256 MiB)


def test_the_bank_definition_over_a_call_split_at_every_position_equals_the_one_call():
    """The case the device is held to in tests/test_hip_group_knn.py: chunk-plus-3's learning call of two streams, cut at every position."""
    c = cases.case("chunk-plus-3")
    x = c["calls"][0]
    (want_best, want_votes), _ = cases.expected("chunk-plus-3")[0]
    whole = cases.store_arrays(cases.run_definition(c, [x])[1])
    T = x["index"].shape[1]
    for cut in range(T + 1):
        d = cases.bank_definition(c["params"], c["streams"])
        parts = [d.update(x["index"][:, a:b], x["words"][:, a:b], x["labels"][:, a:b]) for a, b in ((0, cut), (cut, T))]
        assert np.array_equal(np.concatenate([p[0] for p in parts], 1), want_best) and np.array_equal(np.concatenate([p[1] for p in parts], 1), want_votes), cut
        assert d.total == T and all(np.array_equal(a, b) for a, b in zip(cases.store_arrays(d), whole)), cut
    # a frozen call needs no labels
    d = cases.bank_definition(c["params"], c["streams"])
    best, votes = d.update(x["index"][:, :3], x["words"][:, :3], None, learning=False)
    assert (best == [-1, 0, 0, -1, -1]).all() and not votes.any() and d.count == [0, 0] and d.total == 3
    # a definition loads a store as the device objects load a state: the same answers as the one that stepped through it
    stepped = cases.run_definition(c, [x])[1].defs[0]
    loaded = cases.bank_definition(c["params"], 1).defs[0]
    loaded.load_store(*stepped.store_arrays(), stepped.total)
    assert loaded.update(x["index"][1, :5], x["words"][1, :5], [-1], False)[0].tolist() == stepped.update(x["index"][1, :5], x["words"][1, :5], [-1], False)[0].tolist()
    assert all(np.array_equal(a, b) for a, b in zip(loaded.store_arrays(), stepped.store_arrays()))


def test_the_model_groups_hit_rates_over_the_oracles_states():
    best, votes, bank = cases.group_stream()
    assert bank.count == [36] * cases.MEMBERS and bank.total == 72
    rates = tuple(cases.hit_rate(i, best[i, :, 0]) for i in range(cases.MEMBERS))
    assert rates == cases.HIT_RATES, rates
    want, _, d = one.model_stream()                 # (member 0 is the one-stream case's model)
    assert np.array_equal(best[0], want) and d.count == 36


# ---- the C ABI
def test_the_header_declares_the_bank_abi_and_the_binding_matches_it():
    from bithtm_amd import _lib as L
    header = open(HEADER).read()
    decl = {m.group(1): m.group(2) for m in re.finditer(r"\b(htm_knns_[a-z_]+)\s*\(([^)]*)\)\s*;", header)}
    assert set(decl) == set(ABI)
    for name, params in decl.items():
        assert params.split(",")[0].strip() == ABI[name], (name, params)
        assert len(L.EXPORTS[name][1]) == len(params.split(",")), name
        assert L.EXPORTS[name][0] is C.c_int
    assert L.ABI_VERSION == 4 and re.search(r"#define BITHTM_ABI_VERSION 4\b", header)
    clean = lambda text: [re.sub(r"\s+", " ", x.strip()) for x in text.split(",")]
    one_stream = clean(re.search(r"\bhtm_knn_update\s*\(([^)]*)\)\s*;", header).group(1))
    assert clean(decl["htm_knns_update"]) == one_stream[:2] + ["const void *const *device_pairs"] + one_stream[3:]
    classified = clean(re.search(r"\bhtm_classifiers_tick\s*\(([^)]*)\)\s*;", header).group(1))
    assert clean(decl["htm_knns_tick"]) == classified + ["htm_knn *knn", "const int32_t *labels", "int32_t knn_learn", "int32_t *knn_best", "int32_t *knn_votes"]
    assert L.EXPORTS["htm_knns_tick"][1][:-5] == L.EXPORTS["htm_classifiers_tick"][1]
    assert clean(decl["htm_knns_create"]) == ["htm_handle *h", "const htm_knn_config *cfg", "int32_t n_streams", "htm_knn *share_store_of", "htm_knn **out"]
    body = re.sub(r"/\*.*?\*/", "", re.search(r"typedef struct htm_knns_info_t \{(.*?)\} htm_knns_info_t;", header, re.S).group(1), flags=re.S)
    fields = [n.strip() for x in body.split(";") if x.strip() for n in re.sub(r"^\s*\w+\s+", "", x.strip()).split(",")]
    assert fields == [n for n, _ in L.HtmKnnsInfo._fields_] and C.sizeof(L.HtmKnnsInfo) == 96
    kernels = open(os.path.join(ROOT, "bithtm_amd", "csrc", "htm_knn_bank.h")).read()
    assert int(re.search(r"#define HTM_KNNS_SCRATCH_BYTES \((\d+)ll << 20\)", kernels).group(1)) << 20 == L.KNNS_SCRATCH_BYTES
    assert int(re.search(r"#define HTM_KNNS_MAX_STREAMS (\d+)", kernels).group(1)) == L.KNNS_MAX_STREAMS


def test_the_c_calls_refuse_null_arguments_without_a_gpu():
    from bithtm_amd import _lib as L
    lib = L.load()
    cfg = L.HtmKnnConfig(C.sizeof(L.HtmKnnConfig), 3, 1, 1, 16, 64, 32, 4)
    out = C.c_void_p(1)
    assert lib.htm_knns_create(None, C.byref(cfg), 2, None, C.byref(out)) == -1 and not out.value
    assert b"null" in lib.htm_last_error(None)
    assert lib.htm_knns_update(None, None, None, 1, 1, None, 1, 0, 1, None, None) == -1
    assert lib.htm_knns_labels(None, None, None, 1, C.byref(out)) == -1 and lib.htm_knns_reset(None, None, None) == -1
    assert lib.htm_knns_export(None, None, None, 0) == -1 and lib.htm_knns_import(None, None, None, 0) == -1
    assert lib.htm_knns_info(None, None, None) == -1
    assert lib.htm_knns_tick(None, None, None, 0, None, None, 0, 0, None, None, None, None, None, None, None, 0, None, None, None, None, 0, None, None) == -1


def test_the_python_layer_refuses_before_any_library_call():
    import bithtm_amd as B
    for bad in (dict(streams=0, labels=3), dict(streams=65536, labels=3), dict(streams=2, labels=0), dict(streams=2, labels=3, k=65), dict(streams=2, labels=3, capacity=0)):
        with pytest.raises(ValueError):
            B.KNNClassifierBank(**bad)
    with pytest.raises(ValueError, match="shape"):
        B.KNNClassifierBank(2, 3, shape=(10, 65, 4))
    bank = B.KNNClassifierBank(2, 3, k=2, capacity=4, shape=(10, 5, 4))
    assert not isinstance(bank, B.KNNClassifier) and (bank.streams, bank.labels, bank.k, bank.capacity, bank.total, bank.units) == (2, 3, 2, 4, 0, 50)
    assert bank.count.tolist() == [0, 0] and bank.count.dtype == np.int64
    index, words = np.array([[[0, 1, 2, -1]]] * 2), np.array([[[1, 2, 4, 0xFFFFFFFF]]] * 2, dtype=np.uint32)
    for i, w, g, match in ((index[:1], words[:1], [[0]], r"index int \[2, T, n\]"), (index, words, [[0]], r"labels: int \[2, n\]"), (index, words, [[0, 1], [0, 1]], r"int \[2, 1\]"),
                           (np.array([[[0, 1, 1, 3]]] * 2), np.array([[[1, 2, 4, 1]]] * 2, dtype=np.uint32), [[0], [0]], "twice"), (index, np.array([[[1, 2, 32, 0]]] * 2, dtype=np.uint32), [[0], [0]], "cell_dim"),
                           (np.tile(index, (1, 5, 1)), np.tile(words, (1, 5, 1)), [[-1] * 5, [0, 1, 2, 0, 1]], "stream 1.*capacity")):
        with pytest.raises(ValueError, match=match):
            bank.update_patterns(i, w, g)
    assert bank.check_labels([[0, 2], [3, -4]]).tolist() == [[0, 2], [-1, -1]]
    assert bank.stored_by(np.array([[0, -1, 2], [-1, -1, -1]], np.int32), 1, 7, True).tolist() == [4, 0]
    with pytest.raises(RuntimeError, match="not bound"):
        bank.update_patterns(index, words, [[0], [1]])
    with pytest.raises(RuntimeError, match="not bound"):
        bank.info()
    # an unbound bank holds a loaded state until it is bound; reset(streams=) works on it
    state = bank.state_dict()
    assert state["count"].tolist() == [0, 0] and int(state["streams"]) == 2 and state["pairs"].shape == (0, 4, 2)
    state.update(total=np.int64(9), count=np.array([1, 2]), pairs=np.array([[[5, 7], [-1, 0], [-1, 0], [-1, 0]], [[0, 1], [3, 2], [-1, 0], [-1, 0]],
                                                                           [[5, 7], [-1, 0], [-1, 0], [-1, 0]]], np.int32),
                 labels=np.array([1, 2, 0], np.int32), stamps=np.array([8, 3, 8], np.int64))
    bank.load_state_dict(state)
    again = bank.state_dict()
    assert all(np.array_equal(again[k], state[k]) for k in state) and bank.count.tolist() == [1, 2] and bank.total == 9
    mine = bank.stream_state(1)
    assert int(mine["count"]) == 2 and mine["stamps"].tolist() == [3, 8] and mine["labels"].tolist() == [2, 0] and "streams" not in mine
    solo = B.KNNClassifier(3, k=2, capacity=4)
    solo.load_state_dict(mine)                      # (a one-stream object loads a stream's state)
    assert solo.count == 2 and solo.total == 9 and solo.shape == (10, 5, 4)
    bank.reset([True, False])
    assert bank.count.tolist() == [0, 2] and bank.total == 9 and bank.state_dict()["stamps"].tolist() == [3, 8]
    for key, value, match in (("count", np.array([1, 5]), "count"), ("count", np.array([1, 1]), "pairs"), ("labels", np.array([1, 2, 3], np.int32), "label"),
                              ("stamps", np.array([8, 8, 8], np.int64), "stamps"), ("stamps", np.array([9, 3, 8], np.int64), "stamps"), ("streams", np.int64(3), "streams")):
        with pytest.raises(ValueError, match=match):
            bank.load_state_dict(dict(state, **{key: value}))
    # a shared bank needs a bound one-stream object; the calls a bank does not ride on refuse it before anything else
    with pytest.raises(ValueError, match="not bound"):
        B.KNNClassifierBank.shared(solo, 2)
    with pytest.raises(ValueError, match="one-stream KNNClassifier"):
        B.KNNClassifierBank.shared(bank, 2)
    tm, sp = B.TemporalMemory(64, 4), B.SpatialPooler(32, 64, 4)
    for call in (lambda: tm.run(np.zeros((1, 4), int), 1, knn=bank), lambda: sp.run(np.zeros((1, 32), bool), 1, knn=bank)):
        with pytest.raises(ValueError, match="knn= is not available here"):
            call()
    for method, positional in ((B.HierarchicalTemporalMemory.lookahead, 4), (B.HierarchicalTemporalMemory.forecast, 2)):
        with pytest.raises(ValueError, match="knn= is not available here"):
            method(*[None] * positional, knn=bank)
    from bithtm_amd import _lib as L
    rec = B.GroupTick(np.zeros(2, dtype=L.HtmLiveRow), knn=np.array([[3, 2, 17, 5, 40], [-1, 0, 0, -1, -1]], np.int32))
    assert rec.knn_label.tolist() == [3, -1] and rec.knn_nearest_step.tolist() == [40, -1] and rec.knn_votes_all is None


# ---- the compiler's report
def test_the_bank_kernels_have_no_scratch_and_the_earlier_reports_are_unchanged():
    from bithtm_amd.build import BANK_REPORTS, LATER_REPORTS, OWN_REPORTS, every_kernel_resources, kernel_resources, library_kernel_resources
    assert list(BANK_REPORTS) == ["htm_knn_bank.h"] and list(OWN_REPORTS) == ["htm_knn.h"] and list(LATER_REPORTS) == ["htm_handover.h"]
    new, one_stream, every, whole = kernel_resources("htm_knn_bank.h"), kernel_resources("htm_knn.h"), every_kernel_resources(), library_kernel_resources()
    if new is None or every is None:
        pytest.skip("the library in the tree was not built here")
    assert sorted(re.match(r"_Z\d+(kgknn_[a-z_]+?)\d", k).group(1) for k in new) == NEW_KERNELS, sorted(new)
    assert not set(new) & set(every) and set(whole) == set(new) | set(every) and not [k for k in every if "kgknn_" in k]
    for name, r in new.items():
        print(name, r)
        assert r["scratch_bytes_per_lane"] == 0, (name, r)
        body = re.match(r"_Z\d+kg(knn_[a-z_]+?)\d", name).group(1)
        twin = [v for k, v in one_stream.items() if re.match(r"_Z\d+k" + body + r"\d", k)]
        assert len(twin) == 1 and r["lds_bytes"] == twin[0]["lds_bytes"] and r["occupancy"] >= 4, (name, r, twin)      # (a body of the one-stream kernel)
    with open(os.path.join(ROOT, "tests", "golden", "kernel_resources_before_knn.json")) as f:
        assert kernel_resources() == json.load(f)


# ---- the launch traces
@pytest.fixture(scope="module")
def traces(tmp_path_factory):
    tmp = str(tmp_path_factory.mktemp("group_knn_trace"))
    obj, stub, defsym = _host_objects(tmp)
    lib = os.path.join(tmp, "libbithtm_host_trace.so")
    # the stub writes no trace line for a wait: the engine's hipStreamSynchronize calls go through tests/host_stub/wait_counter.cpp, which
    # counts them in a file of its own and leaves the trace lines what they are
    counter = os.path.join(ROOT, "tests", "host_stub", "wait_counter.cpp")
    subprocess.run([os.path.join(CLANG_DIR, "bin", "clang++"), "-shared", "-fPIC", "-O1", obj, stub, counter, "-Wl,--wrap=hipStreamSynchronize", "-ldl", "-o", lib] + defsym,
                   check=True, capture_output=True)
    env = dict(os.environ, BITHTM_LIBRARY=lib, BITHTM_STUB_TRACE=os.path.join(tmp, "trace.txt"), BITHTM_STUB_WAITS=os.path.join(tmp, "waits.txt"))
    for name in ("LD_PRELOAD", "BITHTM_LEAN", "BITHTM_SCAN_LARGE"):
        env.pop(name, None)
    open(env["BITHTM_STUB_TRACE"], "w").close()
    r = subprocess.run([sys.executable, os.path.join(ROOT, "tests", "host_stub", "group_knn_driver.py")], env=env, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, (r.stdout + r.stderr)[-4000:]
    return json.loads(r.stdout.splitlines()[-1])


def _shape(lines):
    return [(_kernel(x), x.split()[0]) for x in lines]


@needs_hipcc
def test_the_host_code_makes_every_launch_copy_wait_and_refusal_of_the_commit_before_the_fold(traces):
    from test_knn_cpu import _same_as_recorded
    _same_as_recorded("group", traces)              # ("tick_waits" among it: a tick's one wait)


@needs_hipcc
def test_the_earlier_calls_launch_what_they_launched_before_the_banks(traces):
    """tests/golden/group_knn_traces_before.json: the output of `group_knn_driver.py before` on the commit before the banks."""
    with open(os.path.join(ROOT, "tests", "golden", "group_knn_traces_before.json")) as f:
        before = json.load(f)["before"]
    assert set(before) == set(traces["before"]) and len(before) == 11
    for name, lines in before.items():
        assert traces["before"][name] == lines, name
    assert not [x for lines in before.values() for x in lines if "kgknn" in x]


@needs_hipcc
def test_an_update_of_a_bank_is_the_launches_of_one_stream_whatever_the_streams(traces):
    lds = QUERIES * 256 * 4
    up = traces["update"]
    for S in (1, 7):
        blocks = 2 if S > 1 else 1                  # (S = 1: its one stream holds 40 slots; S = 7: the largest holds 300)
        lines = up[f"S={S} frozen T=1"]
        assert lines[0] == f"memcpy {16 * S}"       # (the one table: a pointer and two counts per stream)
        assert [_launch(x) for x in lines[1:]] == [("kgknn_distance_lds", blocks, S, 256, lds), ("kgknn_select", 1, S, 256, 0)], lines
        lines = up[f"S={S} learning T=1"]
        assert lines[:2] == [f"memcpy {4 * S}", f"memcpy {16 * S}"]
        assert [_launch(x) for x in lines[2:]] == [("kgknn_place", S, 1, 256, 0), ("kgknn_append", 1, S, 256, 0), ("kgknn_distance_lds", blocks, S, 256, lds),
                                                   ("kgknn_select", 1, S, 256, 0)], lines
        T = CHUNK + 3
        lines = up[f"S={S} learning T={T}"]
        assert [_launch(x) for x in lines[2:]] == [("kgknn_place", S, 1, 256, 0), ("kgknn_append", -(-T * 8 // 256), S, 256, 0),
                                                   ("kgknn_distance_lds", blocks, S * (CHUNK // QUERIES), 256, lds), ("kgknn_select", CHUNK, S, 256, 0),
                                                   ("kgknn_distance_lds", blocks, S, 256, lds), ("kgknn_select", 3, S, 256, 0)], lines
    for key in ("frozen T=1", "learning T=1", f"learning T={CHUNK + 3}"):
        assert _shape(up[f"S=1 {key}"]) == _shape(up[f"S=7 {key}"]), key
    assert [_kernel(x) for x in traces["unlabelled"][2:]] == ["kgknn_distance_lds", "kgknn_select"] * 2                 # (nothing to store: no place, no append)
    words = one.GLOBAL_SHAPE[0]
    assert [_launch(x) for x in traces["global"][1:]] == [("kgknn_scatter", 1, 2, 256, 0), ("kgknn_distance_global", 1, 2, 256, 8 * -(-words // 32) * 4),
                                                          ("kgknn_select", 5, 2, 256, 0), ("kgknn_scatter", 1, 2, 256, 0)], traces["global"]
    # a shared bank: the one-stream kernels over one flat batch -- the store is streamed once per group of queries, whichever stream they belong to
    sh = traces["shared"]
    assert [_launch(x) for x in sh["S=9 T=1"]] == [("kknn_distance_lds", 2, -(-9 // QUERIES), 256, lds), ("kknn_select", 9, 1, 256, 0)]
    assert [_launch(x) for x in sh["S=64 T=1"]] == [("kknn_distance_lds", 2, 8, 256, lds), ("kknn_select", 64, 1, 256, 0)]
    assert [_launch(x) for x in sh["S=9 T=9"]] == [("kknn_distance_lds", 2, 8, 256, lds), ("kknn_select", 64, 1, 256, 0), ("kknn_distance_lds", 2, 3, 256, lds),
                                                   ("kknn_select", 17, 1, 256, 0)]
    # (waits are not trace lines: the tick test below counts them; an update_patterns call waits in Python, behind its enqueue)


@needs_hipcc
@pytest.mark.parametrize("mode", ["run", "graphs"])
def test_a_group_run_with_a_bank_adds_one_update_per_batch(traces, mode):
    recorded, classified, near, both = traces["before"][f"{mode} recorded"], traces["before"][f"{mode} classified"], traces[f"{mode} knn"], traces[f"{mode} both"]
    tail = ["kgknn_place", "kgknn_append", "kgknn_distance_lds", "kgknn_select"]
    # behind the run: the one table (a pointer and two counts per member) and the update of its 6 steps; in front: the members' capture
    # descriptors and the labels [3][72], once
    assert [_kernel(x) for x in near[-4:]] == tail and near[-5] == "memcpy 48" and _launch(near[-1])[1:] == (6, 3, 256, 0)
    assert near[:2] == ["memcpy 24", f"memcpy {4 * 3 * 72}"]
    body = near[2:-5]
    captures = sum(_kernel(x) == "kgcls_capture" for x in body)
    assert captures == (6 if mode == "run" else 0)  # (one small launch per step for all members; inside the graph when replayed)
    assert [x for x in body if _kernel(x) != "kgcls_capture"] == recorded
    # with a classifier bank as well: the classified run's lines, the labels in front and the KNN update behind -- still one capture per step
    assert [_kernel(x) for x in both[-4:]] == tail and both[0] == f"memcpy {4 * 3 * 72}" and both[1:-5] == classified
    assert sum(_kernel(x) == "kgknn_select" for x in near) == 1 and sum(_kernel(x) == "kgknn_select" for x in both) == 1


@needs_hipcc
def test_a_tick_with_a_bank_does_not_depend_on_the_members(traces):
    t = traces["tick"]
    for n in (1, 7):
        plain, learning, unlabelled, frozen, both, classified = (t[f"B={n} {k}"] for k in ("plain", "learning", "unlabelled", "frozen", "both", "classified"))
        for lines in (plain, learning, unlabelled, frozen, both, classified):                   # one copy in, one copy out, nothing else but launches
            assert [x.split()[0] for x in lines if not x.startswith("launch ")] == ["memcpy", "memcpy"] and lines[0].startswith("memcpy") and lines[-1].startswith("memcpy")
        assert not [x for lines in (learning, unlabelled, frozen, both) for x in lines if _kernel(x) == "kgknn_place"]      # (the slots came in the staging copy)
        captured = [x for x in plain[1:-1]]
        near = [x for x in learning[1:-1] if _kernel(x) != "kgcls_capture"]
        assert near[:len(captured)] == captured and sum(_kernel(x) == "kgcls_capture" for x in learning) == 1
        assert [_launch(x) for x in near[len(captured):]] == [("kgknn_append", 1, n, 256, 0), ("kgknn_distance_lds", 1, n, 256, QUERIES * 256 * 4), ("kgknn_select", 1, n, 256, 0)]
        assert [_kernel(x) for x in frozen[-3:-1]] == ["kgknn_distance_lds", "kgknn_select"] and len(frozen) == len(unlabelled) == len(learning) - 1 == len(plain) + 3
        # the copy in carries four words per member more, the copy out five
        assert int(learning[0].split()[1]) == int(plain[0].split()[1]) + 16 * n and int(learning[-1].split()[1]) >= int(plain[-1].split()[1]) + 20 * n
        # with a classifier bank: the classified tick's launches, the bank's three behind them, the patterns captured once
        assert both[1:-4] == classified[1:-1] and [_kernel(x) for x in both[-4:-1]] == ["kgknn_append", "kgknn_distance_lds", "kgknn_select"]
        assert sum(_kernel(x) == "kgcls_capture" for x in both) == 1
    for k in ("learning", "unlabelled", "frozen", "both"):
        assert _shape(t[f"B=1 {k}"]) == _shape(t[f"B=7 {k}"]), k
    # ... and the waits: one per tick, with a bank or without, at B = 1 and at B = 7
    waits = traces["tick_waits"]
    assert len(waits) == 14 and all(n == 1 for n in waits.values()), waits
    views, plain = t["views B=9"], t["views B=9 plain"]
    assert [_launch(x) for x in views[-3:-1]] == [("kknn_distance_lds", 1, -(-9 // QUERIES), 256, QUERIES * 256 * 4), ("kknn_select", 9, 1, 256, 0)]
    assert len(views) == len(plain) + 3 and views[:10] == plain[:10]
    # the refusals enqueue nothing
    assert traces["refused_lines"] == [] and all(traces["refused"].values()), traces["refused"]
    assert "stream 1" in traces["refused"]["one stream past capacity"] and "stream 1" in traces["refused"]["a tick past capacity"]


# ---- the host code under ASan + UBSan, as a stand-alone program, and the bank header's arithmetic on the host
def _arithmetic_cases():
    lines, expect = [], []
    for n, capacity, words in [(1, 64, 256), (3, 64, 256), (1023, 64, 256), (1024, 64, 256), (65535, 64, 256), (65536, 64, 256), (3, 1 << 20, 256), (2, 1 << 20, 256),
                               (64, 1 << 20, 256), (128, 1 << 20, 256), (129, 1 << 20, 256), (100, 8, 12289), (2, 300, 14000), (9, 4096, 2048), (256, 16384, 2048),
                               (300, 1 << 20, 2048), (40000, 4096, 65536), (1, 1 << 20, 1 << 20), (500, 1 << 20, 1 << 20), (2, 1 << 20, 1 << 26)]:
        lines.append(f"c {n} {capacity} {words}")
        chunk = cases.chunk_of(n, capacity, words)
        shared = cases.chunk_of(1, capacity, words)     # (one stream's chunk under the same budget: below 64 it is not doubled)
        while shared >= CHUNK and shared < n and shared * 2 <= 32768 and cases.scratch_bytes(1, shared * 2, capacity, words) <= cases.SCRATCH_BYTES:
            shared *= 2
        expect.append(f"{chunk} {shared} {cases.scratch_bytes(n, chunk, capacity, words)}")
    for m, per in [(0, 5), (3, 40 * 96), (65534, (1 << 20) * 2047), (7, 0)]:
        lines.append(f"o {m} {per}")
        expect.append(str(m * per))
    for n, nq, q, count in [(3, 24, 8, 257), (1, 1, 8, 1), (7, 64, 8, 300), (7, 3, 8, 300), (2, 5, 8, 33), (1100, 32, 8, 6), (9, 1, 6, 261), (65535, 1, 1, 1 << 20)]:
        lines.append(f"g {n} {nq} {q} {count}")
        expect.append(f"{-(-count // SLOTS)} {n * -(-nq // q)}")
    return lines, expect


@needs_hipcc
def test_the_host_code_runs_clean_under_asan_and_ubsan_and_the_bank_arithmetic_equals_its_twins(tmp_path):
    """tests/host_stub/group_knn_host.cpp and htm_engine.hip (host-only), both with -fsanitize=address,undefined, linked against the stub
    runtime into ONE program that is run directly: nothing is preloaded."""
    tmp = str(tmp_path)
    san = ["-fsanitize=address,undefined", "-fno-sanitize-recover=undefined"]
    obj, stub, defsym = _host_objects(tmp, san)
    clang = os.path.join(CLANG_DIR, "bin", "clang++")
    exe = os.path.join(tmp, "group_knn_host")
    subprocess.run([clang, "-std=c++17", "-O1", "-g", "-fno-omit-frame-pointer", "-ffp-contract=off"] + san +
                   [os.path.join(ROOT, "tests", "host_stub", "group_knn_host.cpp"), obj, stub, "-ldl", "-o", exe] + defsym, check=True, capture_output=True)
    lines, expect = _arithmetic_cases()
    path = os.path.join(tmp, "cases.txt")
    with open(path, "w") as f:
        f.write("\n".join(lines) + "\n")
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=0", UBSAN_OPTIONS="print_stacktrace=1")
    for name in ("LD_PRELOAD", "BITHTM_STUB_TRACE", "BITHTM_LIBRARY"):
        env.pop(name, None)
    r = subprocess.run([exe, path], env=env, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0 and r.stdout.strip().endswith("ok"), (r.stdout + r.stderr)[-6000:]
    assert "runtime error" not in r.stderr and "AddressSanitizer" not in r.stderr, r.stderr[-6000:]
    got = r.stdout.split("\n")[:-2]
    assert len(got) == len(expect) > 25
    wrong = [(line[:80], g[:80], e[:80]) for line, g, e in zip(lines, got, expect) if g != e]
    assert not wrong, wrong[:5]
