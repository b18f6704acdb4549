"""KNN classifier (bithtm_amd/knn.py, KNNClassifier, htm_knn_*) -- what holds without a GPU: a hand-computed
stream of the definition, the path every case of tests/knn_cases.py names (from the kernel header's arithmetic in its Python twin:
the blocks of the distance launch, the select's bins and its walk), the definition over split calls, the model-level hit rate on the
oracle's states, the C ABI's declarations and binding, the refusals, the compiler's report for the new kernels, the launches of an
update and of a run with knn= (the host code built host-only against tests/host_stub/hip_stub_runtime.cpp), and the host code under
ASan + UBSan as a stand-alone program (tests/host_stub/knn_host.cpp), which also evaluates the kernel header's arithmetic on the host."""
import ctypes as C
import json
import os
import re
import subprocess
import sys

import numpy as np
import pytest

import knn_cases as cases
from knn_cases import BINS, CASE_IDS, CHUNK, QUERIES, SLOTS, TABLE_BYTES
from test_likelihood_cpu import CLANG_DIR, HEADER, ROOT, _host_objects, _kernel, _launch, needs_hipcc

KERNELS = os.path.join(ROOT, "bithtm_amd", "csrc", "htm_knn.h")
ABI = {"htm_knn_create": "htm_handle *h", "htm_knn_destroy": "htm_knn *knn", "htm_knn_labels": "htm_knn *knn", "htm_knn_update": "htm_knn *knn",
       "htm_knn_reset": "htm_knn *knn", "htm_knn_export": "htm_knn *knn", "htm_knn_import": "htm_knn *knn", "htm_knn_info": "const htm_knn *knn"}
NEW_KERNELS = ["kknn_append", "kknn_distance_global", "kknn_distance_lds", "kknn_place", "kknn_scatter", "kknn_select"]


# ---- the header's arithmetic, in Python (the stand-alone program at the end holds the header to these)
def table_words(cols, wpc):
    return cols * wpc


def in_lds(words):
    return int(words * 4 <= TABLE_BYTES)


def bitmap_words(words):
    return -(-words // 32)


def has_bitmap(words):
    return int(not in_lds(words) and bitmap_words(words) * 4 <= TABLE_BYTES)


def queries(words):
    if not in_lds(words) and not has_bitmap(words):
        return QUERIES
    return min(QUERIES, TABLE_BYTES // ((words if in_lds(words) else bitmap_words(words)) * 4))


def distance_lds(words):
    return queries(words) * words * 4 if in_lds(words) else queries(words) * bitmap_words(words) * 4 if has_bitmap(words) else 0


def shift_of(max_pairs, K):
    most, s = max_pairs * min(K, 32), 0
    while (most >> s) >= BINS:
        s += 1
    return s


def wave_span(count):
    return -(-(-(-count // 4)) // 64) * 64


def case_shift(p):
    return shift_of(p["shape"][2], p["shape"][1])


# ---- the definition
def test_a_hand_computed_stream_of_four_steps():
    """Patterns over 4 columns of 8 cells, k = 2, min_overlap = 2.  Step 0: A = {(0, 0b0111), (1, 0b0011)}, label 2: the store is
    empty, the row is (-1, 0, 0, -1, -1); A goes into slot 0 with stamp 0.  Step 1: B = {(0, 0b0110), (2, 0b1)}, label 0: overlap with A
    is popcount(0b0110) = 2 >= 2: one neighbour, label 2, one vote; B goes into slot 1, stamp 1.  Step 2: Q = {(0, 0b0101), (1, 0b0010),
    (2, 0b1)}, no label: overlap with A = popcount(0b0101) + popcount(0b0010) = 3, with B = popcount(0b0100) + 1 = 2: both are neighbours,
    one vote each -- the lower label, 0, wins with one vote although the nearest (slot 0, overlap 3, stamp 0) is labelled 2.  Nothing
    is stored.  Step 3: R = {(3, 0xFF), (0, 0b1000)}, label 1: overlaps 0 and 0: no neighbour; R goes into slot 2 with stamp 3."""
    from bithtm_amd.knn import KNNDefinition, overlap
    d = KNNDefinition(3, k=2, min_overlap=2, capacity=4, column_dim=4, cell_dim=8, max_pairs=3)
    assert d.step([(0, 0b0111), (1, 0b0011)], 2) == ([-1, 0, 0, -1, -1], [0, 0, 0])
    assert d.step([(0, 0b0110), (2, 0b1)], 0) == ([2, 1, 2, 0, 0], [0, 0, 1])
    assert d.step([(0, 0b0101), (1, 0b0010), (2, 0b1)], -1) == ([0, 1, 3, 0, 0], [1, 0, 1])
    assert (d.count, d.total) == (2, 3)
    assert d.step([(3, 0xFF), (0, 0b1000)], 1) == ([-1, 0, 0, -1, -1], [0, 0, 0])
    assert (d.count, d.total, d.labels_of, d.stamps) == (3, 4, [2, 0, 1], [0, 1, 3])
    assert overlap({0: 0b0101, 1: 0b0010, 2: 1}, {0: 0b0111, 1: 0b0011}) == 3
    pairs, labels, stamps = d.store_arrays()
    assert pairs.tolist() == [[[0, 7], [1, 3], [-1, 0]], [[0, 6], [2, 1], [-1, 0]], [[3, 255], [0, 8], [-1, 0]]] and stamps.dtype == np.int64
    # a label outside [0, labels) is none; learning off stores nothing; reset empties the store and keeps the total
    d.step([(0, 1)], 3)
    d.step([(0, 1)], 1, learning=False)
    assert (d.count, d.total) == (3, 6)
    d.step([(1, 1)], 0)
    with pytest.raises(ValueError, match="capacity"):
        d.update([[0]], [[1]], [1])
    assert (d.count, d.total) == (4, 7)
    d.reset()
    assert (d.count, d.total) == (0, 7) and d.step([(0, 0b0111)], -1)[0] == [-1, 0, 0, -1, -1]
    # the low 32 bits of a stamp, as an int32
    d.total = (1 << 32) + (1 << 31) + 5
    d.step([(0, 0b11)], 1)
    assert d.step([(0, 0b11)], -1)[0] == [1, 1, 2, 0, -(1 << 31) + 5]


@pytest.mark.parametrize("name", CASE_IDS)
def test_the_selects_twin_equals_the_definition_on_every_case(name):
    """The device's select -- bins, the k-th overlap's bin, the overlaps inside it, the walk in slot order -- written in NumPy
    (knn_cases.select_twin) gives the definition's rows and votes on every step of every case."""
    p, calls, _ = cases.case(name)
    d = cases.definition(p)
    for c in calls:
        for t in range(len(c["index"])):
            ov = cases.overlaps(d, c["index"][t], c["words"][t])
            row, votes, v, tied, took = cases.select_twin(ov, d.labels_of, d.stamps, p["k"], p["min_overlap"], p["labels"], case_shift(p))
            want_row, want_votes = d.step(zip(c["index"][t], c["words"][t]), c["labels"][t], c["learning"])
            assert row == want_row and votes.tolist() == want_votes, (name, t)


def _ties(name):
    """Per step of the case's last call: (the slots tied at the k-th overlap, those of them taken, the overlaps)."""
    p, calls, _ = cases.case(name)
    d = cases.run_definition(p, calls[:-1])[1]
    out = []
    for index, words in zip(calls[-1]["index"], calls[-1]["words"]):
        ov = cases.overlaps(d, index, words)
        row, votes, v, tied, took = cases.select_twin(ov, d.labels_of, d.stamps, p["k"], p["min_overlap"], p["labels"], case_shift(p))
        out.append((tied, took, ov, v))
    return p, d, out


def test_every_case_reaches_the_path_it_names():
    from bithtm_amd import _lib as L
    from bithtm_amd.knn import MAX_CAPACITY, MAX_K, MAX_LABELS, MAX_PAIRS, live_bits
    kernels = open(KERNELS).read()
    for name, value in (("CHUNK", L.KNN_CHUNK), ("SLOTS", L.KNN_SLOTS), ("QUERIES", L.KNN_QUERIES), ("BINS", L.KNN_BINS), ("MAX_LABELS", MAX_LABELS),
                        ("MAX_K", MAX_K), ("MAX_PAIRS", MAX_PAIRS)):
        assert int(re.search(rf"#define HTM_KNN_{name} (\d+)", kernels).group(1)) == value, name
    assert re.search(r"#define HTM_KNN_TABLE_BYTES \(48 \* 1024\)", kernels) and L.KNN_TABLE_BYTES == 48 * 1024
    assert re.search(r"#define HTM_KNN_MAX_CAPACITY \(1 << 20\)", kernels) and MAX_CAPACITY == 1 << 20
    assert MAX_PAIRS * 32 <= 65535                  # (an overlap fits the 16 bits it is kept in)
    assert {c[0] for c in cases.CASES} == set(CASE_IDS) and all(cases.case(n) for n in CASE_IDS)
    counts = {n: cases.expected(n)[1].count for n in CASE_IDS}
    # 1. empty, one slot, k - 1, k, k + 1
    assert counts["empty"] == 0 and all((b == [-1, 0, 0, -1, -1]).all() and not v.any() for b, v in cases.expected("empty")[0])
    assert counts["one-slot"] == 1 and (cases.expected("one-slot")[0][1][0][:, 3] <= 0).all() and (cases.expected("one-slot")[0][1][0][:, 3] == 0).any()
    p, calls, _ = cases.case("around-k")
    sizes, d = [], cases.definition(p)
    for c in calls:
        if not c["learning"]:
            sizes.append(d.count)
        d.update(c["index"], c["words"], c["labels"], c["learning"])
    assert sizes == [p["k"] - 1, p["k"], p["k"] + 1]
    asked = cases.expected("around-k")[0]
    assert asked[1][1].sum(axis=1).max() == 2 and asked[3][1].sum(axis=1).max() == 3 and asked[5][1].sum(axis=1).max() == 3      # (never more than k votes)
    # 2. one slot past a block; several blocks with ties at the k-th overlap on both sides of a block boundary, the lower slots taken
    assert counts["block-plus-one"] == SLOTS + 1 and -(-counts["block-plus-one"] // SLOTS) == 2
    assert len(cases.case("block-plus-one")[1][0]["index"]) == SLOTS + 1 > 4 * CHUNK      # (one learning call of five chunks fills it)
    p, d, ties = _ties("blocks")
    assert d.count == 600 and -(-d.count // SLOTS) == 3
    straddle = [(tied, took) for tied, took, ov, v in ties if len(took) and len(tied) > len(took) and tied.min() < SLOTS <= tied.max()]
    assert straddle, "no query with ties at the k-th overlap on both sides of slot 256"
    for tied, took in straddle:
        assert took.tolist() == sorted(tied.tolist())[:len(took)] and took.max() < tied[len(took):].min()
    assert any(took.max() < SLOTS <= tied[len(took)] for tied, took in straddle) or any(took.max() >= SLOTS for tied, took in straddle)
    span = wave_span(600)
    assert span == 192 and any(len(took) and tied.min() < span <= tied.max() for tied, took, ov, v in ties)     # (and of a wave's share of the walk)
    # 3. the votes
    (b, v), = cases.expected("vote-tie")[0][1:]
    assert v[0].tolist() == [0, 1, 0, 1, 0, 0] and b[0].tolist() == [1, 1, 5, 0, 0] and cases.expected("vote-tie")[1].labels_of[0] == 3
    (b, v), = cases.expected("nearest-loses")[0][1:]
    assert b[0].tolist() == [2, 2, 6, 0, 0] and cases.expected("nearest-loses")[1].labels_of[0] == 0
    # 4. min_overlap
    (b, v), = cases.expected("min-overlap")[0][1:]
    assert b.tolist() == [[2, 1, 4, 0, 0], [-1, 0, 0, -1, -1]]
    # 5. the gate
    (b, v), = cases.expected("gate")[0]
    assert b.tolist() == [[-1, 0, 0, -1, -1], [1, 1, 8, 0, 0], [-1, 0, 0, -1, -1], [1, 1, 8, 0, 0], [3, 1, 6, 2, 2]]
    assert cases.expected("gate")[1].stamps == [0, 1, 2, 4]
    # 6. two words per column
    p, calls, _ = cases.case("wpc2")
    assert p["shape"][1] == 40 and (calls[0]["index"][9] == -1).all() and (calls[0]["index"][3] == -1).sum() == 2 and calls[0]["index"].shape[1] < p["shape"][2]
    high = (calls[0]["index"] >= 0) & (calls[0]["index"] % 2 == 1)
    assert high.any() and (calls[0]["words"][high] < 256).all() and (calls[0]["words"][high] > 0).any()
    p, calls, _ = cases.case("wpc2-dead-bits")
    assert live_bits(1, 0xFFFFFF81, 40, 64) == 0x81 and live_bits(127, 0xFF, 40, 64) == 0xFF and live_bits(128, 0xFF, 40, 64) == 0 and live_bits(-5, 0xFF, 40, 64) == 0
    b = cases.expected("wpc2-dead-bits")[0][1][0]
    assert b.tolist() == [[1, 1, 3, 0, 0], [-1, 0, 0, -1, -1], [-1, 0, 0, -1, -1]] and all(c["raw"] for c in calls)
    # 7. the two forms of the distance launch
    C_, K_, P_ = cases.GLOBAL_SHAPE
    assert (C_ - 1) * 4 == TABLE_BYTES and not in_lds(table_words(C_, 1)) and in_lds(table_words(C_ - 1, 1)) and queries(C_ - 1) == 1
    p, calls, _ = cases.case("global-table")
    assert counts["global-table"] > SLOTS and len(calls[1]["index"]) > CHUNK and (calls[0]["index"] == C_ - 1).any() and (calls[1]["index"] == C_ - 1).any()
    assert in_lds(table_words(*cases.case("lds-twin")[0]["shape"][:1], 1)) and not in_lds(table_words(cases.case("global-twin")[0]["shape"][0], 1))
    C2 = cases.NO_BITMAP_SHAPE[0]
    assert has_bitmap(C_) and not has_bitmap(C2) and has_bitmap(C2 - 1) and queries(C2) == QUERIES and queries(C2 - 1) == 1
    p, calls, _ = cases.case("global-no-bitmap")
    assert (calls[0]["index"] == C2 - 1).any() and (calls[1]["index"] == C2 - 1).any() and counts["global-no-bitmap"] > 0
    # 8. a last group of staged queries that is not full
    p, calls, _ = cases.case("ragged-chunk")
    q = queries(table_words(p["shape"][0], 1))
    assert q == QUERIES and [len(c["index"]) % CHUNK % q for c in calls[1:]] == [3, 5] and len(calls[1]["index"]) > CHUNK
    # 9. capacity
    p, calls, refused = cases.case("capacity")
    assert counts["capacity"] == p["capacity"] and refused is not None
    with pytest.raises(ValueError, match="capacity"):
        cases.run_definition(p, calls + [refused])
    # the two-level bins
    p, d, ties = _ties("two-level-bins")
    assert case_shift(p) == 1 and shift_of(63, 32) == 0 and shift_of(2047, 32) == 5 and (2047 * 32 >> 5) < BINS
    assert any(len(tied) and v % 2 == 1 for tied, took, ov, v in ties) and any(len(tied) and v % 2 == 0 for tied, took, ov, v in ties)
    assert any(len(tied) and ((ov >> 1) == (v >> 1)).sum() > (ov == v).sum() for tied, took, ov, v in ties)      # (another overlap in the k-th bin)


def test_the_definition_over_split_calls_equals_one_call():
    p, calls, _ = cases.case("split-stream")
    c = calls[0]
    (want_best, want_votes), = cases.expected("split-stream")[0]
    d = cases.expected("split-stream")[1]
    assert 0 < d.count < len(c["index"]) and (c["labels"] < 0).any()
    for cut in range(len(c["index"]) + 1):
        parts = [cases.call(c["index"][a:b], c["words"][a:b], c["labels"][a:b]) for a, b in ((0, cut), (cut, len(c["index"])))]
        got, e = cases.run_definition(p, parts)
        assert np.array_equal(np.concatenate([g[0] for g in got]), want_best) and np.array_equal(np.concatenate([g[1] for g in got]), want_votes)
        assert e.slots == d.slots and (e.labels_of, e.stamps, e.total) == (d.labels_of, d.stamps, d.total)
    # first_step: step i reads label (first_step + i) % len(labels)
    e = cases.definition(p)
    best, votes = e.update(c["index"][:4], c["words"][:4], [-1, 1, 0], first_step=2)
    assert e.labels_of == [0, 1, 0] and e.stamps == [0, 2, 3]       # (rows 2, 0, 1, 2)


def test_the_model_level_hit_rate_on_the_oracles_states_is_the_recorded_value():
    best, votes, d = cases.model_stream()
    inputs, labels, names = cases.model_inputs()
    rate = cases.hit_rate(best[:, 0])
    print("hit rate of the later passes", rate)
    assert rate == cases.HIT_RATE == 35 / 36
    assert d.count == cases.MODEL_PATTERNS * cases.LABELLED_EPOCHS and d.total == len(inputs) and (labels < 0).sum() == 36
    assert len(set(names[:6].tolist())) == 6        # (six different labels: a constant guess would be right once in six)
    asked = votes.sum(axis=1)[labels < 0]
    assert (asked >= 1).all() and (asked <= cases.MODEL_K).all() and (asked == cases.MODEL_K).sum() > 30


# ---- the C ABI
def test_the_header_declares_the_knn_abi_and_the_binding_matches_it():
    from bithtm_amd import _lib as L
    header = open(HEADER).read()
    decl = {m.group(1): m.group(2) for m in re.finditer(r"\b(htm_knn_[a-z_]+)\s*\(([^)]*)\)\s*;", header)}
    assert set(decl) == set(ABI)
    for name, params in decl.items():
        assert params.split(",")[0].strip() == ABI[name], (name, params)
        assert len(L.EXPORTS[name][1]) == len(params.split(",")), name
    assert L.EXPORTS["htm_knn_destroy"][0] is None and all(L.EXPORTS[n][0] is C.c_int for n in ABI if n != "htm_knn_destroy")
    assert L.ABI_VERSION == 4 and re.search(r"#define BITHTM_ABI_VERSION 4\b", header)
    body = re.search(r"typedef struct htm_knn_config \{(.*?)\} htm_knn_config;", header, re.S).group(1)
    assert [re.sub(r"\s+", " ", x.strip()) for x in body.split(";") if x.strip()] == [
        "uint32_t struct_bytes", "int32_t labels, k, min_overlap, capacity, units, cell_dim, max_pairs"]
    assert C.sizeof(L.HtmKnnConfig) == 32 and [n for n, _ in L.HtmKnnConfig._fields_] == ["struct_bytes", "labels", "k", "min_overlap", "capacity", "units", "cell_dim", "max_pairs"]
    body = re.sub(r"/\*.*?\*/", "", re.search(r"typedef struct htm_knn_info_t \{(.*?)\} htm_knn_info_t;", header, re.S).group(1), flags=re.S)
    fields = [re.sub(r"\s+", " ", x.strip()) for x in body.split(";") if x.strip()]
    assert fields == ["uint32_t struct_bytes", "int32_t labels, k, min_overlap, capacity, units, cell_dim, max_pairs", "int32_t count", "int32_t table_in_lds",
                      "int32_t queries_per_block", "int32_t bin_shift", "int64_t total", "int64_t state_bytes", "int64_t device_bytes"]
    assert C.sizeof(L.HtmKnnInfo) == 72 and [n for n, _ in L.HtmKnnInfo._fields_][8:] == ["count", "table_in_lds", "queries_per_block", "bin_shift", "total",
                                                                                         "state_bytes", "device_bytes"]
    update = [re.sub(r"\s+", " ", x.strip()) for x in decl["htm_knn_update"].split(",")]
    assert update == ["htm_knn *knn", "htm_handle *h", "const void *device_pairs", "int32_t pairs_per_step", "int32_t n_steps", "const int32_t *device_labels",
                      "int32_t n_labels", "int32_t first_step", "int32_t learn", "int32_t *device_best", "int32_t *device_votes"]


def test_the_c_calls_refuse_null_arguments_without_a_gpu():
    from bithtm_amd import _lib as L
    lib = L.load()
    cfg = L.HtmKnnConfig(C.sizeof(L.HtmKnnConfig), 3, 1, 1, 16, 64, 32, 4)
    out = C.c_void_p(1)
    assert lib.htm_knn_create(None, C.byref(cfg), C.byref(out)) == -1 and not out.value
    assert b"null" in lib.htm_last_error(None)
    assert lib.htm_knn_update(None, None, None, 1, 1, None, 1, 0, 1, None, None) == -1
    assert lib.htm_knn_labels(None, None, None, 1, C.byref(out)) == -1 and lib.htm_knn_reset(None, None) == -1
    assert lib.htm_knn_export(None, None, None, 0) == -1 and lib.htm_knn_import(None, None, None, 0) == -1
    assert lib.htm_knn_info(None, None) == -1
    lib.htm_knn_destroy(None)


def test_the_python_layer_refuses_before_any_library_call():
    import bithtm_amd as B
    from bithtm_amd.knn import check_params
    assert check_params(16, 3, 2, 100) == (16, 3, 2, 100) and check_params(1024, 64, 65535, 1 << 20)
    for bad in (dict(labels=0), dict(labels=1025), dict(labels=3, k=0), dict(labels=3, k=65), dict(labels=3, min_overlap=0), dict(labels=3, min_overlap=65536),
                dict(labels=3, capacity=0), dict(labels=3, capacity=(1 << 20) + 1)):
        with pytest.raises(ValueError):
            B.KNNClassifier(**bad)
    for shape in ((10, 65, 4), (0, 8, 4), (10, 8, 0), (10, 8, 2048)):
        with pytest.raises(ValueError, match="shape"):
            B.KNNClassifier(3, shape=shape)
    knn = B.KNNClassifier(3, k=2, capacity=4, shape=(10, 5, 4))
    assert (knn.labels, knn.k, knn.min_overlap, knn.capacity, knn.count, knn.total, knn.units) == (3, 2, 1, 4, 0, 0, 50)
    ok = (np.array([[0, 1, 2, -1]]), np.array([[1, 2, 4, 0xFFFFFFFF]], dtype=np.uint32), [0])
    for index, words, labels, match in (
            (np.array([[0, 1, 1, 3]]), np.array([[1, 2, 4, 1]], dtype=np.uint32), ok[2], "twice"), (np.array([[0, 1, 2, 10]]), ok[1], ok[2], "at or above 10"),
            (ok[0], np.array([[1, 2, 32, 0]], dtype=np.uint32), ok[2], "cell_dim"), (ok[0], ok[1], [0, 1], r"int \[1\]"), (ok[0], ok[1], [0.5], "labels: int"),
            (ok[0][:, :3], ok[1], ok[2], "index int"), (np.zeros((1, 5), int) + np.arange(5), np.ones((1, 5), np.uint32), ok[2], "max_pairs"),
            (np.tile(ok[0], (5, 1)), np.tile(ok[1], (5, 1)), [0, 1, 2, 0, 1], "capacity")):
        with pytest.raises(ValueError, match=match):
            knn.update_patterns(index, words, labels)
    assert knn.check_labels([0, 2, 3, -4]).tolist() == [0, 2, -1, -1]           # (outside [0, labels): no label)
    assert knn.stored_by(np.array([0, -1, 2], np.int32), 1, 7, True) == 4 and knn.stored_by(np.array([0, -1, 2], np.int32), 1, 7, False) == 0
    with pytest.raises(RuntimeError, match="not bound"):
        knn.update_patterns(*ok)
    with pytest.raises(RuntimeError, match="shape"):
        B.KNNClassifier(3).update_patterns(*ok)
    # an unbound object holds a loaded state until it is bound
    state = knn.state_dict()
    assert (int(state["total"]), int(state["count"])) == (0, 0) and state["pairs"].shape == (0, 4, 2) and state["params"].tolist() == [3, 2, 1, 4, 10, 5, 4]
    state.update(total=np.int64(9), count=np.int64(2), pairs=np.array([[[0, 1], [3, 2], [-1, 0], [-1, 0]], [[5, 7], [-1, 0], [-1, 0], [-1, 0]]], np.int32),
                 labels=np.array([2, 0], np.int32), stamps=np.array([3, 8], np.int64))
    knn.load_state_dict(state)
    again = knn.state_dict()
    assert all(np.array_equal(again[k], state[k]) for k in state) and (knn.count, knn.total) == (2, 9)
    with pytest.raises(ValueError, match="capacity"):
        knn.update_patterns(np.tile(ok[0], (3, 1)), np.tile(ok[1], (3, 1)), [0, 1, 2])      # (two slots are in use)
    knn.reset()
    assert (knn.count, knn.total) == (0, 9) and knn.state_dict()["pairs"].shape == (0, 4, 2)
    with pytest.raises(ValueError, match="parameters"):
        B.KNNClassifier(4, k=2, capacity=4, shape=(10, 5, 4)).load_state_dict(state)
    for key, value, match in (("count", np.int64(5), "count"), ("count", np.int64(1), "pairs"), ("labels", np.array([2, 3], np.int32), "label"),
                              ("stamps", np.array([8, 8], np.int64), "stamps"), ("stamps", np.array([3, 9], np.int64), "stamps"), ("total", np.int64(-1), "total")):
        with pytest.raises(ValueError, match=match):
            knn.load_state_dict(dict(state, **{key: value}))
    fresh = B.KNNClassifier(3, k=2, capacity=4)
    fresh.load_state_dict(state)                    # (the shape comes with the state)
    assert fresh.shape == (10, 5, 4) and fresh.count == 2
    # the calls a KNN classifier does not ride on refuse it before anything else
    tm, sp = B.TemporalMemory(64, 4), B.SpatialPooler(32, 64, 4)
    for call in (lambda: tm.run(np.zeros((1, 4), int), 1, knn=knn), lambda: sp.run(np.zeros((1, 32), bool), 1, knn=knn)):
        with pytest.raises(ValueError, match="knn= is not available here"):
            call()
    for method, positional in ((B.HierarchicalTemporalMemory.lookahead, 4), (B.HierarchicalTemporalMemory.forecast, 2), (B.ModelGroup.run, 3),
                               (B.ModelGroup.tick, 2)):
        with pytest.raises(ValueError, match="knn= is not available here"):
            method(*[None] * positional, knn=knn)


def test_run_record_carries_the_knn_result():
    import bithtm_amd as B
    rec = B.RunRecord(np.arange(2))
    assert all(getattr(rec, f) is None for f in ("knn_label", "knn_votes", "knn_overlap", "knn_nearest_slot", "knn_nearest_step", "knn_votes_all"))
    rows = np.array([[3, 2, 17, 5, 40], [-1, 0, 0, -1, -1]], dtype=np.int32)
    rec = B.RunRecord(np.arange(2), knn=rows, knn_votes_all=np.zeros((2, 6), np.int32))
    assert rec.knn_label.tolist() == [3, -1] and rec.knn_votes.tolist() == [2, 0] and rec.knn_overlap.tolist() == [17, 0]
    assert rec.knn_nearest_slot.tolist() == [5, -1] and rec.knn_nearest_step.tolist() == [40, -1] and rec.knn_votes_all.shape == (2, 6)
    assert B.RunRecord(np.arange(2), knn=rows).knn_votes_all is None and rec.classified_bucket is None


# ---- the compiler's report
def test_the_new_kernels_have_no_scratch_and_the_existing_ones_keep_their_figures():
    """The KNN kernels report into a file of their own (bithtm_amd.build.OWN_REPORTS: the report of the kernels before them is held to
    its set of names by an earlier test); the two reports together are every kernel of the library."""
    from bithtm_amd.build import all_kernel_resources, kernel_resources
    new, old, res = kernel_resources("htm_knn.h"), kernel_resources(), all_kernel_resources()
    if new is None or old is None:
        pytest.skip("the library in the tree was not built here")
    assert sorted(re.match(r"_Z\d+(kknn_[a-z_]+?)\d", k).group(1) for k in new) == NEW_KERNELS, sorted(new)
    assert not set(new) & set(old) and set(res) == set(new) | set(old) and not [k for k in old if "kknn_" in k]
    for name, r in new.items():
        print(name, r)
        assert r["scratch_bytes_per_lane"] == 0, (name, r)
        assert r["lds_bytes"] <= 16 * 1024 and r["occupancy"] >= 4, (name, r)       # (static; the distance launch adds at most 48 KiB of tables)
    old_names = {re.match(r"_Z\d+(k[a-z]*_[a-z_]+)", k).group(1) for k in old if re.match(r"_Z\d+k[a-z]*_", k)}
    for k in new:                                   # (the budget tests find kernels with re.search: no name inside another)
        assert not [s for s in old_names if s in k], k
    # every kernel that existed before the KNN classifier was added: the figures the compiler gave it then, and no other kernel.  The
    # fixture is bithtm_amd/libbithtm_hip.resources.json of a build of the commit before htm_knn.h, copied as it is.
    with open(os.path.join(ROOT, "tests", "golden", "kernel_resources_before_knn.json")) as f:
        before = json.load(f)
    assert len(before) > 100 and not [k for k in before if "kknn_" in k]
    assert old == before, {k: (before.get(k), old.get(k)) for k in set(before) | set(old) if before.get(k) != old.get(k)}


# ---- the launch traces
@pytest.fixture(scope="module")
def traces(tmp_path_factory):
    tmp = str(tmp_path_factory.mktemp("knn_trace"))
    obj, stub, defsym = _host_objects(tmp)
    lib = os.path.join(tmp, "libbithtm_host_trace.so")
    subprocess.run([os.path.join(CLANG_DIR, "bin", "clang++"), "-shared", obj, stub, "-ldl", "-o", lib] + defsym, check=True, capture_output=True)
    env = dict(os.environ, BITHTM_LIBRARY=lib, BITHTM_STUB_TRACE=os.path.join(tmp, "trace.txt"))
    for name in ("LD_PRELOAD", "BITHTM_LEAN", "BITHTM_SCAN_LARGE"):
        env.pop(name, None)
    open(env["BITHTM_STUB_TRACE"], "w").close()
    r = subprocess.run([sys.executable, os.path.join(ROOT, "tests", "host_stub", "knn_driver.py")], env=env, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, (r.stdout + r.stderr)[-4000:]
    return json.loads(r.stdout.splitlines()[-1])


def _same_as_recorded(section, traces):
    """The driver's whole output equals tests/golden/knn_host_traces_parent.json, recorded from the commit before the one-stream and
    the bank host calls were folded into one (the same fixture, the same driver): every key, every line, the refusals' texts."""
    with open(os.path.join(ROOT, "tests", "golden", "knn_host_traces_parent.json")) as f:
        want = json.load(f)[section]
    assert sorted(traces) == sorted(want)
    for key in want:
        if isinstance(want[key], dict):
            assert sorted(traces[key]) == sorted(want[key]), key
            for name in want[key]:
                assert traces[key][name] == want[key][name], (key, name)
        assert traces[key] == want[key], key


@needs_hipcc
def test_the_host_code_makes_every_launch_copy_and_refusal_of_the_commit_before_the_fold(traces):
    _same_as_recorded("knn", traces)


@needs_hipcc
def test_an_update_is_two_launches_per_chunk_and_two_more_for_a_call_that_stores(traces):
    lds = QUERIES * 256 * 4                          # (eight staged tables of 256 words)
    for T in (1, 13, CHUNK, CHUNK + 1, 2 * CHUNK + 3):
        lines = traces["frozen"][f"T={T}"]
        assert lines[0] == f"memcpy {4 * T}"        # (the labels; the pairs went up before the trace began)
        want = []
        for first in range(0, T, CHUNK):
            n = min(CHUNK, T - first)
            want += [("kknn_distance_lds", 2, -(-n // QUERIES), 256, lds), ("kknn_select", n, 1, 256, 0)]     # (300 slots: two blocks)
        assert [_launch(x) for x in lines[1:]] == want, lines
    # below one chunk the launches do not grow with the steps
    assert len(traces["frozen"]["T=1"]) == len(traces["frozen"]["T=13"]) == len(traces["frozen"][f"T={CHUNK}"]) == 3
    for T in (1, 13, CHUNK + 1):
        lines = traces["learning"][f"T={T}"]
        assert [_kernel(x) for x in lines[1:3]] == ["kknn_place", "kknn_append"] and _launch(lines[1])[1:] == (1, 1, 256, 0)
        assert _launch(lines[2])[1:] == (-(-T * 8 // 256), 1, 256, 0)
        assert [_kernel(x) for x in lines[3:]] == ["kknn_distance_lds", "kknn_select"] * -(-T // CHUNK), lines
    assert len(traces["learning"]["T=1"]) == len(traces["learning"]["T=13"]) == 5
    assert [_kernel(x) for x in traces["learning"]["unlabelled"][1:]] == ["kknn_distance_lds", "kknn_select"] * 2      # (nothing to store: no append)
    for T in (5, CHUNK + 1):
        lines = traces["global"][f"T={T}"]
        assert [_kernel(x) for x in lines[1:]] == ["kknn_scatter", "kknn_distance_global", "kknn_select", "kknn_scatter"] * -(-T // CHUNK), lines
        words = cases.GLOBAL_SHAPE[0]               # (the distance launch stages eight presence bitmaps of a bit per table word)
        assert [_launch(x)[4] for x in lines[1:]] == [0, distance_lds(words), 0, 0] * -(-T // CHUNK) and distance_lds(words) == 8 * 385 * 4
    assert not [x for sec in ("frozen", "learning", "global") for v in traces[sec].values() for x in v if x.startswith("sync") or "Synchronize" in x]


@needs_hipcc
@pytest.mark.parametrize("mode", ["run", "graphs"])
def test_a_run_with_knn_adds_a_capture_per_step_and_a_plain_run_is_the_trace_it_was(traces, mode):
    t = traces[mode]
    recorded, near, both, classified = t["recorded"], t["knn"], t["both"], t["classified"]
    # behind the run: the update of its 6 steps (one chunk), and nothing else; in front: the labels and the 8-byte descriptor copy
    assert [_kernel(x) for x in near[-4:]] == ["kknn_place", "kknn_append", "kknn_distance_lds", "kknn_select"], near[-4:]
    assert _launch(near[-1])[1:] == (6, 1, 256, 0) and _launch(near[-2])[1:3] == (1, 1)
    body = near[:-4]
    assert body[:2] == [f"memcpy {4 * 72}", "memcpy 8"] and recorded[0] != "memcpy 8"
    body = body[2:]
    if mode == "run":
        captures = [i for i, x in enumerate(body) if _kernel(x) == "kcls_capture"]
        assert len(captures) == 6 and all(_kernel(body[i - 1]) == "k_rec_step" for i in captures)
        assert [x for x in body if _kernel(x) != "kcls_capture"] == recorded
    else:
        assert body == recorded and "graph_launch" in recorded and not [x for x in body if _kernel(x) == "kcls_capture"]
    # with a classifier as well: the classified run's lines, the labels in front and the KNN update behind -- still one capture per step
    assert [_kernel(x) for x in both[-4:]] == ["kknn_place", "kknn_append", "kknn_distance_lds", "kknn_select"]
    assert both[0] == f"memcpy {4 * 72}" and both[1:-4] == classified
    assert sum(_kernel(x) == "kcls_capture" for x in both) == (6 if mode == "run" else 0)
    # a run without knn=, on a model that has just made such runs, is line for line the trace of the model that never did
    assert t["recorded after"] == recorded and t["plain after"] == t["plain"]
    assert not [x for x in t["plain"] + recorded + classified if "kknn" in x]
    # the Python refusals enqueue nothing
    assert traces["refused_lines"] == [] and all(traces["refused"].values()), traces["refused"]
    assert "capacity" in traces["refused"]["past capacity"] and "shape" in traces["refused"]["another shape"]


# ---- the host code under ASan + UBSan, as a stand-alone program, and the kernel header's arithmetic on the host
def _arithmetic_cases():
    """The lines of the case file and, per line, what the definition and the twins above give (strings as the program prints them)."""
    from bithtm_amd.knn import live_bits
    rng = np.random.default_rng(6)
    lines, expect = [], []
    for a, b in [(0, 0), (0xFFFFFFFF, 0xFFFFFFFF), (0x80000000, 0x80000001), (0b0101, 0b0111)] + rng.integers(0, 1 << 32, (100, 2)).tolist():
        lines.append(f"o {a} {b}")
        expect.append(str(bin(a & b).count("1")))
    for index, word, K, wpc, cols in [(-1, 5, 32, 1, 10), (9, 0xFFFFFFFF, 32, 1, 10), (10, 1, 32, 1, 10), (3, 0xFFFFFFFF, 5, 1, 10), (1, 0xFFFFFF81, 40, 2, 64),
                                      (127, 0xFF, 40, 2, 64), (128, 0xFF, 40, 2, 64), (-5, 0xFF, 40, 2, 64), (7, 0xFFFFFFFF, 48, 2, 10), (12288, 0xF, 4, 1, 12289)]:
        lines.append(f"l {index} {word} {K} {wpc} {cols}")
        expect.append(str(live_bits(index, word, K, cols)))
    for cols, wpc in [(256, 1), (2048, 1), (12288, 1), (12289, 1), (6144, 2), (6145, 2), (65536, 1), (1, 1), (1536, 1), (1537, 1), (1 << 20, 2), (49152, 1),
                      (49153, 1), (393216, 1), (393217, 1), (196609, 2)]:
        lines.append(f"t {cols} {wpc}")
        w = table_words(cols, wpc)
        expect.append(f"{w} {in_lds(w)} {queries(w)} {has_bitmap(w)} {distance_lds(w)}")
    for block, count in [(0, 1), (0, 256), (0, 257), (1, 257), (2, 600), (1, 600), (4095, 1 << 20)]:
        lines.append(f"r {block} {count}")
        expect.append(f"{-(-count // SLOTS)} {block * SLOTS} {min((block + 1) * SLOTS, count)}")
    for nq, q in [(1, 8), (8, 8), (9, 8), (64, 8), (64, 6), (3, 1), (64, 1)]:
        lines.append(f"g {nq} {q}")
        expect.append(str(-(-nq // q)))
    for max_pairs, K in [(8, 8), (40, 32), (63, 32), (64, 32), (64, 40), (96, 48), (2047, 64), (2047, 4), (512, 3), (1, 1)]:
        lines.append(f"s {max_pairs} {K}")
        expect.append(f"{max_pairs * min(K, 32)} {shift_of(max_pairs, K)}")
    for overlap, shift in [(0, 0), (2047, 0), (2048, 1), (2049, 1), (65504, 5), (65503, 5), (31, 5)]:
        lines.append(f"n {overlap} {shift}")
        expect.append(f"{overlap >> shift} {overlap & ((1 << shift) - 1)}")
    for count in [0, 1, 4, 255, 256, 257, 600, 1 << 20]:
        lines.append(f"w {count}")
        expect.append(str(wave_span(count)))
    return lines, expect


def test_the_twins_of_the_header_arithmetic():
    assert [wave_span(n) for n in (0, 1, 256, 257, 600)] == [0, 64, 64, 128, 192]
    assert [queries(w) for w in (256, 1536, 1537, 2048, 12288, 12289)] == [8, 8, 7, 6, 1, 8] and in_lds(12288) and not in_lds(12289)
    # the global-table form: bitmaps of a bit per word while one fits 48 KiB (393 216 words), as many queries as fit
    assert [(has_bitmap(w), queries(w)) for w in (12288, 12289, 49152, 49153, 65536, 393216, 393217)] == [(0, 1), (1, 8), (1, 8), (1, 7), (1, 6), (1, 1), (0, 8)]
    assert [distance_lds(w) for w in (256, 12289, 65536, 393217)] == [8192, 12320, 49152, 0]
    assert [shift_of(p, 32) for p in (40, 63, 64, 127, 128, 2047)] == [0, 0, 1, 1, 2, 5]


@needs_hipcc
def test_the_host_code_runs_clean_under_asan_and_ubsan_and_the_header_arithmetic_equals_the_definition(tmp_path):
    """tests/host_stub/knn_host.cpp and htm_engine.hip (host-only), both with -fsanitize=address,undefined, linked against the stub
    runtime into ONE program that is run directly: nothing is preloaded."""
    tmp = str(tmp_path)
    san = ["-fsanitize=address,undefined", "-fno-sanitize-recover=undefined"]
    obj, stub, defsym = _host_objects(tmp, san)
    clang = os.path.join(CLANG_DIR, "bin", "clang++")
    exe = os.path.join(tmp, "knn_host")
    subprocess.run([clang, "-std=c++17", "-O1", "-g", "-fno-omit-frame-pointer", "-ffp-contract=off"] + san +
                   [os.path.join(ROOT, "tests", "host_stub", "knn_host.cpp"), obj, stub, "-ldl", "-o", exe] + defsym, check=True, capture_output=True)
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
    assert len(got) == len(expect) > 150
    wrong = [(line[:80], g[:80], e[:80]) for line, g, e in zip(lines, got, expect) if g != e]
    assert not wrong, wrong[:5]
