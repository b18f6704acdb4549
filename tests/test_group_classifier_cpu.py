"""Banks of SDR classifiers (bithtm_amd/classifier.py ClassifierBankDefinition, SDRClassifierBank, htm_classifiers_*,
htm_set_group_run_active_cells, htm_classifiers_tick) -- what holds without a GPU: the path every case of
tests/group_classifier_cases.py names, the bank definition against n one-stream definitions, over split calls and with shared weights,
the model-level hit rates on the oracle's states, the C ABI's declarations and binding, the refusals, the compiler's report, the
launches of a classified tick, a classified group run and a bank update (the host code built host-only against
tests/host_stub/hip_stub_runtime.cpp), and the host code under ASan + UBSan as a stand-alone program
(tests/host_stub/group_classifier_host.cpp), which also evaluates the kernels' member-indexing arithmetic on the host."""
import ctypes as C
import json
import os
import re
import subprocess
import sys

import numpy as np
import pytest

import group_classifier_cases as G
from classifier_cases import CHUNK, MODEL_SEQUENCE, MODEL_STEPS, PAIRS, SPLITS, SPLIT_IDS, hit_rate
from test_likelihood_cpu import CLANG_DIR, HEADER, ROOT, _host_objects, _kernel, _launch, needs_hipcc

KERNELS = os.path.join(ROOT, "bithtm_amd", "csrc", "htm_classifier.h")
ABI = {"htm_classifiers_create": "htm_handle *h", "htm_classifiers_update": "htm_classifier *clf", "htm_classifiers_reset": "htm_classifier *clf",
       "htm_classifiers_read_weights": "htm_classifier *clf", "htm_classifiers_write_weights": "htm_classifier *clf",
       "htm_classifiers_state_bytes": "const htm_classifier *clf", "htm_classifiers_export": "htm_classifier *clf",
       "htm_classifiers_import": "htm_classifier *clf", "htm_classifiers_tick": "htm_group *g"}


# ---- the cases and the definition
def test_every_case_reaches_the_path_it_names():
    blocks = lambda n: -(-n // PAIRS)
    pads = lambda b: (b + 3) & ~3
    # mixed gates: by census, ONE step holds a learning member, a member with a missing target that is reset at this step, and a member
    # whose history is shorter than the longer horizon after its own reset; three blocks per (member, horizon)
    p = G.MIXED
    index, words, targets, resets = G.mixed_stream()
    assert index.shape == (3, G.MIXED_T, 7) and p["steps"] == (0, 2) and blocks(p["max_pairs"]) == 3 and p["buckets"] == 3
    census = G.gates(p, targets, resets, G.MIXED_STEP)
    assert census[0][0] >= 2 and census[0][1] == (True, True) and not resets[0, G.MIXED_STEP]
    assert targets[1, G.MIXED_STEP] < 0 and resets[1, G.MIXED_STEP] and census[1] == (0, (False, False))
    assert resets[2, G.MIXED_STEP - 1] and not resets[2, G.MIXED_STEP] and census[2] == (1, (True, False))
    # ... and the gates show in the definition: member 1's count is 1 behind the step, member 2 learned at horizon 0 only
    singles = [G.definition(p) for _ in range(3)]
    for i, d in enumerate(singles):
        d.update(index[i, :G.MIXED_STEP], words[i, :G.MIXED_STEP], targets[i, :G.MIXED_STEP], resets[i, :G.MIXED_STEP])
    before = [d.dense_weights() for d in singles]
    for i, d in enumerate(singles):
        d.update(index[i, G.MIXED_STEP:G.MIXED_STEP + 1], words[i, G.MIXED_STEP:G.MIXED_STEP + 1], targets[i, G.MIXED_STEP:G.MIXED_STEP + 1],
                 resets[i, G.MIXED_STEP:G.MIXED_STEP + 1])
    after = [d.dense_weights() for d in singles]
    changed = [[not np.array_equal(a[h], b[h]) for h in range(2)] for a, b in zip(before, after)]
    assert changed == [[True, True], [False, False], [True, False]] and [d.count for d in singles] == [census[0][0] + 1, 1, 2]
    # the banked cases
    by_name = {b[0]: b for b in G.BANKS}
    _, p, n, args, _ = by_name["wide"]
    assert (n, p["buckets"], p["cell_dim"], len(p["steps"])) == (2, 1024, 64, 1) and pads(1024) // 256 == 4 and (p["cell_dim"] + 31) // 32 == 2
    assert (G.banked("wide")[2][1] == 0xFFFFFFFF).any()
    _, p, n, args, _ = by_name["narrow"]
    assert (n, p["buckets"], p["cell_dim"], p["max_pairs"]) == (7, 1, 4, 1) and pads(1) == 4
    _, p, n, args, _ = by_name["three-h015"]
    index, words, targets, resets = G.banked("three-h015")[2]
    assert n == 3 and len(p["steps"]) == 3 and blocks(p["max_pairs"]) == 2 and resets.any() and not np.array_equal(resets[0], resets[1])
    for name in G.BANK_IDS:                          # (neighbours differ: a member reading another's rows would show)
        index, words, targets, _ = G.banked(name)[2]
        assert not np.array_equal(index[0], index[1]) or not np.array_equal(words[0], words[1]), name
    # frozen chunks
    H = len(G.FROZEN_BANK["steps"])
    assert (G.FROZEN_N, H, G.FROZEN_BANK["max_pairs"]) == (16, 8, 1) and G.chunk_steps(16, 8) == 511 and G.FROZEN_T == 512 > 511
    assert G.FROZEN_BANK["steps"][-1] + 1 == 65 and G.chunk_steps(1, 8) == CHUNK and G.FROZEN_ONE_STEPS == [1, CHUNK, CHUNK + 1]
    kernels = open(KERNELS).read()
    assert "65535 / (n * H)" in kernels and int(re.search(r"#define HTM_CLASSIFIER_CHUNK (\d+)", kernels).group(1)) == CHUNK
    (_, _, _, lr), (_, _, _, fr) = G.frozen_stream(G.FROZEN_N, G.FROZEN_T)
    assert fr.any() and not np.array_equal(fr[0], fr[1])
    # splits: those of the one-stream cases, one with an empty call; shared: four streams, a table that is not zero
    assert any(0 in sp for _, sp in SPLITS) and all(G.split_bank(name)[1][0].shape[:2] == (3, sum(sp)) for name, sp in SPLITS)
    w, (index, words, targets, resets) = G.shared_case()
    assert index.shape[0] == G.SHARED_N == 4 and w.any() and w.shape == (2, 320, 8)
    # the model level
    assert G.GROUP_SIZES == [1, 2, 7] and [G.member_missing(i) for i in range(7)] == [False, False, True, False, False, True, False]
    assert np.isnan(G.member_values(2, True)[7, 0]) and G.member_values(3)[:, 0].tolist() == np.roll(MODEL_SEQUENCE, -3).tolist()


@pytest.mark.parametrize("name", ["mixed-gates"] + G.BANK_IDS)
def test_the_bank_definition_equals_one_definition_per_stream(name):
    p, n, (index, words, targets, resets) = (G.MIXED, 3, G.mixed_stream()) if name == "mixed-gates" else G.banked(name)
    best, dist, bank = G.run_bank_definition(p, index, words, targets, resets)
    want_best, want_dist, singles = G.run_singles(p, index, words, targets, resets)
    assert np.array_equal(best, want_best) and np.array_equal(dist, want_dist)
    assert bank.total == index.shape[1] and bank.counts == [d.count for d in singles]
    assert np.array_equal(bank.dense_weights(), np.stack([d.dense_weights() for d in singles]))
    assert np.array_equal(bank.ring_arrays(p["max_pairs"]), np.stack([d.ring_arrays(p["max_pairs"]) for d in singles]))


@pytest.mark.parametrize("name,splits", SPLITS, ids=SPLIT_IDS)
def test_the_bank_definition_over_split_calls_equals_one_call(name, splits):
    p, (index, words, targets, resets) = G.split_bank(name)
    whole = G.run_bank_definition(p, index, words, targets, resets)
    cut = G.run_bank_definition(p, index, words, targets, resets, splits=splits)
    assert np.array_equal(whole[0], cut[0]) and np.array_equal(whole[1], cut[1])
    a, b = whole[2], cut[2]
    assert np.array_equal(a.dense_weights(), b.dense_weights()) and (a.counts, a.total) == (b.counts, b.total)
    assert np.array_equal(a.ring_arrays(p["max_pairs"]), b.ring_arrays(p["max_pairs"]))


def test_the_shared_definition_reads_one_table_and_refuses_learning():
    from bithtm_amd.classifier import ClassifierBankDefinition
    p = G.SHARED
    w, (index, words, targets, resets) = G.shared_case()
    owner = G.definition(p)
    owner.load_dense_weights(w)
    bank = G.bank_definition(p, G.SHARED_N, shared=True, table=owner)
    with pytest.raises(ValueError, match="learning is refused"):
        bank.update(index, words, targets, resets)
    best, dist = bank.update(index, words, targets, resets, learning=False)
    want_best, want_dist, singles = G.run_singles(p, index, words, targets, resets, learning=False, weights=[w] * G.SHARED_N)
    assert np.array_equal(best, want_best) and np.array_equal(dist, want_dist)
    assert bank.counts == [d.count for d in singles] and bank.total == G.SHARED_T and np.array_equal(owner.dense_weights(), w)
    assert np.array_equal(bank.ring_arrays(p["max_pairs"]), np.stack([d.ring_arrays(p["max_pairs"]) for d in singles]))
    bank.reset([True, False, False, True])
    assert bank.counts == [0, singles[1].count, singles[2].count, 0]
    # the owner learns on: the bank reads the new table
    one = G.stream(p, 4, 7, seed=5)
    owner.update(one[0], one[1], one[2])
    w2 = owner.dense_weights()
    assert not np.array_equal(w2, w)
    _, dist2 = bank.update(index, words, targets, None, learning=False)
    assert np.array_equal(dist2, G.run_singles(p, index, words, targets, None, learning=False, weights=[w2] * G.SHARED_N)[1])
    for bad in (dict(streams=0), dict(weights="both"), dict(table=owner)):
        with pytest.raises(ValueError):
            ClassifierBankDefinition(**dict(dict(streams=2, buckets=3), **bad))
    with pytest.raises(ValueError, match="another config"):
        G.bank_definition(dict(p, buckets=9), 2, shared=True, table=owner)


@pytest.mark.parametrize("name", ["128x4", "128x64"])
def test_the_group_hit_rates_on_the_oracles_states_are_the_recorded_floors(name):
    """The definition over the oracle's states, member by member, on the CPU: the numbers written beside the cases (the GPU test holds the
    device's records to these same streams, bit for bit)."""
    assert len(G.GROUP_HIT_RATE[name]) == max(G.GROUP_SIZES) == 7
    for i in range(max(G.GROUP_SIZES)):
        best, dist, targets = G.group_model_stream(name, i, G.member_missing(i))
        rates = tuple(hit_rate(best, targets, j, h, len(MODEL_SEQUENCE)) for j, h in enumerate(MODEL_STEPS))
        print(name, "member", i, "hit rates per horizon", rates)
        assert rates == G.GROUP_HIT_RATE[name][i], i
        assert rates == ((0.9, 0.9) if G.member_missing(i) else (1.0, 1.0))         # (the NaN row is never a hit)


# ---- the C ABI
def test_the_header_declares_the_bank_abi_and_the_binding_matches_it():
    from bithtm_amd import _lib as L
    header = open(HEADER).read()
    decl = {m.group(1): m.group(2) for m in re.finditer(r"\b(htm_classifiers_[a-z_]+)\s*\(([^)]*)\)\s*;", header)}
    assert set(decl) == set(ABI)
    for name, params in decl.items():
        assert params.split(",")[0].strip() == ABI[name], (name, params)
        assert len(L.EXPORTS[name][1]) == len(params.split(",")), name
    assert L.EXPORTS["htm_classifiers_state_bytes"][0] is C.c_int64 and all(L.EXPORTS[n][0] is C.c_int for n in ABI if n != "htm_classifiers_state_bytes")
    clean = lambda params: [re.sub(r"\s+", " ", x.strip()) for x in params.split(",")]
    assert clean(decl["htm_classifiers_create"]) == ["htm_handle *h", "const htm_classifier_config *cfg", "const int32_t *exp_table2049", "int32_t n_streams",
                                                     "htm_classifier *share_weights_of", "htm_classifier **out"]
    assert clean(decl["htm_classifiers_update"]) == [
        "htm_classifier *clf", "htm_handle *h", "const void *const *device_pairs", "int32_t pairs_per_step", "int32_t n_steps", "const int32_t *const *device_targets",
        "int32_t n_targets", "int32_t first_step", "const uint32_t *const *device_reset_bits", "int32_t learn", "int32_t *device_best", "int32_t *device_dist"]
    # the classified tick is the scored tick's arguments and five more
    scored = clean(re.search(r"\bhtm_likelihood_tick\s*\(([^)]*)\)\s*;", header).group(1))
    tick = clean(decl["htm_classifiers_tick"])
    assert tick[:-5] == scored and tick[-5:] == ["htm_classifier *clf", "const int32_t *targets", "int32_t learn", "int32_t *best", "int32_t *dist"]
    assert L.EXPORTS["htm_classifiers_tick"][1][:-5] == L.EXPORTS["htm_likelihood_tick"][1]
    cap = re.search(r"\bhtm_set_group_run_active_cells\s*\(([^)]*)\)\s*;", header).group(1)
    assert clean(cap) == ["htm_group *g", "void *const *device_pairs"] and len(L.EXPORTS["htm_set_group_run_active_cells"][1]) == 2
    assert L.ABI_VERSION == 4 and re.search(r"#define BITHTM_ABI_VERSION 4\b", header)


def test_the_c_calls_refuse_null_arguments_without_a_gpu():
    from bithtm_amd import _lib as L
    from bithtm_amd.classifier import EXP_TABLE
    lib = L.load()
    cfg = L.HtmClassifierConfig(C.sizeof(L.HtmClassifierConfig), 3, 1, 655, 64, 32, 4, (C.c_int32 * 8)(1))
    out = C.c_void_p(1)
    assert lib.htm_classifiers_create(None, C.byref(cfg), EXP_TABLE.ctypes.data_as(C.c_void_p), 3, None, C.byref(out)) == -1 and not out.value
    assert b"null" in lib.htm_last_error(None)
    assert lib.htm_classifiers_update(None, None, None, 1, 1, None, 1, 0, None, 1, None, None) == -1
    assert lib.htm_classifiers_reset(None, None, None) == -1
    assert lib.htm_classifiers_read_weights(None, None, 0, 0, 0, 1, None) == -1 and lib.htm_classifiers_write_weights(None, None, 0, 0, 0, 1, None) == -1
    assert lib.htm_classifiers_export(None, None, None, 0) == -1 and lib.htm_classifiers_import(None, None, None, 0) == -1
    assert lib.htm_classifiers_state_bytes(None) == -1
    assert lib.htm_set_group_run_active_cells(None, None) == -1
    assert lib.htm_classifiers_tick(None, None, None, 0, None, None, 0, 0, None, None, None, None, None, None, None, 0, None, None) == -1


def test_the_python_layer_refuses_before_any_library_call():
    import bithtm_amd as B
    for bad in (dict(streams=0, buckets=3), dict(streams=65535 // 2 + 1, buckets=3, steps=(0, 1)), dict(streams=2), dict(streams=2, buckets=0),
                dict(streams=2, buckets=3, field=B.ScalarField(0, 1, 16, 3)), dict(streams=2, buckets=3, shape=(10, 65, 4))):
        with pytest.raises(ValueError):
            B.SDRClassifierBank(**bad)
    assert B.SDRClassifierBank(65535 // 2, buckets=3, steps=(0, 1)).streams == 32767
    field = B.ScalarField(0.0, 100.0, 64, 9)
    bank = B.SDRClassifierBank(2, field=field, steps=(0, 2), shape=(10, 5, 4))
    assert (bank.buckets, bank.streams, bank.ring_len, bank.units) == (56, 2, 3, 50) and bank.source is None
    ok = (np.array([[[0, 1, 2, -1]]] * 2), np.array([[[1, 2, 4, 0xFFFFFFFF]]] * 2, dtype=np.uint32), [[0], [55]])
    for index, words, targets, match in (
            (ok[0][:1], ok[1][:1], ok[2][:1], r"index int \[2, T, n\]"), (ok[0][0], ok[1][0], ok[2], r"index int \[2, T, n\]"),
            (np.array([[[0, 1, 1, 3]]] * 2), np.array([[[1, 2, 4, 1]]] * 2, dtype=np.uint32), ok[2], "twice"), (ok[0], np.array([[[1, 2, 32, 0]]] * 2, dtype=np.uint32), ok[2], "cell_dim"),
            (ok[0], ok[1], [[0], [56]], "at or above buckets"), (ok[0], ok[1], [0, 1], r"int \[2, n\]"), (ok[0], ok[1], [[0, 1], [0, 1]], r"int \[2, 1\]"),
            (np.zeros((2, 1, 5), int) + np.arange(5), np.ones((2, 1, 5), np.uint32), ok[2], "max_pairs")):
        with pytest.raises(ValueError, match=match):
            bank.update_patterns(index, words, targets)
    with pytest.raises(ValueError, match=r"bool \[2, 1\]"):
        bank.update_patterns(*ok, resets=[0, 1])
    with pytest.raises(RuntimeError, match="not bound"):
        bank.update_patterns(*ok)
    with pytest.raises(RuntimeError, match="shape"):
        B.SDRClassifierBank(2, buckets=3).update_patterns(*ok)
    with pytest.raises(ValueError, match=r"bool \[2\]"):
        bank.reset([True])
    # an unbound bank holds a loaded state until it is bound
    state = bank.state_dict()
    assert int(state["total"]) == 0 and state["count"].tolist() == [0, 0] and state["ring"].shape == (2, 3, 4, 2) and state["weights"].shape == (2, 2, 50, 56)
    assert (state["ring"][..., 0] == -1).all() and state["params"].tolist() == [2, 56, 66, 10, 5, 4, 0, 2]
    state["total"], state["count"] = np.int64(9), np.array([4, 9])
    state["weights"][1, 1, 7, :3] = (5, -5, 1 << 30)
    bank.load_state_dict(state)
    again = bank.state_dict()
    assert all(np.array_equal(again[k], state[k]) for k in state)
    bank.reset([False, True])
    assert bank.state_dict()["count"].tolist() == [4, 0] and int(bank.state_dict()["total"]) == 9
    bank.reset()
    assert bank.state_dict()["count"].tolist() == [0, 0]
    with pytest.raises(ValueError, match="parameters"):
        B.SDRClassifierBank(3, field=field, steps=(0, 2), shape=(10, 5, 4)).load_state_dict(state)
    for key, value, match in (("count", np.array([10, 0]), "count"), ("count", np.array([-1, 0]), "count"), ("count", np.array([1]), "count"),
                              ("ring", state["ring"][:1], "ring"), ("weights", state["weights"][:1], "weights")):
        with pytest.raises(ValueError, match=match):
            bank.load_state_dict(dict(state, **{key: value}))
    # shared(): a bound one-stream classifier, and no learning
    clf = B.SDRClassifier(buckets=3, shape=(10, 5, 4))
    with pytest.raises(ValueError, match="not bound"):
        B.SDRClassifierBank.shared(clf, 2)
    with pytest.raises(ValueError, match="one-stream"):
        B.SDRClassifierBank.shared(bank, 2)
    # the calls a bank does not ride on refuse it before anything else, with the message of the one-stream classifier; a one-stream
    # classifier on a group call is refused as before
    tm, sp = B.TemporalMemory(64, 4), B.SpatialPooler(32, 64, 4)
    for call in (lambda: tm.run(np.zeros((1, 4), int), 1, classifier=bank), lambda: sp.run(np.zeros((1, 32), bool), 1, classifier=bank)):
        with pytest.raises(ValueError, match="classifier= is not available here"):
            call()
    for method, positional in ((B.HierarchicalTemporalMemory.lookahead, 4), (B.HierarchicalTemporalMemory.forecast, 2), (B.HierarchicalTemporalMemory.run, 3)):
        with pytest.raises(ValueError, match="classifier= is not available here"):
            method(*[None] * positional, classifier=bank)
    for method, positional in ((B.ModelGroup.run, 3), (B.ModelGroup.tick, 2)):
        with pytest.raises(ValueError, match="classifier= is not available here"):
            method(*[None] * positional, classifier=clf)


def test_group_tick_carries_the_classification():
    import bithtm_amd as B
    from bithtm_amd import _lib as L
    from bithtm_amd.group import GroupTick
    rows = np.zeros(2, dtype=L.HtmLiveRow)
    tick = GroupTick(rows)
    assert tick.classified_bucket is None and tick.classified_probability is None and tick.classified_value is None and tick.class_distribution is None
    pairs = np.array([[[3, 65536], [0, 16384]], [[55, 1], [0, 0]]], dtype=np.int32)
    field = B.ScalarField(0.0, 100.0, 64, 9)
    tick = GroupTick(rows, classified=pairs, classified_field=field, class_distribution=np.zeros((2, 2, 56), np.int32))
    assert tick.classified_bucket.tolist() == [[3, 0], [55, 0]] and tick.classified_probability.tolist() == [[1.0, 0.25], [1 / 65536, 0.0]]
    assert np.array_equal(tick.classified_value, field.value_of(tick.classified_bucket)) and tick.class_distribution.shape == (2, 2, 56)


# ---- the compiler's report
def test_the_new_kernels_have_no_scratch_and_the_existing_ones_keep_their_figures():
    from bithtm_amd.build import kernel_resources
    res = kernel_resources()
    if res is None:
        pytest.skip("the library in the tree was not built here")
    new = {re.match(r"_Z\d+(kgcls_[a-z]+)", k).group(1): v for k, v in res.items() if re.match(r"_Z\d+kgcls_", k)}
    assert sorted(new) == ["kgcls_apply", "kgcls_capture", "kgcls_frozen", "kgcls_reset", "kgcls_sum"], sorted(new)
    solo = {re.match(r"_Z\d+(kcls_[a-z]+)", k).group(1): v for k, v in res.items() if re.match(r"_Z\d+kcls_", k)}
    for name, r in new.items():
        print(name, r)
        assert r["scratch_bytes_per_lane"] == 0 and r["occupancy"] >= 4, (name, r)
    # the LDS of a twin is no larger than its solo kernel's
    assert solo["kcls_sum"]["lds_bytes"] == 20560 and solo["kcls_frozen"]["lds_bytes"] == 12368
    for twin in ("sum", "apply", "frozen", "capture"):
        assert new["kgcls_" + twin]["lds_bytes"] <= solo["kcls_" + twin]["lds_bytes"], twin
    # every kernel that existed before the bank was added: the figures the compiler gave it then.  The fixture is
    # bithtm_amd/libbithtm_hip.resources.json of a build of the commit before the bank, copied as it is.
    with open(os.path.join(ROOT, "tests", "golden", "kernel_resources_before_group_classifier.json")) as f:
        before = json.load(f)
    assert len(before) > 100 and not [k for k in before if "kgcls_" in k] and len([k for k in before if "kcls_" in k]) == 4
    changed = {k: (before[k], res.get(k)) for k in before if before[k] != res.get(k)}
    assert not changed, changed
    assert set(res) - set(before) == {k for k in res if "kgcls_" in k}


# ---- the launch traces
@pytest.fixture(scope="module")
def traces(tmp_path_factory):
    tmp = str(tmp_path_factory.mktemp("group_classifier_trace"))
    obj, stub, defsym = _host_objects(tmp)
    lib = os.path.join(tmp, "libbithtm_host_trace.so")
    subprocess.run([os.path.join(CLANG_DIR, "bin", "clang++"), "-shared", obj, stub, "-ldl", "-o", lib] + defsym, check=True, capture_output=True)
    env = dict(os.environ, BITHTM_LIBRARY=lib, BITHTM_STUB_TRACE=os.path.join(tmp, "trace.txt"))
    for name in ("LD_PRELOAD", "BITHTM_LEAN", "BITHTM_SCAN_LARGE"):
        env.pop(name, None)
    r = subprocess.run([sys.executable, os.path.join(ROOT, "tests", "host_stub", "group_classifier_driver.py")], env=env, capture_output=True, text=True,
                       timeout=900)
    assert r.returncode == 0, (r.stdout + r.stderr)[-4000:]
    return json.loads(r.stdout.splitlines()[-1])


def _kernels(lines):
    return [_kernel(x) for x in lines if x.startswith("launch ")]


def _copies(lines):
    return [int(x.split()[1]) for x in lines if x.startswith("memcpy ")]


@needs_hipcc
def test_the_calls_that_existed_launch_and_copy_exactly_what_they_did(traces):
    """Plain and scored ticks at B = 1 and 7, plain and recorded group runs, the recorded run from graphs: line for line the traces of
    the commit before the bank (the fixture), and the same again on groups that have just made classified calls."""
    with open(os.path.join(ROOT, "tests", "golden", "group_classifier_traces_before.json")) as f:
        before = json.load(f)
    assert sorted(before) == ["B=1", "B=7", "graphs"] and "graph_launch" in before["graphs"]
    assert traces["before"] == before
    assert not [x for leg in before.values() for lines in (leg.values() if isinstance(leg, dict) else [leg]) for x in lines if "cls" in x]
    for n in (1, 7):
        assert traces["tick"][f"B={n}"]["plain after"] == before[f"B={n}"]["tick"]
        assert traces["run"][f"B={n}"]["recorded after"] == before[f"B={n}"]["recorded run"]
    assert traces["graphs"]["recorded"] == before["graphs"]


@needs_hipcc
def test_a_classified_tick_adds_capture_and_two_or_one_launches_at_every_group_size(traces):
    H = 2
    for n in (1, 7):
        plain, scored = traces["before"][f"B={n}"]["tick"], traces["before"][f"B={n}"]["scored tick"]
        leg = traces["tick"][f"B={n}"]
        for kind, base, added in (("learning", plain, ["kgcls_sum", "kgcls_apply"]), ("frozen", plain, ["kgcls_frozen"]),
                                  ("scored learning", scored, ["kgcls_sum", "kgcls_apply"])):
            lines = leg[kind]
            # still one copy in and one copy out, with the targets (4 bytes a member) and the classification riding in them
            assert [x.split()[0] for x in lines if not x.startswith("launch ")] == ["memcpy", "memcpy"] and lines[0].startswith("memcpy") and lines[-1].startswith("memcpy")
            assert _copies(lines)[0] == _copies(base)[0] + 4 * n
            assert _copies(lines)[1] == _copies(base)[1] + n * H * 2 * 4 + (0 if kind.startswith("scored") else 8 * n)    # (unscored: the gap of the likelihoods)
            ks, kb = _kernels(lines), _kernels(base)
            at = ks.index("kgcls_capture")
            assert ks[at - 1] == "kgrp_rec_step" and _launch(lines[1 + at]) == ("kgcls_capture", 1, n, 256, 0)
            tail = len(added)
            assert ks[:at] + ks[at + 1:-tail] == kb and ks[-tail:] == added, (kind, ks)
            assert len(ks) == len(kb) + 1 + tail
            for x in lines[-1 - tail:-1]:             # (16 pairs a step: one block; member and horizon on grid y)
                assert _launch(x)[1:] == (1, n * H, 256, 0), x
            assert [x for x in lines if x.startswith("launch ") and "cls" not in x] == [x for x in base if x.startswith("launch ")]
        packed = leg["packed frozen"]
        assert _kernels(packed)[-1] == "kgcls_frozen" and _kernels(packed).count("kgcls_capture") == 1 and len(_copies(packed)) == 2
    # ... whatever B is
    for kind in ("learning", "frozen", "scored learning", "packed frozen"):
        assert _kernels(traces["tick"]["B=1"][kind]) == _kernels(traces["tick"]["B=7"][kind]), kind


def _batches_of(lines):
    """A classified run's trace cut at its recorded group runs -> per batch (steps, the lines behind the last step's launches)."""
    starts = [i for i, x in enumerate(lines) if _kernel(x) == "kgrp_rec_clear"] + [len(lines)]
    return [lines[a:b] for a, b in zip(starts, starts[1:])]


@needs_hipcc
def test_a_classified_group_run_adds_one_capture_per_step_and_one_update_per_batch(traces):
    H = 2
    for n in (1, 7):
        recorded = traces["before"][f"B={n}"]["recorded run"]
        leg = traces["run"][f"B={n}"]
        for kind in ("learning", "frozen", "long frozen"):
            lines = leg[kind]
            ks = _kernels(lines)
            captures = [i for i, k in enumerate(ks) if k == "kgcls_capture"]
            steps = ks.count("kgrp_rec_step")
            assert steps == (6 if kind != "long frozen" else 2 * G.chunk_steps(n, H) + 3)
            assert len(captures) == steps and all(ks[i - 1] == "kgrp_rec_step" for i in captures)
            assert all(_launch(x)[1:] == (1, n, 256, 0) for x in lines if _kernel(x) == "kgcls_capture")
            for batch in _batches_of(lines):
                bk = _kernels(batch)
                t = bk.count("kgrp_rec_step")
                update = [k for k in bk if k in ("kgcls_sum", "kgcls_apply", "kgcls_frozen")]
                if kind == "learning":
                    assert update == ["kgcls_sum", "kgcls_apply"] * t          # (2 x n launches a batch of n steps, whatever B is)
                else:
                    assert update == ["kgcls_frozen"] * -(-t // G.chunk_steps(n, H))
                assert bk[-len(update):] == update                              # (behind the run, in front of the read-back)
                for x in batch:
                    if _kernel(x) in ("kgcls_sum", "kgcls_apply"):
                        assert _launch(x)[1:] == (1, n * H, 256, 0), x
            if kind != "long frozen":
                # without the bank's launches and copies the run is the recorded run it was; the copies: the capture table (8 bytes a
                # member) in front, the update's pointer table (2 x 8 bytes a member; one member: by value) behind
                assert [x for x in lines if x.startswith("launch ") and "cls" not in x] == [x for x in recorded if x.startswith("launch ")]
                extra = sorted(_copies(lines))
                for c in _copies(recorded):
                    extra.remove(c)
                assert extra == sorted([8 * n] + ([3 * 8 * n] if n > 1 else [])), (n, kind, extra)
    for kind in ("learning", "frozen"):
        assert _kernels(traces["run"]["B=1"][kind]) == _kernels(traces["run"]["B=7"][kind]), kind
    # from graphs: the captures are inside the graphs, the same replays as the recorded run
    classified, recorded = traces["graphs"]["classified"], traces["graphs"]["recorded"]
    assert classified.count("graph_launch") == recorded.count("graph_launch") >= 1 and "kgcls_capture" not in _kernels(classified)
    assert [k for k in _kernels(classified) if k not in _kernels(recorded)] == ["kgcls_sum", "kgcls_apply"] * 6


@needs_hipcc
def test_a_bank_update_is_the_launches_of_one_stream_with_the_member_on_grid_y(traces):
    H = 3
    for n in (1, 4):
        leg = traces["update"][f"n={n}"]
        chunk = G.chunk_steps(n, H)
        frozen = [x for x in leg["frozen"] if x.startswith("launch ")]
        assert [_launch(x) for x in frozen] == [("kgcls_frozen", 2, n * chunk * H, 256, 0), ("kgcls_frozen", 2, n * 1 * H, 256, 0)], frozen
        learning = [x for x in leg["learning"] if x.startswith("launch ")]
        assert [_launch(x) for x in learning] == [("kgcls_sum", 3, n * H, 256, 0), ("kgcls_apply", 3, n * H, 256, 0)] * 3, learning
        # one copy of the pointer table per call (three pointers a stream); one stream: by value, no copy
        for kind in ("frozen", "learning"):
            assert _copies(leg[kind]) == ([3 * 8 * n] if n > 1 else []), (n, kind, _copies(leg[kind]))
    # the Python refusals enqueue nothing
    assert traces["refused_lines"] == [] and all(traces["refused"].values()), traces["refused"]
    assert "2 streams" in traces["refused"]["run: streams"] and "not available here" in traces["refused"]["tick: plain classifier"]
    assert "shape" in traces["refused"]["tick: another shape"] and "at or above buckets" in traces["refused"]["run: targets above"]


# ---- the host code under ASan + UBSan, as a stand-alone program, and the kernels' member indexing on the host
def _arithmetic_cases():
    """The lines of the case file and, per line, what the layout of the definition gives (strings as the program prints them)."""
    rng = np.random.default_rng(6)
    lines, expect = [], []
    for n, H in [(1, 1), (1, 8), (3, 2), (7, 1), (16, 8), (8191, 8), (65535, 1), (100, 3)] + [(int(a), int(b)) for a, b in zip(rng.integers(1, 2000, 12), rng.integers(1, 9, 12))]:
        lines.append(f"c {n} {H}")
        chunk = min(CHUNK, 65535 // (n * H))
        expect.append(str(chunk))
        assert 1 <= chunk and n * chunk * H <= 65535
        for m, h in {(0, 0), (n - 1, H - 1), (n // 2, H // 2)}:
            y = m * H + h
            lines += [f"y {y} {H}", f"r {m} {H} {h}", f"o {m} {chunk} {H}"]
            expect += [f"{m} {h}", str(m * H + h), str(m * chunk * H)]
            for step in {0, chunk - 1, chunk // 2}:
                lines.append(f"f {(m * chunk + step) * H + h} {H} {chunk}")
                expect.append(f"{m} {step} {h}")
    return lines, expect


@needs_hipcc
def test_the_host_code_runs_clean_under_asan_and_ubsan_and_the_member_indexing_equals_the_layout(tmp_path):
    """tests/host_stub/group_classifier_host.cpp and htm_engine.hip (host-only), both with -fsanitize=address,undefined, linked against
    the stub runtime into ONE program that is run directly: nothing is preloaded."""
    tmp = str(tmp_path)
    san = ["-fsanitize=address,undefined", "-fno-sanitize-recover=undefined"]
    obj, stub, defsym = _host_objects(tmp, san)
    clang = os.path.join(CLANG_DIR, "bin", "clang++")
    exe = os.path.join(tmp, "group_classifier_host")
    subprocess.run([clang, "-std=c++17", "-O1", "-g", "-fno-omit-frame-pointer", "-ffp-contract=off"] + san +
                   [os.path.join(ROOT, "tests", "host_stub", "group_classifier_host.cpp"), obj, stub, "-ldl", "-o", exe] + defsym, check=True, capture_output=True)
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
    assert len(got) == len(expect) > 100
    wrong = [(line, g, e) for line, g, e in zip(lines, got, expect) if g != e]
    assert not wrong, wrong[:5]
