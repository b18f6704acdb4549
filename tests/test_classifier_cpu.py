"""SDR classifier (bithtm_amd/classifier.py, SDRClassifier, htm_classifier_*, htm_set_run_active_cells) -- what holds
without a GPU: a hand-computed stream of the definition, the exp table's derived error bound, the path every case of
tests/classifier_cases.py names, the definition over split calls, its behaviour on periodic patterns and on the oracle's states, the C
ABI's declarations and binding, the refusals, the compiler's report for the new kernels, the launches of an update and of a classified
run (the host code built host-only against tests/host_stub/hip_stub_runtime.cpp), and the host code under ASan + UBSan as a stand-alone
program (tests/host_stub/classifier_host.cpp), which also evaluates the kernel header's arithmetic on the host against the definition."""
import ctypes as C
import json
import math
import os
import re
import subprocess
import sys

import numpy as np
import pytest

import classifier_cases as cases
from classifier_cases import CHUNK, PAIRS, SPLITS, SPLIT_IDS, STREAMS, STREAM_IDS
from test_likelihood_cpu import CLANG_DIR, HEADER, ROOT, _host_objects, _kernel, _launch, needs_hipcc

KERNELS = os.path.join(ROOT, "bithtm_amd", "csrc", "htm_classifier.h")
ABI = {"htm_classifier_create": "htm_handle *h", "htm_classifier_destroy": "htm_classifier *clf", "htm_classifier_update": "htm_classifier *clf",
       "htm_classifier_reset": "htm_classifier *clf", "htm_classifier_read_weights": "htm_classifier *clf",
       "htm_classifier_write_weights": "htm_classifier *clf", "htm_classifier_state_bytes": "const htm_classifier *clf",
       "htm_classifier_export": "htm_classifier *clf", "htm_classifier_import": "htm_classifier *clf"}


# ---- the definition
def test_a_hand_computed_two_bucket_three_step_stream():
    """Two buckets, horizons (0, 1), alpha_q = 16384 (0.25), cell_dim 4.  Step 0: P0 = units {0, 1}, target 0; all weights 0, so p =
    (32768, 32768) and horizon 0 moves both units by 16384 * (65536 - 32768) >> 16 = +8192 and -8192; horizon 1 has no P_(-1).
    Step 1: P1 = unit {4}, target 1: horizon 0 moves unit 4 by (-8192, +8192); horizon 1 learns P0 -> bucket 1: (-8192, +8192) on
    units 0, 1.  Step 2: P0 again: horizon 0 sees a = (16384, -16384), d = 32768 = 0.5: e = T[32] = round(2^30 exp(-0.5)), p0 =
    (2^30 << 16) // (2^30 + e) = 40793; horizon 1 sees a = (-16384, 16384): bucket 1 with the same p."""
    from bithtm_amd.classifier import EXP_TABLE, ClassifierDefinition
    d = ClassifierDefinition(2, (0, 1), alpha_q=16384, units=8, cell_dim=4)
    b0, q0 = d.step([(0, 0b11)], 0, distribution=True)
    assert b0 == [(0, 32768), (0, 32768)] and q0 == [[32768, 32768]] * 2
    assert d.weights == [{0: [8192, -8192], 1: [8192, -8192]}, {}]
    b1, _ = d.step([(1, 0b1)], 1)
    assert b1 == [(0, 32768), (0, 32768)]
    assert d.weights == [{0: [8192, -8192], 1: [8192, -8192], 4: [-8192, 8192]}, {0: [-8192, 8192], 1: [-8192, 8192]}]
    e = int(EXP_TABLE[32])
    assert e == round((1 << 30) * math.exp(-0.5)) and abs(e / (1 << 30) - math.exp(-0.5)) < 1e-9
    p_hi = ((1 << 30) << 16) // ((1 << 30) + e)
    assert p_hi == 40793 and abs(p_hi / 65536 - 1 / (1 + math.exp(-0.5))) < 2e-5
    b2, q2 = d.step([(0, 0b11)], 0, distribution=True)
    assert b2 == [(0, p_hi), (1, p_hi)]
    assert q2 == [[p_hi, (e << 16) // ((1 << 30) + e)], [(e << 16) // ((1 << 30) + e), p_hi]]
    # horizon 0 learned P0 -> 0 again: delta = 16384 * (65536 - 40793) >> 16 = 6185 and -(16384 * 24742 >> 16) = -6185
    assert (16384 * (65536 - p_hi)) >> 16 == 6185 and q2[0][1] == 24742 and (16384 * 24742) >> 16 == 6185
    assert d.weights[0][0] == [8192 + 6185, -8192 - 6185] and d.weights[0][1] == d.weights[0][0]
    # horizon 1 learned P1 = {4} -> 0 from zero weights
    assert d.weights[1][4] == [8192, -8192]
    assert (d.count, d.total) == (3, 3)


def test_the_exp_table_interpolates_exp_within_its_derived_bound():
    """Linear interpolation of exp(-x) with step h = 1/64: |error| <= h^2 / 8 * max |exp''| = (1/64)^2 / 8 = 3.0518e-5 (the second
    derivative peaks at x = 0 with 1), plus the rounding of the table entries (2^-31 each) and of the interpolation's shift (2^-30).
    Measured over the whole range on every d that is a multiple of 64, and on every d near the cut, against math.exp; e is monotone."""
    from bithtm_amd.classifier import EXP_CUTOFF, EXP_TABLE, exp_q30
    assert EXP_TABLE.shape == (2049,) and EXP_TABLE.dtype == np.int32 and EXP_TABLE[0] == 1 << 30
    assert all(int(EXP_TABLE[i]) == int(round((1 << 30) * math.exp(-i / 64.0))) for i in range(2049))
    bound = (1 / 64) ** 2 / 8 + 2.0 ** -31 + 2.0 ** -30
    assert 3.05e-5 < bound < 3.06e-5
    worst, last = 0.0, 1 << 30
    for d in list(range(0, EXP_CUTOFF, 64)) + list(range(EXP_CUTOFF - 2048, EXP_CUTOFF + 3)) + list(range(0, 4096)):
        e = exp_q30(d)
        worst = max(worst, abs(e / (1 << 30) - math.exp(-d / 65536.0)))
    for d in range(0, EXP_CUTOFF + 1024, 512):
        e = exp_q30(d)
        assert e <= last
        last = e
    print("measured interpolation error", worst, "derived bound", bound)
    assert worst <= bound
    assert exp_q30(EXP_CUTOFF) == 0 and exp_q30(1 << 40) == 0 and exp_q30(1023) > exp_q30(1024) > 0


def test_every_case_reaches_the_path_it_names():
    from bithtm_amd import _lib as L
    from bithtm_amd.classifier import EXP_CUTOFF, W_LIMIT, delta_of, exp_q30, softmax, units_of
    kernels = open(KERNELS).read()
    assert int(re.search(r"#define HTM_CLASSIFIER_CHUNK (\d+)", kernels).group(1)) == L.CLASSIFIER_CHUNK == CHUNK
    assert int(re.search(r"#define HTM_CLASSIFIER_PAIRS (\d+)", kernels).group(1)) == L.CLASSIFIER_PAIRS == PAIRS
    assert int(re.search(r"#define HTM_CLASSIFIER_THREADS (\d+)", kernels).group(1)) == 256           # (four waves)
    by_name = {s[0]: s for s in STREAMS}
    blocks = lambda n: -(-n // PAIRS)
    pads = lambda b: (b + 3) & ~3
    # buckets and padding
    assert sorted({s[1]["buckets"] for s in STREAMS}) == [1, 3, 8, 64, 65, 1024]
    assert pads(1) == 4 and pads(3) == 4 and pads(64) == 64 and pads(65) == 68 and pads(1024) == 1024 and 1024 // 256 == 4
    # horizons
    assert {(0,), (1,), (0, 1, 5), cases.EIGHT} <= {s[1]["steps"] for s in STREAMS} and cases.EIGHT[-1] == 64 and len(cases.EIGHT) == 8
    # pairs on either side of the wave and block boundaries, and several blocks
    counts = sorted({s[2]["n_pairs"] for s in STREAMS})
    assert {1, 3, 4, 5, 15, 16, 17, 33} <= set(counts)
    assert [blocks(n) for n in (15, 16, 17, 33)] == [1, 1, 2, 3] and blocks(by_name["narrow-call"][1]["max_pairs"]) == 3
    # geometry
    assert {s[1]["cell_dim"] for s in STREAMS} == {5, 32, 64}
    assert units_of([(3, 0b10001)], 5) == [15, 19] and units_of([(3, 1 << 31)], 64) == [64 + 32 + 31] and units_of([(2, 1)], 64) == [64]
    # the streams do what the cases say
    for name, p, args, why in STREAMS:
        index, words, targets, resets = cases.stream(p, **args)
        assert index.shape == (args["T"], args["n_pairs"]) and args["n_pairs"] <= p["max_pairs"], name
        live = (index >= 0) & (words != 0)
        assert live.any(axis=1).sum() >= args["T"] - 1, name
        wpc = (p["cell_dim"] + 31) // 32
        top = p["cell_dim"] - (index.astype(np.int64) % wpc) * 32
        assert not ((words.astype(np.int64) >> np.clip(top, 0, 32))[index >= 0] != 0).any(), name
    _, p, args, _ = by_name["B1024-blocks"]
    assert (cases.stream(p, **args)[1] == 0xFFFFFFFF).any()
    _, p, args, _ = by_name["B1-h0-K5"]
    assert cases.stream(p, **args)[1].max() < 32
    for name in ("B64-K64-h015", "h8-to-64"):
        p, (index, words, targets, resets) = cases.streamed(name)
        assert (resets.any() or name == "h8-to-64") and (targets < 0).any(), name
    # resets that empty the history before it is 5 deep: some step has a target, count < 5 and count >= 1
    p, (index, words, targets, resets) = cases.streamed("B64-K64-h015")
    count, seen = 0, set()
    for t in range(len(index)):
        count = 0 if resets[t] else count
        if targets[t] >= 0:
            seen.add(min(count, 5))
        count += 1
    assert seen == {0, 1, 2, 3, 4, 5} or {0, 1, 5} <= seen, seen
    # the long ring is learned from: horizon 64 has weights at the end
    p, (index, words, targets, resets) = cases.streamed("h8-to-64")
    d = cases.run_definition(p, index, words, targets, resets)[2]
    assert d.dense_weights()[7].any() and d.ring_len == 65
    # truncation toward zero, both signs: alpha_q = 1 gives |x| < 65536 -> 0 (a floor would give -1); alpha_q = 66 at p = 21845
    assert delta_of(1, [21845, 21845, 21846], 0) == [0, 0, 0] and (1 * -21845) >> 16 == -1
    assert delta_of(66, [21845, 21845, 21846], 0) == [44, -21, -22] and (66 * -21845) >> 16 == -22
    p, (index, words, targets, resets) = cases.streamed("alpha1")
    assert not cases.run_definition(p, index, words, targets, resets)[2].dense_weights().any()
    assert delta_of(65536, [0, 65536], 0) == [65536, -65536]
    # the clamp cases meet the clamp, one step each
    for sign in (1, -1):
        w, index, words, targets = cases.clamp_case(sign)
        d = cases.run_definition(cases.CLAMP, index, words, targets, weights=w)[2]
        row = d.dense_weights()[0, 0].tolist()
        assert row == ([W_LIMIT - 10 - 21845, W_LIMIT, W_LIMIT - 10 - 21845] if sign > 0 else [-W_LIMIT, -W_LIMIT + 10 + 43691, -W_LIMIT]), row
    # the d edges
    assert cases.D_EDGES == [1023, 1024, (32 << 16) - 1, 32 << 16] and EXP_CUTOFF == 32 << 16
    w, index, words, targets = cases.edge_case()
    best, dist, d = cases.run_definition(cases.EDGES, index, words, targets, learning=False, weights=w)
    for i, dd in enumerate(cases.D_EDGES):
        assert dist[i, 0].tolist() == softmax([0, -dd]) and dist[i, 0, 1] == (exp_q30(dd) << 16) // ((1 << 30) + exp_q30(dd))
    assert exp_q30(1023) > exp_q30(1024) and dist[0, 0, 1] >= dist[1, 0, 1] > 0 and dist[3, 0].tolist() == [65536, 0]      # (i = 0, f = 1023 against i = 1, f = 0)
    # the empty pattern
    index, words, targets, resets = cases.empty_stream()
    best, dist, d = cases.run_definition(cases.EMPTY, index, words, targets)
    assert (dist == 21845).all() and not d.dense_weights().any()
    # splits and frozen calls
    assert cases.FROZEN_STEPS == [1, CHUNK, CHUNK + 1]
    ring = {s[0]: max(s[1]["steps"]) + 1 for s in STREAMS}
    assert any(max(sp) < ring[name] and len(sp) > 1 for name, sp in SPLITS) and any(0 in sp for _, sp in SPLITS)
    assert all(sum(sp) == by_name[name][2]["T"] for name, sp in SPLITS)


@pytest.mark.parametrize("name,splits", SPLITS, ids=SPLIT_IDS)
def test_the_definition_over_split_calls_equals_one_call(name, splits):
    p, (index, words, targets, resets) = cases.streamed(name)
    whole = cases.run_definition(p, index, words, targets, resets)
    cut = cases.run_definition(p, index, words, targets, resets, splits=splits)
    assert np.array_equal(whole[0], cut[0]) and np.array_equal(whole[1], cut[1])
    a, b = whole[2], cut[2]
    assert np.array_equal(a.dense_weights(), b.dense_weights()) and a.ring == b.ring and (a.count, a.total) == (b.count, b.total)


@pytest.mark.parametrize("alpha_q", cases.PERIODIC_ALPHAS)
def test_the_definition_learns_periodic_patterns_at_every_horizon(alpha_q):
    """12 random patterns of 40 units over 2 048 units, 16 buckets, horizons (0, 1, 5), 20 epochs: right at every horizon in the last."""
    p = dict(cases.PERIODIC, alpha_q=alpha_q)
    index, words, targets = cases.periodic_stream()
    best, dist, d = cases.run_definition(p, index, words, targets)
    T = len(index)
    for i, h in enumerate(p["steps"]):
        want = [targets[(t + h) % 12] for t in range(T - 12, T)]
        assert best[T - 12:, i, 0].tolist() == want, (alpha_q, h)
    assert (dist.sum(axis=2) <= 65536).all() and (dist.sum(axis=2) > 65536 - 16).all()


def test_the_model_level_hit_rate_on_the_oracles_states_is_the_recorded_floor():
    """The definition over the oracle's states, on the CPU: the number written beside the case (the GPU test holds the device's record to
    this same stream, bit for bit)."""
    best, dist, targets = cases.model_stream("128x4")
    rates = tuple(cases.hit_rate(best, targets, i, h, len(cases.MODEL_SEQUENCE)) for i, h in enumerate(cases.MODEL_STEPS))
    print("128x4 hit rates per horizon", rates)
    assert rates == cases.HIT_RATE["128x4"]
    assert len(set(targets[:10].tolist())) == 10              # (ten different buckets: a constant guess would be right once in ten)


# ---- the C ABI
def test_the_header_declares_the_classifier_abi_and_the_binding_matches_it():
    from bithtm_amd import _lib as L
    header = open(HEADER).read()
    decl = {m.group(1): m.group(2) for m in re.finditer(r"\b(htm_classifier_[a-z_]+)\s*\(([^)]*)\)\s*;", header)}
    assert set(decl) == set(ABI)
    for name, params in decl.items():
        assert params.split(",")[0].strip() == ABI[name], (name, params)
        assert len(L.EXPORTS[name][1]) == len(params.split(",")), name
    assert L.EXPORTS["htm_classifier_destroy"][0] is None and L.EXPORTS["htm_classifier_state_bytes"][0] is C.c_int64
    assert all(L.EXPORTS[n][0] is C.c_int for n in ABI if n not in ("htm_classifier_destroy", "htm_classifier_state_bytes"))
    cap = re.search(r"\bhtm_set_run_active_cells\s*\(([^)]*)\)\s*;", header).group(1)
    assert [x.strip() for x in cap.split(",")] == ["htm_handle *h", "void *device_pairs"] and len(L.EXPORTS["htm_set_run_active_cells"][1]) == 2
    assert L.ABI_VERSION == 4 and re.search(r"#define BITHTM_ABI_VERSION 4\b", header)
    body = re.search(r"typedef struct htm_classifier_config \{(.*?)\} htm_classifier_config;", header, re.S).group(1)
    assert [re.sub(r"\s+", " ", x.strip()) for x in body.split(";") if x.strip()] == [
        "uint32_t struct_bytes", "int32_t buckets, n_steps, alpha_q, units, cell_dim, max_pairs", "int32_t steps[8]"]
    assert C.sizeof(L.HtmClassifierConfig) == 4 + 6 * 4 + 8 * 4
    assert [n for n, _ in L.HtmClassifierConfig._fields_] == ["struct_bytes", "buckets", "n_steps", "alpha_q", "units", "cell_dim", "max_pairs", "steps"]
    update = [re.sub(r"\s+", " ", x.strip()) for x in decl["htm_classifier_update"].split(",")]
    assert update == ["htm_classifier *clf", "htm_handle *h", "const void *device_pairs", "int32_t pairs_per_step", "int32_t n_steps",
                      "const int32_t *device_targets", "int32_t n_targets", "int32_t first_step", "const uint32_t *device_reset_bits", "int32_t learn",
                      "int32_t *device_best", "int32_t *device_dist"]


def test_the_c_calls_refuse_null_arguments_without_a_gpu():
    from bithtm_amd import _lib as L
    from bithtm_amd.classifier import EXP_TABLE
    lib = L.load()
    cfg = L.HtmClassifierConfig(C.sizeof(L.HtmClassifierConfig), 3, 1, 655, 64, 32, 4, (C.c_int32 * 8)(1))
    out = C.c_void_p(1)
    assert lib.htm_classifier_create(None, C.byref(cfg), EXP_TABLE.ctypes.data_as(C.c_void_p), C.byref(out)) == -1 and not out.value
    assert b"null" in lib.htm_last_error(None)
    assert lib.htm_classifier_update(None, None, None, 1, 1, None, 1, 0, None, 1, None, None) == -1
    assert lib.htm_classifier_reset(None, None) == -1
    assert lib.htm_classifier_read_weights(None, None, 0, 0, 1, None) == -1 and lib.htm_classifier_write_weights(None, None, 0, 0, 1, None) == -1
    assert lib.htm_classifier_export(None, None, None, 0) == -1 and lib.htm_classifier_import(None, None, None, 0) == -1
    assert lib.htm_classifier_state_bytes(None) == -1
    assert lib.htm_set_run_active_cells(None, None) == -1
    lib.htm_classifier_destroy(None)


def test_the_python_layer_refuses_before_any_library_call():
    import bithtm_amd as B
    from bithtm_amd.classifier import check_params, check_patterns
    assert check_params(16, (1, 5), 0.001) == (16, (1, 5), 66) and check_params(3, 2, 1.0) == (3, (2,), 65536)
    for bad in (dict(buckets=0), dict(buckets=1025), dict(buckets=3, steps=()), dict(buckets=3, steps=range(9)), dict(buckets=3, steps=(65,)),
                dict(buckets=3, steps=(-1,)), dict(buckets=3, steps=(2, 2)), dict(buckets=3, steps=(3, 1)), dict(buckets=3, alpha=0.0),
                dict(buckets=3, alpha=1.1), dict(buckets=3, alpha=1e-6)):
        with pytest.raises(ValueError):
            B.SDRClassifier(**bad)
    with pytest.raises(ValueError, match="one of them"):
        B.SDRClassifier()
    with pytest.raises(ValueError, match="one of them"):
        B.SDRClassifier(buckets=3, field=B.ScalarField(0, 1, 16, 3))
    with pytest.raises(ValueError, match="shape"):
        B.SDRClassifier(buckets=3, shape=(10, 65, 4))
    field = B.ScalarField(0.0, 100.0, 64, 9)
    assert B.SDRClassifier(field=field).buckets == 56
    clf = B.SDRClassifier(buckets=3, steps=(0, 2), shape=(10, 5, 4))
    ok = (np.array([[0, 1, 2, -1]]), np.array([[1, 2, 4, 0xFFFFFFFF]], dtype=np.uint32), [0])
    for index, words, targets, match in (
            (np.array([[0, 1, 1, 3]]), np.array([[1, 2, 4, 1]], dtype=np.uint32), ok[2], "twice"), (np.array([[0, 1, 2, 10]]), ok[1], ok[2], "at or above 10"),
            (ok[0], np.array([[1, 2, 32, 0]], dtype=np.uint32), ok[2], "cell_dim"), (ok[0], ok[1], [3], "at or above buckets"),
            (ok[0], ok[1], [0, 1], r"int \[1\]"), (ok[0][:, :3], ok[1], ok[2], "index int"), (ok[0].astype(float), ok[1], ok[2], "index int"),
            (np.zeros((1, 5), int) + np.arange(5), np.ones((1, 5), np.uint32), ok[2], "max_pairs")):
        with pytest.raises(ValueError, match=match):
            clf.update_patterns(index, words, targets)
    with pytest.raises(ValueError, match=r"bool \[1\]"):
        clf.update_patterns(*ok, resets=[0, 1])
    with pytest.raises(RuntimeError, match="not bound"):
        clf.update_patterns(*ok)
    with pytest.raises(RuntimeError, match="shape"):
        B.SDRClassifier(buckets=3).update_patterns(*ok)
    assert check_patterns(np.array([[-1, -1]]), np.array([[7, 7]]), 50, 5)[0].tolist() == [[-1, -1]]       # (dead pairs may repeat)
    # an unbound object holds a loaded state until it is bound
    state = clf.state_dict()
    assert (int(state["total"]), int(state["count"])) == (0, 0) and state["ring"].shape == (3, 4, 2) and state["weights"].shape == (2, 50, 3)
    assert (state["ring"][:, :, 0] == -1).all() and state["params"].tolist() == [3, 66, 10, 5, 4, 0, 2]
    state["total"], state["count"] = np.int64(9), np.int64(4)
    state["weights"][1, 7] = (5, -5, 1 << 30)
    clf.load_state_dict(state)
    again = clf.state_dict()
    assert all(np.array_equal(again[k], state[k]) for k in state)
    clf.reset()
    assert (int(clf.state_dict()["count"]), int(clf.state_dict()["total"])) == (0, 9)
    with pytest.raises(ValueError, match="parameters"):
        B.SDRClassifier(buckets=4, steps=(0, 2), shape=(10, 5, 4)).load_state_dict(state)
    for key, value, match in (("count", np.int64(10), "count"), ("count", np.int64(-1), "count"), ("ring", state["ring"][:2], "ring"),
                              ("weights", state["weights"][:, :49], "weights")):
        with pytest.raises(ValueError, match=match):
            clf.load_state_dict(dict(state, **{key: value}))
    big = state["weights"].copy()
    big[0, 0, 0] = (1 << 30) + 1
    with pytest.raises(ValueError, match="2\\^30"):
        clf.load_state_dict(dict(state, weights=big))
    # the calls a classifier does not ride on refuse it before anything else
    tm, sp = B.TemporalMemory(64, 4), B.SpatialPooler(32, 64, 4)
    for call in (lambda: tm.run(np.zeros((1, 4), int), 1, classifier=clf), lambda: sp.run(np.zeros((1, 32), bool), 1, classifier=clf)):
        with pytest.raises(ValueError, match="classifier= is not available here"):
            call()
    for method, positional in ((B.HierarchicalTemporalMemory.lookahead, 4), (B.HierarchicalTemporalMemory.forecast, 2), (B.ModelGroup.run, 3),
                               (B.ModelGroup.tick, 2)):
        with pytest.raises(ValueError, match="classifier= is not available here"):
            method(*[None] * positional, classifier=clf)


def test_run_record_carries_the_classification():
    import bithtm_amd as B
    rec = B.RunRecord(np.arange(2))
    assert rec.classified_bucket is None and rec.classified_probability is None and rec.classified_value is None and rec.class_distribution is None
    pairs = np.array([[[3, 65536], [0, 16384]], [[55, 1], [0, 0]]], dtype=np.int32)
    field = B.ScalarField(0.0, 100.0, 64, 9)
    rec = B.RunRecord(np.arange(2), classified=pairs, classified_field=field, class_distribution=np.zeros((2, 2, 56), np.int32))
    assert rec.classified_bucket.tolist() == [[3, 0], [55, 0]] and rec.classified_probability.tolist() == [[1.0, 0.25], [1 / 65536, 0.0]]
    assert np.array_equal(rec.classified_value, field.value_of(rec.classified_bucket)) and rec.class_distribution.shape == (2, 2, 56)
    assert B.RunRecord(np.arange(2), classified=pairs).classified_value is None


# ---- the compiler's report
def test_the_new_kernels_have_no_scratch_and_the_existing_ones_keep_their_figures():
    from bithtm_amd.build import kernel_resources
    res = kernel_resources()
    if res is None:
        pytest.skip("the library in the tree was not built here")
    new = {k: v for k, v in res.items() if re.match(r"_Z\d+kcls_", k)}
    assert sorted(re.match(r"_Z\d+(kcls_[a-z]+)", k).group(1) for k in new) == ["kcls_apply", "kcls_capture", "kcls_frozen", "kcls_sum"], sorted(new)
    for name, r in new.items():
        print(name, r)
        assert r["scratch_bytes_per_lane"] == 0, (name, r)
        assert r["lds_bytes"] <= 24 * 1024 and r["occupancy"] >= 4, (name, r)       # (far below the 160 KiB a block may have)
    old_names = {re.match(r"_Z\d+(k[a-z]*_[a-z_]+)", k).group(1) for k in res if k not in new and re.match(r"_Z\d+k[a-z]*_", k)}
    for k in new:                                   # (the budget tests find kernels with re.search: no name inside another)
        assert not [s for s in old_names if s in k], k
    # every kernel that existed before the classifier was added: the figures the compiler gave it then.  The fixture is
    # bithtm_amd/libbithtm_hip.resources.json of a build of the commit before htm_classifier.h, copied as it is.
    with open(os.path.join(ROOT, "tests", "golden", "kernel_resources_before_classifier.json")) as f:
        before = json.load(f)
    assert len(before) > 100 and not [k for k in before if "kcls_" in k]
    changed = {k: (before[k], res.get(k)) for k in before if before[k] != res.get(k)}
    assert not changed, changed


# ---- the launch traces
@pytest.fixture(scope="module")
def traces(tmp_path_factory):
    tmp = str(tmp_path_factory.mktemp("classifier_trace"))
    obj, stub, defsym = _host_objects(tmp)
    lib = os.path.join(tmp, "libbithtm_host_trace.so")
    subprocess.run([os.path.join(CLANG_DIR, "bin", "clang++"), "-shared", obj, stub, "-ldl", "-o", lib] + defsym, check=True, capture_output=True)
    env = dict(os.environ, BITHTM_LIBRARY=lib, BITHTM_STUB_TRACE=os.path.join(tmp, "trace.txt"))
    for name in ("LD_PRELOAD", "BITHTM_LEAN", "BITHTM_SCAN_LARGE"):
        env.pop(name, None)
    r = subprocess.run([sys.executable, os.path.join(ROOT, "tests", "host_stub", "classifier_driver.py")], env=env, capture_output=True, text=True,
                       timeout=600)
    assert r.returncode == 0, (r.stdout + r.stderr)[-4000:]
    return json.loads(r.stdout.splitlines()[-1])


@needs_hipcc
def test_a_frozen_update_is_one_launch_per_chunk_and_a_learning_one_two_per_step(traces):
    H = 3
    for T in (1, CHUNK, CHUNK + 1, 2 * CHUNK + 3):
        lines = traces["frozen"][f"T={T}"]
        sizes = [min(CHUNK, T - first) for first in range(0, T, CHUNK)]
        assert len(sizes) == -(-T // CHUNK)
        # (17 pairs: two blocks along x; step and horizon share grid y)
        assert [re.match(r"launch (\S+) grid (\d+) (\d+)", x).groups()[1:] for x in lines] == [("2", str(H * n)) for n in sizes], lines
        assert [_kernel(x) for x in lines] == ["kcls_frozen"] * len(sizes), lines
    for T in (1, 7):
        lines = traces["learning"][f"T={T}"]
        assert [_launch(x) for x in lines] == [("kcls_sum", 3, H, 256, 0), ("kcls_apply", 3, H, 256, 0)] * T, lines      # (max_pairs 40: three blocks)


@needs_hipcc
@pytest.mark.parametrize("mode", ["run", "graphs"])
def test_a_classified_run_adds_a_capture_per_step_and_a_plain_run_is_the_trace_it_was(traces, mode):
    t = traces[mode]
    recorded, classified = t["recorded"], t["classified"]
    # behind the classified run: the learning update of its 6 steps, and nothing else; in front: the 8-byte descriptor copy
    tail = classified[-12:]
    assert [_kernel(x) for x in tail] == ["kcls_sum", "kcls_apply"] * 6, tail
    assert all(_launch(x)[1:] == (1, 2, 256, 0) for x in tail)           # (8 columns x 2 words = 16 pairs: one block; two horizons)
    body = classified[:-12]
    assert body[0] == "memcpy 8" and recorded[0] != "memcpy 8"
    body = body[1:]
    if mode == "run":
        # eagerly: the recorded run's lines with one kcls_capture directly behind each step's record launch
        captures = [i for i, x in enumerate(body) if _kernel(x) == "kcls_capture"]
        assert len(captures) == 6 and all(_kernel(body[i - 1]) == "k_rec_step" for i in captures)
        assert all(_launch(body[i]) == ("kcls_capture", 1, 1, 256, 0) for i in captures)
        assert [x for x in body if _kernel(x) != "kcls_capture"] == recorded
        assert sum(_kernel(x) == "k_rec_step" for x in recorded) == 6
    else:
        # from graphs: the same replays, copies and eager launches (the capture launches are inside the graphs)
        assert body == recorded and "graph_launch" in recorded and not [x for x in body if _kernel(x) == "kcls_capture"]
    # a run without a classifier, on a model that has just made classified runs, is line for line the trace of the model that never did
    assert t["recorded after"] == recorded and t["plain after"] == t["plain"]
    assert not [x for x in t["plain"] + recorded if "kcls" in x]
    # the Python refusals enqueue nothing
    assert traces["refused_lines"] == [] and all(traces["refused"].values()), traces["refused"]
    assert "at or above buckets" in traces["refused"]["targets above"] and "shape" in traces["refused"]["another shape"]


# ---- the host code under ASan + UBSan, as a stand-alone program, and the kernel header's arithmetic on the host
def _arithmetic_cases():
    """The lines of the case file and, per line, what the definition gives (strings as the program prints them)."""
    from bithtm_amd.classifier import EXP_CUTOFF, EXP_TABLE, W_LIMIT, delta_of, exp_q30, softmax
    rng = np.random.default_rng(5)
    lines, expect = ["T " + " ".join(str(int(x)) for x in EXP_TABLE)], []
    for d in [0, 1, 1023, 1024, 1025, 65535, 65536, EXP_CUTOFF - 1024, EXP_CUTOFF - 1, EXP_CUTOFF, EXP_CUTOFF + 1, 1 << 40, (1 << 62)] + \
            rng.integers(0, EXP_CUTOFF, 300).tolist():
        lines.append(f"e {d}")
        expect.append(str(exp_q30(d)))
    acts = [[0], [5, 5, 5], [0, -1023], [0, -1024], [-(32 << 16), 0, -(32 << 16) + 1], [W_LIMIT * 1280, -W_LIMIT * 1280, 0], [-7] * 1024]
    acts += [rng.integers(-200000, 200000, int(n)).tolist() for n in rng.integers(1, 70, 40)]
    acts += [rng.integers(-(1 << 40), 1 << 40, 5).tolist(), (rng.integers(0, 3, 1024) * 40000).tolist()]
    ps = []
    for a in acts:
        lines.append(f"s {len(a)} " + " ".join(str(x) for x in a))
        p = softmax(a)
        ps.append(p)
        expect.append(" ".join(str(x) for x in [a.index(max(a))] + p))
    for alpha_q in (1, 66, 655, 6554, 65536):
        for p in [0, 1, 21845, 21846, 32768, 65535, 65536] + rng.integers(0, 65537, 10).tolist():
            for g in (0, 1):
                lines.append(f"d {alpha_q} {p} {g}")
                expect.append(str(delta_of(alpha_q, [p], 0 if g else 1)[0]))
    for w, d in [(W_LIMIT - 10, 11), (W_LIMIT - 10, 10), (W_LIMIT, 65536), (-W_LIMIT + 10, -11), (-W_LIMIT, -65536), (0, 0), (5, -9), (W_LIMIT, -1)]:
        lines.append(f"c {w} {d}")
        expect.append(str(max(-W_LIMIT, min(W_LIMIT, w + d))))
    for index, word, K, wpc, cols in [(-1, 5, 32, 1, 10), (9, 0xFFFFFFFF, 32, 1, 10), (10, 1, 32, 1, 10), (3, 0xFFFFFFFF, 5, 1, 10), (3, 32, 5, 1, 10),
                                      (19, 0xFFFFFFFF, 64, 2, 10), (20, 1, 64, 2, 10), (7, 0xFFFFFFFF, 48, 2, 10), (6, 0xFFFFFFFF, 48, 2, 10), (0, 0, 4, 1, 1)]:
        lines.append(f"b {index} {word} {K} {wpc} {cols}")
        if index < 0 or index // wpc >= cols:
            live = 0
        else:
            top = K - (index % wpc) * 32
            live = word if top >= 32 else word & ((1 << top) - 1)
        expect.append(f"{live} {(index // wpc) * K + (index % wpc) * 32 if live else -1}")
    return lines, expect


@needs_hipcc
def test_the_host_code_runs_clean_under_asan_and_ubsan_and_the_header_arithmetic_equals_the_definition(tmp_path):
    """tests/host_stub/classifier_host.cpp and htm_engine.hip (host-only), both with -fsanitize=address,undefined, linked against the
    stub runtime into ONE program that is run directly: nothing is preloaded."""
    tmp = str(tmp_path)
    san = ["-fsanitize=address,undefined", "-fno-sanitize-recover=undefined"]
    obj, stub, defsym = _host_objects(tmp, san)
    clang = os.path.join(CLANG_DIR, "bin", "clang++")
    exe = os.path.join(tmp, "classifier_host")
    subprocess.run([clang, "-std=c++17", "-O1", "-g", "-fno-omit-frame-pointer", "-ffp-contract=off"] + san +
                   [os.path.join(ROOT, "tests", "host_stub", "classifier_host.cpp"), obj, stub, "-ldl", "-o", exe] + defsym, check=True, capture_output=True)
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
    assert len(got) == len(expect) > 400
    wrong = [(line[:80], g[:80], e[:80]) for line, g, e in zip(lines[1:], got, expect) if g != e]
    assert not wrong, wrong[:5]
