"""SDR classifier on the device (SDRClassifier; htm_classifier_*, htm_set_run_active_cells) against its definition,
bithtm_amd/classifier.py.  Every comparison is exact: the (bucket, p) pairs, the distributions, the weights read back, the ring and the
counters.  The stand-alone door (update_patterns) runs the geometry cases of tests/classifier_cases.py without stepping a model; the
model tests hold run(classifier=) to the definition applied to the stepwise twin's cell activations, and the model itself to the same
run without a classifier."""
import ctypes as C

import numpy as np
import pytest

import classifier_cases as cases
from classifier_cases import CHUNK, MODELS, MODEL_ALPHA, MODEL_STEPS, SPLITS, SPLIT_IDS, STREAM_IDS


def _clf(p, **kw):
    import bithtm_amd as B
    clf = B.SDRClassifier(buckets=p["buckets"], steps=p["steps"], alpha=p["alpha_q"] / 65536.0, shape=(p["column_dim"], p["cell_dim"], p["max_pairs"]), **kw)
    assert clf.alpha_q == p["alpha_q"]
    return clf


def _same_state(clf, d, what=""):
    """The device's whole state is the definition's: weights, ring, count, total."""
    got = clf.state_dict()
    assert got["weights"].dtype == np.int32 and np.array_equal(got["weights"], d.dense_weights()), (what, "weights")
    assert np.array_equal(got["ring"], d.ring_arrays(clf.shape[2])), (what, "ring")
    assert (int(got["count"]), int(got["total"])) == (d.count, d.total), (what, "counters")


def _load_weights(clf, w):
    state = clf.state_dict()
    state["weights"] = w
    clf.load_state_dict(state)


# ---- the stand-alone door
@pytest.mark.gpu
@pytest.mark.parametrize("name", STREAM_IDS)
def test_update_patterns_equals_the_definition(name):
    p, (index, words, targets, resets) = cases.streamed(name)
    want_best, want_dist, d = cases.run_definition(p, index, words, targets, resets)
    clf = _clf(p)
    best, dist = clf.update_patterns(index, words, targets, resets=resets, device=0)
    assert np.array_equal(best, want_best), np.argwhere(best != want_best)[:5]
    assert np.array_equal(dist, want_dist), np.argwhere(dist != want_dist)[:5]
    _same_state(clf, d, name)
    assert d.dense_weights().any() or p["buckets"] == 1 or p["alpha_q"] == 1


@pytest.mark.gpu
@pytest.mark.parametrize("name,splits", SPLITS, ids=SPLIT_IDS)
def test_splits_change_nothing(name, splits):
    p, (index, words, targets, resets) = cases.streamed(name)
    want_best, want_dist, d = cases.run_definition(p, index, words, targets, resets)
    clf = _clf(p)
    parts, at = [], 0
    for n in splits:
        parts.append(clf.update_patterns(index[at:at + n], words[at:at + n], targets[at:at + n], resets=resets[at:at + n], device=0))
        at += n
    assert at == len(index)
    assert np.array_equal(np.concatenate([b for b, _ in parts]), want_best)
    assert np.array_equal(np.concatenate([q for _, q in parts]), want_dist)
    _same_state(clf, d, name)


@pytest.mark.gpu
def test_an_empty_pattern_gives_the_uniform_distribution():
    p = cases.EMPTY
    index, words, targets, resets = cases.empty_stream()
    clf = _clf(p)
    best, dist = clf.update_patterns(index, words, targets, device=0)
    assert (dist == 65536 // 3).all() and (best[:, :, 0] == 0).all() and (best[:, :, 1] == 21845).all()
    _same_state(clf, cases.run_definition(p, index, words, targets)[2])
    assert not clf.state_dict()["weights"].any()


@pytest.mark.gpu
@pytest.mark.parametrize("sign", [1, -1], ids=["upper", "lower"])
def test_one_step_meets_the_clamp(sign):
    p = cases.CLAMP
    w, index, words, targets = cases.clamp_case(sign)
    want_best, want_dist, d = cases.run_definition(p, index, words, targets, weights=w)
    clf = _clf(p)
    home = _home()
    clf.bind(home)                                  # (an object with a shape of its own keeps it)
    _load_weights(clf, w)
    best, dist = clf.update_patterns(index, words, targets)
    assert np.array_equal(best, want_best) and np.array_equal(dist, want_dist)
    got = clf.state_dict()["weights"][0, 0]
    assert got.tolist() == d.dense_weights()[0, 0].tolist()
    assert (got.max() == 1 << 30) if sign > 0 else (got.min() == -(1 << 30))


def _home():
    """A small model whose handle the stand-alone objects of a test go through."""
    import bithtm_amd as B
    return B.HierarchicalTemporalMemory(32, 64, 4, active_columns=4)


@pytest.mark.gpu
def test_the_exp_table_edges_on_the_device():
    from bithtm_amd.classifier import exp_q30
    p = cases.EDGES
    w, index, words, targets = cases.edge_case()
    want_best, want_dist, d = cases.run_definition(p, index, words, targets, learning=False, weights=w)
    clf = _clf(p)
    state = clf.state_dict()                         # (unbound: the state waits for the device)
    state["weights"] = w
    clf.load_state_dict(state)
    best, dist = clf.update_patterns(index, words, targets, learning=False, device=0)
    assert np.array_equal(dist, want_dist) and np.array_equal(best, want_best)
    for i, dd in enumerate(cases.D_EDGES):
        e = exp_q30(dd)
        assert dist[i, 0].tolist() == [((1 << 30) << 16) // ((1 << 30) + e), (e << 16) // ((1 << 30) + e)], dd
    assert np.array_equal(clf.state_dict()["weights"], w)


@pytest.mark.gpu
@pytest.mark.parametrize("n", cases.FROZEN_STEPS)
def test_a_frozen_call_equals_learning_off_step_by_step(n):
    p = cases.FROZEN
    index, words, targets, resets = cases.stream(p, 12 + n, 4, seed=20 + n, resets=0.01)
    d = cases.definition(p)
    clf = _clf(p)
    want = [d.update(index[:12], words[:12], targets[:12], resets[:12], True)]
    got = [clf.update_patterns(index[:12], words[:12], targets[:12], resets=resets[:12], device=0)]
    learned = d.dense_weights()
    assert learned.any()
    for t in range(12, 12 + n):                     # (the definition one step at a time, learning off)
        want.append(d.update(index[t:t + 1], words[t:t + 1], targets[t:t + 1], resets[t:t + 1], False))
    got.append(clf.update_patterns(index[12:], words[12:], targets[12:], resets=resets[12:], learning=False))
    assert np.array_equal(np.concatenate([b for b, _ in got]), np.concatenate([b for b, _ in want]))
    assert np.array_equal(np.concatenate([q for _, q in got]), np.concatenate([q for _, q in want]))
    assert np.array_equal(d.dense_weights(), learned)
    _same_state(clf, d, f"frozen {n}")
    # ... and a learning call behind it finds the history the frozen call left
    tail = cases.stream(p, 5, 4, seed=99)
    wb, wq = d.update(*tail[:3], tail[3], True)
    gb, gq = clf.update_patterns(*tail[:3], resets=tail[3])
    assert np.array_equal(gb, wb) and np.array_equal(gq, wq)
    _same_state(clf, d, f"behind frozen {n}")


@pytest.mark.gpu
def test_targets_at_or_above_the_buckets_are_missing_on_the_c_side():
    """The Python layer refuses such a target; the C call takes it as missing."""
    from bithtm_amd import _lib as L
    p, (index, words, targets, resets) = cases.streamed("B3-h1-wave")
    targets = targets.copy()
    targets[::3] = [3, 1 << 20, -7, 3, 2147483647, 3, 4, 5]
    clf = _clf(p)
    home = _home()
    eng = home.engine
    clf.bind(home)
    T, n = index.shape
    pairs = np.empty((T, n, 2), np.int32)
    pairs[:, :, 0], pairs[:, :, 1] = index, words.view(np.int32)
    buf, tbuf = eng.device_buffer(pairs.nbytes, pairs), eng.device_buffer(targets.nbytes, targets)
    try:
        clf.enqueue(eng, buf, n, T, tbuf, T, 0, None, True, True)
        eng.sync()
        best, dist = clf.read(eng, T, True)
    finally:
        eng.sync()
        eng.lib.hipFree(buf)
        eng.lib.hipFree(tbuf)
    want_best, want_dist, d = cases.run_definition(p, index, words, np.where((targets < 0) | (targets >= 3), -1, targets))
    assert np.array_equal(best, want_best) and np.array_equal(dist, want_dist)
    _same_state(clf, d)
    # the refusals of a bound object, with nothing enqueued: the state stays what it was
    lib = eng.lib
    for bad in (dict(pairs=0), dict(pairs=n + 1), dict(steps=-1), dict(targets=0), dict(first=-1)):
        rc = lib.htm_classifier_update(clf._clf, eng.h, C.c_void_p(1), bad.get("pairs", n), bad.get("steps", 1), C.c_void_p(1), bad.get("targets", 1),
                                       bad.get("first", 0), None, 1, C.c_void_p(1), None)
        assert rc == -1, bad
    assert lib.htm_classifier_read_weights(clf._clf, eng.h, 1, 0, 1, C.c_void_p(1)) == -1
    assert lib.htm_classifier_read_weights(clf._clf, eng.h, 0, 10 * 32 - 1, 2, C.c_void_p(1)) == -1
    one = np.array([1 << 30, -(1 << 30), (1 << 30) + 1], np.int32)
    assert lib.htm_classifier_write_weights(clf._clf, eng.h, 0, 0, 1, one.ctypes.data_as(C.c_void_p)) == -1
    assert lib.htm_classifier_export(clf._clf, eng.h, C.c_void_p(1), 8) == -1
    _same_state(clf, d, "after the refusals")
    assert L.ABI_VERSION == lib.htm_abi_version()


@pytest.mark.gpu
def test_reset_and_the_state_round_trip():
    p, (index, words, targets, resets) = cases.streamed("B64-K64-h015")
    d = cases.definition(p)
    clf = _clf(p)
    a = clf.update_patterns(index[:8], words[:8], targets[:8], device=0)
    b = d.update(index[:8], words[:8], targets[:8])
    clf.reset()
    d.reset()
    a2 = clf.update_patterns(index[8:12], words[8:12], targets[8:12])
    b2 = d.update(index[8:12], words[8:12], targets[8:12])
    assert all(np.array_equal(x, y) for x, y in zip(a + a2, b + b2))
    _same_state(clf, d, "behind reset()")
    # a second object takes the state over and goes on as the first
    other = _clf(p)
    other.load_state_dict(clf.state_dict())
    a3 = other.update_patterns(index[12:], words[12:], targets[12:], device=0)
    b3 = d.update(index[12:], words[12:], targets[12:])
    assert all(np.array_equal(x, y) for x, y in zip(a3, b3))
    _same_state(other, d, "the second object")


# ---- classified runs of a model
def _model(name):
    from hip_impl import make_htm
    m = MODELS[name]
    return make_htm(m["input_dim"], m["column_dim"], m["cell_dim"], m["active_columns"], m["seed"], cases.model_permanence(m))


def _model_clf(enc, **kw):
    import bithtm_amd as B
    return B.SDRClassifier(field=enc.fields[0], steps=MODEL_STEPS, alpha=MODEL_ALPHA, **kw)


def _stepwise(name, values, flags, T, first=0):
    """The twin stepped with process(), its cell activations packed into pairs, the definition over them."""
    from bithtm_amd.classifier import ClassifierDefinition
    m = MODELS[name]
    enc = cases.model_encoder()
    twin = _model(name)
    bank, buckets = enc.encode(values), enc.bucket(values)[:, 0]
    d = ClassifierDefinition(enc.fields[0].buckets, MODEL_STEPS, MODEL_ALPHA, units=m["column_dim"] * m["cell_dim"], cell_dim=m["cell_dim"])
    best = np.zeros((T, len(MODEL_STEPS), 2), np.int32)
    dist = np.zeros((T, len(MODEL_STEPS), d.buckets), np.int32)
    for t in range(T):
        r = (first + t) % len(values)
        if flags is not None and flags[r]:
            twin.reset()
        sp, tm = twin.process(bank[r])
        index, words = cases.pairs_of(np.asarray(tm.cell_activation), np.asarray(sp.active_column), m["cell_dim"])
        best[t], dist[t] = d.step(zip(index, words), buckets[r], bool(flags is not None and flags[r]), True, True)
    return best, dist, d, twin


@pytest.mark.gpu
@pytest.mark.parametrize("name", list(MODELS))
def test_a_classified_run_equals_the_stepwise_loop_and_the_oracle_stream(name):
    """run(values, encoder=, classifier=) == process() + State.cell_activation packed into pairs + the definition, bit for bit, which
    is the stream of the definition over the ORACLE's states (classifier_cases.model_stream): its hit rate is the recorded floor."""
    m = MODELS[name]
    enc = cases.model_encoder()
    values, _ = cases.model_values()
    T = m["epochs"] * len(values)
    htm = _model(name)
    clf = _model_clf(enc)
    rec = htm.run(values, T, encoder=enc, classifier=clf, record=("counters", "class_distribution"))
    best, dist, d, twin = _stepwise(name, values, None, T)
    assert np.array_equal(rec.classified_bucket, best[:, :, 0]) and np.array_equal(rec.classified_probability, best[:, :, 1] / 65536.0)
    assert np.array_equal(rec.class_distribution, dist)
    assert np.array_equal(rec.classified_value, enc.fields[0].value_of(best[:, :, 0]))
    o_best, o_dist, targets = cases.model_stream(name)
    assert np.array_equal(best, o_best) and np.array_equal(dist, o_dist)
    for i, h in enumerate(MODEL_STEPS):
        rate = cases.hit_rate(np.stack([rec.classified_bucket, rec.classified_bucket], -1), targets, i, h, len(values))
        print(name, "horizon", h, "hit rate", rate)
        assert rate == cases.HIT_RATE[name][i]
    _same_state(clf, d, name)
    # the model's own state is what the same run without a classifier leaves
    plain = _model(name)
    plain_rec = plain.run(values, T, encoder=enc, record=True)
    a, b, c = htm.state_dict(), plain.state_dict(), twin.state_dict()
    for key in a:
        assert np.array_equal(a[key], b[key]) and np.array_equal(a[key], c[key]), key
    assert np.array_equal(rec.active_cells, plain_rec.active_cells) and np.array_equal(rec.bursting_columns, plain_rec.bursting_columns)


@pytest.mark.gpu
def test_a_classified_run_with_resets_a_missing_value_and_split_calls():
    name = "128x4"
    enc = cases.model_encoder()
    values, flags = cases.model_values(resets=True, missing=True)
    T = 120
    htm = _model(name)
    clf = _model_clf(enc)
    parts = [htm.run(values, n, encoder=enc, classifier=clf, resets=flags, record="class_distribution") for n in (37, 3, 80)]
    best, dist, d, twin = _stepwise(name, values, flags, T)
    assert np.array_equal(np.concatenate([r.classified_bucket for r in parts]), best[:, :, 0])
    assert np.array_equal(np.concatenate([r.class_distribution for r in parts]), dist)
    assert np.array_equal(np.concatenate([r.step_index for r in parts]), np.arange(T))
    _same_state(clf, d)
    o_best, o_dist, _ = cases.model_stream(name, resets=True, missing=True)
    assert np.array_equal(best, o_best[:T]) and np.array_equal(dist, o_dist[:T])
    a, c = htm.state_dict(), twin.state_dict()
    for key in a:
        assert np.array_equal(a[key], c[key]), key
    # explicit targets, learning off for the classifier only: the weights stay, the history goes on
    before = clf.state_dict()
    tg = np.arange(10) % 5
    rec = htm.run(values, 10, encoder=enc, classifier=clf, targets=tg, resets=flags, classifier_learning=False)
    after = clf.state_dict()
    assert np.array_equal(before["weights"], after["weights"]) and int(after["total"]) == T + 10
    assert rec.classified_bucket.shape == (10, 2) and rec.class_distribution is None


@pytest.mark.gpu
def test_a_views_classified_run_learns_its_classifier_and_leaves_the_parent_untouched():
    name = "128x4"
    enc = cases.model_encoder()
    values, _ = cases.model_values()
    parent = _model(name)
    parent.run(values, 100, encoder=enc)
    before = parent.state_dict()
    view = parent.inference_view()
    clf = _model_clf(enc)
    rec = view.run(values, 60, encoder=enc, classifier=clf, classifier_learning=True)
    assert clf.state_dict()["weights"].any() and rec.classified_bucket.shape == (60, 2)
    after = parent.state_dict()
    for key in before:
        assert np.array_equal(before[key], after[key]), key
    frozen = view.run(values, 10, encoder=enc, classifier=clf)             # (follows learning=False)
    w = clf.state_dict()["weights"]
    view.run(values, 10, encoder=enc, classifier=clf)
    assert np.array_equal(w, clf.state_dict()["weights"]) and frozen.classified_bucket.shape == (10, 2)


@pytest.mark.gpu
def test_the_example_prints_the_one_step_hit_rate_per_epoch():
    import io
    from bithtm_amd import example
    np.random.seed(1)
    out = io.StringIO()
    example.main(["--epochs", "12", "--input_patterns", "10", "--input_dim", "200", "--column_dim", "256", "--cell_dim", "8", "--input_noise_probability", "0",
                  "--batched_report", "--classifier"], out=out)
    rates = [float(x.rsplit(" ", 1)[1]) for x in out.getvalue().splitlines() if "1-step hit rate of the classifier" in x]
    assert len(rates) == 12 and all(0.0 <= r <= 1.0 for r in rates)
    assert rates[-1] == 1.0, rates                  # (ten noiseless patterns in a fixed order: learned by heart)
    with pytest.raises(SystemExit, match="--batched_report"):
        example.main(["--classifier"], out=io.StringIO())
