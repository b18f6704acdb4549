"""KNN classifier on the device (KNNClassifier; htm_knn_*) against its definition, bithtm_amd/knn.py.  Every
comparison is exact: the result rows, the votes rows and the exported store -- pairs, labels, stamps, count, total.  The stand-alone
door (update_patterns) runs the cases of tests/knn_cases.py without stepping a model; the model tests hold run(knn=) to the definition
over the oracle's states and over the stepwise twin's, eagerly and from graphs, on a model and on a view."""
import numpy as np
import pytest

import knn_cases as cases
from knn_cases import CASE_IDS, MODEL


def _knn(p, **kw):
    import bithtm_amd as B
    return B.KNNClassifier(p["labels"], k=p["k"], min_overlap=p["min_overlap"], capacity=p["capacity"], shape=p["shape"], **kw)


def _same_store(knn, d, what=""):
    """The device's whole state is the definition's: the slots' pairs, labels and stamps, count and total."""
    got = knn.state_dict()
    pairs, labels, stamps = d.store_arrays()
    assert (int(got["count"]), int(got["total"])) == (d.count, d.total) == (knn.count, knn.total), (what, "counters")
    assert got["pairs"].dtype == np.int32 and np.array_equal(got["pairs"], pairs), (what, "pairs")
    assert np.array_equal(got["labels"], labels) and np.array_equal(got["stamps"], stamps), (what, "labels, stamps")


def _raw_update(knn, c):
    """A call whose pairs update_patterns would refuse, through the doors run() uses: a device buffer, enqueue, read."""
    from bithtm_amd.networks import HierarchicalTemporalMemory
    if knn._last is None:
        knn._home = HierarchicalTemporalMemory(32, 64, 4, active_columns=4, device=0)
        knn.bind(knn._home)
    engine = knn._engine()
    T, n = c["index"].shape
    pairs = np.empty((T, n, 2), dtype=np.int32)
    pairs[..., 0], pairs[..., 1] = c["index"], c["words"].view(np.int32)
    buf = engine.device_buffer(pairs.nbytes, pairs)
    labels = knn.check_labels(c["labels"])
    knn.enqueue(engine, buf, n, T, knn.upload_labels(engine, labels), labels, 0, c["learning"], True)
    engine.sync()
    best, votes = knn.read(engine, T, True)
    knn.lib.hipFree(buf)
    return best.copy(), votes.copy()


def _update(knn, c):
    if c["raw"]:
        return _raw_update(knn, c)
    return knn.update_patterns(c["index"], c["words"], c["labels"], learning=c["learning"], votes=True, device=0)


# ---- the stand-alone door
@pytest.mark.gpu
@pytest.mark.parametrize("name", CASE_IDS)
def test_update_patterns_equals_the_definition(name):
    p, calls, refused = cases.case(name)
    want, d = cases.expected(name)
    knn = _knn(p)
    for n, (c, (want_best, want_votes)) in enumerate(zip(calls, want)):
        best, votes = _update(knn, c)
        assert np.array_equal(best, want_best), (name, n, np.argwhere(best != want_best)[:5], best[:3], want_best[:3])
        assert np.array_equal(votes, want_votes), (name, n, np.argwhere(votes != want_votes)[:5])
    _same_store(knn, d, name)
    info = knn.info()
    words = p["shape"][0] * ((p["shape"][1] + 31) // 32)
    assert info["table_in_lds"] == int(words * 4 <= cases.TABLE_BYTES) and info["count"] == d.count and info["total"] == d.total
    if refused is not None:                         # one more labelled step than fits: refused, and the object answers as before it
        before = knn.state_dict()
        with pytest.raises(ValueError, match="capacity"):
            knn.update_patterns(refused["index"], refused["words"], refused["labels"], device=0)
        after = knn.state_dict()
        assert all(np.array_equal(before[k], after[k]) for k in before)
        best, votes = _update(knn, calls[-1])
        assert np.array_equal(best, want[-1][0]) and np.array_equal(votes, want[-1][1])
        # ... and so does the library, asked directly
        engine = knn._engine()
        labels = knn.check_labels(refused["labels"])
        ptr = knn.upload_labels(engine, labels)
        import ctypes as C
        rc = knn.lib.htm_knn_update(knn._knn, engine.h, C.c_void_p(knn._bufs["best"][0]), 1, len(labels), C.c_void_p(ptr), len(labels), 0, 1,
                                    C.c_void_p(knn._bufs["best"][0]), None)
        assert rc == -3 and b"capacity" in knn.lib.htm_last_error(engine.h)
        assert knn.info()["count"] == d.count


@pytest.mark.gpu
def test_a_call_split_at_every_position_equals_the_one_call():
    p, calls, _ = cases.case("split-stream")
    (want_best, want_votes), = cases.expected("split-stream")[0]
    d = cases.expected("split-stream")[1]
    c = calls[0]
    T = len(c["index"])
    for cut in range(T + 1):
        knn = _knn(p)
        parts = [knn.update_patterns(c["index"][a:b], c["words"][a:b], c["labels"][a:b], votes=True, device=0) for a, b in ((0, cut), (cut, T))]
        assert np.array_equal(np.concatenate([x[0] for x in parts]), want_best), cut
        assert np.array_equal(np.concatenate([x[1] for x in parts]), want_votes), cut
        _same_store(knn, d, cut)


@pytest.mark.gpu
def test_the_global_table_form_equals_the_lds_form():
    a, b = cases.expected("global-twin")[0], cases.expected("lds-twin")[0]
    assert all(np.array_equal(x[0], y[0]) and np.array_equal(x[1], y[1]) for x, y in zip(a, b))
    got = {}
    for name in ("global-twin", "lds-twin"):
        p, calls, _ = cases.case(name)
        knn = _knn(p)
        got[name] = [_update(knn, c) for c in calls]
        # the scratch table is zero between chunks: the same calls again, frozen, over the table the first ones left
        again = _update(knn, dict(calls[-1], learning=False))
        assert np.array_equal(again[0], got[name][-1][0])
    assert all(np.array_equal(x[0], y[0]) and np.array_equal(x[1], y[1]) for x, y in zip(got["global-twin"], got["lds-twin"]))


@pytest.mark.gpu
def test_state_dict_into_a_fresh_object_continues_identically():
    p, calls, _ = cases.case("around-k")
    want, d = cases.expected("around-k")
    knn = _knn(p)
    for c in calls[:3]:
        _update(knn, c)
    state = knn.state_dict()
    fresh = _knn(p)
    fresh.load_state_dict(state)                    # (held until the object is bound)
    assert fresh.count == knn.count == 3 and fresh.total == knn.total
    for c, (want_best, want_votes) in zip(calls[3:], want[3:]):
        best, votes = _update(fresh, c)
        assert np.array_equal(best, want_best) and np.array_equal(votes, want_votes)
    _same_store(fresh, d)
    fresh.reset()
    assert fresh.count == 0 and fresh.total == d.total and fresh.state_dict()["pairs"].shape == (0, 8, 2)
    best, votes = _update(fresh, calls[1])
    assert (best == [-1, 0, 0, -1, -1]).all() and not votes.any()


# ---- on a model
def _model():
    from hip_impl import make_htm
    m = MODEL
    return make_htm(m["input_dim"], m["column_dim"], m["cell_dim"], m["active_columns"], m["seed"], cases.model_permanence())


def _model_knn(capacity=None):
    p = cases.model_params()
    import bithtm_amd as B
    return B.KNNClassifier(p["labels"], k=p["k"], min_overlap=p["min_overlap"], capacity=capacity or p["capacity"])


@pytest.mark.gpu
@pytest.mark.parametrize("use_graph", [False, True], ids=["eager", "graphs"])
def test_a_run_with_knn_equals_the_definition_over_the_oracles_states(use_graph):
    inputs, labels, names = cases.model_inputs()
    want_best, want_votes, d = cases.model_stream()
    htm, knn = _model(), _model_knn()
    T = len(inputs)
    # in three calls: the store and the total go on across them
    parts = [htm.run(inputs, n, knn=knn, labels=labels, record=("counters", "knn_votes_all"), use_graph=use_graph) for n in (10, 1, T - 11)]
    best = np.concatenate([np.stack([r.knn_label, r.knn_votes, r.knn_overlap, r.knn_nearest_slot, r.knn_nearest_step], 1) for r in parts])
    assert np.array_equal(best, want_best), np.argwhere(best != want_best)[:5]
    assert np.array_equal(np.concatenate([r.knn_votes_all for r in parts]), want_votes)
    _same_store(knn, d)
    rate = cases.hit_rate(best[:, 0])
    print("hit rate of the later passes", rate)
    assert rate == cases.HIT_RATE
    # the model is the model of the same run without knn=
    plain = _model()
    plain.run(inputs, T, record=True, use_graph=use_graph)
    a, b = htm.state_dict(), plain.state_dict()
    for key in a:
        assert np.array_equal(a[key], b[key]), key
    assert parts[0].knn_votes_all.shape == (10, 6) and htm.run(inputs, 2, knn=knn, knn_learning=False, record=True).knn_votes_all is None


@pytest.mark.gpu
def test_a_view_asks_a_trained_parents_store_and_never_stores():
    inputs, labels, names = cases.model_inputs()
    want_best, want_votes, d = cases.model_stream()
    stored = cases.MODEL_PATTERNS * cases.LABELLED_EPOCHS
    htm, knn = _model(), _model_knn()
    htm.run(inputs, stored, knn=knn, labels=labels)
    assert knn.count == stored
    # the twin of the view: the parent's weights, a stream of its own, stepped with process()
    from classifier_cases import pairs_of
    view, twin = htm.inference_view(), htm.inference_view()
    rec = view.run(inputs, 12, knn=knn, labels=np.zeros(len(inputs), int), record=("counters", "knn_votes_all"))
    frozen = cases.definition(cases.model_params())
    frozen.slots, frozen._live, frozen.labels_of, frozen.stamps, frozen.total = d.slots[:stored], d._live[:stored], d.labels_of[:stored], d.stamps[:stored], stored
    for t in range(12):
        sp, tm = twin.process(inputs[(stored + t) % len(inputs)], learning=False)       # (a view starts at its parent's step index)
        index, words = pairs_of(np.asarray(tm.cell_activation), np.sort(np.asarray(sp.active_column)), MODEL["cell_dim"])
        row, votes = frozen.step(zip(index, words), 0, learning=False)
        got = [rec.knn_label[t], rec.knn_votes[t], rec.knn_overlap[t], rec.knn_nearest_slot[t], rec.knn_nearest_step[t]]
        assert got == row and rec.knn_votes_all[t].tolist() == votes, t
    assert knn.count == stored and knn.total == stored + 12
    with pytest.raises(ValueError, match="learning=False"):
        view.run(inputs, 1, knn=knn, learning=True)


@pytest.mark.gpu
def test_knn_and_classifier_together_give_what_each_gives_alone():
    import bithtm_amd as B
    inputs, labels, names = cases.model_inputs()
    T = 30

    def clf():
        return B.SDRClassifier(buckets=6, steps=(0, 1), alpha=0.1)
    both, only_knn, only_clf = _model(), _model(), _model()
    k1, k2, c1, c2 = _model_knn(), _model_knn(), clf(), clf()
    r = both.run(inputs, T, knn=k1, labels=labels, classifier=c1, targets=names, record=("counters", "knn_votes_all", "class_distribution"))
    rk = only_knn.run(inputs, T, knn=k2, labels=labels, record=("counters", "knn_votes_all"))
    rc = only_clf.run(inputs, T, classifier=c2, targets=names, record=("counters", "class_distribution"))
    for f in ("knn_label", "knn_votes", "knn_overlap", "knn_nearest_slot", "knn_nearest_step", "knn_votes_all"):
        assert np.array_equal(getattr(r, f), getattr(rk, f)), f
    for f in ("classified_bucket", "classified_probability", "class_distribution", "active_cells"):
        assert np.array_equal(getattr(r, f), getattr(rc, f)), f
    a, b = k1.state_dict(), k2.state_dict()
    assert all(np.array_equal(a[k], b[k]) for k in a)
    a, b = c1.state_dict(), c2.state_dict()
    assert all(np.array_equal(a[k], b[k]) for k in a)
    assert rk.classified_bucket is None and rc.knn_label is None


@pytest.mark.gpu
def test_a_refused_run_enqueues_nothing_and_the_object_answers_as_before():
    inputs, labels, names = cases.model_inputs()
    htm, knn = _model(), _model_knn(capacity=10)
    htm.run(inputs, 8, knn=knn, labels=labels)
    before, steps = knn.state_dict(), htm.engine.steps
    with pytest.raises(ValueError, match="capacity"):
        htm.run(inputs, 3, knn=knn, labels=labels)  # (three more labelled steps: one too many)
    assert htm.engine.steps == steps
    after = knn.state_dict()
    assert all(np.array_equal(before[k], after[k]) for k in before)
    rec = htm.run(inputs, 2, knn=knn, labels=labels)
    assert knn.count == 10 and knn.total == 10 and (rec.knn_nearest_slot < 8).all()
