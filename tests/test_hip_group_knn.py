"""Banks of KNN classifiers on the device (KNNClassifierBank; htm_knns_*) against the definition,
bithtm_amd/knn.py's KNNBankDefinition, and against one-stream KNNClassifiers.  Every comparison is exact: result rows, votes rows and
the exported stores.  The stand-alone door runs the cases of tests/group_knn_cases.py without stepping a model; the group tests hold
ModelGroup.run(knn=bank) to each member run alone with a one-stream object, and a shared bank over views to view.run(knn=) per view."""
import numpy as np
import pytest

import group_knn_cases as cases
import knn_cases as one
from group_knn_cases import CASE_IDS

ROWS = ("knn_label", "knn_votes", "knn_overlap", "knn_nearest_slot", "knn_nearest_step")


def _solo(p, **kw):
    import bithtm_amd as B
    return B.KNNClassifier(p["labels"], k=p["k"], min_overlap=p["min_overlap"], capacity=p["capacity"], shape=p["shape"], **kw)


def _bank(c):
    """The case's bank (and the bound one-stream object a shared case's streams read)."""
    import bithtm_amd as B
    p = c["params"]
    if c["source"] is None:
        return B.KNNClassifierBank(c["streams"], p["labels"], k=p["k"], min_overlap=p["min_overlap"], capacity=p["capacity"], shape=p["shape"]), None
    src = _solo(p)
    for s in c["source"]:
        src.update_patterns(s["index"], s["words"], s["labels"], learning=s["learning"], device=0)
    return B.KNNClassifierBank.shared(src, c["streams"]), src


def _update(bank, x):
    return bank.update_patterns(x["index"], x["words"], x["labels"], learning=x["learning"], votes=True, device=0)


def _same_stores(bank, d, what=""):
    got = bank.state_dict()
    count, pairs, labels, stamps = cases.store_arrays(d)
    assert np.array_equal(got["count"], count) and np.array_equal(bank.count, count) and int(got["total"]) == d.total == bank.total, (what, "counters")
    assert got["count"].dtype == np.int64 and got["pairs"].dtype == np.int32 and np.array_equal(got["pairs"], pairs), (what, "pairs")
    assert np.array_equal(got["labels"], labels) and np.array_equal(got["stamps"], stamps), (what, "labels, stamps")


def _rows(rec):
    return np.stack([getattr(rec, f) for f in ROWS], 1)


# ---- the stand-alone door
@pytest.mark.gpu
@pytest.mark.parametrize("name", CASE_IDS)
def test_update_patterns_equals_the_definition(name):
    c = cases.case(name)
    want, d = cases.expected(name)
    bank, src = _bank(c)
    for n, (x, (want_best, want_votes)) in enumerate(zip(c["calls"], want)):
        best, votes = _update(bank, x)
        assert np.array_equal(best, want_best), (name, n, np.argwhere(best != want_best)[:5], best[best != want_best][:5], want_best[best != want_best][:5])
        assert np.array_equal(votes, want_votes), (name, n, np.argwhere(votes != want_votes)[:5])
    _same_stores(bank, d, name)
    info, p = bank.info(), c["params"]
    words = cases.table_words(p["shape"])
    assert info["n_streams"] == c["streams"] and info["shared"] == int(src is not None) and info["total"] == d.total
    assert info["table_in_lds"] == int(words * 4 <= cases.TABLE_BYTES) and info["queries_per_block"] == cases.queries_of(words)
    if src is None:
        assert info["chunk"] == cases.chunk_of(c["streams"], p["capacity"], words) and info["max_count"] == max(d.count)
        assert info["scratch_bytes"] == cases.scratch_bytes(c["streams"], info["chunk"], p["capacity"], words) <= cases.SCRATCH_BYTES
        # every stream alone is a one-stream object fed the same
        solo = _solo(p)
        solo.load_state_dict(bank.stream_state(c["streams"] - 1))
        assert solo.count == d.count[-1] and solo.total == d.total
    else:
        assert info["chunk"] == cases.CHUNK and info["max_count"] == src.count and src.total == len(c["source"][0]["index"])
        with pytest.raises(ValueError, match="learning is refused"):
            bank.update_patterns(c["calls"][0]["index"], c["calls"][0]["words"], None, learning=True, device=0)
    if c["refused"] is not None:                    # one stream past its capacity: the whole call is refused, every store as it was
        before = bank.state_dict()
        r = c["refused"]
        with pytest.raises(ValueError, match="stream 1.*capacity"):
            bank.update_patterns(r["index"], r["words"], r["labels"], device=0)
        after = bank.state_dict()
        assert all(np.array_equal(before[k], after[k]) for k in before)
        best, votes = _update(bank, c["calls"][-1])
        assert np.array_equal(best, want[-1][0]) and np.array_equal(votes, want[-1][1])
        # ... and so does the library, asked directly (nothing is enqueued: the arguments behind the labels are never looked at)
        import ctypes as C
        engine = bank._engine()
        labels = bank.check_labels(r["labels"])
        ptr = bank.upload_labels(engine, labels)
        best_buf = bank._bufs["best"][0]
        table = (C.c_void_p * c["streams"])(*[best_buf] * c["streams"])
        rc = bank.lib.htm_knns_update(bank._knn, engine.h, table, 1, labels.shape[1], C.c_void_p(ptr), labels.shape[1], 0, 1, C.c_void_p(best_buf), None)
        assert rc == -3 and b"stream 1" in bank.lib.htm_last_error(engine.h)
        assert bank.info()["max_count"] == max(d.count)


@pytest.mark.gpu
def test_a_shared_bank_sees_what_its_source_stores_later():
    c = cases.case("shared-9")
    bank, src = _bank(c)
    x = c["calls"][1]
    first, _ = _update(bank, x)
    d = cases.source_definition(c)
    assert np.array_equal(first, cases.expected("shared-9")[0][1][0])
    more = one.clustered(c["params"]["shape"], 3, 77, centers=3)
    src.update_patterns(*more, device=0)
    d.update(*more)
    from bithtm_amd.knn import KNNBankDefinition
    want, want_votes = KNNBankDefinition.shared(d, c["streams"]).update(x["index"], x["words"], None, False)
    best, votes = _update(bank, x)
    assert np.array_equal(best, want) and np.array_equal(votes, want_votes) and src.count == cases.SLOTS + 8
    assert bank.count.tolist() == [0] * 9 and bank.total == 4 and bank.state_dict()["pairs"].shape == (0, 8, 2)


@pytest.mark.gpu
def test_a_call_split_at_every_position_equals_the_one_call():
    c = cases.case("chunk-plus-3")
    x = c["calls"][0]
    (want_best, want_votes), _ = cases.expected("chunk-plus-3")[0]
    d = cases.run_definition(c, [x])[1]
    T = x["index"].shape[1]
    for cut in range(T + 1):
        bank, _ = _bank(c)
        parts = [bank.update_patterns(x["index"][:, a:b], x["words"][:, a:b], x["labels"][:, a:b], votes=True, device=0) for a, b in ((0, cut), (cut, T))]
        assert np.array_equal(np.concatenate([p[0] for p in parts], 1), want_best), cut
        assert np.array_equal(np.concatenate([p[1] for p in parts], 1), want_votes), cut
        _same_stores(bank, d, cut)
    c = cases.case("mixed-store")                   # (every position of the tick-shaped case: ten calls of one step against one of ten)
    bank, _ = _bank(c)
    whole = {k: np.concatenate([x[k] for x in c["calls"]], 1) for k in ("index", "words", "labels")}
    best, votes = bank.update_patterns(whole["index"], whole["words"], whole["labels"], votes=True, device=0)
    want = cases.expected("mixed-store")[0]
    assert np.array_equal(best, np.concatenate([w[0] for w in want], 1)) and np.array_equal(votes, np.concatenate([w[1] for w in want], 1))
    _same_stores(bank, cases.expected("mixed-store")[1])


@pytest.mark.gpu
def test_reset_of_one_stream_and_a_state_into_a_fresh_bank():
    c = cases.case("counts-0-1-257")
    bank, _ = _bank(c)
    d = cases.run_definition(c, [])[1]
    store, ask = c["calls"]
    _update(bank, store)
    d.update(store["index"], store["words"], store["labels"])
    flags = np.array([False, False, True])
    bank.reset(flags)
    d.reset(flags)
    assert bank.count.tolist() == [0, 1, 0] and bank.total == d.total
    best, votes = _update(bank, ask)
    want = d.update(ask["index"], ask["words"], ask["labels"], False)
    assert np.array_equal(best, want[0]) and np.array_equal(votes, want[1]) and (best[2] == [-1, 0, 0, -1, -1]).all()
    # stream 2 stores again behind its reset: the stamps go on from the one total
    again = cases.call(store["index"][:, :5], store["words"][:, :5], store["labels"][:, :5])
    got, want = _update(bank, again), d.update(again["index"], again["words"], again["labels"])
    assert np.array_equal(got[0], want[0]) and np.array_equal(got[1], want[1])
    _same_stores(bank, d)
    fresh, _ = _bank(c)
    fresh.load_state_dict(bank.state_dict())        # (held until the object is bound)
    assert fresh.count.tolist() == bank.count.tolist() and fresh.total == bank.total
    got, want = _update(fresh, ask), d.update(ask["index"], ask["words"], ask["labels"], False)
    assert np.array_equal(got[0], want[0]) and np.array_equal(got[1], want[1])
    _same_stores(fresh, d)
    bank.reset()
    assert bank.count.tolist() == [0, 0, 0] and bank.state_dict()["pairs"].shape == (0, 8, 2)


# ---- on a group
def _model():
    from hip_impl import make_htm
    m = one.MODEL
    return make_htm(m["input_dim"], m["column_dim"], m["cell_dim"], m["active_columns"], m["seed"], one.model_permanence())


def _model_bank(n):
    import bithtm_amd as B
    p = one.model_params()
    return B.KNNClassifierBank(n, p["labels"], k=p["k"], min_overlap=p["min_overlap"], capacity=p["capacity"])


def _model_knn():
    import bithtm_amd as B
    p = one.model_params()
    return B.KNNClassifier(p["labels"], k=p["k"], min_overlap=p["min_overlap"], capacity=p["capacity"])


@pytest.mark.gpu
@pytest.mark.parametrize("use_graph", [False, True], ids=["eager", "graphs"])
def test_a_group_run_with_a_bank_equals_each_member_alone_with_a_one_stream_object(use_graph):
    import bithtm_amd as Bm
    B = cases.MEMBERS
    want_best, want_votes, d = cases.group_stream()
    members = [cases.member_inputs(i) for i in range(B)]
    inputs, labels = np.stack([m[0] for m in members]), np.stack([m[1] for m in members])
    T = inputs.shape[1]
    group, bank = Bm.ModelGroup([_model() for _ in range(B)]), _model_bank(B)
    solos, knns = [_model() for _ in range(B)], [_model_knn() for _ in range(B)]
    got = [[] for _ in range(B)]
    for n in (10, 1, T - 11):                       # in three calls: the stores and the total go on across them
        recs = group.run(inputs, n, knn=bank, labels=labels, record=("counters", "knn_votes_all"), use_graph=use_graph)
        for i, (rec, solo, knn) in enumerate(zip(recs, solos, knns)):
            alone = solo.run(inputs[i], n, knn=knn, labels=labels[i], record=("counters", "knn_votes_all"), use_graph=use_graph)
            for f in ROWS + ("knn_votes_all", "active_cells", "step_index"):
                assert np.array_equal(getattr(rec, f), getattr(alone, f)), (n, i, f)
            got[i].append(rec)
            state, mine = knn.state_dict(), bank.stream_state(i)
            assert all(np.array_equal(state[k], mine[k]) for k in state), (n, i)
    for i in range(B):
        best = np.concatenate([_rows(r) for r in got[i]])
        assert np.array_equal(best, want_best[i]), (i, np.argwhere(best != want_best[i])[:5])
        assert np.array_equal(np.concatenate([r.knn_votes_all for r in got[i]]), want_votes[i])
        rate = cases.hit_rate(i, best[:, 0])
        print("member", i, "hit rate of the later passes", rate)
        assert rate == cases.HIT_RATES[i]
    _same_stores(bank, d)
    # a frozen call records no votes unless asked, and stores nothing
    rec = group.run(inputs, 2, knn=bank, knn_learning=False, record=True)[1]
    assert rec.knn_votes_all is None and rec.knn_label.shape == (2,) and bank.count.tolist() == [36] * B and bank.total == T + 2


@pytest.mark.gpu
def test_members_at_different_steps_read_their_own_rows_labels():
    import bithtm_amd as Bm
    B = 3
    inputs, labels, _ = one.model_inputs()
    group, bank = Bm.ModelGroup([_model() for _ in range(B)]), _model_bank(B)
    solos, knns = [_model() for _ in range(B)], [_model_knn() for _ in range(B)]
    for i in (1, 2):                                # member i is 2 i steps ahead of member 0 (a group steps members of one parity)
        group.models[i].run(inputs, 2 * i)
        solos[i].run(inputs, 2 * i)
    every = np.stack([inputs] * B), np.stack([labels, np.roll(labels, 1), np.where(labels == 2, -1, labels)])
    recs = group.run(every[0], 20, knn=bank, labels=every[1])
    for i in range(B):
        alone = solos[i].run(inputs, 20, knn=knns[i], labels=every[1][i])
        assert np.array_equal(_rows(recs[i]), _rows(alone)), i
        state, mine = knns[i].state_dict(), bank.stream_state(i)
        assert all(np.array_equal(state[k], mine[k]) for k in state), i


@pytest.mark.gpu
def test_a_refused_group_run_enqueues_nothing_and_the_bank_answers_as_before():
    import bithtm_amd as Bm
    inputs, labels, _ = one.model_inputs()
    p = one.model_params()
    group = Bm.ModelGroup([_model() for _ in range(2)])
    bank = Bm.KNNClassifierBank(2, p["labels"], k=p["k"], capacity=10)
    both = np.stack([inputs] * 2)
    names = np.stack([labels, np.full_like(labels, -1)])
    group.run(both, 8, knn=bank, labels=names)
    before, steps = bank.state_dict(), [m.engine.steps for m in group.models]
    with pytest.raises(ValueError, match="stream 0.*capacity"):
        group.run(both, 3, knn=bank, labels=names)   # (three more labelled steps in stream 0: one too many)
    assert [m.engine.steps for m in group.models] == steps
    after = bank.state_dict()
    assert all(np.array_equal(before[k], after[k]) for k in before)
    group.run(both, 2, knn=bank, labels=names)
    assert bank.count.tolist() == [10, 0] and bank.total == 10
    with pytest.raises(ValueError, match="2 streams"):
        group.run(both, 1, knn=Bm.KNNClassifierBank(3, 6))
    with pytest.raises(ValueError, match="go with knn="):
        group.run(both, 1, labels=names)
    with pytest.raises(ValueError, match="knn= is not available here"):
        group.models[0].run(inputs, 1, knn=bank)


@pytest.mark.gpu
def test_a_shared_bank_over_views_equals_each_view_alone_while_the_parent_keeps_storing():
    import bithtm_amd as Bm
    inputs, labels, _ = one.model_inputs()
    n = 3
    parent, knn, twin_parent = _model(), _model_knn(), _model()
    group = None
    for stored in (12, 12):                         # the parent stores twelve more between the views' calls
        parent.run(inputs, stored, knn=knn, labels=labels)
        twin_parent.run(inputs, stored)
        twin_knn = _model_knn()                     # (a copy of the store as it is now: the lone views' steps advance only the copy's total)
        twin_knn.load_state_dict(knn.state_dict())
        if group is None:
            group, bank = Bm.ModelGroup.views(parent, n), Bm.KNNClassifierBank.shared(knn, n)
            solos = [twin_parent.inference_view() for _ in range(n)]
        rows = np.stack([np.roll(inputs, -5 * i, axis=0) for i in range(n)])
        recs = group.run(rows, 7, knn=bank, record=("counters", "knn_votes_all"))
        for i in range(n):
            alone = solos[i].run(rows[i], 7, knn=twin_knn, record=("counters", "knn_votes_all"))
            for f in ROWS + ("knn_votes_all",):
                assert np.array_equal(getattr(recs[i], f), getattr(alone, f)), (stored, i, f)
        assert (recs[0].knn_nearest_slot >= 0).any()
    assert knn.count == 24 and bank.total == 14 and bank.info()["max_count"] == 24
    with pytest.raises(ValueError, match="learning is refused"):
        group.run(rows, 1, knn=bank, knn_learning=True)


@pytest.mark.gpu
def test_knn_and_classifier_banks_together_give_what_each_gives_alone():
    import bithtm_amd as Bm
    inputs, labels, names = one.model_inputs()
    B, T = 2, 30
    every = np.stack([inputs, np.roll(inputs, -1, axis=0)])
    every_labels, every_names = np.stack([labels, np.roll(labels, -1)]), np.stack([names, np.roll(names, -1)])

    def group():
        return Bm.ModelGroup([_model() for _ in range(B)])

    def clf():
        return Bm.SDRClassifierBank(B, buckets=6, steps=(0, 1), alpha=0.1)
    k1, k2, c1, c2 = _model_bank(B), _model_bank(B), clf(), clf()
    r = group().run(every, T, knn=k1, labels=every_labels, classifier=c1, targets=every_names, record=("counters", "knn_votes_all", "class_distribution"))
    rk = group().run(every, T, knn=k2, labels=every_labels, record=("counters", "knn_votes_all"))
    rc = group().run(every, T, classifier=c2, targets=every_names, record=("counters", "class_distribution"))
    for i in range(B):
        for f in ROWS + ("knn_votes_all",):
            assert np.array_equal(getattr(r[i], f), getattr(rk[i], f)), (i, f)
        for f in ("classified_bucket", "classified_probability", "class_distribution", "active_cells"):
            assert np.array_equal(getattr(r[i], f), getattr(rc[i], f)), (i, f)
        assert rk[i].classified_bucket is None and rc[i].knn_label is None
    a, b = k1.state_dict(), k2.state_dict()
    assert all(np.array_equal(a[k], b[k]) for k in a)
    a, b = c1.state_dict(), c2.state_dict()
    assert all(np.array_equal(a[k], b[k]) for k in a)


# ---- live ticks
@pytest.mark.gpu
@pytest.mark.parametrize("use_graph", [False, True], ids=["eager", "graphs"])
def test_ticks_with_a_bank_equal_a_one_step_run_per_member(use_graph):
    import bithtm_amd as Bm
    B, ticks = cases.MEMBERS, 40
    members = [cases.member_inputs(i) for i in range(B)]
    group, bank = Bm.ModelGroup([_model() for _ in range(B)]), _model_bank(B)
    solos, knns = [_model() for _ in range(B)], [_model_knn() for _ in range(B)]
    for t in range(ticks):
        resets = np.array([t == 7 + i for i in range(B)]) if t in (7, 8, 9) else None       # (a reset does not touch a member's store)
        X, names = np.stack([m[0][t] for m in members]), np.array([m[1][t] for m in members])
        tick = group.tick(X, resets=resets, knn=bank, labels=names, knn_votes_all=True, use_graph=use_graph)
        for i in range(B):
            if resets is not None and resets[i]:
                solos[i].reset()
            alone = solos[i].run(X[i][None], 1, knn=knns[i], labels=names[i:i + 1], record=("counters", "knn_votes_all"), use_graph=use_graph)
            got = [int(getattr(tick, f)[i]) for f in ROWS]
            assert got == _rows(alone)[0].tolist(), (t, i, got, _rows(alone)[0])
            assert np.array_equal(tick.knn_votes_all[i], alone.knn_votes_all[0]) and tick.active_cells[i] == alone.active_cells[0], (t, i)
    for i in range(B):
        state, mine = knns[i].state_dict(), bank.stream_state(i)
        assert all(np.array_equal(state[k], mine[k]) for k in state), i
    assert bank.total == ticks and bank.count.tolist() == [k.count for k in knns] and tick.knn_label.dtype == np.int32 and tick.knn_label.shape == (B,)
    # a frozen tick stores nothing and records no votes unless asked; a full stream refuses the labelled tick with nothing enqueued
    before, steps = bank.state_dict(), [m.engine.steps for m in group.models]
    tick = group.tick(X, knn=bank, labels=names, knn_learning=False, use_graph=use_graph)
    assert tick.knn_votes_all is None and bank.total == ticks + 1 and np.array_equal(bank.count, before["count"])
    full = Bm.KNNClassifierBank(B, 6, k=3, capacity=1)
    group.tick(X, knn=full, labels=np.array([0, -1, -1]), use_graph=use_graph)
    steps = [m.engine.steps for m in group.models]
    with pytest.raises(ValueError, match="stream 0.*capacity"):
        group.tick(X, knn=full, labels=np.array([1, 2, -1]), use_graph=use_graph)
    assert [m.engine.steps for m in group.models] == steps and full.count.tolist() == [1, 0, 0] and full.total == 1


@pytest.mark.gpu
def test_ticks_of_views_with_a_shared_bank_equal_each_view_alone():
    import bithtm_amd as Bm
    inputs, labels, _ = one.model_inputs()
    n = 9                                           # (a last query group of one)
    parent, knn, twin_parent = _model(), _model_knn(), _model()
    parent.run(inputs, 20, knn=knn, labels=labels)
    twin_parent.run(inputs, 20)
    twin_knn = _model_knn()                         # (a copy of the store: the lone views' steps advance only the copy's total)
    twin_knn.load_state_dict(knn.state_dict())
    group, bank = Bm.ModelGroup.views(parent, n), Bm.KNNClassifierBank.shared(knn, n)
    solos = [twin_parent.inference_view() for _ in range(n)]
    for t in range(6):
        if t == 3:                                  # (the parent stores four more between two ticks)
            parent.run(inputs, 4, knn=knn, labels=labels)
            twin_parent.run(inputs, 4)
            twin_knn = _model_knn()
            twin_knn.load_state_dict(knn.state_dict())
        X = np.stack([inputs[(3 * i + t) % len(inputs)] for i in range(n)])
        tick = group.tick(X, knn=bank, knn_votes_all=True)
        for i in range(n):
            alone = solos[i].run(X[i][None], 1, knn=twin_knn, record=("counters", "knn_votes_all"))
            assert [int(getattr(tick, f)[i]) for f in ROWS] == _rows(alone)[0].tolist(), (t, i)
            assert np.array_equal(tick.knn_votes_all[i], alone.knn_votes_all[0]), (t, i)
    assert (tick.knn_nearest_slot >= 0).any() and knn.count == 24 and bank.total == 6 and bank.count.tolist() == [0] * n
    with pytest.raises(ValueError, match="learning is refused"):
        group.tick(X, knn=bank, knn_learning=True)


@pytest.mark.gpu
def test_one_tick_with_everything_equals_the_same_tick_with_each_alone():
    import bithtm_amd as Bm
    B = 3
    enc = Bm.ScalarEncoder([Bm.ScalarField(0.0, 10.0, bits=64, width=9)])
    kw = dict(learning_period=4, estimation_samples=4, history=16, averaging_window=3, reestimation_period=2)

    def parts():
        return (Bm.ModelGroup([_model() for _ in range(B)]), Bm.AnomalyLikelihood(B, **kw), Bm.SDRClassifierBank(B, field=enc.fields[0], steps=(0, 1), alpha=0.1),
                _model_bank(B))
    (ga, la, ca, ka), (gl, ll, _, _), (gc, _, cc, _), (gk, _, _, kk) = parts(), parts(), parts(), parts()
    rng = np.random.default_rng(3)
    for t in range(12):
        values = rng.uniform(0, 10, (B, 1))
        names = rng.integers(-1, 6, B)
        every = ga.tick(values, encoder=enc, likelihood=la, classifier=ca, knn=ka, labels=names, class_distribution=True, knn_votes_all=True)
        scored = gl.tick(values, encoder=enc, likelihood=ll)
        classified = gc.tick(values, encoder=enc, classifier=cc, class_distribution=True)
        near = gk.tick(values, encoder=enc, knn=kk, labels=names, knn_votes_all=True)
        assert np.array_equal(every.anomaly_likelihood, scored.anomaly_likelihood), t
        for f in ("classified_bucket", "classified_probability", "class_distribution"):
            assert np.array_equal(getattr(every, f), getattr(classified, f)), (t, f)
        for f in ROWS + ("knn_votes_all", "active_cells", "predicted_bucket"):
            assert np.array_equal(getattr(every, f), getattr(near, f)), (t, f)
        assert near.classified_bucket is None and classified.knn_label is None and scored.knn_label is None
    a, b = ka.state_dict(), kk.state_dict()
    assert all(np.array_equal(a[k], b[k]) for k in a) and int(a["total"]) == 12
    a, b = ca.state_dict(), cc.state_dict()
    assert all(np.array_equal(a[k], b[k]) for k in a)
