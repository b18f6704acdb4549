"""Banks of SDR classifiers on the device (SDRClassifierBank; htm_classifiers_*, htm_set_group_run_active_cells, htm_classifiers_tick;
DESIGN.md section 25).  The contract of every layer: stream i fed (pairs_i, targets_i, resets_i) equals a one-stream object fed the
same, bit for bit.  The stand-alone door holds the bank to n one-stream definitions (bithtm_amd/classifier.py) over the cases of
tests/group_classifier_cases.py -- outputs, weights, rings, counts, total; the model tests hold group.run(classifier=bank) and
group.tick(classifier=bank) to the same members stepped alone with one-stream SDRClassifiers, and to the definition over the
oracle's states."""
import numpy as np
import pytest

import group_classifier_cases as G
from classifier_cases import MODEL_ALPHA, MODEL_SEQUENCE, MODEL_STEPS, MODELS, SPLITS, SPLIT_IDS, hit_rate, model_encoder, model_permanence
from group_classifier_cases import BANK_IDS, GROUP_SIZES


def _bank(p, n, **kw):
    import bithtm_amd as B
    bank = B.SDRClassifierBank(n, buckets=p["buckets"], steps=p["steps"], alpha=p["alpha_q"] / 65536.0, shape=(p["column_dim"], p["cell_dim"], p["max_pairs"]), **kw)
    assert bank.alpha_q == p["alpha_q"] and bank.streams == n
    return bank


def _same_state(bank, singles, what=""):
    """The device's whole state is the one-stream definitions': per stream weights, ring and count, and the one total."""
    got = bank.state_dict()
    assert got["weights"].dtype == np.int32 and got["weights"].shape[0] == len(singles)
    for i, d in enumerate(singles):
        assert np.array_equal(got["weights"][i], d.dense_weights()), (what, "weights of stream", i)
        assert np.array_equal(got["ring"][i], d.ring_arrays(bank.shape[2])), (what, "ring of stream", i)
        assert (int(got["count"][i]), int(got["total"])) == (d.count, d.total), (what, "counters of stream", i)


def _case(name):
    if name == "mixed-gates":
        return G.MIXED, 3, G.mixed_stream()
    return G.banked(name)


# ---- the stand-alone door
@pytest.mark.gpu
@pytest.mark.parametrize("name", ["mixed-gates"] + BANK_IDS)
def test_update_patterns_equals_one_definition_per_stream(name):
    p, n, (index, words, targets, resets) = _case(name)
    want_best, want_dist, singles = G.run_singles(p, index, words, targets, resets)
    bank = _bank(p, n)
    best, dist = bank.update_patterns(index, words, targets, resets=resets, device=0)
    assert best.shape == want_best.shape and np.array_equal(best, want_best), np.argwhere(best != want_best)[:5]
    assert np.array_equal(dist, want_dist), np.argwhere(dist != want_dist)[:5]
    _same_state(bank, singles, name)
    assert any(d.dense_weights().any() for d in singles) or p["buckets"] == 1
    # the streams differ from one another: a member reading a neighbour's rows would show
    assert n == 1 or not np.array_equal(want_dist[0], want_dist[1]) or p["buckets"] == 1


@pytest.mark.gpu
@pytest.mark.parametrize("name,splits", SPLITS, ids=SPLIT_IDS)
def test_splits_change_nothing(name, splits):
    p, (index, words, targets, resets) = G.split_bank(name)
    want_best, want_dist, singles = G.run_singles(p, index, words, targets, resets)
    bank = _bank(p, 3)
    parts, at = [], 0
    for k in splits:
        parts.append(bank.update_patterns(index[:, at:at + k], words[:, at:at + k], targets[:, at:at + k], resets=resets[:, at:at + k], device=0))
        at += k
    assert at == index.shape[1]
    assert np.array_equal(np.concatenate([b for b, _ in parts], axis=1), want_best)
    assert np.array_equal(np.concatenate([q for _, q in parts], axis=1), want_dist)
    _same_state(bank, singles, name)


def _frozen(n, T):
    """A learned stretch, then T frozen steps in ONE call against the one-stream definitions stepped with learning off."""
    p = G.FROZEN_BANK
    (li, lw, lt, lr), (index, words, targets, resets) = G.frozen_stream(n, T)
    bank = _bank(p, n)
    got = bank.update_patterns(li, lw, lt, resets=lr, device=0)
    want_b, want_q, singles = G.run_singles(p, li, lw, lt, lr)
    assert np.array_equal(got[0], want_b) and np.array_equal(got[1], want_q)
    learned = [d.dense_weights() for d in singles]
    assert all(w.any() for w in learned)
    best, dist = bank.update_patterns(index, words, targets, resets=resets, learning=False)
    for i, d in enumerate(singles):
        b, q = d.update(index[i], words[i], targets[i], resets[i], False)
        assert np.array_equal(best[i], b), (i, np.argwhere(best[i] != b)[:5])
        assert np.array_equal(dist[i], q), i
        assert np.array_equal(d.dense_weights(), learned[i])
    _same_state(bank, singles, f"frozen {n} x {T}")
    # ... and a learning call behind it finds the histories the frozen call left
    tail = G.bank_stream(p, n, 4, 1, seed=97, dead=0.0)
    gb, gq = bank.update_patterns(*tail[:3], resets=tail[3])
    for i, d in enumerate(singles):
        b, q = d.update(tail[0][i], tail[1][i], tail[2][i], tail[3][i], True)
        assert np.array_equal(gb[i], b) and np.array_equal(gq[i], q), i
    _same_state(bank, singles, f"behind frozen {n} x {T}")


@pytest.mark.gpu
def test_a_frozen_call_of_sixteen_streams_crosses_its_shrunk_chunk():
    assert G.chunk_steps(G.FROZEN_N, len(G.FROZEN_BANK["steps"])) == 511 < G.FROZEN_T
    _frozen(G.FROZEN_N, G.FROZEN_T)


@pytest.mark.gpu
@pytest.mark.parametrize("T", G.FROZEN_ONE_STEPS)
def test_a_frozen_call_of_one_stream(T):
    _frozen(1, T)


@pytest.mark.gpu
def test_reset_touches_only_the_named_streams_and_the_state_round_trips():
    p, n, (index, words, targets, resets) = G.banked("three-h015")
    singles = [G.definition(p) for _ in range(n)]
    bank = _bank(p, n)

    def both(lo, hi, b=None):
        b = b or bank
        got = b.update_patterns(index[:, lo:hi], words[:, lo:hi], targets[:, lo:hi], device=0)
        for i, d in enumerate(singles):
            wb, wq = d.update(index[i, lo:hi], words[i, lo:hi], targets[i, lo:hi])
            assert np.array_equal(got[0][i], wb) and np.array_equal(got[1][i], wq), (lo, hi, i)
    both(0, 6)
    bank.reset(streams=[False, True, False])
    singles[1].reset()
    assert bank.state_dict()["count"].tolist() == [6, 0, 6]
    both(6, 9)
    _same_state(bank, singles, "behind reset(streams=)")
    bank.reset()
    for d in singles:
        d.reset()
    both(9, 11)
    _same_state(bank, singles, "behind reset()")
    # a second bank takes the state over and goes on as the first
    other = _bank(p, n)
    other.load_state_dict(bank.state_dict())
    both(11, 14, other)
    _same_state(other, singles, "the second bank")
    with pytest.raises(ValueError, match="parameters"):
        _bank(p, n + 1).load_state_dict(bank.state_dict())


@pytest.mark.gpu
def test_a_shared_bank_reads_one_table_and_refuses_to_write_it():
    import bithtm_amd as B
    p = G.SHARED
    w, (index, words, targets, resets) = G.shared_case()
    home = B.HierarchicalTemporalMemory(32, 64, 4, active_columns=4)
    clf = B.SDRClassifier(buckets=p["buckets"], steps=p["steps"], alpha=p["alpha_q"] / 65536.0, shape=(p["column_dim"], p["cell_dim"], p["max_pairs"]))
    with pytest.raises(ValueError, match="not bound"):
        B.SDRClassifierBank.shared(clf, G.SHARED_N)
    clf.bind(home)
    state = clf.state_dict()
    state["weights"] = w
    clf.load_state_dict(state)
    bank = B.SDRClassifierBank.shared(clf, G.SHARED_N)
    with pytest.raises(ValueError, match="learning is refused"):
        bank.update_patterns(index, words, targets)
    # the state of a shared bank that has made no call yet: the owner's table, once, and it round-trips
    fresh = bank.state_dict()
    assert fresh["weights"].shape == (1,) + w.shape and np.array_equal(fresh["weights"][0], w) and fresh["count"].tolist() == [0] * G.SHARED_N
    bank.load_state_dict(fresh)
    assert not isinstance(bank, B.SDRClassifier) and not isinstance(clf, B.SDRClassifierBank)
    best, dist = bank.update_patterns(index, words, targets, resets=resets, learning=False)
    want_b, want_q, singles = G.run_singles(p, index, words, targets, resets, learning=False, weights=[w] * G.SHARED_N)
    assert np.array_equal(best, want_b) and np.array_equal(dist, want_q)
    got = bank.state_dict()
    assert got["weights"].shape[0] == 1 and np.array_equal(got["weights"][0], w) and np.array_equal(clf.state_dict()["weights"], w)
    for i, d in enumerate(singles):
        assert np.array_equal(got["ring"][i], d.ring_arrays(p["max_pairs"])) and int(got["count"][i]) == d.count and int(got["total"]) == d.total
    # the C side refuses what the Python layer refuses, and weights written through the sharer
    import ctypes as C
    eng = home.engine
    assert eng.lib.htm_classifiers_write_weights(bank._clf, eng.h, 0, 0, 0, 1, w.ctypes.data_as(C.c_void_p)) == -4
    tab = (C.c_void_p * G.SHARED_N)(*[1] * G.SHARED_N)
    assert eng.lib.htm_classifiers_update(bank._clf, eng.h, tab, 7, 1, tab, 1, 0, None, 1, C.c_void_p(1), None) == -4
    assert eng.lib.htm_classifier_update(bank._clf, eng.h, C.c_void_p(1), 7, 1, C.c_void_p(1), 1, 0, None, 0, C.c_void_p(1), None) == -1
    # the owner learns on: the next call through the bank sees the new weights; either object may go first
    one = G.stream(p, 5, 7, seed=77)
    clf.update_patterns(one[0], one[1], one[2])
    w2 = clf.state_dict()["weights"]
    assert not np.array_equal(w2, w)
    best2, dist2 = bank.update_patterns(index, words, targets, learning=False)
    want2 = G.run_singles(p, index, words, targets, None, learning=False, weights=[w2] * G.SHARED_N)
    assert np.array_equal(dist2, want2[1])
    eng.lib.htm_classifier_destroy(clf._clf)         # (the owner goes first: the table lives on with the bank)
    clf._clf = None
    best3, dist3 = bank.update_patterns(index, words, targets, learning=False)
    assert np.array_equal(dist3, dist2)


# ---- classified group runs
def _model(name):
    from hip_impl import make_htm
    m = MODELS[name]
    return make_htm(m["input_dim"], m["column_dim"], m["cell_dim"], m["active_columns"], m["seed"], model_permanence(m))


def _solo_clf(enc, **kw):
    import bithtm_amd as B
    return B.SDRClassifier(field=enc.fields[0], steps=MODEL_STEPS, alpha=MODEL_ALPHA, **kw)


def _model_bank(enc, n):
    import bithtm_amd as B
    return B.SDRClassifierBank(n, field=enc.fields[0], steps=MODEL_STEPS, alpha=MODEL_ALPHA)


def _stream_equals(state, i, solo_state, what):
    assert np.array_equal(state["weights"][i], solo_state["weights"]), (what, "weights", i)
    assert np.array_equal(state["ring"][i], solo_state["ring"]), (what, "ring", i)
    assert (int(state["count"][i]), int(state["total"])) == (int(solo_state["count"]), int(solo_state["total"])), (what, "counters", i)


@pytest.mark.gpu
@pytest.mark.parametrize("B", GROUP_SIZES)
@pytest.mark.parametrize("name", list(MODELS))
def test_a_classified_group_run_equals_the_members_alone_and_the_oracle_stream(name, B):
    """group.run(classifier=bank): member i's record and stream i's state are those of the same model stepped alone with a one-stream
    SDRClassifier through run(classifier=), and both are the definition over the ORACLE's states (every member's), whose
    hit rate is the recorded floor."""
    import bithtm_amd as Bm
    enc = model_encoder()
    T = G.GROUP_EPOCHS[name] * len(MODEL_SEQUENCE)
    values = np.stack([G.member_values(i, G.member_missing(i)) for i in range(B)])
    group = Bm.ModelGroup([_model(name) for _ in range(B)])
    bank = _model_bank(enc, B)
    recs = group.run(values, T, encoder=enc, classifier=bank, record=("counters", "class_distribution"))
    state = bank.state_dict()
    assert int(state["total"]) == T
    for i, rec in enumerate(recs):
        solo, clf = _model(name), _solo_clf(enc)
        want = solo.run(values[i], T, encoder=enc, classifier=clf, record=("counters", "class_distribution"))
        assert np.array_equal(rec.classified_bucket, want.classified_bucket) and np.array_equal(rec.classified_probability, want.classified_probability), i
        assert np.array_equal(rec.class_distribution, want.class_distribution), i
        assert np.array_equal(rec.classified_value, want.classified_value, equal_nan=True) and np.array_equal(rec.active_cells, want.active_cells), i
        _stream_equals(state, i, clf.state_dict(), name)
        a, b = group.models[i].state_dict(), solo.state_dict()
        for key in a:
            assert np.array_equal(a[key], b[key]), (i, key)
        o_best, o_dist, targets = G.group_model_stream(name, i, G.member_missing(i))
        assert np.array_equal(rec.classified_bucket, o_best[:, :, 0]) and np.array_equal(rec.class_distribution, o_dist), i
        rates = tuple(hit_rate(o_best, targets, j, h, len(MODEL_SEQUENCE)) for j, h in enumerate(MODEL_STEPS))
        print(name, "member", i, "hit rates", rates)
        assert rates == G.GROUP_HIT_RATE[name][i]


@pytest.mark.gpu
def test_a_classified_group_run_in_split_calls_with_noise_explicit_targets_and_frozen():
    import bithtm_amd as Bm
    name, B = "128x4", 3
    enc = model_encoder()
    values = np.stack([G.member_values(i) for i in range(B)])
    targets = np.stack([(np.arange(10) * (i + 1)) % 7 for i in range(B)])
    targets[1, 4] = -1
    group = Bm.ModelGroup([_model(name) for _ in range(B)])
    solos = [_model(name) for _ in range(B)]
    group.models[2].run(values[2], 2, encoder=enc)          # (member 2 is two steps ahead of member 0: same parity, other rows)
    solos[2].run(values[2], 2, encoder=enc)
    bank = _model_bank(enc, B)
    clfs = [_solo_clf(enc) for _ in range(B)]
    for n, kw in ((17, {}), (3, dict(noise=0.05, noise_seed=[5, 6, 7])), (20, dict(classifier_learning=False))):
        recs = group.run(values, n, encoder=enc, classifier=bank, targets=targets, **kw)
        for i in range(B):
            solo_kw = dict(kw)
            if "noise_seed" in solo_kw:
                solo_kw["noise_seed"] = kw["noise_seed"][i]
            want = solos[i].run(values[i], n, encoder=enc, classifier=clfs[i], targets=targets[i], **solo_kw)
            assert np.array_equal(recs[i].classified_bucket, want.classified_bucket) and np.array_equal(recs[i].classified_probability, want.classified_probability), (n, i)
            assert recs[i].class_distribution is None and np.array_equal(recs[i].step_index, want.step_index)
    state = bank.state_dict()
    for i in range(B):
        _stream_equals(state, i, clfs[i].state_dict(), "split calls")
    with pytest.raises(ValueError, match="3 streams"):
        group.run(values, 1, encoder=enc, classifier=_model_bank(enc, 2))
    with pytest.raises(ValueError, match=r"int \[3, 10\]"):
        group.run(values, 1, encoder=enc, classifier=bank, targets=targets[:, :9])
    with pytest.raises(ValueError, match="classifier= is not available here"):
        group.run(values, 1, encoder=enc, classifier=clfs[0])
    with pytest.raises(ValueError, match="classifier= is not available here"):
        solos[0].run(values[0], 1, encoder=enc, classifier=bank)
    # a run without a classifier behind the classified ones captures nothing and still equals the members alone
    recs = group.run(values, 5, encoder=enc, record=True)
    for i in range(B):
        assert np.array_equal(recs[i].active_cells, solos[i].run(values[i], 5, encoder=enc, record=True).active_cells)


# ---- classified ticks
def _tick_plan(B, ticks, seed=3):
    """Per tick: values [B, 1] (member i on MODEL_SEQUENCE rolled by i), reset flags [B]; some resets (one of a fresh member) and a NaN."""
    rng = np.random.default_rng(seed)
    seq = np.array(MODEL_SEQUENCE)
    values = np.stack([np.roll(seq, -i)[np.arange(ticks) % len(seq)] for i in range(B)], axis=0)[:, :, None].copy()
    resets = rng.random((ticks, B)) < 0.06
    resets[0, B - 1] = True
    resets[13, 0] = True
    values[min(1, B - 1), 7, 0] = np.nan
    return values, resets


@pytest.mark.gpu
@pytest.mark.parametrize("B", [1, 3])
def test_classified_ticks_equal_reset_plus_a_one_step_classified_solo_run(B):
    """Learning ticks, then frozen ones, with per-member resets and a NaN: tick.classified_* and the bank's state are those of the
    members stepped alone, one classified run of one step per tick (a row's reset flag empties the classifier's history too)."""
    import bithtm_amd as Bm
    name, learn_ticks, ticks = "128x4", 44, 56
    enc = model_encoder()
    values, resets = _tick_plan(B, ticks)
    group = Bm.ModelGroup([_model(name) for _ in range(B)])
    solos, clfs = [_model(name) for _ in range(B)], [_solo_clf(enc) for _ in range(B)]
    bank = _model_bank(enc, B)
    for t in range(ticks):
        learn = t < learn_ticks
        tick = group.tick(values[:, t], encoder=enc, resets=resets[t] if resets[t].any() else None, classifier=bank, classifier_learning=learn,
                          class_distribution=True)
        assert tick.classified_bucket.shape == (B, len(MODEL_STEPS)) and tick.class_distribution.shape == (B, len(MODEL_STEPS), bank.buckets)
        for i in range(B):
            want = solos[i].run(values[i, t][None], 1, encoder=enc, classifier=clfs[i], classifier_learning=learn,
                                resets=np.array([resets[t, i]]), record=("counters", "class_distribution"))
            assert tick.classified_bucket[i].tolist() == want.classified_bucket[0].tolist(), (t, i)
            assert np.array_equal(tick.classified_probability[i], want.classified_probability[0]), (t, i)
            assert np.array_equal(tick.class_distribution[i], want.class_distribution[0]), (t, i)
            assert np.array_equal(tick.classified_value[i], want.classified_value[0], equal_nan=True)
            assert tick.active_cells[i] == want.active_cells[0] and tick.step_index[i] == want.step_index[0]
    state = bank.state_dict()
    assert int(state["total"]) == ticks and state["weights"].any()
    for i in range(B):
        _stream_equals(state, i, clfs[i].state_dict(), "ticks")
        a, b = group.models[i].state_dict(), solos[i].state_dict()
        for key in a:
            assert np.array_equal(a[key], b[key]), (i, key)
    # explicit targets, no distribution; the refusals leave the group usable
    tick = group.tick(values[:, 0], encoder=enc, classifier=bank, targets=np.zeros(B, int))
    assert tick.class_distribution is None and tick.classified_bucket.shape == (B, len(MODEL_STEPS))
    with pytest.raises(ValueError, match="streams"):
        group.tick(values[:, 0], encoder=enc, classifier=_model_bank(enc, B + 1))
    with pytest.raises(ValueError, match="classifier= is not available here"):
        group.tick(values[:, 0], encoder=enc, classifier=clfs[0])
    other = Bm.SDRClassifierBank(B, buckets=bank.buckets, steps=MODEL_STEPS, shape=(MODELS[name]["column_dim"], MODELS[name]["cell_dim"], 3))
    with pytest.raises(ValueError, match="shape"):
        group.tick(values[:, 0], encoder=enc, classifier=other, targets=np.zeros(B, int))
    assert group.tick(values[:, 1], encoder=enc).classified_bucket is None


@pytest.mark.gpu
def test_a_scored_and_classified_tick_returns_the_likelihoods_of_the_scored_tick_alone():
    import bithtm_amd as Bm
    name, B, ticks = "128x4", 3, 24
    enc = model_encoder()
    values, resets = _tick_plan(B, ticks)
    both, scored, plain = (Bm.ModelGroup([_model(name) for _ in range(B)]) for _ in range(3))
    kw = dict(learning_period=4, estimation_samples=4, history=16, averaging_window=3, reestimation_period=2)
    lk_both, lk_scored = Bm.AnomalyLikelihood(B, **kw), Bm.AnomalyLikelihood(B, **kw)
    bank, bank_plain = _model_bank(enc, B), _model_bank(enc, B)
    for t in range(ticks):
        r = resets[t] if resets[t].any() else None
        a = both.tick(values[:, t], encoder=enc, resets=r, likelihood=lk_both, classifier=bank, predicted_input=t % 2 == 0)
        b = scored.tick(values[:, t], encoder=enc, resets=r, likelihood=lk_scored, predicted_input=t % 2 == 0)
        c = plain.tick(values[:, t], encoder=enc, resets=r, classifier=bank_plain, class_distribution=t % 3 == 0)
        assert np.array_equal(a.anomaly_likelihood, b.anomaly_likelihood), t
        assert np.array_equal(a.predicted_bucket, b.predicted_bucket) and np.array_equal(a.active_cells, b.active_cells) and np.array_equal(a.segments, b.segments), t
        assert (a.predicted_input is None) == (t % 2 != 0) and (a.predicted_input is None or np.array_equal(a.predicted_input, b.predicted_input))
        assert np.array_equal(a.classified_bucket, c.classified_bucket) and np.array_equal(a.classified_probability, c.classified_probability), t
    sa, sc = bank.state_dict(), bank_plain.state_dict()
    assert all(np.array_equal(sa[k], sc[k]) for k in sa)


@pytest.mark.gpu
def test_views_ticked_with_a_shared_bank_equal_solo_views_with_copies_of_the_weights():
    import bithtm_amd as Bm
    name, n = "128x4", 4
    enc = model_encoder()
    values = G.member_values(0)
    parent = _model(name)
    clf = _solo_clf(enc)
    parent.run(values, 200, encoder=enc, classifier=clf)
    w = clf.state_dict()["weights"]
    assert w.any()
    group = Bm.ModelGroup.views(parent, n)
    bank = Bm.SDRClassifierBank.shared(clf, n)
    solos = [parent.inference_view() for _ in range(n)]

    def copies():
        out = []
        for _ in range(n):
            c = _solo_clf(enc, shape=clf.shape)
            state = c.state_dict()
            state["weights"] = clf.state_dict()["weights"]
            c.load_state_dict(state)
            out.append(c)
        return out

    def ticks(first, count, clfs):
        for t in range(first, first + count):
            v = np.stack([G.member_values(i)[t % 10] for i in range(n)])
            tick = group.tick(v, encoder=enc, classifier=bank, class_distribution=True)
            for i in range(n):
                want = solos[i].run(v[i][None], 1, encoder=enc, classifier=clfs[i], record=("counters", "class_distribution"))
                assert np.array_equal(tick.class_distribution[i], want.class_distribution[0]), (t, i)
                assert tick.classified_bucket[i].tolist() == want.classified_bucket[0].tolist(), (t, i)
    with pytest.raises(ValueError, match="learning is refused"):
        group.tick(np.stack([values[0]] * n), encoder=enc, classifier=bank, classifier_learning=True)
    ticks(0, 12, copies())
    assert np.array_equal(clf.state_dict()["weights"], w)
    # the parent runs on with its classifier: the next view ticks see the new weights
    parent.run(values[::-1].copy(), 20, encoder=enc, classifier=clf)
    assert not np.array_equal(clf.state_dict()["weights"], w)
    ticks(12, 6, copies())


@pytest.mark.gpu
def test_the_capacity_overflow_tick_carries_its_classification():
    import bithtm_amd as Bm
    from bithtm_amd.engine import CapacityError
    I, Cn, K, k, B = 300, 512, 48, 48, 2            # (48 bursting columns a step against pools of 64 rows: the second tick overflows)

    def member(seed):
        tm = Bm.TemporalMemory(Cn, K, distal_projection=Bm.PredictiveProjection(Cn * K, segment_capacity=64), seed=seed)
        np.random.seed(seed)
        return Bm.HierarchicalTemporalMemory(I, Cn, K, active_columns=k, temporal_memory=tm)
    group = Bm.ModelGroup([member(3), member(4)])
    twins = [member(3), member(4)]
    for m, t in zip(group.models, twins):
        t.engine.set_permanence(m.engine.get_permanence())
    bank = Bm.SDRClassifierBank(B, buckets=5, steps=(0, 1))
    clfs = [Bm.SDRClassifier(buckets=5, steps=(0, 1)) for _ in range(B)]
    rng = np.random.default_rng(8)
    X = rng.random((B, 14, I)) < 0.14
    X[0] = X[0, :1]
    raised = overflowed = 0
    for t in range(14):
        targets = np.array([t % 5, (t * 2) % 5])
        try:
            tick = group.tick(X[:, t], classifier=bank, targets=targets)
        except CapacityError as e:
            tick, raised = e.tick, raised + 1
        for i, twin in enumerate(twins):
            try:
                want = twin.run(X[i, t][None, :], 1, classifier=clfs[i], targets=targets[i:i + 1])
                best = np.stack([want.classified_bucket[0], np.rint(want.classified_probability[0] * 65536).astype(np.int64)], axis=-1)
            except CapacityError:
                # the twin's run raised behind its classifier's update and read-back: the step's (bucket, p) pairs are still in the
                # classifier's output buffer on the device -- the overflowing member's tick is held to them
                overflowed += 1
                twin.engine.sync()
                best = clfs[i].read(twin.engine, 1)[0][0]
            assert tick.classified_bucket[i].tolist() == best[:, 0].tolist(), (t, i)
            assert np.rint(tick.classified_probability[i] * 65536).astype(np.int64).tolist() == best[:, 1].tolist(), (t, i)
    assert raised >= 1 and overflowed >= 1 and tick.classified_bucket.shape == (B, 2)
    state = bank.state_dict()
    for i in range(B):
        _stream_equals(state, i, clfs[i].state_dict(), "capacity")
