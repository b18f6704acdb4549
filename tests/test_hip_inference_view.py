"""Inference views (HierarchicalTemporalMemory.inference_view, ModelGroup.views; htm_create_view): models that share one
trained model's weights in device memory and step streams of their own with learning=False.  The oracle of a view is its twin:
a full copy of the parent (load_state_dict(parent.state_dict())) after reset(), stepped with learning=False -- bit for bit,
alone, in groups (the shared scan, several member chunks, two words per column, rows longer than a chunk), while the parent
keeps learning between view calls, and after the parent is gone.  The parent's weights never move under its views."""

import ctypes as C
import gc

import numpy as np
import pytest

I, CN = 300, 1024
ALL = ("counters", "active_column", "column_prediction", "predicted_input")


def _model(K, seed=5, slots=128, cap=65536):
    import bithtm_amd as B
    tm = B.TemporalMemory(CN, K, distal_projection=B.PredictiveProjection(CN * K, segment_capacity=cap, segment_slots=slots), seed=seed)
    np.random.seed(seed)                          # (the SP's permanences are drawn from NumPy's global stream)
    return B.HierarchicalTemporalMemory(I, CN, K, temporal_memory=tm)


def _inputs(rows, seed, density=0.06):
    return np.random.RandomState(seed).rand(rows, I) < density


def _trained(K, steps=48, seed=5, slots=128, populate=False):
    """A parent that learned a few repeated patterns: its store has matching and active segments."""
    m = _model(K, seed, slots)
    if populate:                                  # (rows of 48 synapses: two chunks each)
        m.engine.populate(1, synapses=48, seed=9, cell_begin=0, cell_end=CN * K // 4)
    pats = _inputs(6, 100 + seed)
    for t in range(steps):
        m.process(pats[t % 6])
    return m, pats


def _twin(parent, K, seed=5, slots=128):
    t = _model(K, seed, slots)
    t.load_state_dict(parent.state_dict())
    t.reset()
    return t


def _i32(a):
    return np.ascontiguousarray(np.asarray(a, np.float32)).view(np.int32)


def _same_step(a, b, what):
    (sa, ta), (sb, tb) = a, b
    for f in ("active_column", "overlaps", "boosted_overlaps"):
        assert np.array_equal(getattr(sa, f), getattr(sb, f)), (what, f)
    for f in ("cell_activation", "cell_prediction"):
        assert np.array_equal(getattr(ta, f), getattr(tb, f)), (what, f)
    wa, wb = ta.winner_cell, tb.winner_cell
    assert (wa is None) == (wb is None), what
    if wa is not None:
        assert all(np.array_equal(x, y) for x, y in zip(wa, wb)), (what, "winner_cell")
    da, db = ta.distal_state, tb.distal_state
    assert (da is None) == (db is None), what
    if da is not None:
        for f in ("matching_segment", "matching_segment_activation", "matching_segment_active", "segment_potential"):
            assert np.array_equal(getattr(da, f), getattr(db, f)), (what, f)
        for f in ("matching_segment_jittered_potential", "max_jittered_potential"):
            assert np.array_equal(_i32(getattr(da, f)), _i32(getattr(db, f))), (what, f)


def _same_stream(v, t, what):
    """Everything the two engines hold: the stream state and the (shared / copied) store, the duty cycles, the step index."""
    a, b = v.engine.export_tm_state(), t.engine.export_tm_state()
    assert a.keys() == b.keys(), what
    for k in a:
        x, y = np.asarray(a[k]), np.asarray(b[k])
        if x.dtype.kind == "f":
            x, y = _i32(x) if x.dtype == np.float32 else x.view(np.int64), _i32(y) if y.dtype == np.float32 else y.view(np.int64)
        assert np.array_equal(x, y), (what, k)
    assert np.array_equal(_i32(v.engine.read_duty_cycle()), _i32(t.engine.read_duty_cycle())), (what, "duty")
    assert v.engine.steps == t.engine.steps, what


def _same_record(r, s, what, fields=ALL):
    from bithtm_amd.engine import RECORD_COUNTERS
    assert np.array_equal(r.step_index, s.step_index), what
    for f in fields:
        if f == "counters":
            for name in RECORD_COUNTERS:
                assert np.array_equal(getattr(r, name), getattr(s, name)), (what, name)
        else:
            assert np.array_equal(getattr(r, f), getattr(s, f)), (what, f)


def _adopt_weights(twin, parent, reset=False):
    """The twin keeps its own stream state and takes the parent's current weights: sp_permanence and the store keys replaced
    (the per-segment potentials of its last scan padded to the new segment count: rows added since were not scanned)."""
    st, ps = twin.state_dict(), parent.state_dict()
    st["sp_permanence"] = ps["sp_permanence"]
    for k in ("tm_S", "tm_slots", "tm_seg_cell", "tm_seg_nsyn", "tm_presyn", "tm_perm", "tm_segcount"):
        st[k] = ps[k]
    if "tm_segment_potential" in st:
        pot = np.zeros(int(ps["tm_S"]), np.asarray(st["tm_segment_potential"]).dtype)
        old = np.asarray(st["tm_segment_potential"])[:len(pot)]
        pot[:len(old)] = old
        st["tm_segment_potential"] = pot
    twin.load_state_dict(st)
    if reset:
        twin.reset()


def _weights(m):
    st = m.engine.read_store()
    return m.engine.get_permanence().tobytes(), {k: np.asarray(v).tobytes() for k, v in st.items()}


@pytest.mark.gpu
@pytest.mark.parametrize("K", [8, 40])
def test_view_equals_its_twin(K):
    """process() for 40 steps, then recorded runs with resets (eager: 20 steps, graphs: 80), bit for bit against the twin."""
    import bithtm_amd as B
    parent, pats = _trained(K)
    v, t = parent.inference_view(), _twin(parent, K)
    assert isinstance(v, B.InferenceView) and v.temporal_memory.last_state.distal_state is None
    xs = _inputs(40, 7)
    for i, x in enumerate(xs):
        _same_step(v.process(x), t.process(x, learning=False), f"process {i}")
    _same_stream(v, t, "after process")
    bank = np.concatenate([pats, _inputs(3, 8)])
    resets = np.zeros(len(bank), bool)
    resets[[0, 4]] = True
    for n in (20, 80):
        r = v.run(bank, n, record=ALL, resets=resets)
        s = t.run(bank, n, learning=False, record=ALL, resets=resets)
        _same_record(r, s, f"run {n}")
        _same_stream(v, t, f"after run {n}")
    v.reset(), t.reset()
    assert np.array_equal(v.predicted_input(), t.predicted_input())
    _same_step(v.process(xs[0]), t.process(xs[0], learning=False), "after reset")


@pytest.mark.gpu
@pytest.mark.parametrize("lean", ["0", "1", "2"])
def test_views_leave_the_parent_weights_alone(lean, monkeypatch):
    """Every schedule a view can take (the launch schedules, pipeline=False, recorded, decoded, with resets, host-fed): the
    parent's permanences and store are byte-identical afterwards."""
    monkeypatch.setenv("BITHTM_LEAN", lean)       # (read when the parent's handle is created; its views take its knobs)
    parent, pats = _trained(8)
    before = _weights(parent)
    views = [parent.inference_view() for _ in range(2)]
    resets = np.zeros(len(pats), bool)
    resets[2] = True
    for v in views:
        for x in pats:
            v.process(x)
        v.run(pats, 70)
        v.run(pats, 30, pipeline=False)
        v.run(pats, 70, record=ALL, resets=resets)
        v.run(pats, 12, record=("predicted_input",), pipeline=False)
        v.predicted_input()
        v.reset()
    import bithtm_amd as B
    group = B.ModelGroup(views)
    group.run(np.stack([pats, pats[::-1]]), 40, record=("counters", "predicted_input"))
    group.process(np.stack([pats[0], pats[1]]))
    after = _weights(parent)
    assert before[0] == after[0]
    assert before[1] == after[1]


ON = {"BITHTM_SHARED_SCAN": "1"}
SHARED = [(ON, 8, 128, False), (dict(ON, BITHTM_SHARED_SCAN_MEMBERS="2"), 8, 128, False), (ON, 40, 128, False),
          (dict(ON, BITHTM_SHARED_SCAN_MEMBERS="2"), 40, 64, True), ({}, 8, 128, False)]
SHARED_IDS = ["K8", "K8-M2", "K40", "K40-M2-long-rows", "K8-per-member-scan"]


@pytest.mark.gpu
@pytest.mark.parametrize("env,K,slots,populate", SHARED, ids=SHARED_IDS)
def test_shared_group_equals_views_alone_and_twins(env, K, slots, populate, monkeypatch):
    """ModelGroup.views(parent, 5), every member on inputs of its own: group.run with records (graphs and eager) and
    group.process, against the same views stepped alone and against twins."""
    import bithtm_amd as B
    for k, val in env.items():
        monkeypatch.setenv(k, val)
    parent, pats = _trained(K, slots=slots, populate=populate)
    if populate:
        assert int(parent.engine.read_store()["seg_nsyn"].max()) > 32
    n = 5
    group = B.ModelGroup.views(parent, n)
    alone = [parent.inference_view() for _ in range(n)]
    twins = [_twin(parent, K, slots=slots) for _ in range(n)]
    banks = np.stack([np.concatenate([pats, _inputs(2, 20 + i)]) for i in range(n)])
    for steps in (70, 9):
        recs = group.run(banks, steps, record=ALL)
        for i in range(n):
            r = alone[i].run(banks[i], steps, record=ALL)
            s = twins[i].run(banks[i], steps, learning=False, record=ALL)
            _same_record(recs[i], r, f"member {i} vs alone, {steps}")
            _same_record(recs[i], s, f"member {i} vs twin, {steps}")
    xs = np.stack([_inputs(1, 40 + i)[0] for i in range(n)])
    rec = group.process(xs)
    for i in range(n):
        alone[i].process(xs[i])
        s = twins[i].run(xs[i][None], 1, learning=False, record=("counters",))
        from bithtm_amd.engine import RECORD_COUNTERS
        for name in RECORD_COUNTERS:
            assert getattr(rec, name)[i] == getattr(s, name)[0], (i, name)
    for i in range(n):
        _same_stream(group.models[i], twins[i], f"member {i}")
        _same_stream(alone[i], twins[i], f"alone {i}")


@pytest.mark.gpu
def test_views_follow_the_parent_while_it_keeps_learning():
    """Parent learns, views step, parent learns more, views step again: after every round the view equals a twin T that keeps
    its own stream state and takes the parent's new weights (sp_permanence and the store) through load_state_dict."""
    import bithtm_amd as B
    K = 8
    parent, pats = _trained(K, steps=24)
    v = parent.inference_view()
    w = parent.inference_view()
    group = B.ModelGroup([w])
    t = _twin(parent, K)
    tw = _twin(parent, K)
    for rnd in range(3):
        if rnd:
            for x in _inputs(10, 200 + rnd):
                parent.process(x)
            parent.run(pats, 20)
            for twin in (t, tw):
                _adopt_weights(twin, parent)
        xs = _inputs(12, 300 + rnd)
        for i, x in enumerate(xs):
            _same_step(v.process(x), t.process(x, learning=False), f"round {rnd} step {i}")
        r = group.run(xs[None], 12, record=ALL)[0]
        s = tw.run(xs, 12, learning=False, record=ALL)
        _same_record(r, s, f"round {rnd} group")
        _same_stream(v, t, f"round {rnd}")
        _same_stream(w, tw, f"round {rnd} group member")


@pytest.mark.gpu
def test_view_lifetime_and_refusals():
    import bithtm_amd as B
    from bithtm_amd import _lib as L
    from bithtm_amd.engine import HtmError
    K = 8
    gc.collect()                                  # (other tests' models on streams of their own would keep the parent unpipelined)
    parent, pats = _trained(K)
    views = [parent.inference_view() for _ in range(2)]
    snap = parent.state_dict()                    # (the views' starting point: the twins are made from it below)
    # a parent left ahead by a streamed run refuses its views' calls until it finishes
    assert parent.engine.run_plan(5, continuing=True)["pipelined"]
    parent.run(pats, 5, continuing=True)
    with pytest.raises(HtmError, match="ahead"):
        views[0].process(pats[0])
    with pytest.raises(HtmError, match="ahead"):
        B.ModelGroup(views).process(np.stack([pats[0], pats[1]]))
    parent.run(pats, 1)
    twins = [_model(K) for _ in range(2)]
    for tw in twins:
        tw.load_state_dict(snap)
        tw.reset()
    # refusals
    v = views[0]
    for call in (lambda: v.process(pats[0], learning=True), lambda: v.run(pats, 3, learning=True), v.state_dict,
                 lambda: v.save("x.npz"), lambda: v.load_state_dict({}), v.grow_pool, v.inference_view):
        with pytest.raises(ValueError):
            call()
    group = B.ModelGroup(views)
    with pytest.raises(ValueError):
        group.run(np.stack([pats, pats]), 2, learning=True)
    with pytest.raises(ValueError):
        group.process(np.stack([pats[0], pats[1]]), learning=True)
    lib = v.engine.lib
    assert lib.htm_write(v.engine.h, L.F_SEG_NSYN, np.zeros(4, np.int32).ctypes.data_as(C.c_void_p), 4) == -4
    assert lib.htm_step(v.engine.h, np.zeros(10, np.uint32).ctypes.data_as(C.c_void_p), 1) == -4
    out = C.c_void_p()
    assert lib.htm_create_view(v.engine.h, C.byref(out)) == -4 and out.value is None
    # the parent (and its engine) goes first: the views keep the weights and still equal their twins
    for tw in twins:                               # (the twins take the parent's last weights: it learned in the runs above)
        _adopt_weights(tw, parent, reset=True)
    for vv in views:
        vv.reset()
    del parent
    gc.collect()
    xs = _inputs(20, 77)
    for i, x in enumerate(xs):
        for vv, tw in zip(views, twins):
            _same_step(vv.process(x), tw.process(x, learning=False), f"orphan step {i}")
    r = group.run(np.stack([xs, xs[::-1]]), 10, record=ALL)
    for i, tw in enumerate(twins):
        _same_record(r[i], tw.run(xs if i == 0 else xs[::-1], 10, learning=False, record=ALL), f"orphan group {i}")
    del group
    # after the parent's engine is re-created (grow_pool), its old views are refused
    p2, pats2 = _trained(K, steps=8)
    old = p2.inference_view()
    p2.grow_pool()
    with pytest.raises(ValueError, match="re-created"):
        old.process(pats2[0])
    with pytest.raises(ValueError, match="re-created"):
        B.ModelGroup([old]).run(pats2[None], 2)
    p2.inference_view().process(pats2[0])        # (new views are fine)


@pytest.mark.gpu
def test_a_view_is_small():
    """At 65 536 columns x 32 cells with the default pool the view's own device bytes are under 10 % of the parent's."""
    import bithtm_amd as B
    m = B.HierarchicalTemporalMemory(1000, 65536, 32)
    v = m.inference_view()
    pb, vb = m.engine.device_bytes(), v.engine.device_bytes()
    assert 0 < vb < 0.1 * pb, (vb, pb)
    v.process(np.random.RandomState(0).rand(1000) < 0.05)
