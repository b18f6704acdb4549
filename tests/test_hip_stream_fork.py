"""Stream forks (HierarchicalTemporalMemory.fork, InferenceView.sync / fork, ModelGroup.views(fork=True); htm_view_sync) and the
rolling look-ahead built on them (lookahead()).  The oracle of a fork is its twin: a full copy of the source
(load_state_dict(source.state_dict())) WITHOUT reset(), stepped with learning=False -- bit for bit, at once and over process(),
recorded runs and forecasts, for both step parities and one and two words per column, while the source is left exactly as it
was.  The oracle of lookahead() is its definition: run(every), fork().forecast(horizon), per window, on a full copy."""

import numpy as np
import pytest

from test_hip_inference_view import ALL, CN, I, _adopt_weights, _inputs, _same_record, _same_step, _same_stream, _weights

ACTIVE = 64


def _model(K, seed=5, slots=128, cap=65536):
    """test_hip_inference_view's _model with 64 active columns instead of the default 20: with 20 a new segment samples at most 20
    synapses of which 15 must be met again, which the Spatial Pooler's learning columns never allow inside 50 steps -- no segment
    ever matches, nothing is predicted (measured: 0 matching segments after 48, 49 and 96 steps), and a fork would be compared
    with its twin on an empty Temporal Memory state.  With 64, steps 48 and 49 end with 50 / 10 predictive cells, 90 / 70
    matching segments and 270 to 300 voted inputs."""
    import bithtm_amd as B
    tm = B.TemporalMemory(CN, K, distal_projection=B.PredictiveProjection(CN * K, segment_capacity=cap, segment_slots=slots), seed=seed)
    np.random.seed(seed)                          # (the SP's permanences are drawn from NumPy's global stream)
    return B.HierarchicalTemporalMemory(I, CN, K, active_columns=ACTIVE, temporal_memory=tm)


def _trained(K, steps=48, seed=5, slots=128, populate=False, density=0.06):
    """test_hip_inference_view's _trained on that model: a parent that learned six repeated patterns."""
    m = _model(K, seed, slots)
    if populate:                                  # (rows of 48 synapses: two chunks each)
        m.engine.populate(1, synapses=48, seed=9, cell_begin=0, cell_end=CN * K // 4)
    pats = _inputs(6, 100 + seed, density)
    for t in range(steps):
        m.process(pats[t % 6])
    return m, pats


def _copy(model, K, slots=128, cap=65536, seed=5):
    """The twin of a fork: a full copy of `model` (test_hip_inference_view's _twin WITHOUT its reset())."""
    t = _model(K, seed, slots, cap)
    t.load_state_dict(model.state_dict())
    return t


def _view_twin(parent, K, context, n):
    """The twin of a view that ran `n` steps of `context` since it was made."""
    t = _copy(parent, K)
    t.reset()
    t.run(context, n, learning=False)
    return t


@pytest.mark.gpu
@pytest.mark.parametrize("K,steps,slots,populate", [(8, 48, 128, False), (8, 49, 128, False), (40, 48, 128, False), (40, 49, 128, False),
                                                    (40, 49, 128, True)], ids=["K8-even", "K8-odd", "K40-even", "K40-odd", "K40-long-rows"])
def test_fork_equals_its_twin(K, steps, slots, populate):
    """Both parities of the step index, one and two words per column, rows longer than 32 synapses: the fork is its twin at
    once, over 40 process() steps, and over recorded runs with resets (eager: 20 steps, graphs: 80)."""
    import bithtm_amd as B
    parent, pats = _trained(K, steps=steps, slots=slots, populate=populate)
    if populate:
        assert int(parent.engine.read_store()["seg_nsyn"].max()) > 32
    info = parent.engine.info()
    assert parent.temporal_memory.last_state.cell_prediction.any() and info.matching_segments > 0 and info.has_distal_state
    before = _weights(parent)
    f, t = parent.fork(), _copy(parent, K, slots=slots)
    assert isinstance(f, B.InferenceView) and f.engine.steps == steps
    _same_stream(f, t, "at once")
    _same_stream(f, parent, "fork vs parent")
    assert np.array_equal(f.temporal_memory.last_state.cell_prediction, parent.temporal_memory.last_state.cell_prediction)
    assert np.array_equal(f.predicted_input(), t.predicted_input()) and f.predicted_input().any()
    xs = np.concatenate([_inputs(34, 7), pats])     # (the learned patterns last: the runs below start from predictions)
    for i, x in enumerate(xs):
        _same_step(f.process(x), t.process(x, learning=False), f"process {i}")
    _same_stream(f, t, "after process")
    bank = np.concatenate([pats, _inputs(3, 8)])
    resets = np.zeros(len(bank), bool)
    resets[[2, 5]] = True                           # (the first recorded step, which reads row 7 or 8, is not reset)
    for n in (20, 80):
        r = f.run(bank, n, record=ALL, resets=resets)
        s = t.run(bank, n, learning=False, record=ALL, resets=resets)
        if n == 20:                                 # the first recorded step: "predicted before" is the synced state's
            assert r.predicted_columns_before[0] > 0
            assert r.predicted_columns_before[0] == s.predicted_columns_before[0]
        _same_record(r, s, f"run {n}")
        _same_stream(f, t, f"after run {n}")
    assert _weights(parent) == before


@pytest.mark.gpu
@pytest.mark.parametrize("lean", ["0", "1", "2"])
def test_forks_leave_the_source_alone(lean, monkeypatch):
    """A and its full copy B learn the same inputs, by process() and by pipelined run() calls; A is forked right behind each of
    them (its last launch held back after process()), and the fork runs, forecasts, is synced again and reset in between."""
    monkeypatch.setenv("BITHTM_LEAN", lean)
    a, pats = _trained(8, steps=30)
    b = _copy(a, 8)
    bank = np.concatenate([pats, _inputs(4, 31)])
    f = None
    for rnd in range(3):
        for x in bank[:5]:
            a.process(x), b.process(x)
        f = a.fork() if f is None else f.sync()     # (A's tail is held back here)
        f.process(bank[1])
        f.forecast(3)
        n = 33 + rnd
        a.run(bank, n), b.run(bank, n)
        f.sync()
        f.run(bank, 9, record=ALL)
        f.reset()
        f.run(bank, 4)
        g = f.fork()
        g.forecast(2, min_votes=2)
        f.sync(a)
    assert _weights(a) == _weights(b)
    _same_stream(a, b, "A vs B")
    _same_step(a.process(bank[2]), b.process(bank[2]), "one more step")


@pytest.mark.gpu
def test_resync_overwrites_a_stale_stream():
    K = 8
    parent, pats = _trained(K)
    f = parent.fork()
    foreign = _inputs(9, 77, density=0.12)
    resets = np.zeros(9, bool)
    resets[4] = True
    f.run(foreign, 25, resets=resets)
    s0 = parent.engine.info().segments
    more = np.concatenate([pats[:3], _inputs(5, 78)])
    parent.run(more, 30)
    assert parent.engine.info().segments > s0
    assert f.sync() is f
    t = _copy(parent, K)
    _same_stream(f, t, "after re-sync")
    r, s = f.run(more, 12, record=ALL), t.run(more, 12, learning=False, record=ALL)
    _same_record(r, s, "after re-sync")
    _same_stream(f, t, "after re-sync + run")
    # from a parent just after reset(): no distal state
    parent.reset()
    assert parent.engine.info().has_distal_state == 0
    f.sync()
    t = _copy(parent, K)
    assert f.temporal_memory.last_state.distal_state is None and not f.temporal_memory.last_state.cell_prediction.any()
    _same_stream(f, t, "after the parent's reset")
    for i, x in enumerate(more[:4]):
        _same_step(f.process(x), t.process(x, learning=False), f"after the parent's reset {i}")
    # from a fresh parent at step 0 with an empty store
    fresh = _model(K)
    g, t = fresh.fork(), _copy(fresh, K)
    assert g.engine.steps == 0 and fresh.engine.info().segments == 0
    for i, x in enumerate(more[:4]):
        _same_step(g.process(x), t.process(x, learning=False), f"fresh {i}")
    _same_stream(g, t, "fresh")


@pytest.mark.gpu
def test_fork_of_a_view():
    K = 8
    parent, pats = _trained(K)
    context = np.concatenate([pats[:4], _inputs(3, 41)])
    v = parent.inference_view()
    v.run(context, 7)
    w = v.fork()
    t = _view_twin(parent, K, context, 7)
    _same_stream(w, v, "sibling vs view")
    _same_stream(w, t, "sibling vs twin")
    bank = _inputs(6, 42)
    rv, rw, rt = (m.run(bank, 15, record=ALL, **kw) for m, kw in ((v, {}), (w, {}), (t, dict(learning=False))))
    _same_record(rw, rv, "sibling vs view")
    _same_record(rw, rt, "sibling vs twin")
    _same_stream(w, t, "after the runs")
    assert np.array_equal(w.forecast(4), t.forecast(4))


@pytest.mark.gpu
def test_group_of_forks():
    import bithtm_amd as B
    K, n = 8, 3
    parent, pats = _trained(K)
    group = B.ModelGroup.views(parent, n, fork=True)
    twins = [_copy(parent, K) for _ in range(n)]
    banks = np.stack([np.concatenate([pats, _inputs(2, 50 + i)]) for i in range(n)])
    recs = group.run(banks, 21, record=ALL)
    for i in range(n):
        assert recs[i].predicted_columns_before[0] > 0
        _same_record(recs[i], twins[i].run(banks[i], 21, learning=False, record=ALL), f"member {i}")
        assert np.array_equal(group.models[i].forecast(3), twins[i].forecast(3)), i
        _same_stream(group.models[i], twins[i], f"member {i}")


def _definition(m, inputs, steps, horizon, every, min_votes, max_bits, fork_of, **kw):
    rows, parts = [], []
    for j in range(steps // every):
        parts.append(m.run(inputs, every, **kw))
        rows.append(fork_of(m).forecast(horizon, min_votes, max_bits))
    return np.stack(rows), parts


def _same_parts(record, parts, every, what):
    from bithtm_amd.engine import RECORD_COUNTERS
    for j, p in enumerate(parts):
        sl = slice(j * every, (j + 1) * every)
        assert np.array_equal(record.step_index[sl], p.step_index), (what, j)
        for name in RECORD_COUNTERS + tuple(f for f in ALL if f != "counters"):
            assert np.array_equal(getattr(record, name)[sl], getattr(p, name)), (what, j, name)


@pytest.mark.gpu
@pytest.mark.parametrize("every", [1, 3])
def test_lookahead_equals_its_definition(every):
    K, steps, horizon, min_votes, max_bits = 8, 24, 5, 1, 40
    # (dense patterns, 90 of 300 inputs on: the 15 inputs the noise flips per step leave the active columns, and with them the
    # predictions the windows start from, largely in place -- at 18 inputs on, the windows of every=3 all started from nothing)
    a, pats = _trained(K, density=0.3)
    b = _copy(a, K)
    bank = pats                                     # (the learned cycle goes on: step 48 reads row 0)
    resets = np.zeros(len(bank), bool)
    resets[3] = True
    kw = dict(learning=True, record=ALL, resets=resets, noise=0.05, noise_seed=11)
    a.lookahead_chunk = 3
    rows, rec = a.lookahead(bank, steps, horizon, min_votes, max_bits, every=every, **kw)
    want, parts = _definition(b, bank, steps, horizon, every, min_votes, max_bits, lambda m: m.fork(), **kw)
    assert rows.shape == (steps // every, horizon, I) and rows.dtype == np.bool_
    print("bits per window and row:", want.sum(axis=2).tolist())
    assert want.any() and want[:, 0].any() and (want.sum(axis=2) <= max_bits).all()
    assert np.array_equal(rows, want)
    assert len(rec) == steps
    _same_parts(rec, parts, every, "lookahead")
    assert _weights(a) == _weights(b)
    _same_stream(a, b, "after lookahead")
    _same_step(a.process(bank[1]), b.process(bank[1]), "one more step")


@pytest.mark.gpu
def test_lookahead_on_a_view_and_while_the_pool_grows():
    K, every, horizon = 8, 2, 4
    parent, pats = _trained(K)
    bank = np.concatenate([pats, _inputs(2, 62)])
    v, t = parent.inference_view(), _copy(parent, K)
    t.reset()
    v.lookahead_chunk = 2
    rows = v.lookahead(bank, 10, horizon, every=every)
    want, _ = _definition(t, bank, 10, horizon, every, 1, 0, lambda m: m.fork(), learning=False)
    assert want.any() and np.array_equal(rows, want)
    _same_stream(v, t, "view after lookahead")
    with pytest.raises(ValueError):
        v.lookahead(bank, 4, 2, learning=True)
    # a default-sized pool that has to grow inside the call: the engine, and with it the kept fork, is made anew
    import bithtm_amd as B
    models = []
    for _ in range(2):
        np.random.seed(3)
        m = B.HierarchicalTemporalMemory(I, 256, K, active_columns=16, seed=3)
        # (16 active columns: a new segment samples 16 synapses, one more than the matching threshold -- with fewer it would be
        # recycled at once and the pool would never fill.)  3 900 of the default pool's 8 192 segments are taken: the look between
        # two chunks asks for growth once fewer than 129 x 2 x 16 = 4 128 are free, 165 new segments from here -- a dozen steps of
        # new inputs, inside the call's first chunks
        m.engine.populate(2, synapses=16, seed=9, cell_begin=0, cell_end=1950)
        models.append(m)
    a, b = models
    noisy = _inputs(72, 63, density=0.1)
    first, cap = a.engine, a.engine.segment_capacity
    assert a.engine._auto_grow and cap == 8192 and a.engine.info().segments == 3900
    a.lookahead_chunk = 3
    steps = 72
    rows = a.lookahead(noisy, steps, 3, every=6)
    want, _ = _definition(b, noisy, steps, 3, 6, 1, 0, lambda m: m.fork())
    assert a.engine is not first and a.engine.segment_capacity > cap
    assert np.array_equal(rows, want)
    assert _weights(a) == _weights(b)
    _same_stream(a, b, "after growth")


def _stream_bytes(m):
    """The stream part of what an engine exports (not the store, which is the parent's), as bytes."""
    st = m.engine.export_tm_state()
    keys = [k for k in st if k.startswith(("prev_", "matching_", "max_", "has_")) or k == "step_index"]
    assert len(keys) >= 8, keys
    return {k: np.asarray(st[k]).tobytes() for k in keys}, m.engine.read_duty_cycle().tobytes(), m.engine.steps


@pytest.mark.gpu
def test_an_open_phase_is_refused():
    """A source with a step open phase by phase (htm_sp_phase: a winner list from the host) is refused by the library and by
    sync() and fork(); the fork is unchanged, and once the step is closed the sync goes through.  (A view cannot have a phase
    open -- htm_sp_phase refuses views -- so that side of the library's check is asserted through that refusal.)"""
    from bithtm_amd import _lib as L
    K = 8
    parent, pats = _trained(K)
    f = parent.fork()
    f.process(pats[0])
    lib = parent.engine.lib
    before = _stream_bytes(f)
    cols = np.arange(0, 2 * ACTIVE, 2, dtype=np.int32)
    parent.engine.sp_phase(L.SP_ACTIVE, cols, np.int32)
    assert lib.htm_view_sync(f.engine.h, parent.engine.h) == -4 and b"open" in lib.htm_last_error(f.engine.h)
    for call in (f.sync, parent.fork, f.fork, lambda: parent.lookahead(pats, 2, 2)):
        with pytest.raises(ValueError):
            call()
    assert _stream_bytes(f) == before
    assert lib.htm_sp_phase(f.engine.h, L.SP_ACTIVE, cols.ctypes.data_as(L.C.c_void_p), cols.size) == -4      # (no phase opens on a view)
    assert _stream_bytes(f) == before
    parent.engine.tm_step(cols, learning=False)     # the step is closed
    f.sync()
    _same_stream(f, parent, "once the step is closed")
    t = _copy(parent, K)
    _same_step(f.process(pats[1]), t.process(pats[1], learning=False), "the fork of the closed step")


@pytest.mark.gpu
def test_sync_to_an_older_view_clears_rows_above_its_count():
    """v1 stopped when the store had S1 segments.  The parent learns on; v2, made afterwards, steps on the new weights and ends
    with matching segments at and above S1.  v2.sync(v1) must leave those rows "not matching": v2 then equals v1's twin (a full
    copy that ran v1's steps, given the parent's current weights), whose bitmap never had them -- also once the next call has
    raised the count to the parent's again."""
    K = 8
    parent, pats = _trained(K)
    context = np.concatenate([pats[:4], _inputs(3, 41)])
    v1 = parent.inference_view()
    v1.run(context, 7)
    t = _view_twin(parent, K, context, 7)
    s1 = parent.engine.info().segments
    fresh = _inputs(4, 91)
    parent.run(fresh, 40)                           # four new patterns, ten laps: their segments have ids from S1 on
    assert parent.engine.info().segments > s1
    v2 = parent.inference_view()
    v2.run(fresh, 9)
    stale = np.asarray(v2.engine.export_tm_state()["matching_segment"])
    assert (stale >= s1).any(), "v2 matches no segment above v1's count: the test would show nothing"
    assert v2.sync(v1) is v2
    _adopt_weights(t, parent)
    # a call that steps nothing raises both views' counts to the parent's (view_enter): v2's matching segments are then read over
    # all the rows it had set in its earlier life, and must be v1's -- none at or above S1
    v1.predicted_input(), v2.predicted_input()
    m1, m2 = (np.asarray(v.engine.export_tm_state()["matching_segment"]) for v in (v1, v2))
    assert v2.engine.info().segments > s1 and np.array_equal(m2, m1) and not (m2 >= s1).any()
    bank = np.concatenate([fresh, pats[:2]])
    r2, r1, rt = (m.run(bank, 13, record=ALL, **kw) for m, kw in ((v2, {}), (v1, {}), (t, dict(learning=False))))
    _same_record(r2, r1, "v2 vs v1")
    _same_record(r2, rt, "v2 vs v1's twin")
    _same_stream(v2, t, "after the runs")


@pytest.mark.gpu
def test_a_source_that_is_ahead_is_refused():
    """A model left ahead by a streamed run (the only model alive: another one on another stream would keep it from working
    ahead) refuses to be forked or synced to, in the library and in Python, until the stream has ended; its fork is unchanged."""
    import bithtm_amd as B
    parent, pats = _trained(8)
    f = parent.fork()
    f.process(pats[0])
    lib = parent.engine.lib
    before = f.engine.export_tm_state()
    assert parent.engine.run_plan(5, continuing=True)["pipelined"]
    parent.run(pats, 5, continuing=True)
    assert lib.htm_view_sync(f.engine.h, parent.engine.h) == -4 and b"ahead" in lib.htm_last_error(f.engine.h)
    for call in (f.sync, parent.fork, f.fork, lambda: parent.lookahead(pats, 2, 2), lambda: B.ModelGroup.views(parent, 2, fork=True)):
        with pytest.raises(ValueError):
            call()
    parent.run(pats, 2)
    after = f.engine.export_tm_state()
    assert f.engine.steps == 49 and before.keys() == after.keys()
    stream = [k for k in before if k.startswith(("prev_", "matching_", "max_", "has_")) or k == "step_index"]      # (the store is the parent's, which learned)
    assert len(stream) >= 8, stream
    for key in stream:
        assert np.asarray(before[key]).tobytes() == np.asarray(after[key]).tobytes(), key
    f.sync()
    _same_stream(f, parent, "once the stream has ended")


@pytest.mark.gpu
def test_refusals_change_nothing():
    import bithtm_amd as B
    from bithtm_amd.engine import HtmError
    K = 8
    parent, pats = _trained(K)
    other, _ = _trained(K, steps=20, seed=6)
    f, t = parent.fork(), _copy(parent, K)
    f.process(pats[0]), t.process(pats[0], learning=False)
    lib = parent.engine.lib
    # the library's refusals
    assert lib.htm_view_sync(None, parent.engine.h) == -1 and lib.htm_view_sync(f.engine.h, None) == -1
    for view, source, word in ((f, f, b"one handle"), (parent, f, b"not an inference view"), (f, other, b"share weights"),
                               (f, other.inference_view(), b"share weights")):
        assert lib.htm_view_sync(view.engine.h, source.engine.h) == -4
        assert word in lib.htm_last_error(view.engine.h)
    with pytest.raises(HtmError):
        f.engine.view_sync(other.engine)
    # the Python surface
    for call in (lambda: f.sync(other), lambda: f.sync(other.inference_view()), lambda: f.sync(f), lambda: f.sync(object()),
                 lambda: f.lookahead(pats, 4, 2, learning=True), lambda: parent.lookahead(pats, 5, 2, every=2),
                 lambda: parent.lookahead(pats, 4, 0), lambda: parent.lookahead(pats, 4, 2, every=0),
                 lambda: parent.lookahead(pats, 4, 2, min_votes=0), lambda: parent.lookahead(pats, 4, 2, record=("nothing",)),
                 lambda: parent.lookahead(pats, 4, 2, resets=np.zeros(3, bool)), lambda: parent.lookahead(pats, 4, 2, noise=1.5),
                 lambda: parent.lookahead(pats[:, :7], 4, 2)):
        with pytest.raises(ValueError):
            call()
    assert getattr(parent, "_la_fork", None) is None          # (a look-ahead refused for its arguments has made no view)
    _same_stream(f, t, "the fork after the refused calls")
    _same_step(f.process(pats[1]), t.process(pats[1], learning=False), "the fork after the refused calls")
    # models that cannot be forked
    wide = B.HierarchicalTemporalMemory(I, 64, 65)
    host = B.HierarchicalTemporalMemory(I, CN, K, spatial_pooler=B.SpatialPooler(I, CN, 20, boosting=_Boost(CN, 20)))
    assert host.engine is not None and not host.spatial_pooler._plain
    for m in (wide, host):
        with pytest.raises(ValueError):
            m.fork()
        with pytest.raises(ValueError):
            m.lookahead(pats, 2, 1)
    # a view whose parent's engine was re-created
    six = parent.engine.steps
    parent.grow_pool()
    assert parent.engine.steps == six
    for call in (f.sync, f.fork, lambda: f.lookahead(pats, 2, 1)):
        with pytest.raises(ValueError):
            call()
    g = parent.fork()                               # (new forks are made of the new engine)
    _same_stream(g, parent, "a fork of the regrown parent")


def _Boost(output_dim, active_outputs):
    """A plug-in boosting object that lives on the host: a subclass of the device's own kind is not the device's own."""
    import bithtm_amd as B

    class Boost(B.ExponentialBoosting):
        pass
    return Boost(output_dim, active_outputs)
