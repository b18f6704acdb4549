"""Batched stand-alone Temporal Memory runs (include/bithtm_hip.h: htm_tm_run): TemporalMemory.run over
a device bank of active-column lists against the same steps taken one by one with process() (and reset()) -- every record
field and the whole state left behind, bit for bit -- and against the oracle; list order and edge shapes; resets; how calls
compose; graph reuse; the device's guard against a bad row; the refusals; and that a fused model beside it is untouched."""

import gc
from types import SimpleNamespace

import numpy as np
import pytest

from test_hip_run_record import ALL, _assert_record, _bank, _twins
from test_hip_sequence_reset import RESETS, _assert_reset_steps, _assert_same_state

SHAPES = [(1024, 8, 40), (512, 48, 48)]
SHAPE_IDS = ["1024x8", "512x48"]


def _lists(C, n, rows=8, seed=3, base=4):
    """`rows` lists of n distinct columns: `base` random rows, then the same rows with a tenth of their ids exchanged (so that
    the Temporal Memory comes to predict), each in random order."""
    rng = np.random.RandomState(seed)
    out = [rng.choice(C, n, replace=False) for _ in range(min(base, rows))]
    for r in range(base, rows):
        row = out[r % base].copy()
        m = max(1, n // 10)
        row[rng.choice(n, m, replace=False)] = rng.choice(np.setdiff1d(np.arange(C), row), m, replace=False)
        out.append(row)
    return np.asarray(out, dtype=np.int32)


def _tms(C, K, count=2, seed=5):
    import bithtm_amd as B
    return [B.TemporalMemory(C, K, seed=seed) for _ in range(count)]


def _expected(tm, lists, start, steps, learning=True, resets=None):
    """Step `tm` through rows start, start + 1, ... of `lists` with process() (reset() before a flagged row): (counters, sorted
    lists, column predictions) as test_hip_run_record._expected reads them from the States and info()."""
    counters, cols, preds = [], [], []
    for t in range(start, start + steps):
        row = lists[t % len(lists)]
        if resets is not None and resets[t % len(lists)]:
            tm.reset()
        before = int(tm.last_state.cell_prediction.any(axis=1).sum())
        st = tm.process(SimpleNamespace(active_column=row), learning=learning)
        info = tm._engine.info()
        pred = st.cell_prediction.any(axis=1)
        counters.append([len(row), int(st.active_column_bursting.sum()), before, int(pred.sum()), len(st.active_cell[0]),
                         len(st.winner_cell[0]), info.segments, info.recycled_segments + info.appended_segments])
        cols.append(np.sort(row))
        preds.append(pred)
    return (np.asarray(counters, np.int32).reshape(steps, 8), np.asarray(cols, np.int32).reshape(steps, lists.shape[1]),
            np.asarray(preds, bool).reshape(steps, tm.column_dim))


def _assert_same_tm(a, b, but=()):
    """The whole exported state (cell words, winner list, the last scan's State fields, the store with its float32 permanences,
    segments per cell), the counters of info() with the sticky flags (every field but those of `but`), and the step index."""
    from bithtm_amd import _lib as L
    ea, eb = a._engine, b._engine
    sa, sb = ea.export_tm_state(), eb.export_tm_state()
    assert set(sa) == set(sb)
    for key in sa:
        x, y = np.asarray(sa[key]), np.asarray(sb[key])
        if x.dtype == np.float32:
            x, y = x.view(np.uint32), y.view(np.uint32)
        assert np.array_equal(x, y), key
    assert np.array_equal(ea.read(L.F_WINNER_WORDS, np.uint32, ea.cell_words), eb.read(L.F_WINNER_WORDS, np.uint32, eb.cell_words))
    ia, ib = ea.info(), eb.info()
    for name, _ in L.HtmInfo._fields_:
        assert name in but or getattr(ia, name) == getattr(ib, name), name
    assert ea.steps == eb.steps


@pytest.mark.gpu
@pytest.mark.parametrize("eager", [False, True], ids=["graph", "eager"])
@pytest.mark.parametrize("shape", SHAPES, ids=SHAPE_IDS)
def test_run_equals_stepwise(shape, eager, monkeypatch):
    """80 learning steps, 20 with learning off, every record field and the state == the twin stepped with process(); then an
    unrecorded 37-step call; by graph replay, and launched eagerly under the library's own policy for short calls."""
    if eager:
        monkeypatch.setenv("BITHTM_EAGER_BELOW", "64")
    C, K, n = shape
    lists = _lists(C, n)
    tm, twin = _tms(C, K)
    rec = tm.run(lists, 80, record=ALL)
    _assert_record(rec, _expected(twin, lists, 0, 80), what="learning")
    assert rec.predicted_columns.max() > 0 and rec.new_segments.sum() > 0      # (not an idle Temporal Memory)
    assert np.array_equal(rec.step_index, np.arange(80)) and rec.predicted_input is None
    rec = tm.run(lists, 20, learning=False, record=ALL)
    _assert_record(rec, _expected(twin, lists, 80, 20, learning=False), what="learning off")
    _assert_same_tm(tm, twin)
    last, want = tm.last_state, twin.last_state
    assert np.array_equal(last.cell_prediction, want.cell_prediction) and np.array_equal(last.active_column_bursting, want.active_column_bursting)
    assert np.array_equal(last.active_cell[0], want.active_cell[0]) and np.array_equal(last.winner_cell[1], want.winner_cell[1])
    assert tm.run(lists, 37) is None
    _expected(twin, lists, 100, 37)
    _assert_same_tm(tm, twin)
    assert tm._engine.graph_count() > 0                         # (the 80-step call replays graphs under either policy)


@pytest.mark.gpu
@pytest.mark.parametrize("K", [8, 48])
def test_run_equals_the_oracle(K):
    """TemporalMemoryOracle over 90 steps: per step the recorded column predictions and counts of one 90-step call, and the
    active cells, winner cells and predictions of a second Temporal Memory that takes the steps as one-step run() calls; then
    the segment store."""
    from oracle import TemporalMemoryOracle, canonical_synapses
    C, n, steps = 1024, 40, 90
    lists = _lists(C, n, rows=10, seed=21)
    tm, single = _tms(C, K)
    ora = TemporalMemoryOracle(C, K, seed=5)
    rec = tm.run(lists, steps, record=ALL)
    for t in range(steps):
        o = ora.step(np.sort(lists[t % 10]).astype(np.int64))
        single.run(lists, 1)
        s = single.last_state
        assert np.array_equal(rec.column_prediction[t], o.cell_prediction.any(axis=1)), t
        assert rec.active_cells[t] == len(o.active_cell[0]) and rec.winner_cells[t] == len(o.winner_cell[0]), t
        assert rec.bursting_columns[t] == int(o.active_column_bursting.sum()), t
        assert np.array_equal(s.cell_activation, o.cell_activation) and np.array_equal(s.cell_prediction, o.cell_prediction), t
        got, want = (np.sort(w[0].astype(np.int64) * K + w[1]) for w in (s.winner_cell, o.winner_cell))
        assert np.array_equal(got, want), t
        assert np.array_equal(s.distal_state.matching_segment, o.distal_state.matching_segment), t
    assert rec.predicted_columns.max() > 0 and rec.new_segments.sum() > 0
    co = canonical_synapses(ora.seg_cell[:ora.S], ora.presyn[:ora.S], ora.perm[:ora.S])
    for x in (tm, single):
        st = x._engine.read_store()
        cx = canonical_synapses(st["seg_cell"], st["presyn"], st["perm"])
        assert len(cx) == len(co) and all(p[0] == q[0] and np.array_equal(p[1], q[1]) and np.array_equal(p[2].view(np.int32), q[2].view(np.int32))
                                          for p, q in zip(cx, co))


@pytest.mark.gpu
def test_row_order_does_not_matter():
    """Each row shuffled: the same record and the same state as the sorted rows."""
    C, K, n = 1024, 8, 40
    lists = _lists(C, n)
    a, b = _tms(C, K)
    ra = a.run(np.sort(lists, axis=1), 60, record=ALL)
    rng = np.random.RandomState(1)
    rb = b.run(np.stack([row[rng.permutation(n)] for row in lists]), 60, record=ALL)
    for f in ("active_column", "column_prediction", "bursting_columns", "predicted_columns", "active_cells", "winner_cells", "segments", "new_segments"):
        assert np.array_equal(getattr(ra, f), getattr(rb, f)), f
    assert (np.diff(ra.active_column, axis=1) > 0).all() and ra.predicted_columns.max() > 0
    _assert_same_tm(a, b)


@pytest.mark.gpu
def test_edge_shapes():
    """column_dim = 1000 (no multiple of 32) with ids 0 and 999; n = 1; n = active_columns and n < active_columns on one handle,
    with -1 in the pad slots at the C ABI; one row; steps that are no multiple of the rows; a call that starts at an odd step."""
    C, K = 1000, 8
    inner = _lists(C - 2, 38, rows=8, seed=7) + 1               # ids 1 .. 998, and in every row 0 and 999
    lists = np.concatenate([inner[:, :19], np.full((8, 1), 999, np.int32), inner[:, 19:], np.zeros((8, 1), np.int32)], axis=1)
    assert all(0 in row and 999 in row and len(set(row)) == 40 for row in lists)
    tm, twin = _tms(C, K)
    rec = tm.run(lists, 43, record=ALL)                        # (43: no multiple of 8; the next call starts at an odd step)
    _assert_record(rec, _expected(twin, lists, 0, 43), what="1000 columns")
    assert (rec.active_column[:, 0] == 0).all() and (rec.active_column[:, -1] == 999).all()
    rec = tm.run(lists, 30, record=ALL)
    _assert_record(rec, _expected(twin, lists, 43, 30), what="from an odd step")
    assert rec.step_index[0] == 43 and rec.predicted_columns.max() > 0 and rec.new_segments.sum() > 0
    # fewer columns than the handle's active_columns, on the same handle: the record says n, the pad slots of the ABI's rows -1
    short = _lists(C, 24, rows=5, seed=8)
    rec = tm.run(short, 21, record=ALL)
    _assert_record(rec, _expected(twin, short, 73, 21), what="n < active_columns")
    assert (rec.active_columns == 24).all() and rec.active_column.shape == (21, 24)
    eng = tm._engine
    assert eng.active_columns == 40
    raw = eng.tm_run(eng.upload_lists(short), 5, 24, 6, record=("active_column", "counters"))
    _expected(twin, short, 94, 6)
    assert (raw["active_column"][:, 24:] == -1).all() and raw["active_column"].shape == (6, 40) and (raw["counters"][:, 0] == 24).all()
    assert np.array_equal(raw["active_column"][:, :24], np.sort(short[(94 + np.arange(6)) % 5], axis=1))
    one = np.array([[999], [0], [517]], dtype=np.int32)         # n = 1
    rec = tm.run(one, 7, record=ALL)
    _assert_record(rec, _expected(twin, one, 100, 7), what="n = 1")
    single = lists[3:4]                                         # n_rows = 1
    rec = tm.run(single, 9, record=ALL)
    _assert_record(rec, _expected(twin, single, 107, 9), what="one row")
    _assert_same_tm(tm, twin)


@pytest.mark.gpu
def test_resets_in_a_run_equal_reset_and_process():
    """resets=[1,0,0,1,1,0,0,0] == reset() + process(): record and state; reset steps predict nothing before and score 1; the
    same run without flags differs."""
    C, K, n = 1024, 8, 40
    lists = _lists(C, n)
    tm, twin, plain = _tms(C, K, 3)
    rec = tm.run(lists, 80, record=ALL, resets=RESETS)
    _assert_record(rec, _expected(twin, lists, 0, 80, resets=RESETS), what="learning")
    _assert_reset_steps(rec, RESETS, 0)
    assert rec.predicted_columns.max() > 0 and rec.new_segments.sum() > 0
    rec2 = tm.run(lists, 21, learning=False, record=ALL, resets=RESETS)
    _assert_record(rec2, _expected(twin, lists, 80, 21, learning=False, resets=RESETS), what="learning off")
    _assert_reset_steps(rec2, RESETS, 80)
    _assert_same_tm(tm, twin)
    other = plain.run(lists, 80, record=ALL)
    assert not np.array_equal(rec.predicted_columns_before, other.predicted_columns_before)
    assert other.predicted_columns_before[40:][RESETS[np.arange(40, 80) % 8]].max() > 0


@pytest.mark.gpu
def test_calls_compose():
    """30 + 1 + 49 steps == one 80-step call; process() calls between run() calls; reset() before a run."""
    C, K, n = 1024, 8, 40
    lists = _lists(C, n)
    a, b, c, twin = _tms(C, K, 4)
    whole = a.run(lists, 80, record=ALL)
    parts = [b.run(lists, m, record=ALL) for m in (30, 1, 49)]
    for f in ("active_column", "column_prediction", "predicted_columns_before", "predicted_columns", "bursting_columns", "segments", "new_segments"):
        assert np.array_equal(getattr(whole, f), np.concatenate([getattr(p, f) for p in parts])), f
    _assert_same_tm(a, b)
    done = 0
    for m, how in ((11, "run"), (3, "process"), (20, "run"), (1, "process"), (25, "run")):
        if how == "run":
            rec = c.run(lists, m, record=ALL)
            _assert_record(rec, _expected(twin, lists, done, m), what=f"run of {m} from {done}")
        else:
            for t in range(done, done + m):
                x = SimpleNamespace(active_column=lists[t % 8])
                got, want = c.process(x), twin.process(x)
                assert np.array_equal(got.cell_prediction, want.cell_prediction), t
        done += m
    c.reset()
    twin.reset()
    rec = c.run(lists, 12, record=ALL)
    _assert_record(rec, _expected(twin, lists, done, 12), what="after reset()")
    assert rec.predicted_columns_before[0] == 0 and rec.anomaly_score[0] == 1
    _assert_same_tm(c, twin)


@pytest.mark.gpu
def test_default_pool_grows_inside_a_run():
    """A default-sized pool that grows in the middle of run(): the lists are uploaded to the new engine too."""
    C, K, n = 1024, 8, 20
    rng = np.random.RandomState(4)
    lists = np.stack([rng.choice(C, n, replace=False) for _ in range(300)]).astype(np.int32)     # (no repeats: nearly every column bursts)
    tm, twin = _tms(C, K)
    tm.run(lists, 1)
    first = tm._engine
    rec = tm.run(lists, 299, record=ALL)
    assert tm._engine is not first                              # (the pool did grow)
    want = _expected(twin, lists, 0, 300)
    _assert_record(rec, tuple(w[1:] for w in want), what="growing pool")
    assert np.array_equal(rec.step_index, np.arange(1, 300))
    _assert_same_tm(tm, twin)


@pytest.mark.gpu
def test_graphs_are_captured_once():
    """A second call with the same arguments, and one with other reset bits, replay the graphs of the one before."""
    C, K, n = 1024, 8, 40
    lists = _lists(C, n)
    tm, = _tms(C, K, 1)
    tm.run(lists, 80)
    eng = tm._engine
    assert eng.graph_count() > 0
    tm.run(lists, 40, learning=False, record=ALL)
    g = eng.graph_count()
    tm.run(lists, 40, learning=False, record=("counters",))     # (other buffers and fields: the descriptor, not the graphs)
    assert eng.graph_count() == g
    tm.run(lists, 40, learning=False, record=ALL, resets=RESETS)
    g = eng.graph_count()
    other = np.zeros(8, bool)
    other[5] = True
    tm.run(lists, 40, learning=False, record=ALL, resets=other)
    assert eng.graph_count() == g
    tm.run(np.sort(lists, axis=1), 40, learning=False, record=ALL)           # (another bank: other graphs)
    assert eng.graph_count() > g


@pytest.mark.gpu
def test_bad_rows():
    """Python refuses a bad bank before anything is enqueued.  At the C ABI, a bank uploaded without that check, with one
    repeated id and one id equal to column_dim: the call raises, bit 128 is set, no HIP error; a fresh Temporal Memory on the
    device then runs correctly."""
    from bithtm_amd.engine import CapacityError, HtmError
    C, K, n = 1024, 8, 40
    lists = _lists(C, n)
    bad = lists.copy()
    bad[2, 5] = bad[2, 6]
    bad[4, 0] = C
    tm, = _tms(C, K, 1)
    tm.run(lists, 3)
    with pytest.raises(ValueError, match="row 4 has a column id outside"):
        tm.run(bad, 8)
    only_twice = lists.copy()
    only_twice[2, 5] = only_twice[2, 6]
    with pytest.raises(ValueError, match="row 2 lists a column twice"):
        tm.run(only_twice, 8)
    eng = tm._engine
    assert eng.steps == 3 and eng.info().step_index == 3 and eng.info().capacity_error == 0      # nothing ran
    dev = eng.upload_lists(bad, check=False)
    with pytest.raises(HtmError) as e:
        eng.tm_run(dev, 8, n, 8, record=("active_column",))
    assert isinstance(e.value, CapacityError) and "htm_tm_run met a list row" in str(e.value) and "HIP" not in str(e.value)
    info = eng.info()
    assert info.capacity_error == 128 and info.step_index == 11
    eng.sync()                                                  # (no HIP error: the stream is healthy)
    cols = eng._record_read("active_column", 8 * n, np.int32).reshape(8, n)
    assert (np.diff(cols, axis=1) > 0).all() and cols.min() >= 0 and cols.max() < C       # n distinct in-range ids all the same
    fresh, twin = _tms(C, K)
    rec = fresh.run(lists, 20, record=ALL)
    _assert_record(rec, _expected(twin, lists, 0, 20), what="after the bad bank")
    _assert_same_tm(fresh, twin)


@pytest.mark.gpu
def test_refusals():
    """A view, a fused model's Temporal Memory, cell_dim = 65, record=("predicted_input",), a resets array of the wrong length,
    n > active_columns: each raises its documented error, and the Temporal Memory still runs afterwards."""
    import bithtm_amd as B
    from bithtm_amd.engine import HtmError
    C, K, n = 1024, 8, 40
    lists = _lists(C, n)
    htm, _ = _twins(300, C, K, active_columns=n)
    htm.run(_bank(8, 300, 3), 10)
    view = htm.inference_view()
    for model in (view, htm):
        with pytest.raises(ValueError, match="fused into a HierarchicalTemporalMemory"):
            model.temporal_memory.run(lists, 4)
    dev = view.engine.upload_lists(lists)
    with pytest.raises(HtmError, match=r"\(-4\).*inference view"):
        view.engine.tm_run(dev, 8, n, 4)
    with pytest.raises(ValueError, match="cell_dim above 64"):
        B.TemporalMemory(C, 65).run(lists, 4)
    tm, twin = _tms(C, K)
    tm.run(lists, 5)
    with pytest.raises(ValueError, match="no proximal mask"):
        tm.run(lists, 4, record=("predicted_input",))
    with pytest.raises(ValueError, match="one flag per row"):
        tm.run(lists, 4, resets=np.zeros(7, bool))
    eng = tm._engine
    wide = _lists(C, n + 1)
    with pytest.raises(HtmError, match=r"\(-1\).*active_columns"):
        eng.tm_run(eng.upload_lists(wide), 8, n + 1, 4)
    eng.set_run_resets(eng.upload_resets(np.zeros(7, bool)), 7)             # (bits for a bank of 7 rows, a bank of 8)
    with pytest.raises(HtmError, match=r"\(-1\).*n_rows"):
        eng.tm_run(eng.upload_lists(lists), 8, n, 4)
    eng.set_run_resets(None, 0)
    assert eng.steps == 5 and eng.info().step_index == 5
    rec = tm.run(lists, 30, record=ALL)
    _assert_record(rec, tuple(w[5:] for w in _expected(twin, lists, 0, 35)), what="after the refusals")
    _assert_same_tm(tm, twin)
    view.run(_bank(8, 300, 3), 4)                               # (and so does the view)


@pytest.mark.gpu
def test_a_fused_model_beside_it_is_untouched():
    """A fused model's run() interleaved with tm.run on another handle: no new graph, and the state of a twin that never
    saw a Temporal Memory run."""
    I, C, K, n = 300, 1024, 8, 40
    bank, lists = _bank(8, I, 3), _lists(C, n)
    tm, = _tms(C, K, 1)
    tm.run(lists, 2)                                            # (the handle exists before the fused models' first graphs)
    htm, twin = _twins(I, C, K, active_columns=n)
    for m in (htm, twin):
        m.run(bank, 64)
        m.run(bank, 64, learning=False)
    g = htm.engine.graph_count()
    for _ in range(3):
        tm.run(lists, 30)
        htm.run(bank, 64, learning=False)
        twin.run(bank, 64, learning=False)
    assert htm.engine.graph_count() == g and twin.engine.graph_count() == g
    _assert_same_state(htm, twin)
    gc.collect()
