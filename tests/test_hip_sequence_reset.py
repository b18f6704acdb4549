"""Sequence resets (include/bithtm_hip.h: htm_reset, htm_set_run_resets).  A batched run with reset bits
against the same steps taken one by one with process() and reset() -- records, winner lists, column predictions and the state
left behind -- in every schedule of the batched run; the stand-alone Temporal Memory's three ways to reset against the oracle;
the reference's `last_state = get_empty_state()` idiom on a fused model; resets across call boundaries and pool growth; the
argument checks."""

import ctypes as C
import io
from types import SimpleNamespace

import numpy as np
import pytest

from test_hip_run_record import ALL, SCHEDULES, SCHEDULE_IDS, SIZES, _assert_record, _bank, _rows, _twins


def _expected(htm, inputs, resets, start, learning=True):
    """Step `htm` through `inputs` (steps start, start + 1, ...) with process(), reset() before every step whose bank row has
    its flag: (counters, active columns, column predictions) as test_hip_run_record._expected reads them."""
    counters, cols, preds = [], [], []
    for i, x in enumerate(inputs):
        if resets[(start + i) % len(resets)]:
            htm.reset()
        before = int(htm.temporal_memory.last_state.cell_prediction.any(axis=1).sum())
        sp, tm = htm.process(x, learning=learning)
        info = htm.engine.info()
        pred = tm.cell_prediction.any(axis=1)
        winners = 0 if tm.winner_cell is None else len(tm.winner_cell[0])
        counters.append([len(sp.active_column), int(tm.active_column_bursting.sum()), before, int(pred.sum()),
                         len(tm.active_cell[0]), winners, info.segments, info.recycled_segments + info.appended_segments])
        cols.append(np.sort(sp.active_column))
        preds.append(pred)
    n = len(counters)
    return (np.asarray(counters, np.int32).reshape(n, 8), np.asarray(cols, np.int32).reshape(n, htm.active_columns),
            np.asarray(preds, bool).reshape(n, htm.column_dim))


def _assert_same_state(a, b):
    sa, sb = a.state_dict(), b.state_dict()
    for key in sa:
        assert np.array_equal(sa[key], sb[key]), key


def _assert_reset_steps(rec, resets, start):
    hit = np.array([resets[(start + i) % len(resets)] for i in range(len(rec))])
    assert hit.any()
    assert (rec.predicted_columns_before[hit] == 0).all()
    assert np.array_equal(rec.bursting_columns[hit], rec.active_columns[hit])
    assert (rec.anomaly_score[hit] == 1).all()
    assert (rec.correct_columns[hit] == 0).all() and (rec.incorrect_columns[hit] == 0).all()


# rows 0, 3 and 4: a reset at a call's first step, two consecutive resets
RESETS = np.array([1, 0, 0, 1, 1, 0, 0, 0], bool)


@pytest.mark.gpu
@pytest.mark.parametrize("pipeline", [True, False], ids=["pipelined", "unpipelined"])
@pytest.mark.parametrize("env", SCHEDULES, ids=SCHEDULE_IDS)
@pytest.mark.parametrize("size", SIZES, ids=["1024x8", "2048x32", "512x48"])
def test_run_with_resets_equals_stepwise_resets(size, env, pipeline, monkeypatch):
    """run(resets=) == process() with reset() at the same rows: every record field, a learning stretch and one with learning
    off, and the state left behind (store included); graph replay or eager launches, each schedule, pipelined or not."""
    for k, v in env.items():
        monkeypatch.setenv(k, v)
    I, Cn, K, k = size
    bank = _bank(8, I, 3)
    htm, twin = _twins(I, Cn, K, active_columns=k)
    rec = htm.run(bank, 80, record=ALL, pipeline=pipeline, resets=RESETS)
    _assert_record(rec, _expected(twin, _rows(bank, 0, 80), RESETS, 0), what="learning")
    assert rec.predicted_columns.max() > 0 and rec.new_segments.sum() > 0
    _assert_reset_steps(rec, RESETS, 0)
    rec = htm.run(bank, 20, learning=False, record=ALL, pipeline=pipeline, resets=RESETS)
    _assert_record(rec, _expected(twin, _rows(bank, 80, 20), RESETS, 80, learning=False), what="learning off")
    _assert_reset_steps(rec, RESETS, 80)
    _assert_same_state(htm, twin)
    # and an unrecorded run with resets leaves the twin's state too
    htm.run(bank, 37, pipeline=pipeline, resets=RESETS)
    _expected(twin, _rows(bank, 100, 37), RESETS, 100)
    _assert_same_state(htm, twin)


@pytest.mark.gpu
def test_resets_change_what_is_learned():
    """(that the bits do something) the same run without resets predicts the reset rows' columns and scores them lower"""
    I, Cn, K, k = 300, 1024, 16, 64
    bank = _bank(8, I, 3)
    a, b = _twins(I, Cn, K, active_columns=k)
    ra = a.run(bank, 120, record=ALL, resets=RESETS)
    rb = b.run(bank, 120, record=ALL)
    assert not np.array_equal(ra.predicted_columns_before, rb.predicted_columns_before)
    assert rb.predicted_columns_before[80:][RESETS[np.arange(80, 120) % 8]].max() > 0


@pytest.mark.gpu
@pytest.mark.parametrize("K", [8, 48])
def test_three_ways_to_reset_and_the_oracle(K):
    """run(resets=) == reset() + process() == process(prev_state=get_empty_state()) == the oracle stepped with the empty
    prev_state, on the winner lists the batched run's Spatial Pooler chose."""
    import bithtm_amd as B
    from oracle import TemporalMemoryOracle, canonical_synapses
    I, Cn, k, steps = 300, 1024, 40, 90
    bank = _bank(10, I, 21)
    resets = np.zeros(10, bool)
    resets[[0, 4, 5]] = True
    htm, _ = _twins(I, Cn, K, active_columns=k)
    rec = htm.run(bank, steps, record=ALL, resets=resets)
    tm_a, tm_b = B.TemporalMemory(Cn, K, seed=5), B.TemporalMemory(Cn, K, seed=5)
    ora = TemporalMemoryOracle(Cn, K, seed=5)
    empty = SimpleNamespace(cell_prediction=np.zeros((Cn, K), bool), cell_activation=np.zeros((Cn, K), bool), winner_cell=None,
                            distal_state=None)
    for t in range(steps):
        cols = rec.active_column[t].astype(np.int64)
        sp = SimpleNamespace(active_column=cols)
        if resets[t % 10]:
            tm_a.reset()
            assert not tm_a.last_state.cell_prediction.any() and tm_a.last_state.distal_state is None
            a = tm_a.process(sp)
            b = tm_b.process(sp, prev_state=tm_b.get_empty_state())
            o = ora.step(cols, prev_state=empty)
        else:
            a, b, o = tm_a.process(sp), tm_b.process(sp), ora.step(cols)
        pred = a.cell_prediction.any(axis=1)
        assert np.array_equal(pred, rec.column_prediction[t]), t
        assert int(a.active_column_bursting.sum()) == rec.bursting_columns[t], t
        for x in (b, o):
            assert np.array_equal(a.cell_activation, x.cell_activation), t
            assert np.array_equal(a.cell_prediction, x.cell_prediction), t
            assert np.array_equal(a.active_column_bursting, x.active_column_bursting), t
            assert np.array_equal(a.distal_state.matching_segment, x.distal_state.matching_segment), t
        assert np.array_equal(a.winner_cell[0], b.winner_cell[0]) and np.array_equal(a.winner_cell[1], b.winner_cell[1]), t
    sa, sb = tm_a._engine.read_store(), tm_b._engine.read_store()
    ca, cb = (canonical_synapses(s["seg_cell"], s["presyn"], s["perm"]) for s in (sa, sb))
    co = canonical_synapses(ora.seg_cell[:ora.S], ora.presyn[:ora.S], ora.perm[:ora.S])
    for x in (cb, co):
        assert len(ca) == len(x) and all(p[0] == q[0] and np.array_equal(p[1], q[1]) and np.array_equal(p[2].view(np.int32), q[2].view(np.int32))
                                         for p, q in zip(ca, x))


@pytest.mark.gpu
def test_fused_model_takes_the_reference_idiom_and_checkpoints_a_reset():
    """`htm.temporal_memory.last_state = get_empty_state()` on a fused model, then process(): the twin stepped with reset();
    a state_dict() taken right after reset() loads into a model that behaves as reset; other assignments are refused."""
    I, Cn, K, k = 300, 1024, 16, 64
    bank = _bank(8, I, 4)
    a, b = _twins(I, Cn, K, active_columns=k)
    c, _ = _twins(I, Cn, K, active_columns=k)
    for x in _rows(bank, 0, 60):
        a.process(x)
        b.process(x)
    assert a.temporal_memory.last_state.cell_prediction.any()
    old = a.temporal_memory.last_state
    a.temporal_memory.last_state = old                       # (assigning the current state: nothing)
    a.temporal_memory.last_state = a.temporal_memory.get_empty_state()
    assert not a.temporal_memory.last_state.cell_prediction.any() and a.temporal_memory.last_state.distal_state is None
    b.reset()
    c.load_state_dict(b.state_dict())                        # (a checkpoint of the reset model)
    assert c.engine.info().has_distal_state == 0 and c.engine.info().has_winner_cells == 0
    for x in _rows(bank, 60, 30):
        sa, ta = a.process(x)
        sb, tb = b.process(x)
        sc, tc = c.process(x)
        for t in (tb, tc):
            assert np.array_equal(ta.cell_activation, t.cell_activation)
            assert np.array_equal(ta.cell_prediction, t.cell_prediction)
    _assert_same_state(a, b)
    _assert_same_state(a, c)
    with pytest.raises(ValueError, match="prev_state"):
        a.temporal_memory.last_state = old


@pytest.mark.gpu
@pytest.mark.parametrize("before", ["fresh", "process", "load_state_dict", "unrecorded_run", "continuing_run"])
def test_reset_at_the_first_step_of_a_call_after(before):
    """The bank row of a call's first step has its bit set, whatever closed the step before it."""
    I, Cn, K, k = 300, 1024, 16, 64
    bank = _bank(8, I, 6)
    htm, twin = _twins(I, Cn, K, active_columns=k)
    done = 56                                                # (a multiple of 8: the call starts at row 0, which resets)
    if before == "process":
        for x in _rows(bank, 0, done):
            htm.process(x)
    elif before == "unrecorded_run":
        htm.run(bank, done)
    elif before == "continuing_run":
        htm.run(bank, done, continuing=True)
    elif before == "load_state_dict":
        src, _ = _twins(I, Cn, K, active_columns=k)
        src.run(bank, done)
        htm.load_state_dict(src.state_dict())
    else:
        done = 0
    for x in _rows(bank, 0, done):
        twin.process(x)
    rec = htm.run(bank, 1, record=ALL, resets=RESETS)
    _assert_record(rec, _expected(twin, _rows(bank, done, 1), RESETS, done), what="one step")
    assert rec.predicted_columns_before[0] == 0 and rec.anomaly_score[0] == 1
    rec = htm.run(bank, 25, record=ALL, resets=RESETS)
    _assert_record(rec, _expected(twin, _rows(bank, done + 1, 25), RESETS, done + 1), what="after one")


@pytest.mark.gpu
@pytest.mark.parametrize("use_graph", [True, False], ids=["graph", "eager"])
def test_resets_across_continuing_chunks(use_graph):
    """run(continuing=True, resets=) in chunks: the bits follow the bank rows across the call boundaries."""
    I, Cn, K, k = 300, 1024, 16, 64
    bank = _bank(8, I, 7)
    htm, twin = _twins(I, Cn, K, active_columns=k)
    parts, start = [], 0
    for i, n in enumerate((1, 2, 17, 20, 3, 33)):
        parts.append(htm.run(bank, n, use_graph=use_graph, continuing=i < 5, record=ALL, resets=RESETS))
        start += n
    counters = np.concatenate([np.stack([p.predicted_columns_before, p.bursting_columns, p.predicted_columns], 1) for p in parts])
    want = _expected(twin, _rows(bank, 0, start), RESETS, 0)[0]
    assert np.array_equal(counters, want[:, [2, 1, 3]])
    _assert_same_state(htm, twin)


@pytest.mark.gpu
def test_pool_growth_inside_a_run_with_resets():
    """A default-sized pool that grows in the middle of run(resets=): the bits are uploaded to the new engine too."""
    I, Cn, K = 400, 1024, 8
    bank = _bank(500, I, 8, density=0.1)           # (no repeats: nearly every column bursts and asks for a new segment)
    resets = np.zeros(500, bool)
    resets[::7] = True
    htm, twin = _twins(I, Cn, K)
    first = htm.engine
    rec = htm.run(bank, 500, record=ALL, resets=resets)
    assert htm.engine is not first                  # (the pool did grow)
    assert np.array_equal(rec.step_index, np.arange(500))
    _assert_record(rec, _expected(twin, _rows(bank, 0, 500), resets, 0))
    _assert_reset_steps(rec, resets, 0)


@pytest.mark.gpu
def test_clear_bits_equal_no_bits_and_the_same_graphs():
    """All bits clear == no bits, bit for bit; a call with other bits replays the graphs of the one before."""
    I, Cn, K, k = 300, 1024, 16, 64
    bank = _bank(8, I, 9)
    a, b = _twins(I, Cn, K, active_columns=k)
    ra = a.run(bank, 100, record=ALL, resets=np.zeros(8, bool))
    rb = b.run(bank, 100, record=ALL)
    assert np.array_equal(ra.column_prediction, rb.column_prediction) and np.array_equal(ra.active_column, rb.active_column)
    assert np.array_equal(ra.predicted_columns_before, rb.predicted_columns_before)
    _assert_same_state(a, b)
    n = a.engine.graph_count()
    other = np.zeros(8, bool)
    other[5] = True
    a.run(bank, 100, record=ALL, resets=other)
    assert a.engine.graph_count() == n


@pytest.mark.gpu
def test_full_size_graph_replay_with_resets():
    """65 536 x 32, graph replay, resets every 50 rows: the recorded run == its stepwise twin."""
    I, Cn, K = 1024, 65536, 32
    bank = _bank(100, I, 11, density=0.05)
    resets = np.zeros(100, bool)
    resets[::50] = True
    htm, twin = _twins(I, Cn, K)
    rec = htm.run(bank, 150, record=("counters",), resets=resets)
    want = _expected(twin, _rows(bank, 0, 150), resets, 0)
    _assert_record(rec, want, fields=("counters",), what="full size")
    _assert_reset_steps(rec, resets, 0)


@pytest.mark.gpu
def test_example_sequence_length_batched_report_prints_the_stepwise_lines():
    """example.py --sequence_length 10: --batched_report prints what the stepwise mode prints."""
    from bithtm_amd import example
    outs = []
    for extra in ([], ["--batched_report"]):
        np.random.seed(1)
        buf = io.StringIO()
        example.main(["--epochs", "12", "--input_patterns", "30", "--column_dim", "2048", "--sequence_length", "10"] + extra, out=buf)
        outs.append(buf.getvalue().splitlines())
    assert len(outs[0]) == 12 * 30 + 1
    assert outs[0][:-1] == outs[1][:-1]
    assert any(" correct columns:  0," not in line for line in outs[0][:-1])


@pytest.mark.gpu
def test_errors():
    """A bank of another size than the bits': HTM_ERR_ARGUMENT; reset while the Spatial Pooler is ahead: HTM_ERR_STATE;
    a wrong number of flags: ValueError."""
    from bithtm_amd.engine import HtmError
    import gc
    I, Cn, K, k = 300, 1024, 16, 64
    bank = _bank(8, I, 9)
    htm = _twins(I, Cn, K, active_columns=k)[0]
    gc.collect()                                             # (the twin's handle gone: the schedule can pipeline again)
    eng = htm.engine
    ptr = eng.upload_resets(RESETS)
    dev = eng.upload_bank(bank)
    eng.set_run_resets(ptr, 9)
    with pytest.raises(HtmError, match=r"\(-1\)"):
        eng.run(dev, 8, 4)
    eng.set_run_resets(None, 0)
    eng.run(dev, 8, 4)
    with pytest.raises(ValueError, match="one flag per row"):
        htm.run(bank, 4, resets=np.zeros(7, bool))
    htm.run(bank, 70, continuing=True)
    if htm.engine.run_plan(3)["pipelined"]:                  # (the Spatial Pooler is ahead only where the schedule pipelines)
        with pytest.raises(HtmError, match=r"\(-4\)"):
            htm.reset()
    htm.run(bank, 3)
    htm.reset()
    assert not htm.temporal_memory.last_state.cell_prediction.any()


@pytest.mark.gpu
def test_sharded_handles_reject_resets():
    """Column-sharded handles: htm_reset and htm_set_run_resets give HTM_ERR_STATE, the models NotImplementedError."""
    from bithtm_amd.distributed import LocalGroup
    I, Cn, K = 300, 1024, 16
    group = LocalGroup(2, I, Cn, K, permanence=np.random.RandomState(0).rand(Cn, I) * 0.1)
    g = group.engines[0]
    assert g.lib.htm_reset(g.h) == -4
    assert g.lib.htm_set_run_resets(g.h, None, 0) == -4
    with pytest.raises(NotImplementedError):
        group.reset()
