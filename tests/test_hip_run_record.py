"""The per-step record of a batched run (htm_run_recorded; HierarchicalTemporalMemory.run(record=...)) against the same steps
taken one by one with process() and read back from the States -- every counter, the winner lists and the packed column
predictions -- in every schedule the batched run has, across call boundaries, and at full size; plus the argument checks and
the record's derived fields (CPU)."""

import ctypes as C
import io

import numpy as np
import pytest

ALL = ("counters", "active_column", "column_prediction")


def _expected(htm, inputs, learning=True):
    """Step `htm` through `inputs` with process(): (counters int32[n, 8] in htm_step_record order, active_column, column
    prediction bool[n, C]) read from its States and engine.info()."""
    counters, cols, preds = [], [], []
    for x in inputs:
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


def _counters(rec):
    from bithtm_amd.engine import RECORD_COUNTERS
    return np.stack([getattr(rec, name) for name in RECORD_COUNTERS], axis=1) if len(rec) else np.zeros((0, 8), np.int32)


def _assert_record(rec, expected, fields=ALL, what=""):
    counters, cols, preds = expected
    assert len(rec) == len(counters), what
    if "counters" in fields:
        got = _counters(rec)
        bad = np.argwhere(got != counters)
        assert not len(bad), f"{what}: first (step, field) mismatches {bad[:5].tolist()}: got {got[bad[0][0]]}, want {counters[bad[0][0]]}"
    if "active_column" in fields:
        assert np.array_equal(rec.active_column, cols), what
    if "column_prediction" in fields:
        assert rec.column_prediction.dtype == bool and np.array_equal(rec.column_prediction, preds), what


def _bank(rows, I, seed, density=0.06):
    return np.random.RandomState(seed).rand(rows, I) < density


def _twins(I, C, K, seed=5, **kw):
    """Two identical models (a larger winner list than the default 2 % where `active_columns` is given: predictions within a
    few passes over a small bank)."""
    import bithtm_amd as B
    out = []
    for _ in range(2):
        np.random.seed(seed)                     # (the SP's permanences are drawn from NumPy's global stream)
        out.append(B.HierarchicalTemporalMemory(I, C, K, seed=seed, **kw))
    return out


def _rows(bank, start, n):
    return [bank[(start + t) % len(bank)] for t in range(n)]


SIZES = [(300, 1024, 8, 64), (400, 2048, 32, 64), (300, 512, 48, 48)]
SCHEDULES = [{}, {"BITHTM_LEAN": "1"}, {"BITHTM_LEAN": "0"}, {"BITHTM_SCAN_LARGE": "1"}, {"BITHTM_SCAN_LARGE": "1", "BITHTM_LEAN": "0"},
             {"BITHTM_EAGER_BELOW": "100000"}]
SCHEDULE_IDS = ["two-launch", "three-launch", "four-launch", "scan-large", "scan-large-four-launch", "eager"]


@pytest.mark.gpu
@pytest.mark.parametrize("pipeline", [True, False], ids=["pipelined", "unpipelined"])
@pytest.mark.parametrize("env", SCHEDULES, ids=SCHEDULE_IDS)
@pytest.mark.parametrize("size", SIZES, ids=["1024x8", "2048x32", "512x48"])
def test_record_equals_the_stepwise_states(size, env, pipeline, monkeypatch):
    """Every record field of a learning stretch and a stretch with learning off == the twin's States, step by step; graph
    replay (the suite's default) or eager launches, each schedule, pipelined or not; the state left behind is the twin's."""
    for k, v in env.items():
        monkeypatch.setenv(k, v)
    I, Cn, K, k = size
    bank = _bank(8, I, 3)
    htm, twin = _twins(I, Cn, K, active_columns=k)
    plan = htm.engine.run_plan(80, pipeline=pipeline)
    if "BITHTM_SCAN_LARGE" in env:
        assert plan["scan_large"]
    rec = htm.run(bank, 80, record=ALL, pipeline=pipeline)
    _assert_record(rec, _expected(twin, _rows(bank, 0, 80)), what="learning")
    assert rec.predicted_columns.max() > 0 and rec.new_segments.sum() > 0     # (the stretch learned something)
    rec = htm.run(bank, 20, learning=False, record=ALL, pipeline=pipeline)
    _assert_record(rec, _expected(twin, _rows(bank, 80, 20), learning=False), what="learning off")
    assert np.array_equal(rec.step_index, np.arange(80, 100))
    a, b = htm.state_dict(), twin.state_dict()
    for key in a:
        assert np.array_equal(a[key], b[key]), key


@pytest.mark.gpu
def test_record_equals_the_oracle():
    """At one size, every counter against the oracle's own States (not through the twin): new_segments from the oracle's
    own rule -- the step's winner cells without a matching segment in the state before (projections.py:271)."""
    from hip_impl import make_htm
    from oracle import HTMOracle
    I, Cn, K, k, steps = 300, 2048, 16, 64, 100
    np.random.seed(9)
    ora = HTMOracle(I, Cn, K, active_columns=k, seed=9, permanence=np.random.randn(Cn, I) * 0.1)
    htm = make_htm(I, Cn, K, k, 9, ora.spatial_pooler.permanence.copy())
    bank = _bank(8, I, 10)
    rec = htm.run(bank, steps, record=ALL)
    prev = np.zeros(Cn, bool)
    tmo = ora.temporal_memory
    for t in range(steps):
        before = tmo.prev_distal
        o_sp, o_tm = ora.step(bank[t % 8])
        pred = o_tm.cell_prediction.any(axis=1)
        winners = o_tm.winner_cell[0].astype(np.int64) * K + o_tm.winner_cell[1]
        new = 0 if before is None else int((before.max_jittered_potential[winners] < tmo.eps).sum())
        want = [len(o_sp.active_column), int(o_tm.active_column_bursting.sum()), int(prev.sum()), int(pred.sum()),
                len(o_tm.active_cell[0]), len(o_tm.winner_cell[0]), tmo.S, new]
        got = _counters(rec)[t].tolist()
        assert got == want, (t, got, want)
        assert np.array_equal(rec.active_column[t], o_sp.active_column), t
        assert np.array_equal(rec.column_prediction[t], pred), t
        prev = pred
    assert rec.predicted_columns.max() > 0 and rec.new_segments.sum() > 0


@pytest.mark.gpu
def test_a_second_recorded_call_replays_the_same_graphs():
    """Recorded calls with other buffers and other fields replay the graphs htm_prepare_recorded built: none is captured again
    (learning off after a learned stretch, so that nothing else a graph is keyed on -- the pool's size -- changes)."""
    I, Cn, K = 300, 1024, 32
    bank = _bank(8, I, 9)
    htm, twin = _twins(I, Cn, K, active_columns=64)
    htm.run(bank, 60)
    htm.run(bank, 40, learning=False)
    eng = htm.engine
    eng.info()
    eng.prepare(htm._bank[1], len(bank), 40, learning=False, record=True)
    n_graphs = eng.graph_count()
    assert n_graphs > 0
    r1 = htm.run(bank, 40, learning=False, record=("counters",))
    assert eng.graph_count() == n_graphs
    r2 = htm.run(bank, 40, learning=False, record=ALL)
    assert eng.graph_count() == n_graphs
    _expected(twin, _rows(bank, 0, 60))
    _expected(twin, _rows(bank, 60, 40), learning=False)
    _assert_record(r1, _expected(twin, _rows(bank, 100, 40), learning=False), fields=("counters",))
    _assert_record(r2, _expected(twin, _rows(bank, 140, 40), learning=False))


@pytest.mark.gpu
def test_recording_changes_nothing():
    """The same calls with and without a record leave bit-identical states."""
    I, Cn, K = 300, 1024, 32
    bank = _bank(8, I, 4)
    a, b = _twins(I, Cn, K, active_columns=64)
    for n, learning in ((30, True), (1, True), (17, False), (40, True)):
        assert a.run(bank, n, learning=learning) is None
        assert len(b.run(bank, n, learning=learning, record=("counters", "column_prediction"))) == n
    sa, sb = a.state_dict(), b.state_dict()
    for key in sa:
        assert np.array_equal(sa[key], sb[key]), key


@pytest.mark.gpu
@pytest.mark.parametrize("before", ["fresh", "process", "load_state_dict", "unrecorded_run", "continuing_run"])
def test_first_step_of_a_call_after(before):
    """predicted_columns_before of a call's first step, whatever closed the step before it; runs of 1 and 0 steps."""
    I, Cn, K, k = 300, 1024, 16, 64
    bank = _bank(8, I, 6)
    htm, twin = _twins(I, Cn, K, active_columns=k)
    done = 0
    if before != "fresh":                         # (a step count after which the last state predicts something)
        _, probe = _twins(I, Cn, K, active_columns=k)
        probe.run(bank, 50)
        done = 50
        while done < 120 and not probe.temporal_memory.last_state.cell_prediction.any():
            probe.process(bank[done % len(bank)])
            done += 1
    if before == "process":
        for x in _rows(bank, 0, done):
            htm.process(x)
    elif before == "unrecorded_run":
        htm.run(bank, done)
    elif before == "continuing_run":
        htm.run(bank, done, continuing=True)      # (the Spatial Pooler stays ahead into the recorded call)
    elif before == "load_state_dict":
        src, _ = _twins(I, Cn, K, active_columns=k)
        src.run(bank, done)
        htm.load_state_dict(src.state_dict())
    _expected(twin, _rows(bank, 0, done))
    empty = htm.run(bank, 0, record=ALL)
    assert len(empty) == 0 and empty.column_prediction.shape == (0, Cn) and empty.active_column.shape == (0, htm.active_columns)
    rec = htm.run(bank, 1, record=ALL)
    want = _expected(twin, _rows(bank, done, 1))
    _assert_record(rec, want, what="one step")
    if before != "fresh":
        assert rec.predicted_columns_before[0] > 0
    else:
        assert rec.predicted_columns_before[0] == 0
    rec = htm.run(bank, 25, record=ALL)
    _assert_record(rec, _expected(twin, _rows(bank, done + 1, 25)), what="after one")


@pytest.mark.gpu
@pytest.mark.parametrize("use_graph", [True, False], ids=["graph", "eager"])
def test_continuing_chunks_concatenate_to_one_run(use_graph):
    """run(continuing=True) in chunks: the records put end to end are the record of one long run (and the twin's)."""
    I, Cn, K = 300, 2048, 8
    bank = _bank(8, I, 7)
    htm, long_run = _twins(I, Cn, K, active_columns=64)
    parts = [htm.run(bank, n, use_graph=use_graph, continuing=i < 5, record=ALL) for i, n in enumerate((1, 2, 17, 20, 3, 33))]
    whole = long_run.run(bank, 76, use_graph=use_graph, record=ALL)
    for f in ("active_column", "column_prediction", "step_index"):
        assert np.array_equal(np.concatenate([getattr(p, f) for p in parts]), getattr(whole, f)), f
    assert np.array_equal(np.concatenate([_counters(p) for p in parts]), _counters(whole))
    _, twin = _twins(I, Cn, K, active_columns=64)
    _assert_record(whole, _expected(twin, _rows(bank, 0, 76)))
    assert whole.predicted_columns.max() > 0


@pytest.mark.gpu
def test_pool_growth_inside_a_recorded_run():
    """A default-sized pool that has to grow in the middle of run() (the engine is re-created between batches): one
    contiguous record, equal to the twin's."""
    I, Cn, K = 400, 1024, 8
    bank = _bank(500, I, 8, density=0.1)           # (no repeats: nearly every column bursts and asks for a new segment)
    htm, twin = _twins(I, Cn, K)
    first = htm.engine
    rec = htm.run(bank, 500, record=ALL)
    assert htm.engine is not first                  # (the pool did grow)
    assert np.array_equal(rec.step_index, np.arange(500))
    _assert_record(rec, _expected(twin, _rows(bank, 0, 500)))


@pytest.mark.gpu
def test_prepared_recorded_graphs_and_other_buffers():
    """htm_prepare_recorded builds the graphs a recorded call replays; calls with other buffers (other fields, other sizes)
    replay them and write where they are told -- an unrecorded call in between writes nothing into the old buffers."""
    I, Cn, K = 300, 1024, 32
    bank = _bank(8, I, 9)
    htm, twin = _twins(I, Cn, K, active_columns=64)
    htm.run(bank, 5)
    eng = htm.engine
    eng.prepare(htm._bank[1], len(bank), 40, record=True)
    r1 = htm.run(bank, 40, record=("counters",))
    kept = eng._record_read("counters", 40 * 8, np.int32)
    htm.run(bank, 20)
    assert np.array_equal(eng._record_read("counters", 40 * 8, np.int32), kept)
    r2 = htm.run(bank, 40, record=("active_column", "column_prediction"))
    assert r2.active_columns is None and r1.active_column is None
    _expected(twin, _rows(bank, 0, 5))
    want = _expected(twin, _rows(bank, 5, 40))
    _assert_record(r1, want, fields=("counters",))
    _expected(twin, _rows(bank, 45, 20))
    _assert_record(r2, _expected(twin, _rows(bank, 65, 40)), fields=("active_column", "column_prediction"))


@pytest.mark.gpu
def test_full_size_graph_replay():
    """65 536 columns x 32 cells, 300 steps of graph replay over a cycle of 25 patterns (learned after the first cycles):
    every field equals the twin's."""
    I, Cn, K = 1000, 65536, 32
    bank = _bank(25, I, 12, density=0.2)
    htm, twin = _twins(I, Cn, K)
    assert htm.engine.run_plan(300)["hip_graph"]
    rec = htm.run(bank, 300, record=ALL)
    _assert_record(rec, _expected(twin, _rows(bank, 0, 300)))
    assert rec.correct_columns.max() > 0           # (a learned stretch)


@pytest.mark.gpu
def test_example_batched_report_prints_the_stepwise_lines():
    from bithtm_amd import example
    outs = []
    for extra in ([], ["--batched_report"]):
        np.random.seed(1)
        buf = io.StringIO()
        example.main(["--epochs", "12", "--input_patterns", "10", "--column_dim", "2048"] + extra, out=buf)
        outs.append(buf.getvalue().splitlines())
    assert len(outs[0]) == 12 * 10 + 1 and outs[0][-1].endswith("seconds.")
    assert outs[0][:-1] == outs[1][:-1]
    assert outs[1][-1].endswith("seconds.")


@pytest.mark.gpu
def test_record_errors():
    import bithtm_amd as B
    from bithtm_amd import _lib as L
    from bithtm_amd.distributed import LocalGroup
    I, Cn, K = 200, 1024, 8
    htm, _ = _twins(I, Cn, K)
    bank = _bank(4, I, 2)
    htm.run(bank, 2)
    eng, dev_bank = htm.engine, htm._bank[1]
    words = eng._record_buffer("counters", 64)
    rec = L.HtmRunRecord()
    rec.struct_bytes = C.sizeof(L.HtmRunRecord) + 4
    rec.records = words
    assert eng.lib.htm_run_recorded(eng.h, C.c_void_p(dev_bank), 4, 2, 1, 1, C.byref(rec)) == -1       # HTM_ERR_ARGUMENT
    rec.struct_bytes, rec.records = C.sizeof(L.HtmRunRecord), None
    assert eng.lib.htm_run_recorded(eng.h, C.c_void_p(dev_bank), 4, 2, 1, 1, C.byref(rec)) == -1       # no buffer
    assert eng.lib.htm_run_recorded(eng.h, C.c_void_p(dev_bank), 4, 2, 1, 1, None) == 0               # NULL: htm_run
    with pytest.raises(ValueError):
        htm.run(bank, 2, record=("counters", "overlaps"))
    group = LocalGroup(2, I, Cn, K, permanence=np.random.RandomState(0).rand(Cn, I) * 0.1)
    g = group.engines[0]
    rec.records = words
    assert g.lib.htm_run_recorded(g.h, C.c_void_p(dev_bank), 4, 2, 1, 1, C.byref(rec)) == -4           # HTM_ERR_STATE

    class UserTM:                                   # a Temporal Memory of the user's own, on the host
        def process(self, sp_state, learning=True):
            return sp_state
    plug = B.HierarchicalTemporalMemory(I, Cn, K, temporal_memory=UserTM())
    with pytest.raises(RuntimeError):
        plug.run(bank, 2, record=True)


def test_run_record_derived_fields_on_synthetic_arrays():
    """CPU: RunRecord's per-field arrays and the derived report of example.py:55-57 and the anomaly score."""
    from bithtm_amd import RunRecord
    from bithtm_amd.engine import RECORD_COUNTERS
    from bithtm_amd.networks import _record_fields
    assert RECORD_COUNTERS == ("active_columns", "bursting_columns", "predicted_columns_before", "predicted_columns", "active_cells",
                               "winner_cells", "segments", "new_segments")
    counters = np.array([[40, 40, 0, 3, 1280, 40, 40, 40],
                         [40, 10, 35, 38, 400, 40, 50, 10],
                         [40, 0, 44, 40, 40, 40, 50, 0],
                         [0, 0, 5, 0, 0, 0, 50, 0]], np.int32)
    rec = RunRecord(np.arange(7, 11), counters=counters)
    assert len(rec) == 4 and rec.fields == ("counters",)
    assert rec.active_column is None and rec.column_prediction is None
    assert rec.bursting_columns.tolist() == [40, 10, 0, 0] and rec.segments.dtype == np.int32
    assert rec.correct_columns.tolist() == [0, 30, 40, 0]
    assert rec.incorrect_columns.tolist() == [0, 5, 4, 5]
    assert np.allclose(rec.anomaly_score, [1.0, 0.25, 0.0, 0.0])
    assert rec.step_index.tolist() == [7, 8, 9, 10]
    only = RunRecord(np.arange(2), active_column=np.zeros((2, 3), np.int32))
    assert only.fields == ("active_column",) and only.correct_columns is None and only.anomaly_score is None
    assert _record_fields(True) == ("counters",)
    assert _record_fields(("column_prediction", "counters")) == ("counters", "column_prediction")
    for bad in ((), ("counters", "overlaps"), "segments"):
        with pytest.raises(ValueError):
            _record_fields(bad)


def test_header_declares_the_record_abi():
    """CPU: the C layout the binding assumes is the header's (eight int32 counts; a size word and three device pointers)."""
    import os
    import re
    from bithtm_amd import _lib as L
    header = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "bithtm_hip.h")).read()
    body = re.search(r"typedef struct htm_step_record \{(.*?)\} htm_step_record;", header, re.S).group(1)
    assert re.findall(r"int32_t (\w+);", body) == [name for name, _ in L.HtmStepRecord._fields_]
    assert C.sizeof(L.HtmStepRecord) == 32 and C.sizeof(L.HtmRunRecord) == 32
    body = re.search(r"typedef struct htm_run_record \{(.*?)\} htm_run_record;", header, re.S).group(1)
    assert re.findall(r"(\w+);", body) == [name for name, _ in L.HtmRunRecord._fields_]
