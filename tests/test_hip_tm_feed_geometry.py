"""The feed launch of batched stand-alone Temporal Memory runs (k_tm_feed, bithtm_amd/csrc/htm_tm_feed.h) at
the shapes of tests/tm_feed_cases.py: bits owned by threads of several waves, a wave without bits between two with some, 4, 8 and
64 bitmap words a thread, a last run cut by the bitmap's end, one to three passes over the row, a full bitmap word, the clearing
loop's second iteration, the 64 KiB launch and the refusal one column behind it.  Every step's recorded list against the NumPy
contract (feed_contract), every record field and the whole state against a twin stepped with process(), one case against the
oracle; bad rows (through the C ABI, unchecked) against the exact repair the header documents.  All comparisons are exact."""

import numpy as np
import pytest

import tm_feed_cases as F
from test_hip_run_record import ALL
from test_hip_tm_run import _assert_record, _assert_same_tm, _expected


def _pair(case, count=2, seed=5):
    """Identical Temporal Memories of the case's shape, each with a pool of its own (explicit where the case names one)."""
    import bithtm_amd as B
    out = []
    for _ in range(count):
        distal = None
        if case.segment_capacity is not None:
            distal = B.PredictiveProjection(case.C * case.K, segment_capacity=case.segment_capacity, segment_slots=case.segment_slots)
        out.append(B.TemporalMemory(case.C, case.K, distal_projection=distal, seed=seed))
    return out


def _contract_rows(rows, C, start, steps):
    fixed = F.repaired(rows, C)
    return fixed[(start + np.arange(steps)) % len(rows)]


def _run_case(case, tm, twin, start=0):
    """The case's calls on `tm` against process() on `twin` and against the contract; the step index afterwards."""
    done, grown = start, 0
    for m in case.calls:
        rec = tm.run(case.rows, m, record=ALL)
        assert np.array_equal(rec.active_column, _contract_rows(case.rows, case.C, done, m)), (case.name, done)
        _assert_record(rec, _expected(twin, case.rows, done, m), what=f"{case.name}: {m} steps from {done}")
        assert np.array_equal(rec.step_index, np.arange(done, done + m)) and (rec.active_columns == case.n).all()
        done, grown = done + m, grown + int(rec.new_segments.sum())
    assert grown > 0                                            # (learning is on, and it learns)
    _assert_same_tm(tm, twin)
    return done


@pytest.mark.gpu
@pytest.mark.parametrize("name", [n for n in F.CASE_IDS if n not in ("all-four-waves", "lds-cap")])
def test_case_equals_the_contract_and_stepwise(name):
    case = F.BY_NAME[name]
    tm, twin = _pair(case)
    _run_case(case, tm, twin)
    assert tm._engine.graph_count() > 0
    tm._engine.sync()


@pytest.mark.gpu
@pytest.mark.parametrize("eager", [False, True], ids=["graph", "eager"])
def test_all_four_waves_and_then_a_shorter_list(eager, monkeypatch):
    """all-four-waves, by graph replay and launched eagerly; then, on the same handle (active_columns = 300), lists of 260: two
    passes and two record blocks still, the record says 260, and the pad slots of the C ABI's rows hold -1."""
    if eager:
        monkeypatch.setenv("BITHTM_EAGER_BELOW", "64")
    case, short = F.BY_NAME["all-four-waves"], F.n_below_active()
    tm, twin = _pair(case)
    done = _run_case(case, tm, twin)
    assert (tm._engine.graph_count() == 0) == eager
    done = _run_case(short, tm, twin, start=done)
    eng = tm._engine
    assert eng.active_columns == case.n
    raw = eng.tm_run(eng.upload_lists(short.rows), len(short.rows), short.n, 6, record=("active_column", "counters"))
    _expected(twin, short.rows, done, 6)
    assert raw["active_column"].shape == (6, case.n) and (raw["active_column"][:, short.n:] == -1).all() and (raw["counters"][:, 0] == short.n).all()
    assert np.array_equal(raw["active_column"][:, :short.n], _contract_rows(short.rows, short.C, done, 6))
    _assert_same_tm(tm, twin)


@pytest.mark.gpu
def test_wave1_one_thread_equals_the_oracle():
    """wave1-one-thread for 60 steps against TemporalMemoryOracle, as test_hip_tm_run.test_run_equals_the_oracle: a geometry case
    pinned to the independent reference, not only to the library's other entry point."""
    from oracle import TemporalMemoryOracle, canonical_synapses
    case, steps = F.BY_NAME["wave1-one-thread"], 60
    C, K, rows = case.C, case.K, case.rows
    tm, single = _pair(case)
    ora = TemporalMemoryOracle(C, K, seed=5)
    rec = tm.run(rows, steps, record=ALL)
    assert np.array_equal(rec.active_column, _contract_rows(rows, C, 0, steps))
    for t in range(steps):
        o = ora.step(np.sort(rows[t % len(rows)]).astype(np.int64))
        single.run(rows, 1)
        s = single.last_state
        assert np.array_equal(rec.column_prediction[t], o.cell_prediction.any(axis=1)), t
        assert rec.active_cells[t] == len(o.active_cell[0]) and rec.winner_cells[t] == len(o.winner_cell[0]), t
        assert rec.bursting_columns[t] == int(o.active_column_bursting.sum()), t
        assert np.array_equal(s.cell_activation, o.cell_activation) and np.array_equal(s.cell_prediction, o.cell_prediction), t
        got, want = (np.sort(w[0].astype(np.int64) * K + w[1]) for w in (s.winner_cell, o.winner_cell))
        assert np.array_equal(got, want), t
    assert rec.predicted_columns.max() > 0 and rec.new_segments.sum() > 0
    assert rec.column_prediction[:, C - 1].any()                # (the last column, alone in its ballot word, comes to be predicted)
    co = canonical_synapses(ora.seg_cell[:ora.S], ora.presyn[:ora.S], ora.perm[:ora.S])
    for x in (tm, single):
        st = x._engine.read_store()
        cx = canonical_synapses(st["seg_cell"], st["presyn"], st["perm"])
        assert len(cx) == len(co) and all(p[0] == q[0] and np.array_equal(p[1], q[1]) and np.array_equal(p[2].view(np.int32), q[2].view(np.int32))
                                          for p, q in zip(cx, co))


@pytest.mark.gpu
def test_the_lds_cap_and_one_column_more():
    """column_dim 524 032: 64 words a thread and exactly 64 KiB of dynamic LDS -- no HIP error, and the contract.  524 033: refused with
    HTM_ERR_ARGUMENT, the handle's step index unchanged."""
    import bithtm_amd as B
    from types import SimpleNamespace
    from bithtm_amd.engine import HtmError
    case = F.BY_NAME["lds-cap"]
    assert case.C == F.LDS_CAP_C
    tm, twin = _pair(case)
    _run_case(case, tm, twin)
    tm._engine.sync()                                           # (no HIP error: the stream is healthy)
    assert tm._engine.info().capacity_error == 0
    C = case.C + 1
    over = B.TemporalMemory(C, case.K, distal_projection=B.PredictiveProjection(C * case.K, segment_capacity=4096, segment_slots=128), seed=5)
    over.process(SimpleNamespace(active_column=case.rows[0]))  # (the stepwise path takes the shape)
    eng = over._engine
    with pytest.raises(HtmError, match=r"\(-1\).*does not fit the LDS \(column_dim above 524032\)") as e:
        eng.tm_run(eng.upload_lists(case.rows), len(case.rows), case.n, 4)
    assert "HIP" not in str(e.value)
    assert eng.steps == 1 and eng.info().step_index == 1 and eng.info().capacity_error == 0
    eng.sync()


def _prediction_bits(words, C):
    return np.unpackbits(np.ascontiguousarray(words).view(np.uint8), axis=1, bitorder="little")[:, :C].astype(bool)


@pytest.mark.gpu
@pytest.mark.parametrize("name", F.BAD_IDS)
def test_bad_row_is_repaired_exactly(name, monkeypatch):
    """One bad row among good ones, uploaded unchecked: the documented CapacityError (no HIP error), bit 128, a healthy stream; every
    step's recorded list == feed_contract, the repaired row's too; records and the state left == a twin stepped with process() over
    the repaired lists, every info() field but capacity_error; and a fresh Temporal Memory on the device runs a good case."""
    from bithtm_amd.engine import CapacityError
    b = {x.name: x for x in F.BAD_ROWS}[name]
    R, n, steps = len(b.rows), b.n, b.steps
    fixed = F.repaired(b.rows, b.C)
    tm, twin = _pair(b)
    eng = tm._ensure_engine(n)
    eng.use_epsilon(1e-8)                                       # (process()'s default, as TemporalMemory.run sets it)
    raw = eng.tm_run(eng.upload_lists(b.rows, check=False), R, n, steps, record=ALL, check=False)
    with pytest.raises(CapacityError) as e:
        eng.check_capacity()
    assert "htm_tm_run met a list row" in str(e.value) and "HIP" not in str(e.value)
    info = eng.info()
    assert info.capacity_error & 128 and info.capacity_error == 128 and info.step_index == steps
    eng.sync()                                                  # (no HIP error: the stream is healthy)
    assert raw["active_column"].shape == (steps, n)
    assert np.array_equal(raw["active_column"], fixed[np.arange(steps) % R])
    counters, cols, preds = _expected(twin, fixed, 0, steps)
    assert np.array_equal(raw["counters"], counters) and np.array_equal(raw["active_column"], cols)
    assert np.array_equal(_prediction_bits(raw["column_prediction"], b.C), preds)
    monkeypatch.setattr(eng, "check_capacity", eng.info)        # (reading the state of a flagged handle: the flag is compared below)
    _assert_same_tm(tm, twin, but=("capacity_error",))
    assert twin._engine.info().capacity_error == 0
    good = F.BY_NAME["wave1-one-thread"]
    fresh, other = _pair(good)
    rec = fresh.run(good.rows, 7, record=ALL)
    assert np.array_equal(rec.active_column, _contract_rows(good.rows, good.C, 0, 7))
    _assert_record(rec, _expected(other, good.rows, 0, 7), what="after the bad bank")
    _assert_same_tm(fresh, other)
