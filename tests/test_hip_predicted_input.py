"""Predicted-input decoding on the device (HierarchicalTemporalMemory.predicted_input, run(record=("predicted_input", ...)),
ModelGroup.run(record=...); htm_predicted_input / htm_set_run_predicted_input): the reference's votes after every process()
(tests/golden/predicted_input.npz), batched runs against the same steps taken one by one in every schedule, the overlap
identity at full size, group members against solo twins, the graphs of undecoded calls, and the refusals.

The votes kernel's geometry -- input_dim beyond one pass of its bit loop, partial and empty column chunks, the unroll tail,
the second cell word, the connected mask on the threshold and under learning -- is held to the definition on hand-built
states in tests/test_hip_topdown_geometry.py (cases: tests/topdown_cases.py)."""

import ctypes as C
import os

import numpy as np
import pytest

from test_hip_run_record import SCHEDULES, SCHEDULE_IDS, _bank, _rows, _twins

FIXTURE = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "predicted_input.npz")
RESETS = np.array([0, 0, 1, 0, 0, 0, 1, 1], bool)          # rows 2, 6 and 7: two consecutive resets
PIN = ("predicted_input",)


def _stepwise(htm, inputs, start, resets=None, learning=True):
    """process() step by step (reset() before every step whose bank row has its flag): int32[n, input_dim] of
    predicted_input() after each step."""
    out = []
    for i, x in enumerate(inputs):
        if resets is not None and resets[(start + i) % len(resets)]:
            htm.reset()
        htm.process(x, learning=learning)
        out.append(htm.predicted_input())
    return np.asarray(out, np.int32).reshape(len(inputs), -1)


def _same_votes(got, want, what):
    assert got.dtype == np.int32 and got.shape == want.shape, what
    bad = np.argwhere((got != want).any(axis=1)).ravel()
    assert not len(bad), f"{what}: steps {bad[:5].tolist()} differ (first: {np.flatnonzero(got[bad[0]] != want[bad[0]])[:8].tolist()})"


@pytest.mark.gpu
def test_process_votes_equal_the_reference():
    """predicted_input() after each process() -- with the fixture's resets and learning flags -- gives the unmodified
    reference's votes, bit for bit; a fresh model's are zero."""
    import bithtm_amd as B
    import refdiff
    from test_predicted_input_cpu import fixture_inputs
    rec = dict(np.load(FIXTURE))
    seed, I, Cn, K, k = (int(rec[f]) for f in ("seed", "input_dim", "column_dim", "cell_dim", "active_columns"))
    np.random.seed(seed)
    htm = B.HierarchicalTemporalMemory(I, Cn, K, active_columns=k, seed=seed)
    assert refdiff.digest(htm.engine.get_permanence()) == rec["permanence_digest"]
    assert not htm.predicted_input().any()
    resets = set(rec["resets"].tolist())
    for t, x in enumerate(fixture_inputs(rec)):
        if t in resets:
            htm.reset()
        htm.process(x, learning=bool(rec["learning"][t]))
        votes = htm.predicted_input()
        assert votes.dtype == np.int32 and votes.shape == (I,)
        assert int(votes.sum()) == int(rec["votes_total"][t]), f"step {t}"
        assert refdiff.digest(votes) == rec["votes_digest"][t], f"step {t}: votes differ from the reference's"


@pytest.mark.gpu
@pytest.mark.parametrize("pipeline", [True, False], ids=["pipelined", "unpipelined"])
@pytest.mark.parametrize("env", SCHEDULES, ids=SCHEDULE_IDS)
@pytest.mark.parametrize("size", [(300, 1024, 8, 64), (300, 512, 48, 48)], ids=["1024x8", "512x48"])
def test_run_votes_equal_stepwise_votes(size, env, pipeline, monkeypatch):
    """run(record=("predicted_input", ...)) == predicted_input() after each process(), with resets, a stretch with learning
    off and continuing chunks; in every schedule, graphs or eager, pipelined or not.  (The four-launch schedule applies the
    next step's SP rows before a step's predictions: a decoding call must not take it.)"""
    for key, v in env.items():
        monkeypatch.setenv(key, v)
    I, Cn, K, k = size
    bank = _bank(8, I, 3)
    htm, twin = _twins(I, Cn, K, active_columns=k)
    rec = htm.run(bank, 80, record=("counters",) + PIN, pipeline=pipeline, resets=RESETS)
    want = _stepwise(twin, _rows(bank, 0, 80), 0, RESETS)
    _same_votes(rec.predicted_input, want, "learning")
    assert (want.sum(axis=1) > 0).sum() > 20 and rec.predicted_columns.max() > 0
    assert np.array_equal(rec.predicted_input.sum(axis=1) > 0, rec.predicted_columns > 0)
    rec = htm.run(bank, 20, learning=False, record=PIN, pipeline=pipeline)
    _same_votes(rec.predicted_input, _stepwise(twin, _rows(bank, 80, 20), 80, learning=False), "learning off")
    parts = [htm.run(bank, 15, record=PIN, pipeline=pipeline, continuing=True) for _ in range(2)]
    parts.append(htm.run(bank, 9, record=PIN, pipeline=pipeline))
    got = np.concatenate([p.predicted_input for p in parts])
    _same_votes(got, _stepwise(twin, _rows(bank, 100, 39), 100), "continuing chunks")
    assert np.array_equal(htm.predicted_input(), got[-1])
    st, sw = htm.state_dict(), twin.state_dict()
    for key in st:
        assert np.array_equal(st[key], sw[key]), key


@pytest.mark.gpu
@pytest.mark.parametrize("lean", ["2", "1", "0"])
def test_decoding_calls_take_a_schedule_without_rows_ahead(lean, monkeypatch):
    """htm_run_plan: a handle with decoding rows set runs pipelined only where the schedule applies a step's rows within it
    (the two- and three-launch ones); clearing the rows gives the plan back."""
    monkeypatch.setenv("BITHTM_LEAN", lean)
    import bithtm_amd as B
    htm = B.HierarchicalTemporalMemory(300, 1024, 8, active_columns=64, seed=2)
    eng = htm.engine
    plain = eng.run_plan(100)
    assert plain["pipelined"]
    buf = eng._record_buffer("predicted_input", 100 * 300)
    eng.set_run_predicted_input(buf)
    try:
        assert eng.run_plan(100)["pipelined"] == (lean != "0")
    finally:
        eng.set_run_predicted_input(None)
    assert eng.run_plan(100) == plain


@pytest.mark.gpu
def test_overlap_identity_at_full_size():
    """65 536 x 32 (the benchmark's shape), learning: votes_t . x_{t+1} == the sum of step t+1's overlaps (the device's own
    sp_state.overlaps) over the columns step t predicts; a decoded graph-replayed run ends on the votes predicted_input() reads."""
    import bithtm_amd as B
    I, Cn, K = 1024, 65536, 32
    np.random.seed(9)
    htm = B.HierarchicalTemporalMemory(I, Cn, K, seed=9)
    bank = _bank(50, I, 4, density=0.02)
    htm.run(bank, 600)
    checked = 0
    for t in range(600, 612):
        votes = htm.predicted_input()
        pred = htm.temporal_memory.last_state.cell_prediction.any(axis=1)
        x = bank[t % len(bank)]
        sp, _ = htm.process(x)
        assert int(votes.astype(np.int64) @ x) == int(np.asarray(sp.overlaps)[pred].sum()), t
        checked += bool(pred.any())
    assert checked >= 1
    rec = htm.run(bank, 128, record=PIN + ("column_prediction",))
    assert np.array_equal(rec.predicted_input[-1], htm.predicted_input())
    assert np.array_equal(rec.predicted_input.sum(axis=1) > 0, rec.column_prediction.any(axis=1))


@pytest.mark.gpu
@pytest.mark.parametrize("eager", [False, True], ids=["graphs", "eager"])
def test_group_members_equal_solo_twins(eager, monkeypatch):
    """ModelGroup.run(record=("predicted_input", ...)): one array per member, each equal to its solo twin's run(record=)."""
    if eager:
        monkeypatch.setenv("BITHTM_EAGER_BELOW", "100000")
    from test_hip_model_group import _banks, _group
    group, twins, _ = _group((300, 1024, 8, 64), 3)
    inputs = _banks(3, 8, 300, 3)
    recs = group.run(inputs, 120, record=PIN + ("counters",))
    assert len(recs) == 3
    for i, t in enumerate(twins):
        want = t.run(inputs[i], 120, record=PIN + ("counters",))
        _same_votes(recs[i].predicted_input, want.predicted_input, f"member {i}")
        assert np.array_equal(recs[i].predicted_columns, want.predicted_columns)
    assert max(int(r.predicted_input.sum()) for r in recs) > 0
    recs = group.run(inputs, 10, learning=False, record=PIN)
    for i, t in enumerate(twins):
        _same_votes(recs[i].predicted_input, t.run(inputs[i], 10, learning=False, record=PIN).predicted_input, f"member {i}, learning off")
        assert np.array_equal(group.models[i].predicted_input(), recs[i].predicted_input[-1])


@pytest.mark.gpu
def test_undecoded_calls_capture_no_new_graphs():
    """Decoding calls capture graphs of their own, once; undecoded calls after them replay what they replayed before, and a
    decoded call with other rows replays the decoded graphs.  (A fixed pool: growth would re-create the engine.)"""
    from test_hip_model_group import _model, _twin
    bank = _bank(8, 300, 3)
    htm = _model(300, 1024, 8, 5, k=64, capacity=1 << 16)
    twin = _twin(htm, capacity=1 << 16)
    htm.run(bank, 300)
    twin.run(bank, 300)
    plain = htm.engine.graph_count()
    assert plain == twin.engine.graph_count()
    htm.run(bank, 300)
    assert htm.engine.graph_count() == plain
    htm.run(bank, 300, record=PIN)
    decoded = htm.engine.graph_count()
    assert decoded > plain
    htm.run(bank, 300)
    htm.run(bank, 600, record=PIN)                  # (a larger buffer: other rows)
    assert htm.engine.graph_count() == decoded
    for n in (300, 300, 300, 600):
        twin.run(bank, n)
    assert twin.engine.graph_count() == plain
    st, sw = htm.state_dict(), twin.state_dict()
    for key in st:
        assert np.array_equal(st[key], sw[key]), key


@pytest.mark.gpu
def test_pool_growth_inside_a_decoded_run():
    """A default-sized pool that grows in the middle of run(record=("predicted_input",)): one contiguous array, equal to the
    stepwise votes."""
    I, Cn, K = 400, 1024, 8
    bank = _bank(500, I, 8, density=0.1)           # (no repeats: nearly every column bursts and asks for a new segment)
    htm, twin = _twins(I, Cn, K)
    first = htm.engine
    rec = htm.run(bank, 500, record=PIN)
    assert htm.engine is not first                  # (the pool did grow)
    assert rec.predicted_input.shape == (500, I) and np.array_equal(rec.step_index, np.arange(500))
    _same_votes(rec.predicted_input, _stepwise(twin, _rows(bank, 0, 500), 0), "growth")


@pytest.mark.gpu
def test_refusals():
    import bithtm_amd as B
    import bithtm_amd.regularizations as R
    from bithtm_amd.distributed import LocalGroup
    from bithtm_amd.engine import HtmError
    I, Cn, K, k = 300, 1024, 8, 64
    bank = _bank(8, I, 3)

    class Boost(R.ExponentialBoosting):          # a plug-in (a subclass runs on the host)
        pass
    plug = B.HierarchicalTemporalMemory(I, Cn, K, spatial_pooler=B.SpatialPooler(I, Cn, k, boosting=Boost(Cn, k)))
    with pytest.raises(RuntimeError, match="plug-in"):
        plug.predicted_input()
    with pytest.raises(RuntimeError):
        plug.run(bank, 2, record=PIN)
    wide = B.HierarchicalTemporalMemory(I, Cn, 80, active_columns=k)       # cell_dim > 64: the Temporal Memory on the host
    with pytest.raises(RuntimeError, match="host"):
        wide.predicted_input()
    with pytest.raises(ValueError):
        B.HierarchicalTemporalMemory(I, Cn, K, active_columns=k).run(bank, 2, record=("counters", "overlaps"))
    # the Spatial Pooler ahead (HTM_RUN_CONTINUE): refused until the stream ends
    htm = B.HierarchicalTemporalMemory(I, Cn, K, active_columns=k)
    htm.run(bank, 20, continuing=True)
    if htm.engine.run_plan(20, continuing=True)["pipelined"]:
        with pytest.raises(HtmError):
            htm.predicted_input()
    htm.run(bank, 5)
    assert htm.predicted_input().shape == (I,)
    # column-sharded handles, at the C ABI and in Python
    group = LocalGroup(2, I, Cn, K, permanence=np.random.RandomState(0).rand(Cn, I) * 0.1)
    g = group.engines[0]
    buf = htm.engine._record_buffer("predicted_input", I)
    assert g.lib.htm_set_run_predicted_input(g.h, C.c_void_p(buf)) == -4                # HTM_ERR_STATE
    out = np.zeros(I, np.int32)
    assert g.lib.htm_predicted_input(g.h, out.ctypes.data_as(C.c_void_p)) == -4
    assert g.lib.htm_set_run_predicted_input(g.h, None) == 0
    with pytest.raises(NotImplementedError):
        group.predicted_input()
    # a handle without a Temporal Memory (an SP-only engine)
    sp = B.SpatialPooler(I, Cn, k)
    eng = sp._ensure_engine()
    assert eng.lib.htm_set_run_predicted_input(eng.h, C.c_void_p(buf)) == -4
    assert eng.lib.htm_predicted_input(eng.h, out.ctypes.data_as(C.c_void_p)) == -4
    assert htm.engine.lib.htm_predicted_input(htm.engine.h, None) == -1
