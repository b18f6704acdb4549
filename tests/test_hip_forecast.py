"""Closed-loop forecasting on the device (HierarchicalTemporalMemory.forecast / predicted_bits, InferenceView.forecast,
ModelGroup.forecast; htm_encode_votes / htm_set_run_feedback): the recorded run of the unmodified reference
(tests/golden/forecast.npz), the stepwise host loop predicted_input() -> encode -> process(learning=False) on a twin in every
schedule, call and chunk boundaries, the encoding kernel on its own (ties, odd input_dim, votes beyond one radix digit), views
against full copies, group members against solo forecasts, the graphs of calls without feedback, and the refusals.

The encoding kernel's layout cases -- rows of one chunk and of hundreds per wave, a tie quota that ends on a lane, chunk or
wave-run boundary, every input on one vote, candidates == max_bits, the raw row's pad bits and neighbours -- and the
feeding launches at input_dim 1 025 / 2 049 are in tests/test_hip_topdown_geometry.py (cases: tests/topdown_cases.py)."""

import ctypes as C

import numpy as np
import pytest

from forecast_fixture import CASES, FIXTURE, encode, training_inputs, unpack_rows
from test_hip_run_record import ALL, SCHEDULES, SCHEDULE_IDS, _assert_record, _bank, _expected, _twins

SIZES = [(300, 1024, 8, 64), (300, 512, 48, 48)]
SIZE_IDS = ["1024x8", "512x48"]
FIELDS = ALL + ("predicted_input",)
# 45 passes over the 8-row bank.  How long a closed loop stays alive is a property of the learned model, not of the code under
# test, so what the tests below assert about non-empty rows was read off the ORACLE run through the same scenarios (seed 5,
# this bank): after 360 learning steps the 1 024 x 8 model follows its sequence for 70 steps and more under (1, 10) and (8, 18),
# the 512 x 48 model for 9 and 5 steps; after 160 steps (the first choice) the 1 024 x 8 loop died after two rows.
TRAIN = 360


def _trained(size, n=2, seed=5):
    """n identical models of `size` after TRAIN learning steps over the same bank, and the bank."""
    I, Cn, K, k = size
    bank = _bank(8, I, 3)
    models = _twins(I, Cn, K, seed=seed, active_columns=k)
    while len(models) < n:
        models += _twins(I, Cn, K, seed=seed, active_columns=k)
    for m in models[:n]:
        m.run(bank, TRAIN)
    return models[:n], bank


def _host_loop(htm, n, min_votes, max_bits):
    """The loop forecast() replaces, on calls that exist without it: (rows, the record's fields as _expected gives them, votes)."""
    rows, parts, votes = [], [], []
    for _ in range(n):
        x = encode(htm.predicted_input(), min_votes, max_bits)
        parts.append(_expected(htm, [x], learning=False))
        rows.append(x)
        votes.append(htm.predicted_input())
    return (np.asarray(rows, bool), tuple(np.concatenate([p[i] for p in parts]) for i in range(3)), np.asarray(votes, np.int32))


def _same_state(a, b, what=""):
    x, y = a.state_dict(), b.state_dict()
    assert x.keys() == y.keys()
    for key in x:
        assert np.array_equal(np.asarray(x[key]), np.asarray(y[key])), f"{what}: {key}"


def _same_rows(got, want, what=""):
    assert got.dtype == np.bool_ and got.shape == want.shape, what
    bad = np.flatnonzero((got != want).any(axis=1))
    assert not len(bad), f"{what}: rows {bad[:5].tolist()} differ (first: got {np.flatnonzero(got[bad[0]]).tolist()}, want {np.flatnonzero(want[bad[0]]).tolist()})"


_fixture_model = {}


def _fixture_trained():
    """The fixture's record, a fresh model of its shape, and the state after its training and context steps (trained once per
    module; only the state is kept -- a live handle on a stream of its own would take the pipelined schedules from every
    later test)."""
    import bithtm_amd as B
    import refdiff
    rec = _fixture_model.get("rec")
    if rec is None:
        rec = _fixture_model["rec"] = dict(np.load(FIXTURE))
    seed, I, Cn, K, k = (int(rec[f]) for f in ("seed", "input_dim", "column_dim", "cell_dim", "active_columns"))
    np.random.seed(seed)
    htm = B.HierarchicalTemporalMemory(I, Cn, K, active_columns=k, seed=seed)
    if "state" not in _fixture_model:
        assert refdiff.digest(htm.engine.get_permanence()) == rec["permanence_digest"]
        bank, n_train, n_all = training_inputs(rec)
        htm.run(bank, n_train)
        htm.run(bank, n_all - n_train, learning=False)
        _fixture_model["state"] = htm.state_dict()
    return rec, htm, _fixture_model["state"]


@pytest.mark.gpu
@pytest.mark.parametrize("case", range(len(CASES)), ids=[f"min{a}-max{b}" for a, b in CASES])
def test_forecast_equals_the_reference(case):
    """forecast() from the fixture's trained state == the unmodified reference's closed loop: every row, the votes each step
    leaves, every step's active columns -- the sustained cases and the one whose rows go empty."""
    import refdiff
    rec, htm, state = _fixture_trained()
    htm.load_state_dict(state)
    min_votes, max_bits = CASES[case]
    steps, I = int(rec["steps"]), int(rec["input_dim"])
    assert refdiff.digest(htm.predicted_input()) == rec["seed_votes_digest"][case]
    rows, record = htm.forecast(steps, min_votes, max_bits, record=("active_column", "predicted_input"))
    _same_rows(rows, unpack_rows(rec["rows"][case], I), f"case {CASES[case]}")
    assert [refdiff.digest(v) for v in record.predicted_input] == rec["votes_digest"][case].tolist()
    assert np.array_equal(record.active_column, rec["active_column"][case])
    assert np.array_equal(record.step_index, int(state["tm_step_index"]) + np.arange(steps))
    if case == 2:
        assert not rows[-1].any() and not htm.predicted_input().any()      # (empty rows: still a step of the reference's loop)


@pytest.mark.gpu
@pytest.mark.parametrize("env", SCHEDULES, ids=SCHEDULE_IDS)
@pytest.mark.parametrize("size", SIZES, ids=SIZE_IDS)
def test_forecast_equals_the_host_loop(size, env, monkeypatch):
    """forecast(n) == n times predicted_input() -> encode -> process(learning=False) on a twin: the rows, every record field,
    the state left behind; a call below BITHTM_EAGER_BELOW (launched eagerly) and one above it (graphs), in every schedule the
    handle could otherwise take (a feeding call runs unpipelined in all of them)."""
    for key, v in env.items():
        monkeypatch.setenv(key, v)
    (htm, twin), bank = _trained(size)
    for n, (min_votes, max_bits) in ((20, (1, 10)), (70, (8, 18))):
        for m in (htm, twin):                       # (context: each call starts on the learned sequence, with predictions)
            m.run(bank, 8, learning=False)
        rows, rec = htm.forecast(n, min_votes, max_bits, record=FIELDS)
        want_rows, want_rec, want_votes = _host_loop(twin, n, min_votes, max_bits)
        _same_rows(rows, want_rows, f"{n} steps")
        _assert_record(rec, want_rec, what=f"{n} steps")
        assert np.array_equal(rec.predicted_input, want_votes)
        assert rows[0].any() and rows.sum(axis=1).max() <= max_bits
        assert rows[-1].any() or size != SIZES[0]                   # (1 024 x 8: alive to the end of both calls)
    _same_state(htm, twin)
    assert np.array_equal(htm.temporal_memory.last_state.cell_prediction, twin.temporal_memory.last_state.cell_prediction)
    assert np.array_equal(htm.predicted_input(), twin.predicted_input())


@pytest.mark.gpu
@pytest.mark.parametrize("lean", ["2", "0"])
def test_feeding_calls_are_planned_unpipelined(lean, monkeypatch):
    """htm_run_plan: with feedback set a run is reported unpipelined, whatever schedule the handle has; clearing gives it back."""
    monkeypatch.setenv("BITHTM_LEAN", lean)
    (htm,), _ = _trained(SIZES[0], n=1)
    eng = htm.engine
    plain = eng.run_plan(100)
    assert plain["pipelined"]
    bank = htm._zero_bank(eng, 9)
    eng.set_run_feedback(bank, 9, 1, 0)
    try:
        plan = eng.run_plan(100, continuing=True)
        assert not plan["pipelined"] and not plan["lean"] and plan["hip_graph"]
    finally:
        eng.set_run_feedback(None)
    assert eng.run_plan(100) == plain


@pytest.mark.gpu
def test_call_and_chunk_boundaries_change_nothing():
    """Two consecutive forecast() calls == one of the summed length == one cut into chunks of 7 steps (forecast_chunk)."""
    (a, b, c), _ = _trained(SIZES[0], n=3)
    whole, rec_whole = a.forecast(70, 1, 10, record=FIELDS)
    first, rec1 = b.forecast(31, 1, 10, record=FIELDS)
    second, rec2 = b.forecast(39, 1, 10, record=FIELDS)
    _same_rows(np.concatenate([first, second]), whole, "two calls")
    c.forecast_chunk = 7
    chunked, rec_c = c.forecast(70, 1, 10, record=FIELDS)
    _same_rows(chunked, whole, "chunks of 7")
    for name in ("active_column", "predicted_input", "column_prediction", "active_columns", "bursting_columns", "predicted_columns_before",
                 "predicted_columns", "step_index"):
        assert np.array_equal(np.concatenate([getattr(rec1, name), getattr(rec2, name)]), getattr(rec_whole, name)), name
        assert np.array_equal(getattr(rec_c, name), getattr(rec_whole, name)), name
    assert whole[-1].any()                          # (the loop was still alive at the end: the boundaries were crossed with predictions)
    _same_state(a, b, "two calls")
    _same_state(a, c, "chunks")
    assert len(rec_whole) == 70 and a.engine.steps == TRAIN + 70


PARAMS = [(1, 0), (1, 10), (1, 1), (2, 7), (3, 0), (1, 100000), (1000, 3)]


@pytest.mark.gpu
@pytest.mark.parametrize("size", SIZES + [(1000, 1024, 8, 64)], ids=SIZE_IDS + ["input1000"])
def test_predicted_bits_equal_the_encoded_votes(size):
    """predicted_bits() == encode(predicted_input()): the threshold form and the capped form with many ties at the cut-off
    (min_votes 1, max_bits 10: most candidates have the same few votes), input_dim 1000 (no multiple of 128: pad bits)."""
    (htm,), _ = _trained(size, n=1)
    votes = htm.predicted_input()
    assert (votes > 0).sum() > 10 and np.bincount(votes[votes > 0]).max() > 1        # (candidates, and ties among them)
    for min_votes, max_bits in PARAMS:
        got = htm.predicted_bits(min_votes, max_bits)
        assert got.dtype == np.bool_ and got.shape == (size[0],)
        assert np.array_equal(got, encode(votes, min_votes, max_bits)), (min_votes, max_bits)
    assert np.array_equal(htm.predicted_input(), votes)             # (the scratch votes are the call's own)
    assert htm.engine.steps == TRAIN


@pytest.mark.gpu
def test_encode_kernel_beyond_one_radix_digit():
    """Votes above 4 096 (the select's second 12-bit pass), with ties at the cut-off on both sides of a digit boundary: a model
    whose every column is predicted and whose column c is connected to input i iff c < want[i], so votes == want."""
    import bithtm_amd as B
    I, Cn, K = 333, 8192, 4
    rng = np.random.RandomState(2)
    want = rng.choice([0, 1, 5, 4095, 4096, 4097, 8191, 8192, 6000], size=I).astype(np.int32)
    want[-1] = 8192
    htm = B.HierarchicalTemporalMemory(I, Cn, K, active_columns=64, seed=1)
    htm.engine.set_permanence(np.where(np.arange(Cn)[:, None] < want[None, :], 1.0, -1.0))       # (connected: permanence >= 0.0)
    htm.engine.import_prev_state(np.ones((Cn, K), bool), np.zeros((Cn, K), bool), None, None)
    assert np.array_equal(htm.predicted_input(), want)
    for min_votes, max_bits in [(1, 0), (4096, 0), (1, 1), (1, 40), (1, 75), (1, 150), (2, 200), (4097, 30), (1, 333), (9000, 5)]:
        assert np.array_equal(htm.predicted_bits(min_votes, max_bits), encode(want, min_votes, max_bits)), (min_votes, max_bits)


@pytest.mark.gpu
def test_view_forecast_equals_a_full_copy_and_leaves_the_parent_alone():
    """view.run(context); view.forecast(k) == the same on a full copy of the parent after reset(); the parent's state_dict() is
    what it was."""
    (parent, copy_), bank = _trained(SIZES[1])
    before = parent.state_dict()
    view = parent.inference_view()
    copy_.reset()
    for m in (view, copy_):
        m.run(bank, 11, learning=False)
    rows, rec = view.forecast(40, 1, 10, record=FIELDS)
    want, want_rec = copy_.forecast(40, 1, 10, record=FIELDS)
    _same_rows(rows, want, "view")
    assert rows.any()
    for name in ("active_column", "predicted_input", "column_prediction", "bursting_columns", "step_index"):
        assert np.array_equal(getattr(rec, name), getattr(want_rec, name)), name
    assert np.array_equal(view.predicted_bits(1, 10), copy_.predicted_bits(1, 10))
    assert np.array_equal(view.temporal_memory.last_state.cell_prediction, copy_.temporal_memory.last_state.cell_prediction)
    after = parent.state_dict()
    for key in before:
        assert np.array_equal(before[key], after[key]), key
    with pytest.raises(ValueError):
        view.forecast(3, learning=True)


@pytest.mark.gpu
@pytest.mark.parametrize("eager", [False, True], ids=["graphs", "eager"])
def test_group_members_equal_their_solo_forecasts(eager, monkeypatch):
    """ModelGroup.forecast with 3 differently trained members and per-member parameters: each member == its twin's solo
    forecast (rows, record, state); cut into chunks too."""
    if eager:
        monkeypatch.setenv("BITHTM_EAGER_BELOW", "100000")
    from test_hip_model_group import _banks, _group
    group, twins, _ = _group(SIZES[0], 3)
    inputs = _banks(3, 8, 300, 3)
    group.run(inputs, TRAIN)
    for t, x in zip(twins, inputs):
        t.run(x, TRAIN)
    min_votes, max_bits = [1, 2, 1], [10, 18, 0]
    group.forecast_chunk = 64                       # (70 steps: a chunk of 64, replayed as graphs of several steps, and one of 6)
    rows, recs = group.forecast(70, min_votes, max_bits, record=FIELDS)
    assert rows.shape == (3, 70, 300) and rows[:, 0].any(axis=1).all()
    for i, t in enumerate(twins):
        want, want_rec = t.forecast(70, min_votes[i], max_bits[i], record=FIELDS)
        _same_rows(rows[i], want, f"member {i}")
        for name in ("active_column", "predicted_input", "column_prediction", "bursting_columns", "predicted_columns", "step_index"):
            assert np.array_equal(getattr(recs[i], name), getattr(want_rec, name)), (i, name)
        _same_state(group.models[i], t, f"member {i}")
    again = group.forecast(5, 1, 10)                # (scalars: every member the same; no record: just the rows)
    for i, t in enumerate(twins):
        _same_rows(again[i], t.forecast(5, 1, 10), f"member {i}, second call")


@pytest.mark.gpu
def test_group_of_views_and_a_group_that_mixes_fed_and_free_members():
    """Views of one parent in a group: each equals a solo view stepped the same way.  Then, through the C calls, a group call
    in which member 0 feeds back and member 1 reads a data bank: member 0 == a solo forecast, member 1 == a solo run."""
    import bithtm_amd as B
    (parent,), bank = _trained(SIZES[0], n=1)
    views = B.ModelGroup.views(parent, 3)
    solo = [parent.inference_view() for _ in range(3)]
    context = np.stack([np.roll(bank, s, axis=0) for s in range(3)])
    views.run(context, 12)
    for v, x in zip(solo, context):
        v.run(x, 12)
    rows = views.forecast(30, 1, 10)
    for i, v in enumerate(solo):
        _same_rows(rows[i], v.forecast(30, 1, 10), f"view {i}")
        assert np.array_equal(views.models[i].predicted_input(), v.predicted_input())
    assert rows.any(axis=2).all()
    # fed and free members in one group call
    (m0, m1, t0, t1), _ = _trained(SIZES[0], n=4)
    group = B.ModelGroup([m0, m1])
    data = _bank(9, 300, 12)
    e0, e1 = m0.engine, m1.engine
    fed = m0._zero_bank(e0, 9)
    e0.encode_votes(1, 10, fed, 9, e0.steps % 9)
    e0.set_run_feedback(fed, 9, 1, 10)
    banks = (C.c_void_p * 2)(fed, e1.upload_bank(data))
    try:
        assert group.lib.htm_group_run(group._g, banks, 9, 8, 0, 1, None) == 0, group.lib.htm_group_last_error(group._g)
        wrong = (C.c_void_p * 2)(banks[1], banks[1])
        assert group.lib.htm_group_run(group._g, wrong, 9, 8, 0, 1, None) == -1        # member 0's bank is not the one set
        assert group.lib.htm_group_run(group._g, banks, 9, 8, 1, 1, None) == -1        # learning
    finally:
        e0.set_run_feedback(None)
    for m in (m0, m1):
        m.engine.steps += 8
        m.temporal_memory._new_state(None)
    got = e0.read_bank(fed, 9)[(TRAIN + np.arange(8)) % 9]
    _same_rows(got, t0.forecast(8, 1, 10), "fed member")
    t1.run(data, 8, learning=False)
    _same_state(m0, t0, "fed member")
    _same_state(m1, t1, "free member")


@pytest.mark.gpu
def test_calls_without_feedback_capture_and_compute_what_they_did():
    """Feeding calls capture graphs of their own, once; a plain run() after a forecast replays the graphs it had, and a model
    that forecast ends bit-identical to a twin that took the same steps through the host loop and never had feedback set."""
    from test_hip_model_group import _model, _twin
    bank = _bank(8, 300, 3)
    htm = _model(300, 1024, 8, 5, k=64, capacity=1 << 16)
    twin = _twin(htm, capacity=1 << 16)
    for m in (htm, twin):
        m.run(bank, 300)
        m.run(bank, 100, learning=False)
    plain = htm.engine.graph_count()
    assert plain == twin.engine.graph_count()
    rows = htm.forecast(70, 1, 10)
    fed = htm.engine.graph_count()
    assert fed > plain
    htm.forecast(70, 1, 10)
    htm.forecast(80, 2, 18)                         # (other parameters: the same graphs, the descriptor differs)
    assert htm.engine.graph_count() == fed
    want, _, _ = _host_loop(twin, 70, 1, 10)
    _same_rows(rows, want)
    _host_loop(twin, 70, 1, 10)
    _host_loop(twin, 80, 2, 18)
    for m in (htm, twin):                           # (learning off: the pool, and with it the scan's form, stays what it was)
        m.run(bank, 100, learning=False)
    assert htm.engine.graph_count() == fed and twin.engine.graph_count() == plain
    for m in (htm, twin):
        m.run(bank, 300)
    _same_state(htm, twin)


@pytest.mark.gpu
def test_refusals():
    import bithtm_amd as B
    import bithtm_amd.regularizations as R
    from bithtm_amd.distributed import LocalGroup
    from bithtm_amd.engine import HtmError
    I, Cn, K, k = SIZES[0]
    (htm,), bank = _trained(SIZES[0], n=1)
    eng, lib = htm.engine, htm.engine.lib
    with pytest.raises(ValueError, match="learning"):
        htm.forecast(5, learning=True)
    for bad in ((0, 0), (-1, 0), (1, -1)):
        with pytest.raises(ValueError):
            htm.forecast(5, *bad)
        with pytest.raises(ValueError):
            htm.predicted_bits(*bad)
    with pytest.raises(ValueError):
        htm.forecast(5, record=("overlaps",))
    fed, other = htm._zero_bank(eng, 9), eng.upload_bank(bank)
    # the C calls' argument checks
    assert lib.htm_encode_votes(eng.h, 0, 0, C.c_void_p(fed), 9, 0) == -1
    assert lib.htm_encode_votes(eng.h, 1, -1, C.c_void_p(fed), 9, 0) == -1
    assert lib.htm_encode_votes(eng.h, 1, 0, C.c_void_p(fed), 9, 9) == -1
    assert lib.htm_encode_votes(eng.h, 1, 0, C.c_void_p(fed), 9, -1) == -1
    assert lib.htm_encode_votes(eng.h, 1, 0, None, 9, 0) == -1
    assert lib.htm_encode_votes(eng.h, 1, 0, C.c_void_p(fed + 4), 9, 0) == -1          # not 16-byte aligned
    assert lib.htm_set_run_feedback(eng.h, C.c_void_p(fed), 9, 0, 0) == -1
    assert lib.htm_set_run_feedback(eng.h, C.c_void_p(fed), 0, 1, 0) == -1
    assert lib.htm_set_run_feedback(eng.h, C.c_void_p(fed + 8), 9, 1, 0) == -1
    # while feedback is set: learning, another bank, another n_inputs, reset bits
    eng.set_run_feedback(fed, 9, 1, 10)
    try:
        assert lib.htm_run(eng.h, C.c_void_p(fed), 9, 4, 1, 1) == -1
        assert lib.htm_run(eng.h, C.c_void_p(other), 8, 4, 0, 1) == -1
        assert lib.htm_run(eng.h, C.c_void_p(fed), 8, 4, 0, 1) == -1
        assert lib.htm_prepare(eng.h, C.c_void_p(other), 9, 100, 0, 1) == -1
        eng.set_run_resets(eng.upload_resets(np.arange(9) == 3), 9)
        try:
            assert lib.htm_run(eng.h, C.c_void_p(fed), 9, 4, 0, 1) == -1
        finally:
            eng.set_run_resets(None, 0)
        assert eng.steps == TRAIN and eng.info().step_index == TRAIN              # (nothing was enqueued)
    finally:
        eng.set_run_feedback(None)
    htm.run(bank, 3, learning=False)                # (cleared: a plain run again)
    # a streamed run in the middle
    htm.run(bank, 20, continuing=True)
    with pytest.raises(RuntimeError, match="streamed"):
        htm.forecast(5)
    if eng.run_plan(20, continuing=True)["pipelined"]:          # (the handle is ahead)
        assert lib.htm_set_run_feedback(eng.h, C.c_void_p(fed), 9, 1, 0) == -4
        assert lib.htm_encode_votes(eng.h, 1, 0, C.c_void_p(fed), 9, 0) == -4
    htm.run(bank, 5)
    assert htm.forecast(3).shape == (3, I)
    # plug-ins and layers on the host
    class Boost(R.ExponentialBoosting):
        pass
    plug = B.HierarchicalTemporalMemory(I, Cn, K, spatial_pooler=B.SpatialPooler(I, Cn, k, boosting=Boost(Cn, k)))
    with pytest.raises(RuntimeError, match="plug-in"):
        plug.forecast(3)
    with pytest.raises(RuntimeError):
        B.HierarchicalTemporalMemory(I, Cn, 80, active_columns=k).predicted_bits()
    # column-sharded handles and handles without a Temporal Memory
    group = LocalGroup(2, I, Cn, K, permanence=np.random.RandomState(0).rand(Cn, I) * 0.1)
    g = group.engines[0]
    assert g.lib.htm_set_run_feedback(g.h, C.c_void_p(fed), 9, 1, 0) == -4
    assert g.lib.htm_encode_votes(g.h, 1, 0, C.c_void_p(fed), 9, 0) == -4
    assert g.lib.htm_set_run_feedback(g.h, None, 0, 1, 0) == 0
    sp = B.SpatialPooler(I, Cn, k)._ensure_engine()
    assert sp.lib.htm_set_run_feedback(sp.h, C.c_void_p(fed), 9, 1, 0) == -4
    assert sp.lib.htm_encode_votes(sp.h, 1, 0, C.c_void_p(fed), 9, 0) == -4
    with pytest.raises(HtmError):
        g.encode_votes(1, 0, fed, 9, 0)
