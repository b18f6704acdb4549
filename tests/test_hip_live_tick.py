"""Live ticks of model groups on the device (ModelGroup.tick / ModelGroup.reset; htm_live_tick, htm_live_reset; DESIGN.md
section 21).  The definition a tick is held to is built from calls that exist without it -- per member, in order,

    if resets[i]: m.reset()
    rec = m.run(values[i][None, :], 1, learning=learning, encoder=encoder, record=("counters", "predicted_value"))

-- row i of the tick equals row 0 of `rec`, capacity_error[i] equals m.engine.info().capacity_error and m.state_dict() equals the
twin's, bit for bit.  Every comparison is exact.  Twins are built as tests/test_hip_model_group.py builds them (same seed,
parameters and SP permanences); both launch policies (BITHTM_EAGER_BELOW = 0: graphs, 64: eager) as the group tests have them."""
import numpy as np
import pytest

from live_tick_cases import (EAGER, EAGER_IDS, MID, REFERENCE, SMALL, decoded, derived, encoded_rows, encoder_for, periodic_values,
                             stream_values)
from test_hip_model_group import _banks, _same_state

COUNTERS = ("counters",)
VALUE = ("counters", "predicted_value")
# At 8 active columns a segment samples at most 8 synapses a step: with the default thresholds (15) no segment of the small shape
# would ever match, and nothing would be predicted.  Members and twins of that shape get thresholds such a segment can reach.
TM_PARAMS = {SMALL: dict(segment_activation_threshold=5, segment_matching_threshold=4)}


def _model(size, seed, capacity=None):
    """A fused model of `size`, as tests/test_hip_model_group.py makes its members (TM_PARAMS on top)."""
    import bithtm_amd as B
    I, Cn, K, k = size
    tm = B.TemporalMemory(Cn, K, distal_projection=B.PredictiveProjection(Cn * K, segment_capacity=capacity, **TM_PARAMS.get(size, {})), seed=seed)
    np.random.seed(seed)                         # (the SP's permanences are drawn from NumPy's global stream)
    return B.HierarchicalTemporalMemory(I, Cn, K, active_columns=k, temporal_memory=tm)


def _group(size, B, capacity=None):
    """(group of B members with other seeds, their twins: same seed, parameters and SP permanences, fresh models; None)."""
    import bithtm_amd as Bm
    models = [_model(size, 11 + 7 * i, capacity) for i in range(B)]
    twins = [_model(size, 11 + 7 * i, capacity) for i in range(B)]
    for m, t in zip(models, twins):
        t.engine.set_permanence(m.engine.get_permanence())
    return Bm.ModelGroup(models), twins, None


def _setenv(env, monkeypatch):
    for k, v in env.items():
        monkeypatch.setenv(k, v)


def _twin_step(t, row, enc, reset=False, learning=True, votes=False):
    """The definition's two lines for one member."""
    if reset:
        t.reset()
    fields = (VALUE if enc is not None else COUNTERS) + (("predicted_input",) if votes else ())
    return t.run(row[None, :], 1, learning=learning, encoder=enc, record=fields)


def _same_row(tick, i, rec, t, what):
    from bithtm_amd.engine import RECORD_COUNTERS
    assert tick.step_index[i] == rec.step_index[0], (what, "step_index")
    for name in RECORD_COUNTERS:
        assert getattr(tick, name)[i] == getattr(rec, name)[0], (what, name, int(getattr(tick, name)[i]), int(getattr(rec, name)[0]))
    for name in ("correct_columns", "incorrect_columns", "anomaly_score"):
        assert getattr(tick, name)[i] == getattr(rec, name)[0], (what, name)
    if rec.predicted_bucket is not None:
        assert np.array_equal(tick.predicted_bucket[i], rec.predicted_bucket[0]), (what, "predicted_bucket")
        assert np.array_equal(tick.predicted_score[i], rec.predicted_score[0]), (what, "predicted_score")
        assert np.array_equal(tick.predicted_value[i], rec.predicted_value[0], equal_nan=True), (what, "predicted_value")
    if rec.predicted_input is not None:
        assert np.array_equal(tick.predicted_input[i], rec.predicted_input[0]), (what, "predicted_input")
    assert tick.capacity_error[i] == t.engine.info().capacity_error, (what, "capacity_error")


def _check_tick(tick, twins, rows, enc, resets=None, learning=True, votes=False, what=""):
    """One tick against every twin's step; returns the twins' records."""
    recs = []
    for i, t in enumerate(twins):
        rec = _twin_step(t, rows[i], enc, reset=resets is not None and bool(resets[i]), learning=learning, votes=votes)
        _same_row(tick, i, rec, t, f"{what} member {i}")
        recs.append(rec)
    assert tick.step_index.dtype == np.int64 and tick.capacity_error.dtype == np.int32 and len(tick) == len(twins)
    return recs


CASES = [(SMALL, "default", 3), (MID, "default", 3), (SMALL, "sixteen", 3)]
CASE_IDS = ["128x4", "512x48", "128x4-sixteen-fields"]


def _ticks_equal_the_definition(size, layout, B, train, ticks, epochs=1, jitter=0.01):
    """Training: `epochs` passes over `train` periodic value rows (a whole number of periods), the group and the twins alike."""
    enc = encoder_for(size, layout)
    group, twins, _ = _group(size, B)
    values = stream_values(enc, B, train, ticks, 31, jitter=jitter)
    group.run(values[:, :train], epochs * train, encoder=enc)
    for i, t in enumerate(twins):
        t.run(values[i, :train], epochs * train, encoder=enc)
    recs = []
    for n in range(ticks):
        rows = values[:, train + n]
        tick = group.tick(rows, encoder=enc)
        recs += _check_tick(tick, twins, rows, enc, what=f"tick {n}")
        assert tick.predicted_input is None
    for i, (m, t) in enumerate(zip(group.models, twins)):
        _same_state(m, t, f"member {i}")
    # (that the comparison is of something: the twins' own results)
    k = twins[0].active_columns
    assert any((r.predicted_score > 0).any() for r in recs)
    assert any(np.isnan(r.predicted_value).any() for r in recs)
    assert any(0 < int(r.bursting_columns[0]) < k for r in recs)


@pytest.mark.gpu
@pytest.mark.parametrize("env", EAGER, ids=EAGER_IDS)
@pytest.mark.parametrize("size,layout,B", CASES, ids=CASE_IDS)
def test_ticks_equal_the_definition(size, layout, B, env, monkeypatch):
    """B = 3, trained with group.run over 150 periodic value rows (edge values among them: NaN, +-inf, the range's ends, far
    outside), then 40 ticks: every GroupTick field equals the twin's one-step record, and the states are equal at the end."""
    _setenv(env, monkeypatch)
    _ticks_equal_the_definition(size, layout, B, 150, 40)


@pytest.mark.gpu
def test_ticks_equal_the_definition_at_the_reference_shape():
    """Once at 1 000 -> 2 048 x 32 with the default active columns, B = 5 (two fields of 500 bits, one periodic).  Three passes
    over the 150 rows: at this shape the Spatial Pooler's boosting keeps moving the columns of a value for some 300 steps, and
    nothing is predicted before they settle (the NumPy oracle shows the same)."""
    _ticks_equal_the_definition(REFERENCE, "default", 5, 150, 40, epochs=3, jitter=0.002)


def _learned_unequally(size, enc, seed=41):
    """Three members with different segment counts, one still empty, all at an even step: (group, twins, values [3, rows, F])."""
    group, twins, _ = _group(size, 3)
    values = stream_values(enc, 3, 100, 100, seed)
    for i, n in ((0, 100), (1, 40)):
        group.models[i].run(values[i, :n], n, encoder=enc)
        twins[i].run(values[i, :n], n, encoder=enc)
    return group, twins, values


@pytest.mark.gpu
@pytest.mark.parametrize("env", EAGER, ids=EAGER_IDS)
@pytest.mark.parametrize("size", [SMALL, MID], ids=["128x4", "512x48"])
def test_mixed_resets(size, env, monkeypatch):
    """Flags [1, 0, 1], [0, 0, 0] and [1, 1, 1] on consecutive ticks, starting at an even and at an odd step: a reset member's step
    has no columns predicted before, every active column bursting and no new segment, as its twin after reset(); the others are
    untouched (they equal twins that were not reset)."""
    _setenv(env, monkeypatch)
    enc = encoder_for(size)
    group, twins, values = _learned_unequally(size, enc)
    segments = [t.engine.info().segments for t in twins]
    assert segments[0] > segments[1] > segments[2] == 0
    k, n = twins[0].active_columns, 100
    for parity in (0, 1):
        assert group.models[0].engine.steps % 2 == parity
        for flags in ([1, 0, 1], [0, 0, 0], [1, 1, 1]):
            flags = np.array(flags, bool)
            rows = values[:, n]
            n += 1
            tick = group.tick(rows, encoder=enc, resets=flags)
            recs = _check_tick(tick, twins, rows, enc, resets=flags, what=f"parity {parity} flags {flags.astype(int)}")
            for i, rec in enumerate(recs):
                if flags[i]:
                    assert rec.predicted_columns_before[0] == 0 and rec.bursting_columns[0] == rec.active_columns[0] == k, (parity, i)
                    assert rec.new_segments[0] == 0 and tick.new_segments[i] == 0, (parity, i)
                    assert tick.predicted_columns_before[i] == 0 and tick.anomaly_score[i] == 1.0
        if parity == 0:                             # (four more ticks -- all-false flags, then none -- leave an odd step behind)
            for j in range(4):
                rows = values[:, n]
                n += 1
                _check_tick(group.tick(rows, encoder=enc, resets=np.zeros(3, bool) if j < 2 else None), twins, rows, enc, what="between")
    for i, (m, t) in enumerate(zip(group.models, twins)):
        _same_state(m, t, f"member {i}")


@pytest.mark.gpu
@pytest.mark.parametrize("env", EAGER, ids=EAGER_IDS)
def test_group_reset_equals_the_members_own_reset(env, monkeypatch):
    """group.reset(mask) == reset() of the flagged members: state_dict() right after it and after two further steps; None resets
    all members; members of either parity."""
    _setenv(env, monkeypatch)
    size = MID
    enc = encoder_for(size)
    group, twins, values = _learned_unequally(size, enc)
    n = 100
    for mask in (np.array([1, 0, 1], bool), np.array([0, 1, 0], bool), None):
        for _ in range(3):                          # (an odd number of steps: the next reset meets the other parity)
            rows = values[:, n]
            n += 1
            _check_tick(group.tick(rows, encoder=enc), twins, rows, enc, what="before the reset")
        assert group.models[0].temporal_memory.last_state.cell_prediction.any()
        group.reset(mask)
        for i, t in enumerate(twins):
            if mask is None or mask[i]:
                t.reset()
        for i, (m, t) in enumerate(zip(group.models, twins)):
            _same_state(m, t, f"right after reset({mask}), member {i}")
            if mask is None or mask[i]:
                assert not m.temporal_memory.last_state.cell_prediction.any()
        for step in range(2):
            rows = values[:, n]
            n += 1
            recs = _check_tick(group.tick(rows, encoder=enc), twins, rows, enc, what=f"step {step} after reset({mask})")
            if step == 0:
                assert all(r.predicted_columns_before[0] == 0 for i, r in enumerate(recs) if mask is None or mask[i])
        for i, (m, t) in enumerate(zip(group.models, twins)):
            _same_state(m, t, f"two steps after reset({mask}), member {i}")
    # one member a step further (the group's ticks would refuse the parities): a reset takes members of either parity
    group.models[1].run(values[1, :1], 1, encoder=enc)
    twins[1].run(values[1, :1], 1, encoder=enc)
    group.reset()
    for i, (m, t) in enumerate(zip(group.models, twins)):
        t.reset()
        _same_state(m, t, f"mixed parities, member {i}")


@pytest.mark.gpu
@pytest.mark.parametrize("env", EAGER, ids=EAGER_IDS)
def test_views_tick_without_learning(env, monkeypatch):
    """ModelGroup.views(parent, 3) ticks with learning=False and per-member resets: each view equals a full copy of the parent
    after reset(), stepped with learning=False; the parent is unchanged."""
    _setenv(env, monkeypatch)
    import bithtm_amd as Bm
    size = MID
    enc = encoder_for(size)
    values = stream_values(enc, 4, 100, 40, 43)
    parent = _model(size, 5)
    parent.run(values[3, :100], 100, encoder=enc)
    before = parent.state_dict()
    twins = []
    for _ in range(3):
        t = _model(size, 5)
        t.load_state_dict(before)
        t.reset()
        twins.append(t)
    group = Bm.ModelGroup.views(parent, 3)
    with pytest.raises(ValueError, match="learning=False only"):
        group.tick(values[:3, 100], encoder=enc, learning=True)
    recs = []
    for n in range(30):
        rows = np.stack([values[3, 100 + n + i] for i in range(3)])      # (the parent's sequence, each view at a phase of its own)
        flags = np.array([n % 7 == 3, n % 5 == 1, False]) if n % 2 else None
        tick = group.tick(rows, encoder=enc, resets=flags, learning=None if n % 3 else False, predicted_input=True)
        recs += _check_tick(tick, twins, rows, enc, resets=flags, learning=False, votes=True, what=f"tick {n}")
    assert any((r.predicted_score > 0).any() for r in recs) and any(int(r.predicted_columns[0]) > 0 for r in recs)
    after = parent.state_dict()
    assert before.keys() == after.keys()
    for key in before:
        assert np.array_equal(np.asarray(before[key]), np.asarray(after[key])), key


@pytest.mark.gpu
@pytest.mark.parametrize("env", EAGER, ids=EAGER_IDS)
@pytest.mark.parametrize("size", [SMALL, MID], ids=["128x4", "512x48"])
def test_ticks_without_an_encoder_equal_group_process(size, env, monkeypatch):
    """bool rows: a tick equals group.process on twins (the counters and the state), and each twin's own one-step run; with
    predicted_input=True the votes equal each twin's predicted_input()."""
    _setenv(env, monkeypatch)
    import bithtm_amd as Bm
    B = 3
    group, twins, _ = _group(size, B)
    other = Bm.ModelGroup(twins)
    stream = _banks(B, 8, size[0], 7, density=0.15)
    for n in range(40):
        X = stream[:, n % 8]
        want_votes = n % 2 == 1
        tick = group.tick(X, learning=n != 30, predicted_input=want_votes)
        rec = other.process(X, learning=n != 30)
        assert np.array_equal(tick.step_index, rec.step_index)
        for name in ("active_columns", "bursting_columns", "predicted_columns_before", "predicted_columns", "active_cells", "winner_cells",
                     "segments", "new_segments", "anomaly_score", "correct_columns", "incorrect_columns"):
            assert np.array_equal(getattr(tick, name), getattr(rec, name)), (n, name)
        assert tick.predicted_bucket is None and tick.predicted_value is None and (tick.predicted_input is not None) == want_votes
        if want_votes:
            for i, t in enumerate(twins):
                assert np.array_equal(tick.predicted_input[i], t.predicted_input()), (n, i)
        assert not tick.capacity_error.any()
    assert int(rec.predicted_columns.max()) > 0 and int(tick.predicted_input.max()) > 0
    for i, (m, t) in enumerate(zip(group.models, twins)):
        _same_state(m, t, f"member {i}")
    # ... and against the definition's own line, a one-step run without an encoder
    lone = [_model(size, m.temporal_memory.seed) for m in group.models]
    for m, t in zip(group.models, lone):
        t.load_state_dict(m.state_dict())
    X = stream[:, 3]
    _check_tick(group.tick(X, predicted_input=True), lone, X, None, votes=True, what="one-step run")


@pytest.mark.gpu
def test_ticks_interleave_with_group_runs_and_solo_calls():
    """A tick, then group.run, then a member's own process(): the tick refuses the parity mismatch with the group's message and
    enqueues nothing; the other member steps alone and ticks resume.  A member's own decoding rows
    (htm_set_run_predicted_input) are still set after a tick: a recorded solo run writes them."""
    from bithtm_amd.engine import HtmError
    size = MID
    enc = encoder_for(size)
    group, twins, _ = _group(size, 2)
    values = stream_values(enc, 2, 62, 58, 47)
    _check_tick(group.tick(values[:, 0], encoder=enc), twins, values[:, 0], enc, what="first tick")
    group.run(values[:, 1:61], 60, encoder=enc)
    for i, t in enumerate(twins):
        t.run(values[i, 1:61], 60, encoder=enc)
    x = encoded_rows(enc, values[0, 61])
    group.models[0].process(x)
    twins[0].process(x)
    with pytest.raises(HtmError, match="a group steps members of the same step parity only"):
        group.tick(values[:, 62], encoder=enc)
    assert [m.engine.steps for m in group.models] == [62, 61]
    x = encoded_rows(enc, values[1, 61])
    group.models[1].process(x)
    twins[1].process(x)
    for n in range(62, 70):
        _check_tick(group.tick(values[:, n], encoder=enc, predicted_input=True), twins, values[:, n], enc, votes=True, what=f"tick {n}")
    # a member's own decoding rows stay set across a tick: its next recorded run writes them
    m, t = group.models[1], twins[1]
    eng = m.engine
    own = eng.device_buffer(4 * size[0] * 2)
    eng.set_run_predicted_input(own)
    try:
        _check_tick(group.tick(values[:, 70], encoder=enc), twins, values[:, 70], enc, what="with rows set")
        rec = m.run(values[1, 71:73], 2, encoder=enc, record=COUNTERS)
        got = eng.read_words(own, 2 * size[0], np.int32).reshape(2, size[0])
    finally:
        eng.set_run_predicted_input(None)
        eng.lib.hipFree(own)
    want = t.run(values[1, 71:73], 2, encoder=enc, record=COUNTERS + ("predicted_input",))
    assert np.array_equal(got, want.predicted_input) and int(got.max()) > 0
    assert np.array_equal(rec.bursting_columns, want.bursting_columns) and np.array_equal(rec.segments, want.segments)
    group.models[0].run(values[0, 71:73], 2, encoder=enc)
    twins[0].run(values[0, 71:73], 2, encoder=enc)
    _check_tick(group.tick(values[:, 73], encoder=enc), twins, values[:, 73], enc, what="last tick")
    for i, (a, b) in enumerate(zip(group.models, twins)):
        _same_state(a, b, f"member {i}")


@pytest.mark.gpu
@pytest.mark.parametrize("env", EAGER, ids=EAGER_IDS)
def test_an_overflow_is_raised_in_its_tick_with_the_finished_tick(env, monkeypatch):
    """Fixed pools of 64 rows; member 0 sees one repeated row, member 1 random rows: CapacityError in the tick that overflowed,
    its .tick holding every member's finished row and the flags each twin's info() reports after the same step."""
    _setenv(env, monkeypatch)
    from bithtm_amd.engine import CapacityError
    size = MID
    group, twins, _ = _group(size, 2, capacity=64)
    X = _banks(2, 12, size[0], 14)
    X[0, :] = X[0, 0]
    err = None
    for n in range(12):
        try:
            tick = group.tick(X[:, n])
        except CapacityError as e:
            tick, err = e.tick, e
        recs = []
        for i, t in enumerate(twins):
            try:
                recs.append(t.run(X[i, n][None, :], 1, record=COUNTERS))
            except CapacityError:
                recs.append(None)
        flags = [t.engine.info().capacity_error for t in twins]
        assert tick.capacity_error.tolist() == flags, (n, tick.capacity_error, flags)
        assert (err is not None) == any(flags), (n, flags)
        for i, rec in enumerate(recs):
            if rec is not None:
                _same_row(tick, i, rec, twins[i], f"tick {n} member {i}")
        if err is not None:
            break
    assert err is not None and flags[1] != 0 and flags[0] == 0, flags
    assert recs[0] is not None and "member 1" in str(err) and "member 0" not in str(err)


def _tick_launches(B):
    """{launch name: launches} of one warm tick of a group of B, profiled on member 0 (the handle the group's launches count on)."""
    size = MID
    enc = encoder_for(size)
    group, _, _ = _group(size, B)
    values = periodic_values(enc, B, 4, 53)
    flags = np.zeros(B, bool)
    flags[0] = True
    group.tick(values[:, 0], encoder=enc)
    eng = group.models[0].engine
    eng.profile(True)
    try:
        group.tick(values[:, 1], encoder=enc, resets=flags, predicted_input=True)
        eng.sync()
        return {name: int(n) for name, (_, n) in eng.profile_read().items()}
    finally:
        eng.profile(False)


@pytest.mark.gpu
def test_the_launch_list_of_a_tick_does_not_depend_on_b():
    one, five = _tick_launches(1), _tick_launches(5)
    assert one == five, (one, five)
    assert one["live:reset"] == 1 and one["live:encode"] == 1 and one["live:finish"] == 1, one
    assert sum(one.values()) <= 20, one


@pytest.mark.gpu
def test_one_member_against_the_oracle():
    """Member 1 of 3 against the NumPy oracle, driven with encoder.encode(values) and stepped with the empty previous state where
    the tick resets it: 60 ticks -- the active columns, the bursting count and the oracle's column predictions (as votes through
    its connected mask, decoded with encoder.decode) at every tick, the whole store at the end."""
    import bithtm_amd as Bm
    from types import SimpleNamespace
    from bithtm_amd import _lib as L
    from hip_impl import compare_store_with_oracle, make_htm
    from oracle import HTMOracle, SPParams
    I, Cn, K, k, train, ticks = 300, 1024, 16, 32, 150, 60
    enc = encoder_for(MID)
    np.random.seed(9)
    ora = HTMOracle(I, Cn, K, active_columns=k, seed=9, permanence=np.random.randn(Cn, I) * 0.1)
    htm = make_htm(I, Cn, K, k, 9, ora.spatial_pooler.permanence.copy())
    others = [make_htm(I, Cn, K, k, s, np.random.RandomState(s).randn(Cn, I) * 0.1) for s in (4, 5)]
    group = Bm.ModelGroup([others[0], htm, others[1]])
    values = stream_values(enc, 3, train, ticks, 59)
    group.run(values[:, :train], train, encoder=enc)                 # (something learned before the ticks: the oracle alike)
    for row in encoded_rows(enc, values[1, :train]):
        ora.step(row)
    values = values[:, train:]
    resets = np.zeros((ticks, 3), bool)
    resets[[0, 17, 18, 40], 1] = True
    resets[[5, 17], 0] = True
    empty = SimpleNamespace(cell_prediction=np.zeros((Cn, K), bool), cell_activation=np.zeros((Cn, K), bool), winner_cell=None, distal_state=None)
    threshold = SPParams().permanence_threshold
    scored = 0
    for n in range(ticks):
        tick = group.tick(values[:, n], encoder=enc, resets=resets[n] if resets[n].any() else None, predicted_input=True)
        o_sp = ora.spatial_pooler.step(encoded_rows(enc, values[1, n]))
        o_tm = ora.temporal_memory.step(o_sp.active_column, prev_state=empty if resets[n, 1] else None)
        cols = htm.engine.read(L.F_ACTIVE_COLUMN, np.int32, k)
        assert np.array_equal(cols, o_sp.active_column), n
        assert tick.bursting_columns[1] == int(o_tm.active_column_bursting.sum()), n
        pred = o_tm.cell_prediction.any(axis=1)
        assert tick.predicted_columns[1] == int(pred.sum()), n
        votes = (ora.spatial_pooler.permanence[pred] >= threshold).sum(axis=0).astype(np.int32)
        assert np.array_equal(tick.predicted_input[1], votes), n
        bucket, score, value = decoded(enc, votes)
        assert np.array_equal(tick.predicted_bucket[1], bucket) and np.array_equal(tick.predicted_score[1], score), n
        assert np.array_equal(tick.predicted_value[1], value, equal_nan=True), n
        correct, _, anomaly = derived(k, int(o_tm.active_column_bursting.sum()), 0)
        assert tick.correct_columns[1] == correct and tick.anomaly_score[1] == anomaly, n
        scored += int((score > 0).any())
    assert scored > 0
    compare_store_with_oracle(train + ticks - 1, ora, htm)
