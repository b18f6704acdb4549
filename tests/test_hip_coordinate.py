"""Coordinate fields on the device (CoordinateField in a ScalarEncoder: kcoord_bank, kcoord_votes, kcoord_finish of bithtm_amd/csrc/
htm_coord.h).  The NumPy definition (bithtm_amd/encoders.py) is the only yardstick and every comparison is
exact: the kernels alone on the cases of tests/coordinate_cases.py, then every door that takes an encoder -- run(encoder=) with
records, noise and resets, a view, lookahead, forecast_values, group runs, live ticks with resets, a likelihood and a classifier
bank -- against the same call over host-encoded rows.  Models are 256 columns of 4 cells."""
import ctypes as C

import numpy as np
import pytest

import coordinate_cases as cases
from test_hip_input_noise import _peek, _poke, _pack, _same_record, _same_state, _sp_engine
from test_hip_run_record import ALL
from test_hip_scalar_encoder import LAYOUTS, _decode_on_device, _same_decoded, _special_values

I, COLUMNS, CELLS, ACTIVE = 300, 256, 4, 24
WITH_VOTES = ALL + ("predicted_input",)
COORD_COLUMNS = [1, 2, 3]                           # of cases.track_encoder(): column 0 is the linear speed field


# ---- the kernels alone (a 64-column stand-alone Spatial Pooler engine: they read no state)

@pytest.mark.gpu
@pytest.mark.parametrize("name", list(cases.CASES))
def test_bank_encode_equals_the_definition(name):
    """Engine.bank_encode + a raw read == the packed encoder.encode(values), word for word, pad bits 0, for the windows (first_row,
    n_rows) = whole bank, (1, 2), (last, 1), (2, 0): the bank starts as all-ones sentinel words, pad words included, and every row
    outside the window keeps them."""
    enc = cases.encoder(name)
    eng = _sp_engine(enc.input_dim)
    W = eng.words
    values = cases.values(name)
    R = len(values)
    assert 3 <= R <= 64
    want_rows = _pack(enc.encode(values), W)
    d_values, d_bank = eng.upload_values(values), eng.zero_bank(R)
    sentinel = np.full((R, W), 0xFFFFFFFF, np.uint32)
    for first, n in ((0, R), (1, 2), (R - 1, 1), (2, 0)):
        _poke(eng, d_bank, sentinel)
        eng.bank_encode(enc, d_values, n, d_bank, R, first)
        got = _peek(eng, d_bank, R * W).reshape(R, W)
        want = sentinel.copy()
        want[first:first + n] = want_rows[:n]
        assert np.array_equal(got, want), (first, n, np.flatnonzero((got != want).any(axis=1)).tolist())
    eng.sync()
    eng.lib.hipFree(C.c_void_p(d_values))


@pytest.mark.gpu
def test_decode_votes_gives_nothing_for_the_coordinate_columns_and_the_other_fields_unchanged():
    """The mixed case's table: votes rows of zeros, ones, counts and random ones.  The coordinate group's three columns decode to
    (-1, 0) whatever the votes of the field's bits; the linear, hashed and category columns are the definition's, and are those of
    the same fields in a table without the coordinate field (which launches the older twins)."""
    from bithtm_amd import ScalarEncoder
    enc = cases.encoder("linear + hashed + category + coordinate")
    without = ScalarEncoder([f for f in enc.fields[:3]], enc.input_dim)
    eng = _sp_engine(enc.input_dim)
    rng = np.random.RandomState(7)
    votes = np.concatenate([np.zeros((1, 600), np.int64), np.ones((1, 600), np.int64), rng.randint(0, 2048, (3, 600)), rng.randint(0, 2, (3, 600))])
    want_b, want_s = enc.decode(votes)
    got_b, got_s = _decode_on_device(eng, enc, votes)
    assert np.array_equal(got_b, want_b) and np.array_equal(got_s, want_s), (got_b.tolist(), want_b.tolist())
    assert (got_b[:, 3:6] == -1).all() and not got_s[:, 3:6].any() and (got_b[1:, [0, 1, 2, 6]] >= 0).all()
    old_b, old_s = _decode_on_device(eng, without, votes)
    assert np.array_equal(old_b, got_b[:, :3]) and np.array_equal(old_s, got_s[:, :3])


@pytest.mark.gpu
def test_a_linear_table_beside_an_unused_coordinate_field_gives_what_it_gave():
    """Layout A of tests/test_hip_scalar_encoder.py (input_dim 300) with a coordinate field in its four trailing bits whose radius is
    always missing: the rows and the decoded pairs of the three linear fields are those of the linear table alone (which launches
    the older kernels), and the coordinate field sets and decodes nothing."""
    from bithtm_amd import CoordinateField, ScalarEncoder, ScalarField
    linear = ScalarEncoder([ScalarField(*f) for f in LAYOUTS[300][0]], 300)
    beside = ScalarEncoder(list(linear.fields) + [CoordinateField(4, 2, 3, seed=4)], 300)
    eng = _sp_engine(300)
    values = _special_values(linear, 6, 300)
    R = len(values)
    more = np.concatenate([values, np.full((R, 1), 5.0), np.full((R, 1), -5.0), np.full((R, 1), np.nan)], axis=1)
    d_values, d_more, d_bank, d_bank2 = eng.upload_values(values), eng.upload_values(more), eng.zero_bank(R), eng.zero_bank(R)
    eng.bank_encode(linear, d_values, R, d_bank, R)
    eng.bank_encode(beside, d_more, R, d_bank2, R)
    a, b = _peek(eng, d_bank, R * eng.words), _peek(eng, d_bank2, R * eng.words)
    assert np.array_equal(a, b) and np.array_equal(a.reshape(R, -1), _pack(linear.encode(values), eng.words))
    votes = np.random.RandomState(4).randint(0, 50, (6, 300))
    lb, ls = _decode_on_device(eng, linear, votes)
    mb, ms = _decode_on_device(eng, beside, votes)
    assert np.array_equal(mb[:, :3], lb) and np.array_equal(ms[:, :3], ls) and (mb[:, 3:] == -1).all() and not ms[:, 3:].any()
    assert np.array_equal(lb, linear.decode(votes)[0])
    for ptr in (d_values, d_more):
        eng.lib.hipFree(C.c_void_p(ptr))


# ---- model paths, against a twin stepped over the host-encoded rows

def _twins(seed=5):
    import bithtm_amd as B
    out = []
    for _ in range(2):
        np.random.seed(seed)                        # (the SP's permanences are drawn from NumPy's global stream)
        out.append(B.HierarchicalTemporalMemory(I, COLUMNS, CELLS, seed=seed, active_columns=ACTIVE))
    return out


def _no_coordinate_decode(bucket, score, value):
    assert (bucket[..., COORD_COLUMNS] == -1).all() and not score[..., COORD_COLUMNS].any() and np.isnan(value[..., COORD_COLUMNS]).all()


@pytest.fixture(scope="module")
def trained():
    """(encoder, the loop's values, a model run over them through the encoder, its twin run over the host-encoded rows)."""
    enc = cases.track_encoder(I)
    values = cases.track_values(6, 5, every=7)      # (the plain loop: nothing missing)
    htm, twin = _twins()
    htm.run(values, 150, encoder=enc)
    twin.run(enc.encode(values), 150)
    return enc, values, htm, twin


@pytest.mark.gpu
def test_predicted_value_of_a_trained_model(trained):
    enc, values, htm, twin = trained
    value, score = htm.predicted_value(enc)
    bucket, want = enc.decode(twin.predicted_input())
    assert np.array_equal(score, want) and np.array_equal(value, enc.value_of(bucket), equal_nan=True)
    assert score[0] > 0 and not np.isnan(value[0])                  # (the speed field predicts something by now)
    _no_coordinate_decode(bucket, score, value)
    assert np.array_equal(htm.predicted_input(), twin.predicted_input())
    _same_state(htm, twin)


@pytest.mark.gpu
def test_run_over_coordinate_values_equals_the_run_over_the_host_encoded_bank():
    """record=("counters", "predicted_value", "predicted_input"): the counters of the twin's run over encoder.encode(values), the
    recorded votes its votes, bucket and score their NumPy decode, the value value_of; then with noise= and resets=, continuing,
    and with a likelihood."""
    import bithtm_amd as B
    enc = cases.track_encoder(I)
    values = cases.track_values(12, 1)
    rows = enc.encode(values)
    assert (enc.bucket(values) == -1).any() and rows[:, 60:].any()
    htm, twin = _twins()
    resets = np.zeros(12, bool)
    resets[[0, 7]] = True
    params = dict(learning_period=5, estimation_samples=3, history=16, averaging_window=4, reestimation_period=7)
    lk, lk_twin = B.AnomalyLikelihood(1, **params), B.AnomalyLikelihood(1, **params)
    for n, kw in ((120, {}), (40, dict(noise=0.05, noise_seed=9, resets=resets)), (15, dict(continuing=True)), (20, dict(likelihood=True))):
        if kw.pop("likelihood", False):
            got = htm.run(values, n, record=("counters", "predicted_value", "predicted_input"), encoder=enc, likelihood=lk, **kw)
            want = twin.run(rows, n, record=("counters", "predicted_input"), likelihood=lk_twin, **kw)
            assert np.array_equal(got.anomaly_likelihood.view(np.uint64), want.anomaly_likelihood.view(np.uint64))
        else:
            got = htm.run(values, n, record=("counters", "predicted_value", "predicted_input"), encoder=enc, **kw)
            want = twin.run(rows, n, record=("counters", "predicted_input"), **kw)
        assert np.array_equal(got.step_index, want.step_index)
        for name in ("active_columns", "bursting_columns", "predicted_columns", "segments"):
            assert np.array_equal(getattr(got, name), getattr(want, name)), (n, name)
        assert np.array_equal(got.predicted_input, want.predicted_input), n
        _same_decoded(got, enc, want.predicted_input, f"{n} steps")
        _no_coordinate_decode(got.predicted_bucket, got.predicted_score, got.predicted_value)
    assert got.predicted_score.max() > 0
    _same_state(htm, twin)


@pytest.mark.gpu
def test_forecast_values_and_lookahead_and_a_view(trained):
    enc, values, htm, twin = trained
    rows = enc.encode(values)
    votes0 = twin.predicted_input()
    _, rec = twin.forecast(5, record=("predicted_input",))
    value, score = htm.forecast_values(5, enc)
    bucket, want = enc.decode(np.concatenate([votes0[None], rec.predicted_input[:-1]]))
    assert np.array_equal(score, want) and np.array_equal(value, enc.value_of(bucket), equal_nan=True) and score[0, 0] > 0
    _no_coordinate_decode(bucket, score, value)
    got_rows, got = htm.lookahead(values, 8, 3, every=2, record=("counters", "predicted_value"), encoder=enc)
    want_rows, want = twin.lookahead(rows, 8, 3, every=2, record=("counters", "predicted_input"))
    assert np.array_equal(got_rows, want_rows) and np.array_equal(got.bursting_columns, want.bursting_columns)
    _same_decoded(got, enc, want.predicted_input, "lookahead")
    view, copy = htm.inference_view(), twin.inference_view()
    got = view.run(values, 12, record=ALL + ("predicted_value",), encoder=enc)
    want = copy.run(rows, 12, record=WITH_VOTES)
    _same_record(got, want, "view")
    _same_decoded(got, enc, want.predicted_input, "view")
    _same_state(htm, twin)


@pytest.mark.gpu
def test_group_run_over_coordinate_values():
    from bithtm_amd import ModelGroup
    enc = cases.track_encoder(I)
    values = cases.track_values(12, 21, B=2)
    np.random.seed(5)
    group = ModelGroup.create(2, I, COLUMNS, CELLS, seeds=[4, 5], active_columns=ACTIVE)
    np.random.seed(5)
    alone = ModelGroup.create(2, I, COLUMNS, CELLS, seeds=[4, 5], active_columns=ACTIVE).models
    recs = group.run(values, 120, record=ALL + ("predicted_value",), encoder=enc)
    for i, (m, rec) in enumerate(zip(alone, recs)):
        want = m.run(enc.encode(values[i]), 120, record=WITH_VOTES)
        _same_record(rec, want, f"member {i}")
        _same_decoded(rec, enc, want.predicted_input, f"member {i}")
        _same_state(group.models[i], m, f"member {i}")
    value, score = group.predicted_value(enc)
    for i, m in enumerate(alone):
        bucket, want = enc.decode(m.predicted_input())
        assert np.array_equal(score[i], want) and np.array_equal(value[i], enc.value_of(bucket), equal_nan=True), i
    assert score[:, 0].max() > 0


# ---- live ticks: member by member reset() plus a one-step recorded run() over the host-encoded row

def _tick_group(B):
    import bithtm_amd as Bm
    models, twins = [], []
    for i in range(B):
        for out in (models, twins):
            np.random.seed(11 + 7 * i)
            out.append(Bm.HierarchicalTemporalMemory(I, COLUMNS, CELLS, seed=11 + 7 * i, active_columns=ACTIVE))
    return Bm.ModelGroup(models), twins


def _check_tick(tick, twins, row_values, enc, resets=None, likelihoods=None, what=""):
    from bithtm_amd.engine import RECORD_COUNTERS
    for i, t in enumerate(twins):
        if resets is not None and resets[i]:
            t.reset()
        kw = {} if likelihoods is None else dict(likelihood=likelihoods[i])
        rec = t.run(enc.encode(row_values[i])[None, :], 1, record=("counters", "predicted_input"), **kw)
        assert tick.step_index[i] == rec.step_index[0], (what, i)
        for name in RECORD_COUNTERS:
            assert getattr(tick, name)[i] == getattr(rec, name)[0], (what, i, name)
        bucket, score = enc.decode(rec.predicted_input[0])
        assert np.array_equal(tick.predicted_bucket[i], bucket), (what, i, tick.predicted_bucket[i].tolist(), bucket.tolist())
        assert np.array_equal(tick.predicted_score[i], score), (what, i)
        assert np.array_equal(tick.predicted_value[i], enc.value_of(bucket), equal_nan=True), (what, i)
        if tick.predicted_input is not None:
            assert np.array_equal(tick.predicted_input[i], rec.predicted_input[0]), (what, i)
        if likelihoods is not None:
            assert np.float64(tick.anomaly_likelihood[i]).view(np.uint64) == np.float64(rec.anomaly_likelihood[0]).view(np.uint64), (what, i)
    _no_coordinate_decode(tick.predicted_bucket, tick.predicted_score, tick.predicted_value)


@pytest.mark.gpu
@pytest.mark.parametrize("B", [1, 3])
def test_ticks_with_a_coordinate_encoder_equal_the_definition(B):
    """Trained over 120 rows, then 20 ticks with missing values among them, every third with per-member resets and with the votes."""
    enc = cases.track_encoder(I)
    group, twins = _tick_group(B)
    values = cases.track_values(12, 31, B=B)
    group.run(values, 120, encoder=enc)
    for i, t in enumerate(twins):
        t.run(enc.encode(values[i]), 120)
    live = cases.track_values(20, 31, B=B, every=4)
    seen = 0
    for n in range(20):
        resets = (np.arange(B) + n) % 3 == 0 if n % 3 == 2 else None
        tick = group.tick(live[:, n], encoder=enc, resets=resets, predicted_input=n % 3 == 2)
        _check_tick(tick, twins, live[:, n], enc, resets, what=f"tick {n}")
        seen += int((tick.predicted_score > 0).sum())
    assert seen > 0
    for i, (m, t) in enumerate(zip(group.models, twins)):
        _same_state(m, t, f"member {i}")


@pytest.mark.gpu
def test_scored_ticks_and_a_linear_tick_behind_a_coordinate_one():
    import bithtm_amd as Bm
    B = 3
    params = dict(learning_period=5, estimation_samples=3, history=16, averaging_window=4, reestimation_period=7)
    enc = cases.track_encoder(I)
    linear = Bm.ScalarEncoder([Bm.ScalarField(0.0, 30.0, 60, 9), Bm.ScalarField(-1.0, 1.0, 200, 21, periodic=True)], I)
    group, twins = _tick_group(B)
    lk, solo = Bm.AnomalyLikelihood(B, **params), [Bm.AnomalyLikelihood(1, **params) for _ in range(B)]
    values = cases.track_values(12, 3, B=B)
    group.run(values, 120, encoder=enc)             # (trained: the bursting counts of the ticks below vary, and so do the likelihoods)
    for i, t in enumerate(twins):
        t.run(enc.encode(values[i]), 120)
    live = cases.track_values(24, 3, B=B, every=4)
    moved = False
    for n in range(24):
        tick = group.tick(live[:, n], encoder=enc, likelihood=lk)
        _check_tick(tick, twins, live[:, n], enc, likelihoods=solo, what=f"scored tick {n}")
        moved |= bool((tick.anomaly_likelihood != 0.5).any())
    assert moved
    # a linear encoder right behind a coordinate tick, and a coordinate one behind that, on the same group
    other = np.random.RandomState(8).uniform(-1, 31, (B, 4, 2))
    for n in range(4):
        e, rows = (linear, other[:, n]) if n % 2 == 0 else (enc, live[:, n])
        tick = group.tick(rows, encoder=e)
        if e is linear:
            for i, t in enumerate(twins):
                rec = t.run(e.encode(rows[i])[None, :], 1, record=("counters", "predicted_input"))
                bucket, score = e.decode(rec.predicted_input[0])
                assert np.array_equal(tick.predicted_bucket[i], bucket) and np.array_equal(tick.predicted_score[i], score), (n, i)
        else:
            _check_tick(tick, twins, rows, e, what=f"alternating tick {n}")
    for i, (m, t) in enumerate(zip(group.models, twins)):
        _same_state(m, t, f"member {i}")


@pytest.mark.gpu
def test_ticks_with_a_classifier_bank_on_the_linear_field_of_the_same_table():
    """The bank's field is the speed column of the track encoder; its targets come from encoder.bucket on the host.  The ticks'
    classifications and the bank's state are those of the members stepped alone over host-encoded rows with those targets; a
    classifier on the coordinate field or one of its axes is refused."""
    import bithtm_amd as Bm
    B, ticks = 3, 30
    enc = cases.track_encoder(I)
    group, twins = _tick_group(B)
    bank = Bm.SDRClassifierBank(B, field=enc.fields[0], steps=(1, 2))
    clfs = [Bm.SDRClassifier(field=enc.fields[0], steps=(1, 2)) for _ in range(B)]
    live = cases.track_values(ticks, 13, B=B, every=6)
    for n in range(ticks):
        tick = group.tick(live[:, n], encoder=enc, classifier=bank, class_distribution=True)
        for i, t in enumerate(twins):
            want = t.run(enc.encode(live[i, n])[None, :], 1, classifier=clfs[i], targets=enc.bucket(live[i, n][None])[:, 0],
                         record=("counters", "class_distribution"))
            assert tick.classified_bucket[i].tolist() == want.classified_bucket[0].tolist(), (n, i)
            assert np.array_equal(tick.classified_probability[i], want.classified_probability[0]), (n, i)
            assert np.array_equal(tick.class_distribution[i], want.class_distribution[0]), (n, i)
            assert tick.active_cells[i] == want.active_cells[0] and tick.step_index[i] == want.step_index[0]
    state = bank.state_dict()
    assert int(state["total"]) == ticks and state["weights"].any()
    for i, (m, t) in enumerate(zip(group.models, twins)):
        _same_state(m, t, f"member {i}")
    for j in COORD_COLUMNS:
        with pytest.raises(ValueError, match="coordinate"):
            Bm.SDRClassifierBank(B, field=enc.fields[j])
        with pytest.raises(ValueError, match="coordinate"):
            Bm.SDRClassifier(field=enc.fields[j])
