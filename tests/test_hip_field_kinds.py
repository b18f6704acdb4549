"""Field kinds on the device (CategoryField and HashedField beside linear fields in one ScalarEncoder: kenc_bank, kenc_votes,
kenc_finish of bithtm_amd/csrc/htm_fields.h).  The NumPy definition (bithtm_amd/encoders.py) is the only
yardstick and every comparison is exact: the kernels alone on the cases of tests/field_kind_cases.py, then every path that takes
an encoder -- predicted_value, run(encoder=) with records, noise and resets, forecast_values, lookahead, group runs, live ticks
with resets and a likelihood -- against the same call over host-encoded rows, its recorded votes decoded in NumPy."""
import ctypes as C

import numpy as np
import pytest

import field_kind_cases as cases
from live_tick_cases import MID, periodic_values, with_edges
from test_hip_input_noise import _peek, _poke, _pack, _same_record, _same_state, _sp_engine
from test_hip_run_record import ALL, _twins
from test_hip_scalar_encoder import LAYOUTS, SHAPE, _decode_on_device, _same_decoded, _special_values

WITH_VOTES = ALL + ("predicted_input",)


# ---- the kernels alone (a 64-column stand-alone Spatial Pooler engine: they read no state)

@pytest.mark.gpu
@pytest.mark.parametrize("name", list(cases.CASES))
def test_bank_encode_equals_the_definition(name):
    """Engine.bank_encode + a raw read == the packed encoder.encode(values), pad bits 0, for the windows (first_row, n_rows) =
    whole bank, (3, 4), (last, 1), (2, 0): the bank starts as all-ones sentinel words, pad words included, and every row outside
    the window keeps them."""
    enc = cases.encoder(name)
    eng = _sp_engine(enc.input_dim)
    W = eng.words
    values = cases.values(enc, 8, 3)
    R = len(values)
    want_rows = _pack(enc.encode(values), W)
    d_values, d_bank = eng.upload_values(values), eng.zero_bank(R)
    sentinel = np.full((R, W), 0xFFFFFFFF, np.uint32)
    for first, n in ((0, R), (3, 4), (R - 1, 1), (2, 0)):
        _poke(eng, d_bank, sentinel)
        eng.bank_encode(enc, d_values, n, d_bank, R, first)
        got = _peek(eng, d_bank, R * W).reshape(R, W)
        want = sentinel.copy()
        want[first:first + n] = want_rows[:n]
        assert np.array_equal(got, want), (first, n, np.flatnonzero((got != want).any(axis=1)).tolist())
    eng.sync()
    eng.lib.hipFree(C.c_void_p(d_values))


@pytest.mark.gpu
@pytest.mark.parametrize("name", cases.DECODED)
def test_decode_votes_equals_the_definition(name):
    """The vote rows of tests/field_kind_cases.py -- zeros, ties, counts up to column_dim, a hot bit a hashed window hits twice --
    and random ones; cap-8200 holds the hashed field of exactly 8 192 positions."""
    enc = cases.encoder(name)
    eng = _sp_engine(enc.input_dim)
    rng = np.random.RandomState(7)
    votes = np.concatenate([cases.vote_rows(enc, 2048, 5), rng.randint(0, 9, (3, enc.input_dim)), rng.randint(0, 2, (2, enc.input_dim))])
    want_b, want_s = enc.decode(votes)
    got_b, got_s = _decode_on_device(eng, enc, votes)
    assert np.array_equal(got_b, want_b), np.argwhere(got_b != want_b).tolist()[:8]
    assert np.array_equal(got_s, want_s), np.argwhere(got_s != want_s).tolist()[:8]


@pytest.mark.gpu
def test_one_bucket_above_the_cap_is_refused_by_the_decode_and_taken_by_the_encode():
    from bithtm_amd import HashedField, HtmError, ScalarEncoder
    enc = ScalarEncoder([HashedField(0, 1, 5000, 64, buckets=8130, seed=2)], 8200)
    eng = _sp_engine(8200)
    values = np.array([[0.0], [1.0], [0.37], [np.nan]])
    d_values, d_bank = eng.upload_values(values), eng.zero_bank(4)
    eng.bank_encode(enc, d_values, 4, d_bank, 4)
    assert np.array_equal(eng.read_bank(d_bank, 4), enc.encode(values))
    d_votes = eng.device_buffer(8200 * 4, np.zeros(8200, np.int32))
    with pytest.raises(HtmError, match=r"\(-1\).*8192"):
        eng.decode_votes(enc, d_votes, 1, d_bank)
    for ptr in (d_values, d_votes):
        eng.lib.hipFree(C.c_void_p(ptr))


@pytest.mark.gpu
def test_a_linear_table_beside_an_unused_hashed_field_gives_what_it_gave():
    """Layout A of tests/test_hip_scalar_encoder.py (input_dim 300) with a hashed field in its four trailing bits whose value is
    always missing: the rows and the decoded pairs of the three linear fields are those of the linear table alone (which launches
    the older kernels), and the hashed field sets and decodes nothing."""
    from bithtm_amd import HashedField, ScalarEncoder, ScalarField
    linear = ScalarEncoder([ScalarField(*f) for f in LAYOUTS[300][0]], 300)
    beside = ScalarEncoder(list(linear.fields) + [HashedField(0, 1, 4, 2, buckets=9, seed=4)], 300)
    eng = _sp_engine(300)
    values = _special_values(linear, 6, 300)
    R = len(values)
    more = np.concatenate([values, np.full((R, 1), np.nan)], axis=1)
    d_values, d_more, d_bank, d_bank2 = eng.upload_values(values), eng.upload_values(more), eng.zero_bank(R), eng.zero_bank(R)
    eng.bank_encode(linear, d_values, R, d_bank, R)
    eng.bank_encode(beside, d_more, R, d_bank2, R)
    a, b = _peek(eng, d_bank, R * eng.words), _peek(eng, d_bank2, R * eng.words)
    assert np.array_equal(a, b) and np.array_equal(a.reshape(R, -1), _pack(linear.encode(values), eng.words))
    votes = np.random.RandomState(4).randint(0, 50, (6, 300))
    votes[:, 296:] = 0
    lb, ls = _decode_on_device(eng, linear, votes)
    mb, ms = _decode_on_device(eng, beside, votes)
    assert np.array_equal(mb[:, :3], lb) and np.array_equal(ms[:, :3], ls) and (mb[:, 3] == -1).all() and not ms[:, 3].any()
    assert np.array_equal(lb, linear.decode(votes)[0])
    for ptr in (d_values, d_more):
        eng.lib.hipFree(C.c_void_p(ptr))


# ---- model paths, against a twin stepped over the host-encoded rows

def _values(enc, n, seed, B=None):
    """n rows of a periodic sequence (something to learn) with the edge values of tests/live_tick_cases.py among them."""
    v = with_edges(periodic_values(enc, B or 1, n, seed, period=6), enc, every=5)
    return v if B else v[0]


def _trained(steps=150):
    I, Cn, K, k = SHAPE
    enc = cases.encoder("mixed-300")
    values = periodic_values(enc, 1, 6, 5, period=6)[0]
    htm, twin = _twins(I, Cn, K, active_columns=k)
    htm.run(values, steps, encoder=enc)
    twin.run(enc.encode(values), steps)
    return enc, values, htm, twin


@pytest.mark.gpu
def test_predicted_value_of_a_trained_model():
    enc, values, htm, twin = _trained()
    value, score = htm.predicted_value(enc)
    bucket, want = enc.decode(twin.predicted_input())
    assert np.array_equal(score, want) and np.array_equal(value, enc.value_of(bucket), equal_nan=True)
    assert score.min() > 0 and not np.isnan(value).any()            # (every kind predicts something by now)
    assert np.array_equal(htm.predicted_input(), twin.predicted_input())
    _same_state(htm, twin)


@pytest.mark.gpu
def test_run_over_mixed_values_equals_the_run_over_the_host_encoded_bank():
    """record=("counters", "predicted_value", "predicted_input"): the counters of the twin's run over encoder.encode(values), the
    recorded votes its votes, bucket and score their NumPy decode, the value value_of; then once with noise= and resets=, and a
    streamed call with a likelihood."""
    import bithtm_amd as B
    I, Cn, K, k = SHAPE
    enc = cases.encoder("mixed-300")
    values = _values(enc, 12, 1)
    rows = enc.encode(values)
    assert (enc.bucket(values) == -1).any()
    htm, twin = _twins(I, Cn, K, active_columns=k)
    resets = np.zeros(12, bool)
    resets[[0, 7]] = True
    lk, lk_twin = B.AnomalyLikelihood(1, learning_period=5, estimation_samples=3, history=16, averaging_window=4, reestimation_period=7), \
        B.AnomalyLikelihood(1, learning_period=5, estimation_samples=3, history=16, averaging_window=4, reestimation_period=7)
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
    assert got.predicted_score.max() > 0
    _same_state(htm, twin)


@pytest.mark.gpu
def test_forecast_values_and_lookahead_and_a_view():
    enc, values, htm, twin = _trained()
    rows = enc.encode(values)
    votes0 = twin.predicted_input()
    _, rec = twin.forecast(5, record=("predicted_input",))
    value, score = htm.forecast_values(5, enc)
    bucket, want = enc.decode(np.concatenate([votes0[None], rec.predicted_input[:-1]]))
    assert np.array_equal(score, want) and np.array_equal(value, enc.value_of(bucket), equal_nan=True) and score[0].min() > 0
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
def test_group_run_predicted_value_and_forecast_values():
    from bithtm_amd import ModelGroup
    I, Cn, K, k = SHAPE
    enc = cases.encoder("mixed-300")
    values = _values(enc, 12, 21, B=2)
    np.random.seed(5)
    group = ModelGroup.create(2, I, Cn, K, seeds=[4, 5], active_columns=k)
    np.random.seed(5)
    alone = ModelGroup.create(2, I, Cn, K, seeds=[4, 5], active_columns=k).models
    recs = group.run(values, 120, record=ALL + ("predicted_value",), encoder=enc)
    for i, (m, rec) in enumerate(zip(alone, recs)):
        want = m.run(enc.encode(values[i]), 120, record=WITH_VOTES)
        _same_record(rec, want, f"member {i}")
        _same_decoded(rec, enc, want.predicted_input, f"member {i}")
    value, score = group.predicted_value(enc)
    for i, m in enumerate(alone):
        bucket, want = enc.decode(m.predicted_input())
        assert np.array_equal(score[i], want) and np.array_equal(value[i], enc.value_of(bucket), equal_nan=True), i
    assert score.max() > 0
    value, score = group.forecast_values(3, enc)
    for i, m in enumerate(alone):
        votes0 = m.predicted_input()
        _, rec = m.forecast(3, record=("predicted_input",))
        bucket, want = enc.decode(np.concatenate([votes0[None], rec.predicted_input[:-1]]))
        assert np.array_equal(score[i], want) and np.array_equal(value[i], enc.value_of(bucket), equal_nan=True), i
        _same_state(group.models[i], m, f"member {i}")


# ---- live ticks: member by member reset() plus a one-step recorded run() over the host-encoded row

def _tick_group(B):
    from test_hip_live_tick import _group
    return _group(MID, B)[:2]


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


@pytest.mark.gpu
@pytest.mark.parametrize("B", [1, 3])
def test_ticks_with_a_mixed_encoder_equal_the_definition(B):
    """Trained over 120 rows, then 20 ticks with edge values among them, every third with per-member resets and with the votes."""
    enc = cases.encoder("mixed-300")
    group, twins = _tick_group(B)
    values = _values(enc, 12, 31, B=B)
    group.run(values, 120, encoder=enc)
    for i, t in enumerate(twins):
        t.run(enc.encode(values[i]), 120)
    live = with_edges(periodic_values(enc, B, 20, 31, period=6), enc, every=4)
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
def test_scored_ticks_and_a_linear_tick_behind_a_mixed_one():
    import bithtm_amd as Bm
    from live_tick_cases import encoder_for
    B = 3
    params = dict(learning_period=5, estimation_samples=3, history=16, averaging_window=4, reestimation_period=7)
    enc, linear = cases.encoder("mixed-300"), encoder_for(MID)
    group, twins = _tick_group(B)
    lk, solo = Bm.AnomalyLikelihood(B, **params), [Bm.AnomalyLikelihood(1, **params) for _ in range(B)]
    values = _values(enc, 12, 3, B=B)
    group.run(values, 120, encoder=enc)             # (trained: the bursting counts of the ticks below vary, and so do the likelihoods)
    for i, t in enumerate(twins):
        t.run(enc.encode(values[i]), 120)
    live = with_edges(periodic_values(enc, B, 24, 3, period=6), enc, every=4)
    moved = False
    for n in range(24):
        tick = group.tick(live[:, n], encoder=enc, likelihood=lk)
        _check_tick(tick, twins, live[:, n], enc, likelihoods=solo, what=f"scored tick {n}")
        moved |= bool((tick.anomaly_likelihood != 0.5).any())
    assert moved
    # the linear encoder of the live-tick tests right behind a mixed tick, and a mixed one behind that, on the same group
    other = periodic_values(linear, B, 4, 8)
    for n in range(4):
        e, rows = (linear, other[:, n]) if n % 2 == 0 else (enc, live[:, n])
        tick = group.tick(rows, encoder=e)
        _check_tick(tick, twins, rows, e, what=f"alternating tick {n}")
    for i, (m, t) in enumerate(zip(group.models, twins)):
        _same_state(m, t, f"member {i}")
