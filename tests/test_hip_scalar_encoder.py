"""Scalar streams on the device (htm_bank_encode, htm_decode_votes, htm_predicted_value; run(encoder=), record "predicted_value",
predicted_value(), forecast_values()).  The NumPy definition (bithtm_amd/encoders.py) is the only
yardstick: the two kernels alone against it -- sentinel rows, pad bits, windows, special values, ties, wraps, the LDS cap -- and
every run over values against a twin stepped over encoder.encode(values), its recorded votes decoded in NumPy."""

import ctypes as C

import numpy as np
import pytest

from test_hip_input_noise import _peek, _poke, _pack, _same_record, _same_state, _sp_engine
from test_hip_run_record import ALL, SCHEDULES, SCHEDULE_IDS, _twins

SHAPE = (300, 1024, 8, 64)                          # the forecast and noise fixtures' small shape: input_dim, columns, cells, k
ERR_ARGUMENT = -1


def _encoder(fields, input_dim):
    from bithtm_amd import ScalarEncoder, ScalarField
    return ScalarEncoder([ScalarField(*f) for f in fields], input_dim)


def _layout_a():
    """Three fields at the unaligned offsets 0, 130 and 226, four trailing bits."""
    return _encoder([(0, 100, 130, 21), (0, 24, 96, 11, True), (-5, 5, 70, 1)], 300)


LAYOUTS = {70: [[(0, 1, 30, 30), (0, 24, 25, 4, True), (-5, 5, 15, 1)]],                     # fills the 70 bits; bits == width
           300: [[(0, 100, 130, 21), (0, 24, 96, 11, True), (-5, 5, 70, 1)]],
           1000: [[(0, 100, 400, 21), (0, 24, 330, 33, True), (-5, 5, 70, 1), (0, 1, 64, 64)]],
           1024: [[(0, 100, 500, 21), (0, 24, 300, 11, True), (-5, 5, 160, 1), (0, 1, 64, 64)],      # fills the row exactly
                  [(0, 100, 130, 21), (0, 24, 96, 11, True), (-5, 5, 70, 1)]],
           40000: [[(0, 100, 20000, 301), (0, 24, 19990, 777, True)]]}      # 313 stores per row: the block of four waves loops


def _special_values(enc, extra, seed):
    """Per field the table of special values (ten rows), then `extra` random rows over and beyond every range."""
    rng = np.random.RandomState(seed)
    cols = []
    for f in enc.fields:
        lo, hi = f.minimum, f.maximum
        table = [0.5 * (lo + hi), lo, hi, np.nextafter(lo, -np.inf), np.nan, np.inf, -np.inf, 1e300, lo - 1e-300 if lo else -1e-300,
                 hi + 3 * (hi - lo)]
        cols.append(np.concatenate([table, rng.uniform(lo - 0.2 * (hi - lo), hi + 0.2 * (hi - lo), extra)]))
    return np.ascontiguousarray(np.stack(cols, axis=1))


def _raw_table(rows):
    """An htm_scalar_field array from (minimum, scale, offset, bits, width, buckets, periodic) tuples, unchecked."""
    from bithtm_amd import _lib
    tab = (_lib.HtmScalarField * len(rows))()
    for t, (minimum, scale, offset, bits, width, buckets, periodic) in zip(tab, rows):
        t.minimum, t.scale, t.offset, t.bits, t.width, t.buckets, t.periodic = minimum, scale, offset, bits, width, buckets, periodic
    return tab


# ---- the kernels alone (a 64-column stand-alone Spatial Pooler engine: they read no state)

@pytest.mark.gpu
@pytest.mark.parametrize("I", [70, 300, 1000, 1024, 40000])
def test_bank_encode_equals_the_definition(I):
    """Engine.bank_encode + a raw read == the packed encoder.encode(values), pad bits 0, for the windows (first_row, n_rows) =
    whole bank, (3, 4), (last, 1), (2, 0): the bank starts as all-ones sentinel words, pad words included, and every row outside
    the window keeps them.  The values hold the special-value table of every field."""
    eng = _sp_engine(I)
    W = eng.words
    assert W % 4 == 0 and W * 32 >= I
    for li, fields in enumerate(LAYOUTS[I]):
        enc = _encoder(fields, I)
        values = _special_values(enc, 6, I + li)
        R = len(values)
        want_rows = _pack(enc.encode(values), W)
        assert (enc.bucket(values) == -1).any() and (enc.bucket(values) > 0).any()
        d_values, d_bank = eng.upload_values(values), eng.zero_bank(R)
        sentinel = np.full((R, W), 0xFFFFFFFF, np.uint32)
        for first, n in ((0, R), (3, 4), (R - 1, 1), (2, 0)):
            _poke(eng, d_bank, sentinel)
            eng.bank_encode(enc, d_values, n, d_bank, R, first)
            got = _peek(eng, d_bank, R * W).reshape(R, W)
            want = sentinel.copy()
            want[first:first + n] = want_rows[:n]                   # (values row r -> bank row first + r)
            assert np.array_equal(got, want), (li, first, n, np.flatnonzero((got != want).any(axis=1)).tolist())
        eng.bank_encode(enc, d_values, 1, d_bank, R, R - 1)
        assert np.array_equal(eng.read_bank(d_bank, R)[R - 1], enc.encode(values[0]))      # (read_bank sees the rows as run() will)
        eng.sync()
        eng.lib.hipFree(C.c_void_p(d_values))


@pytest.mark.gpu
def test_bank_encode_and_decode_refusals():
    """HTM_ERR_ARGUMENT, the bank untouched, and the handle usable afterwards."""
    I = 300
    eng = _sp_engine(I)
    enc = _layout_a()
    W, R = eng.words, 5
    values = _special_values(enc, 0, 1)[:R]
    d_values, d_bank = eng.upload_values(values), eng.zero_bank(R)
    d_votes, d_out = eng.device_buffer(R * I * 4, np.zeros((R, I), np.int32)), eng.device_buffer(R * 3 * 2 * 4)
    sentinel = np.full((R, W), 0xFFFFFFFF, np.uint32)
    _poke(eng, d_bank, sentinel)
    good = [(0.0, 1.1, 0, 130, 21, 110, 0), (0.0, 4.0, 130, 96, 11, 96, 1), (-5.0, 7.0, 226, 70, 1, 70, 0)]

    def swapped(j, **kw):
        names = ("minimum", "scale", "offset", "bits", "width", "buckets", "periodic")
        rows = [list(r) for r in good]
        for k, v in kw.items():
            rows[j][names.index(k)] = v
        return _raw_table(rows)
    ok = _raw_table(good)
    bad_tables = [swapped(0, bits=0, width=0, buckets=0), swapped(0, width=0), swapped(0, width=131), swapped(0, buckets=111),
                  swapped(1, buckets=86), swapped(0, offset=-1), swapped(2, offset=231), swapped(1, offset=129), swapped(0, minimum=np.nan),
                  swapped(0, minimum=np.inf), swapped(0, scale=np.inf), swapped(0, scale=0.0), swapped(0, scale=-1.0), swapped(2, scale=np.nan)]
    lib, h = eng.lib, eng.h
    void = C.c_void_p
    calls = [lambda t=t: lib.htm_bank_encode(h, t, 3, void(d_values), R, void(d_bank), R, 0) for t in bad_tables]
    calls += [lambda t=t: lib.htm_decode_votes(h, t, 3, void(d_votes), R, void(d_out)) for t in bad_tables]
    calls += [lambda: lib.htm_bank_encode(h, None, 3, void(d_values), R, void(d_bank), R, 0),
              lambda: lib.htm_bank_encode(h, ok, 3, None, R, void(d_bank), R, 0),
              lambda: lib.htm_bank_encode(h, ok, 3, void(d_values), R, None, R, 0),
              lambda: lib.htm_bank_encode(h, ok, 0, void(d_values), R, void(d_bank), R, 0),
              lambda: lib.htm_bank_encode(h, ok, 17, void(d_values), R, void(d_bank), R, 0),
              lambda: lib.htm_bank_encode(h, ok, 3, void(d_values), -1, void(d_bank), R, 0),
              lambda: lib.htm_bank_encode(h, ok, 3, void(d_values), R, void(d_bank), R, -1),
              lambda: lib.htm_bank_encode(h, ok, 3, void(d_values), R, void(d_bank), R, 1),
              lambda: lib.htm_bank_encode(h, ok, 3, void(d_values), 2, void(d_bank), R, 4),
              lambda: lib.htm_bank_encode(h, ok, 3, void(d_values), 1, void(d_bank + 4), R, 0),
              lambda: lib.htm_decode_votes(h, None, 3, void(d_votes), R, void(d_out)),
              lambda: lib.htm_decode_votes(h, ok, 3, None, R, void(d_out)),
              lambda: lib.htm_decode_votes(h, ok, 3, void(d_votes), R, None),
              lambda: lib.htm_decode_votes(h, ok, 0, void(d_votes), R, void(d_out)),
              lambda: lib.htm_decode_votes(h, ok, 3, void(d_votes), -1, void(d_out)),
              lambda: lib.htm_predicted_value(h, ok, 3, None)]
    for i, call in enumerate(calls):
        assert call() == ERR_ARGUMENT, i
        assert lib.htm_last_error(h)
    assert lib.htm_bank_encode(h, ok, 3, void(d_values), 0, void(d_bank), R, 2) == 0         # (no rows: HTM_OK, nothing done)
    assert lib.htm_decode_votes(h, ok, 3, void(d_votes), 0, void(d_out)) == 0
    assert np.array_equal(_peek(eng, d_bank, R * W).reshape(R, W), sentinel)
    # a stand-alone Spatial Pooler has no predictions to decode: HTM_ERR_STATE, as htm_predicted_input
    out = np.zeros((3, 2), np.int32)
    assert lib.htm_predicted_value(h, ok, 3, out.ctypes.data_as(void)) == -4
    # ... and the handle goes on
    eng.bank_encode(enc, d_values, R, d_bank, R)
    assert np.array_equal(eng.read_bank(d_bank, R), enc.encode(values))
    for ptr in (d_values, d_votes, d_out):
        eng.lib.hipFree(void(ptr))


def _decode_on_device(eng, enc, votes):
    votes = np.ascontiguousarray(votes, np.int32)
    n, F = len(votes), len(enc)
    d_votes, d_out = eng.device_buffer(votes.nbytes, votes), eng.device_buffer(n * F * 2 * 4, np.full(n * F * 2, -7, np.int32))
    eng.decode_votes(enc, d_votes, n, d_out)
    eng.sync()
    out = eng.read_words(C.c_void_p(d_out), n * F * 2, np.int32).reshape(n, F, 2)
    for ptr in (d_votes, d_out):
        eng.lib.hipFree(C.c_void_p(ptr))
    return out[:, :, 0], out[:, :, 1]


@pytest.mark.gpu
def test_decode_votes_equals_the_definition():
    """Votes poked into device memory, layout A: random rows, plateaus (the tie goes to the lowest bucket), a periodic maximum
    whose window wraps the field's end, a maximum in the last bucket, an all-zero row, an all-zero field beside a live one, votes
    up to 2^20 on the width-1 field and the width-11 one."""
    enc = _layout_a()
    eng = _sp_engine(300)
    rng = np.random.RandomState(4)
    votes = np.zeros((14, 300), np.int64)
    votes[0:4] = rng.randint(0, 50, (4, 300))
    votes[4, 10:60], votes[4, 130 + 20:130 + 70], votes[4, 226:296] = 3, 9, 2         # plateaus in every field
    votes[5, 40:61], votes[5, 80:101] = 7, 7                                          # two equal windows: buckets 40 and 80
    votes[6, 130 + 90:130 + 96], votes[6, 130:130 + 5] = 6, 6                         # periodic bucket 90: bits 90..95 and 0..4
    votes[6, 130 + 40:130 + 50] = 6                                                   # (one vote short of the wrapped window)
    votes[7, 109:130], votes[7, 130 + 95], votes[7, 226 + 69] = 1, 1, 1               # maxima in the last buckets 109, 95 (and 85..95 tie), 69
    votes[9, 130:226] = rng.randint(1, 4, 96)                                         # row 8 all zero; row 9: a live field between zero ones
    votes[10] = rng.randint(0, 1 << 20, 300)
    votes[10, 226 + 33] = 1 << 20
    votes[11, 296:300] = 99                                                           # only the trailing bits: no field sees them
    votes[12, 129], votes[12, 130], votes[12, 225], votes[12, 226] = 5, 6, 7, 8       # the fields' first and last bits
    votes[13] = 1                                                                     # every bucket ties: bucket 0 everywhere
    want_b, want_s = enc.decode(votes)
    assert want_b[5, 0] == 40 and want_b[6, 1] == 90 and want_b[7].tolist() == [109, 85, 69] and (want_b[8] == -1).all()
    assert want_b[9].tolist()[0::2] == [-1, -1] and want_b[9, 1] >= 0 and (want_b[11] == -1).all() and (want_b[13] == 0).all()
    assert want_s[10, 2] == 1 << 20 and want_s[10, 1] > 1 << 20
    got_b, got_s = _decode_on_device(eng, enc, votes)
    assert np.array_equal(got_b, want_b), np.argwhere(got_b != want_b).tolist()
    assert np.array_equal(got_s, want_s), np.argwhere(got_s != want_s).tolist()


@pytest.mark.gpu
@pytest.mark.parametrize("I,fields", [(3072, [(0, 1, 3000, 37, True), (0, 1, 72, 5)]), (3072, [(0, 1, 72, 72), (0, 1, 3000, 1)]),
                                      (8200, [(0, 1, 8192, 100, True)]), (8200, [(0, 1, 5, 2), (0, 1, 8192, 8192)])],
                         ids=["3000-periodic", "3000-width-1", "cap-periodic", "cap-one-bucket"])
def test_decode_votes_of_long_fields(I, fields):
    """Fields the scan takes in many passes of the block -- 3 000 bits, and the cap of 8 192 -- at aligned and unaligned offsets:
    random rows, a maximum at the very end (wrapping where the field is periodic), a lone vote in the last bit."""
    enc = _encoder(fields, I)
    eng = _sp_engine(I)
    rng = np.random.RandomState(I + len(fields))
    votes = rng.randint(0, 9, (5, I)).astype(np.int64)
    for f, off in zip(enc.fields, enc.offsets):
        votes[1, off:off + f.bits] = 0
        votes[1, off + f.bits - 1] = 4
        votes[2, off + f.bits - 3:off + f.bits] = 50
        votes[2, off:off + 3] = 50
    votes[3] = 0
    votes[4] = 2
    want_b, want_s = enc.decode(votes)
    got_b, got_s = _decode_on_device(eng, enc, votes)
    assert np.array_equal(got_b, want_b) and np.array_equal(got_s, want_s), (got_b.tolist(), want_b.tolist(), got_s.tolist(), want_s.tolist())


@pytest.mark.gpu
def test_decode_refuses_a_field_above_the_cap_and_encode_takes_it():
    from bithtm_amd import HtmError
    enc = _encoder([(0, 1, 8193, 3)], 8200)
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


# ---- runs over values against a twin stepped over the encoded rows

WITH_VOTES = ALL + ("predicted_input",)


def _values(n, seed):
    """n rows of values for layout A that cycle cleanly: a ramp, a clock and a small signal, with a missing value and one out of
    range among them."""
    t = np.arange(n, dtype=np.float64)
    rng = np.random.RandomState(seed)
    v = np.stack([10.0 + 80.0 * t / n, (3.5 * t) % 24.0, 4.0 * np.sin(t) + rng.uniform(-0.5, 0.5, n)], axis=1)
    if n > 4:
        v[2, 2], v[4, 0] = np.nan, 140.0
    return v


def _same_full_record(got, want, what=""):
    _same_record(got, want, what)
    assert (got.predicted_input is None) == (want.predicted_input is None), what
    if want.predicted_input is not None:
        assert np.array_equal(got.predicted_input, want.predicted_input), what


def _same_decoded(rec, enc, votes, what=""):
    """rec's "predicted_value" arrays == the NumPy decode of the twin's recorded votes."""
    bucket, score = enc.decode(votes)
    assert rec.predicted_bucket.dtype == np.int32 and rec.predicted_score.dtype == np.int32 and rec.predicted_value.dtype == np.float64
    assert np.array_equal(rec.predicted_bucket, bucket), (what, np.argwhere(rec.predicted_bucket != bucket)[:5].tolist())
    assert np.array_equal(rec.predicted_score, score), what
    assert np.array_equal(rec.predicted_value, enc.value_of(bucket), equal_nan=True), what


@pytest.mark.gpu
@pytest.mark.parametrize("env", SCHEDULES, ids=SCHEDULE_IDS)
def test_run_over_values_equals_the_twin_over_encoded_rows(env, monkeypatch):
    """run(values, steps, encoder=) == run(encoder.encode(values), steps) in every schedule: every record field of a learning
    call, of a second call (the cached bank) with the votes recorded as well, and of a call with learning off; the state left;
    and the same number of graphs."""
    for key, v in env.items():
        monkeypatch.setenv(key, v)
    I, Cn, K, k = SHAPE
    enc, values = _layout_a(), _values(7, 1)
    rows = enc.encode(values)
    htm, twin = _twins(I, Cn, K, active_columns=k)
    for n, learning, record in ((70, True, ALL), (45, True, WITH_VOTES), (20, False, ALL)):
        got = htm.run(values, n, learning=learning, record=record, encoder=enc)
        want = twin.run(rows, n, learning=learning, record=record)
        assert got.fields == want.fields
        _same_full_record(got, want, f"call of {n}")
    assert want.predicted_columns.max() > 0
    _same_state(htm, twin)
    assert htm.engine.graph_count() == twin.engine.graph_count()
    assert len(htm.engine._value_bufs) == 1                         # (one upload of the values, one encode launch)


@pytest.mark.gpu
def test_run_over_values_with_resets_noise_and_streaming():
    """`resets=`, `noise=` with a 9-row ring that the run wraps (the ring reads the encoded bank), a streamed call
    (continuing=True) and a plain one: all over the encoded bank as over an uploaded one."""
    I, Cn, K, k = SHAPE
    enc, values = _layout_a(), _values(5, 2)
    rows = enc.encode(values)
    resets = np.array([1, 0, 0, 1, 0], bool)
    htm, twin = _twins(I, Cn, K, active_columns=k)
    htm.noise_chunk = twin.noise_chunk = 7
    for n, kw in ((40, dict(resets=resets)), (33, dict(noise=0.05, noise_seed=77)), (25, dict(resets=resets, noise=0.1, noise_seed=3)),
                  (11, dict(continuing=True)), (17, dict()), (9, dict(learning=False, noise=0.05))):
        got = htm.run(values, n, record=ALL, encoder=enc, **kw)
        want = twin.run(rows, n, record=ALL, **kw)
        _same_full_record(got, want, f"{n} steps, {sorted(kw)}")
    _same_state(htm, twin)
    assert htm.engine.graph_count() == twin.engine.graph_count()


@pytest.mark.gpu
def test_pool_growth_inside_a_run_over_values():
    """A default-sized pool that grows in the middle of the run: the values are encoded again into a bank of the new engine."""
    from bithtm_amd import ScalarEncoder, ScalarField
    I, Cn, K = 400, 1024, 8
    enc = ScalarEncoder([ScalarField(0, 100, 180, 21), ScalarField(0, 24, 120, 11, periodic=True), ScalarField(-5, 5, 90, 9)], I)
    rng = np.random.RandomState(8)
    values = np.stack([rng.uniform(0, 100, 500), rng.uniform(0, 24, 500), rng.uniform(-5, 5, 500)], axis=1)
    htm, twin = _twins(I, Cn, K)
    first = htm.engine
    got = htm.run(values, 500, record=ALL + ("predicted_value",), encoder=enc)
    assert htm.engine is not first and len(htm.engine._value_bufs) == 1      # (the pool did grow; the bank is the new engine's)
    want = twin.run(enc.encode(values), 500, record=WITH_VOTES)
    _same_record(got, want, "growth")
    _same_decoded(got, enc, want.predicted_input, "growth")
    _same_state(htm, twin, "growth")


@pytest.mark.gpu
def test_predicted_value_records():
    """record=("predicted_value",) alone, with "predicted_input" and "counters", across two calls: bucket and score == the NumPy
    decode of the twin's recorded votes, the values value_of of the buckets; and the first step after a reset decodes what its
    votes say (a model that had predictions in those rows before)."""
    I, Cn, K, k = SHAPE
    enc, values = _layout_a(), _values(6, 5)
    rows = enc.encode(values)
    htm, twin = _twins(I, Cn, K, active_columns=k)
    got = htm.run(values, 150, record=("predicted_value",), encoder=enc)
    want = twin.run(rows, 150, record=("predicted_input",))
    assert got.fields == ("predicted_value",) and got.predicted_input is None and got.active_columns is None
    _same_decoded(got, enc, want.predicted_input, "alone")
    assert got.predicted_score[-20:].min() > 0 and not np.isnan(got.predicted_value[-1]).any()      # (the model does predict by now)
    got = htm.run(values, 30, learning=False, record=("counters", "predicted_input", "predicted_value"), encoder=enc)
    want = twin.run(rows, 30, learning=False, record=("counters", "predicted_input"))
    assert got.fields == ("counters", "predicted_input", "predicted_value")
    assert np.array_equal(got.predicted_input, want.predicted_input) and np.array_equal(got.active_columns, want.active_columns)
    _same_decoded(got, enc, want.predicted_input, "with votes and counters")
    # a reset before the first step of a call: that step bursts and its row says what the twin's votes say
    resets = np.zeros(6, bool)
    resets[htm.engine.steps % 6] = True
    got = htm.run(values, 8, learning=False, record=("predicted_value",), resets=resets, encoder=enc)
    want = twin.run(rows, 8, learning=False, record=("predicted_input", "counters"), resets=resets)
    assert want.bursting_columns[0] == want.active_columns[0]
    _same_decoded(got, enc, want.predicted_input, "after a reset")
    _same_state(htm, twin)
    # a fresh model whose first step is behind a reset: nothing stale in rows nobody wrote before
    fresh, ftwin = _twins(I, Cn, K, active_columns=k)
    got = fresh.run(values, 3, record=("predicted_value",), resets=np.array([1, 0, 0, 0, 0, 0], bool), encoder=enc)
    want = ftwin.run(rows, 3, record=("predicted_input",), resets=np.array([1, 0, 0, 0, 0, 0], bool))
    _same_decoded(got, enc, want.predicted_input, "fresh")


@pytest.mark.gpu
def test_predicted_value_needs_an_encoder_that_fits():
    from bithtm_amd import ScalarEncoder, ScalarField
    I, Cn, K, k = SHAPE
    htm, _ = _twins(I, Cn, K, active_columns=k)
    bank = np.zeros((3, I), bool)
    with pytest.raises(ValueError, match="encoder"):
        htm.run(bank, 4, record=("predicted_value",))
    with pytest.raises(ValueError, match="encoder"):
        htm.forecast(4, record=("counters", "predicted_value"))
    with pytest.raises(ValueError, match="encoder"):
        htm.lookahead(bank, 4, 2, record=("predicted_value",))
    small = ScalarEncoder([ScalarField(0, 1, 100, 5)])
    with pytest.raises(ValueError, match="input_dim"):
        htm.run(np.zeros((3, 1)), 4, encoder=small)
    with pytest.raises(ValueError, match="input_dim"):
        htm.predicted_value(small)
    with pytest.raises(ValueError):
        htm.run(np.zeros((3, 2)), 4, encoder=_layout_a())           # (two values per row for three fields)
    assert htm.engine.steps == 0


def _trained(n_steps=150, seed=5):
    I, Cn, K, k = SHAPE
    enc, values = _layout_a(), _values(6, seed)
    htm, twin = _twins(I, Cn, K, active_columns=k)
    htm.run(values, n_steps, encoder=enc)
    twin.run(enc.encode(values), n_steps)
    return enc, values, htm, twin


@pytest.mark.gpu
def test_predicted_value_of_the_current_state():
    """predicted_value(encoder) == decode(predicted_input()) after a trained run, after reset() (NaN and 0), and on a view."""
    enc, values, htm, twin = _trained()

    def check(model, votes, what):
        value, score = model.predicted_value(enc)
        bucket, want = enc.decode(votes)
        assert np.array_equal(score, want) and score.dtype == np.int32, what
        assert np.array_equal(value, enc.value_of(bucket), equal_nan=True) and value.dtype == np.float64, what
        return value, score
    value, score = check(htm, twin.predicted_input(), "trained")
    assert score.min() > 0 and not np.isnan(value).any()
    view = htm.inference_view()
    value, score = check(view, np.zeros(300, np.int32), "a new view")
    assert np.isnan(value).all() and not score.any()
    view.run(values, 9, encoder=enc)
    tview = twin.inference_view()
    tview.run(enc.encode(values), 9)
    value, score = check(view, tview.predicted_input(), "a stepped view")
    assert score.max() > 0
    htm.reset()
    twin.reset()
    value, score = check(htm, twin.predicted_input(), "reset")
    assert np.isnan(value).all() and not score.any()
    fresh, _ = _twins(*SHAPE[:3], active_columns=SHAPE[3])
    value, score = fresh.predicted_value(enc)
    assert np.isnan(value).all() and not score.any()


@pytest.mark.gpu
@pytest.mark.parametrize("on_view", [False, True], ids=["model", "view"])
def test_forecast_values(on_view):
    """forecast_values(steps, encoder): row 0 = the decode of the votes before the call, row j >= 1 = the decode of the votes the
    twin's forecast step j - 1 leaves; the state left is the twin's after forecast(steps).  Chunked (forecast_chunk = 5) too, and
    with min_votes = 20, which feeds back only the strongly voted bits.  (Whether the model still predicts something a few steps into
    its own feedback is the model's property: printed, not asserted.)"""
    enc, values, htm, twin = _trained()
    if on_view:
        htm, twin = htm.fork(), twin.fork()
    for chunk, steps, min_votes in ((1024, 9, 1), (5, 12, 20), (1024, 1, 1)):
        htm.forecast_chunk = twin.forecast_chunk = chunk
        votes0 = twin.predicted_input()
        rows, rec = twin.forecast(steps, min_votes, record=("predicted_input",))
        votes = np.concatenate([votes0[None], rec.predicted_input[:-1]])
        value, score = htm.forecast_values(steps, enc, min_votes)
        bucket, want = enc.decode(votes)
        assert value.shape == (steps, 3) and np.array_equal(score, want), (chunk, steps)
        assert np.array_equal(value, enc.value_of(bucket), equal_nan=True), (chunk, steps)
        assert np.array_equal(htm.predicted_input(), twin.predicted_input()) and htm.engine.steps == twin.engine.steps
        print(f"forecast_values({steps}, min_votes={min_votes}): rows with a prediction {(score.max(axis=1) > 0).sum()}")
        if steps == 9:
            assert score[0].min() > 0                               # (the trained model's own next value, in every field)
    value, score = htm.forecast_values(0, enc)
    assert value.shape == (0, 3) and score.shape == (0, 3)
    if not on_view:
        _same_state(htm, twin)


@pytest.mark.gpu
def test_view_runs_and_lookahead_over_values():
    """InferenceView.run(values, encoder=) against a second view stepped over the encoded rows (records, votes); lookahead(values,
    encoder=, record=("predicted_value",)) on the model against its twin's lookahead over the rows."""
    enc, values, htm, twin = _trained()
    rows = enc.encode(values)
    view, copy = htm.inference_view(), twin.inference_view()
    got = view.run(values, 20, record=ALL + ("predicted_value",), encoder=enc)
    want = copy.run(rows, 20, record=WITH_VOTES)
    _same_record(got, want, "view")
    _same_decoded(got, enc, want.predicted_input, "view")
    assert got.predicted_score.max() > 0
    assert np.array_equal(view.predicted_input(), copy.predicted_input())
    htm.lookahead_chunk = twin.lookahead_chunk = 3
    got_rows, got = htm.lookahead(values, 16, 4, every=2, record=("counters", "predicted_value"), encoder=enc)
    want_rows, want = twin.lookahead(rows, 16, 4, every=2, record=("counters", "predicted_input"))
    assert np.array_equal(got_rows, want_rows) and np.array_equal(got.bursting_columns, want.bursting_columns)
    _same_decoded(got, enc, want.predicted_input, "lookahead")
    _same_state(htm, twin)


@pytest.mark.gpu
def test_group_run_over_values():
    """ModelGroup.run with B = 3 members and per-member values [B, n, F], member for member against the same model run alone
    over its encoded rows: records, decoded votes, state; and the group's predicted_value and forecast_values against each
    twin's."""
    from bithtm_amd import ModelGroup
    I, Cn, K, k = SHAPE
    enc = _layout_a()
    values = np.stack([_values(6, 11 + i) + [3.0 * i, i, 0.1 * i] for i in range(3)])
    np.random.seed(5)
    group = ModelGroup.create(3, I, Cn, K, seeds=[4, 5, 6], active_columns=k)
    np.random.seed(5)
    alone = ModelGroup.create(3, I, Cn, K, seeds=[4, 5, 6], active_columns=k).models
    recs = group.run(values, 120, record=ALL + ("predicted_value",), encoder=enc)
    for i, (m, rec) in enumerate(zip(alone, recs)):
        want = m.run(enc.encode(values[i]), 120, record=WITH_VOTES)
        _same_record(rec, want, f"member {i}")
        _same_decoded(rec, enc, want.predicted_input, f"member {i}")
        _same_state(group.models[i], m, f"member {i}")
    assert max(rec.predicted_score.max() for rec in recs) > 0
    assert group.run(values, 5, encoder=enc) is None                # (no record: the banks are cached)
    for i, m in enumerate(alone):
        m.run(enc.encode(values[i]), 5)
    value, score = group.predicted_value(enc)                       # (every member's predicted_value, stacked)
    for i, m in enumerate(alone):
        bucket, want = enc.decode(m.predicted_input())
        assert np.array_equal(score[i], want) and np.array_equal(value[i], enc.value_of(bucket), equal_nan=True), i
    assert value.shape == (3, 3) and score.max() > 0
    value, score = group.forecast_values(4, enc)
    for i, m in enumerate(alone):
        votes0 = m.predicted_input()
        _, rec = m.forecast(4, record=("predicted_input",))
        bucket, want = enc.decode(np.concatenate([votes0[None], rec.predicted_input[:-1]]))
        assert np.array_equal(score[i], want) and np.array_equal(value[i], enc.value_of(bucket), equal_nan=True), i
        _same_state(group.models[i], m, f"forecast, member {i}")
