"""GPU: the top-down pass -- role_pin's votes (htm_decode.h), role_encode's feedback row (htm_forecast.h), k_decode_votes' value
(htm_scalar.h) -- on the hand-built states of tests/topdown_cases.py, against the definition itself: tests/forecast_fixture.py's
votes_of and encode (the reference's own expressions) and ScalarEncoder.decode, over arrays this module sets with
engine.set_permanence and engine.import_prev_state.  Every comparison is exact integer equality.

tests/test_topdown_cases_cpu.py proves, without a device, that each case reaches the path it is named for (a named wrong
implementation differs from the definition there) and that the learning scenario moves mask bits every way.  Here:
  * the votes at every shape, prediction family and permanence family, twice in a row, with the handle's step parity both ways;
  * the recorded paths (k_pin_step, kgrp_pin_*, k_feed_votes / k_feed_step) at two odd shapes after training, every row against
    the definition over the device's own float64 rows and the recorded column predictions -- not against a twin;
  * the connected mask the votes read against get_permanence() >= threshold after every learning step, host-fed and batched, in
    every launch schedule;
  * the feedback row through predicted_bits() and as raw words in a bank of sentinels;
  * the chain votes -> value; the record's predicted_columns_before on a second-word-only prediction.
No case, shape or schedule is skipped; nothing is repeated to catch a race; no mutated kernel is run."""

import numpy as np
import pytest

import topdown_cases as td
from forecast_fixture import encode, votes_of
from test_hip_input_noise import _peek, _poke
from test_hip_run_record import ALL, SCHEDULES, SCHEDULE_IDS, _bank

pytestmark = pytest.mark.gpu

REC = ("column_prediction", "predicted_input")
ODD = [(1025, 1025, 64), (2049, 3000, 48)]
ODD_IDS = ["1025x1025x64", "2049x3000x48"]
# 50 passes over the 8-row bank, then 12 recorded steps.  When a model starts to predict is a property of the model, not of the
# code under test, so the length was read off the ORACLE on the same bank (seed 5): 1 025 x 64 predicts from step 32 on, 3 000 x 48
# predicts its first column at step 223 and 12 to 26 columns a step from step 400 on (at the first choice, 104 steps, none).
TRAIN, STEPS = 400, 12


def _model(shape, thr, permanence, params=None):
    """A fused model of a crafted shape over a crafted permanence (threshold `thr`, or the oracle SPParams `params`)."""
    from hip_impl import make_htm
    from oracle import SPParams
    I, C, K = shape
    htm = make_htm(I, C, K, td.active_columns(C), 1, permanence, params or SPParams(permanence_threshold=thr))
    assert htm.engine.words == td.enc_layout(I).W
    return htm


def _same(got, want, what):
    got, want = np.asarray(got), np.asarray(want)
    assert got.shape == want.shape and got.dtype == want.dtype, (what, got.shape, got.dtype)
    bad = np.flatnonzero(got != want)
    assert not len(bad), (what, f"{len(bad)} differ, first at {bad[:8].tolist()}: got {got[bad[:8]].tolist()}, want {want[bad[:8]].tolist()}")


def _set(eng, pred):
    eng.import_prev_state(pred, np.zeros_like(pred), None, None)


@pytest.mark.parametrize("family", td.PERMANENCE_FAMILIES)
@pytest.mark.parametrize("shape", td.SHAPES, ids=td.SHAPE_IDS)
def test_votes_equal_the_definition(shape, family):
    """predicted_input() == votes_of(permanence, threshold, prediction) for every column set x cell placement of the shape, asked
    twice in a row (the output row is zeroed per call), with the state imported at step 0 (k_pin reads prediction parity 1) and
    again after one process(learning=False) (parity 0).
      * the bit loop ending after one pass, or a second pass reading the first pass's mask words: inputs from 1 024 on differ;
      * a block over a partial chunk reading columns past C, or no block for it: the votes of columns from 1 024 k on differ;
      * the early return of an empty chunk taken by the wrong block; the list's tail of n % 8 columns dropped or counted twice;
      * the second prediction word of a column not read: a column predicted in cell 32 alone gives no votes;
      * a mask through float32, with `>`, or by the sign bit: the boundary families' votes differ at every input."""
    I, C, K, k, thr, perm, cases = td.vote_cases(shape, family)
    htm = _model(shape, thr, perm)
    eng = htm.engine
    want = {}
    for parity in (1, 0):
        if parity == 0:
            htm.process(np.random.RandomState(5).rand(I) < 0.1, learning=False)
            assert eng.steps == 1
        for name, cols, pred in cases:
            key = cols.tobytes()
            if key not in want:
                want[key] = votes_of(perm, thr, pred)
            _set(eng, pred)
            for call in (1, 2):
                _same(htm.predicted_input(), want[key], (name, f"parity {parity}", f"call {call}"))
    assert any(v.any() for v in want.values())


def _rows_equal_the_definition(perm, thr, rec, what):
    assert len(rec) == STEPS and rec.column_prediction.any(), what
    for t in range(len(rec)):
        _same(rec.predicted_input[t], votes_of(perm, thr, rec.column_prediction[t][:, None]), (what, f"step {t}"))
    assert rec.predicted_input.any(), what


def _trained(shape, seed=5, boost_intensity=None):
    import bithtm_amd as B
    I, C, K = shape
    np.random.seed(seed)                            # (the SP's permanences are drawn from NumPy's global stream)
    sp = None if boost_intensity is None else B.SpatialPooler(I, C, 48, boosting=B.ExponentialBoosting(C, 48, intensity=boost_intensity))
    htm = B.HierarchicalTemporalMemory(I, C, K, active_columns=48, seed=seed, spatial_pooler=sp)
    bank = _bank(8, I, 3)
    htm.run(bank, TRAIN)
    return htm, bank, htm.spatial_pooler.proximal_projection.permanence_threshold


@pytest.mark.parametrize("env", SCHEDULES, ids=SCHEDULE_IDS)
@pytest.mark.parametrize("shape", ODD, ids=ODD_IDS)
def test_recorded_votes_equal_the_definition(shape, env, monkeypatch):
    """run(record=("column_prediction", "predicted_input")) after training, in every schedule: recorded row t (rows are slot * I
    apart, I = 1 025 / 2 049) == the definition over the device's own float64 rows and the columns step t predicts."""
    for key, v in env.items():
        monkeypatch.setenv(key, v)
    htm, bank, thr = _trained(shape)
    rec = htm.run(bank, STEPS, learning=False, record=REC)
    _rows_equal_the_definition(htm.engine.get_permanence(), thr, rec, "run")
    _same(htm.predicted_input(), rec.predicted_input[-1], "after the run")


@pytest.mark.parametrize("shape", ODD, ids=ODD_IDS)
def test_recorded_votes_of_a_view_equal_the_definition(shape):
    htm, bank, thr = _trained(shape)
    view = htm.inference_view()
    view.run(bank, 16, learning=False)
    rec = view.run(bank, STEPS, learning=False, record=REC)
    _rows_equal_the_definition(htm.engine.get_permanence(), thr, rec, "view")


@pytest.mark.parametrize("shape", ODD, ids=ODD_IDS)
def test_recorded_votes_of_group_members_equal_the_definition(shape):
    """kgrp_pin_begin / kgrp_pin_step, one member per grid row: three members with other seeds over other banks."""
    import bithtm_amd as B
    from test_hip_model_group import _banks, _model as _member
    I, C, K = shape
    models = [_member(I, C, K, 11 + 7 * i, k=48) for i in range(3)]
    group = B.ModelGroup(models)
    banks = _banks(3, 8, I, 3)
    group.run(banks, TRAIN)
    recs = group.run(banks, STEPS, learning=False, record=REC)
    assert len(recs) == 3
    for i, (m, rec) in enumerate(zip(models, recs)):
        _rows_equal_the_definition(m.engine.get_permanence(), m.spatial_pooler.proximal_projection.permanence_threshold, rec, f"member {i}")
    assert not np.array_equal(recs[0].predicted_input, recs[1].predicted_input)


@pytest.mark.parametrize("shape", ODD, ids=ODD_IDS)
def test_forecast_rows_and_votes_equal_the_definition(shape):
    """forecast(n, 1, 10, record=...): k_feed_votes + k_feed_step per step.  Row 0 == encode(the votes before the call), row t ==
    encode(the recorded votes of step t - 1); every recorded votes row == the definition.
    How long a closed loop lives is a property of the model: on the ORACLE, with the default boosting, ten fed-back bits of a 61-bit
    pattern select none of the trained columns at either shape and the loop is dead at its first step.  With boosting off
    (intensity 0.0) step 0 follows the sequence and leaves predictions (153 and 114 inputs with votes), so row 1 is k_feed_step's
    capped row over k_feed_votes' votes of a non-empty prediction; the loop is dead from step 1 on."""
    htm, bank, thr = _trained(shape, boost_intensity=0.0)
    before = htm.predicted_input()
    assert (before > 0).sum() > 10 and np.bincount(before[before > 0]).max() > 1           # (the cap bites, among ties)
    rows, rec = htm.forecast(STEPS, 1, 10, record=REC)
    perm = htm.engine.get_permanence()
    _rows_equal_the_definition(perm, thr, rec, "forecast")
    fed = np.concatenate([before[None], rec.predicted_input[:-1]])
    for t in range(STEPS):
        _same(rows[t], encode(fed[t], 1, 10), ("forecast row", t))
    assert rows[0].sum() == 10 and rows[1].sum() == 10


def _mask_equals_the_rows(sc, htm, winners, what):
    """All columns predicted: votes == (get_permanence() >= thr).sum(0); then the winners alone, in cell K - 1.  Returns the rows."""
    eng = htm.engine
    perm = eng.get_permanence()
    _set(eng, np.ones((sc.C, sc.K), bool))
    _same(htm.predicted_input(), (perm >= sc.thr).sum(axis=0).astype(np.int32), (what, "every column"))
    pred = td.prediction(sc.C, sc.K, winners, [sc.K - 1])
    _set(eng, pred)
    _same(htm.predicted_input(), votes_of(perm, sc.thr, pred), (what, "the winners"))
    return perm


@pytest.mark.parametrize("mode", ["host-fed", "batched"])
@pytest.mark.parametrize("env", SCHEDULES, ids=SCHEDULE_IDS)
@pytest.mark.parametrize("name", list(td.SCENARIOS))
def test_the_mask_the_votes_read_follows_the_rows(name, env, mode, monkeypatch):
    """topdown_cases.learning_scenario: six learning steps whose winners are designated and whose updates move entries across the
    threshold both ways and exactly onto it.  After every process() (host-fed), and after one run() over the bank (batched), the
    votes of an all-columns prediction == (get_permanence() >= threshold).sum(0), the winners' votes == the definition over their
    rows, the rows are the oracle's bit for bit, and the crossings the CPU test promised are there on the device's own rows.
      * a mask bit set with `>`, or from a float32 copy, or not rewritten for an entry that lands exactly on the threshold;
      * a word of a winner's mask row left stale (the scenario's last inputs lie past 1 024);
      * a schedule that applies the rows but not the mask, or the mask a step late."""
    from oracle.htm_oracle import SpatialPoolerOracle
    for key, v in env.items():
        monkeypatch.setenv(key, v)
    sc = td.learning_scenario(name)
    htm = _model((sc.I, sc.C, sc.K), sc.thr, sc.permanence.copy(), sc.params)
    assert htm.active_columns == sc.k
    ora = SpatialPoolerOracle(sc.I, sc.C, sc.k, params=sc.params, permanence=sc.permanence.copy())
    P, total = len(sc.bank), {}
    before = _mask_equals_the_rows(sc, htm, sc.winners[0], "before")
    _same(before.view(np.int64), sc.permanence.view(np.int64), "the rows as set")
    if mode == "host-fed":
        for t in range(sc.steps):
            sp, _ = htm.process(sc.bank[t % P], learning=True)
            won = np.sort(np.asarray(sp.active_column)).astype(np.int64)
            _same(won, sc.winners[t % P], ("winners", t))
            ora.step(sc.bank[t % P], learning=True)
            after = _mask_equals_the_rows(sc, htm, won, f"step {t}")
            _same(after.view(np.int64), ora.permanence.view(np.int64), ("rows", t))
            td.add_crossings(total, td.crossings(before, after, sc.thr))
            before = after
        assert all(total[key] >= sc.k for key in ("up", "down", "on_from_below", "on_from_above")), total
    else:
        rec = htm.run(sc.bank, sc.steps, learning=True, record=("active_column",))
        for t in range(sc.steps):
            _same(np.sort(rec.active_column[t]).astype(np.int64), sc.winners[t % P], ("winners", t))
            ora.step(sc.bank[t % P], learning=True)
        after = _mask_equals_the_rows(sc, htm, sc.winners[(sc.steps - 1) % P], "end")
        _same(after.view(np.int64), ora.permanence.view(np.int64), "rows at the end")
        total = td.crossings(before, after, sc.thr)
        assert all(total[key] >= 1 for key in ("up", "down", "on_from_below", "on_from_above")), total


@pytest.mark.parametrize("shape", td.SHAPES, ids=td.SHAPE_IDS)
def test_feedback_rows_equal_the_definition(shape):
    """For every vote row of the shape (a staircase permanence under an all-columns prediction: votes == want) and every
    (min_votes, max_bits) of the row: predicted_bits() == encode(want, ...), twice; and htm_encode_votes into row 1 of a 3-row
    bank of all-ones words, twice: every word of row 1 written, its pad bits 0, rows 0 and 2 untouched.  (The second call also
    proves that the first left the scratch votes zero: role_pin adds into them.)
      * ties to the higher index; a quota per wave or per chunk; a cut one lane off at lane 63 / 64 or at a wave's run boundary;
      * an idle wave (input_dim <= 128) that writes, or a last wave whose short run leaves words unwritten;
      * one histogram bin for all 64 lanes counted once; candidates == max_bits capped, or max_bits + 1 not capped;
      * the second radix pass (votes from 4 096) ranking by the low digit."""
    I, C, K = shape
    rows = td.encoder_rows(shape)
    htm = _model(shape, 0.0, td.staircase_permanence(C, rows[0][1]))
    eng = htm.engine
    _set(eng, np.ones((C, K), bool))
    R, r, W = 3, 1, eng.words
    bank = eng.zero_bank(R)
    ones = np.full(R * W, 0xFFFFFFFF, np.uint32)
    for n, (name, want, pairs, cut) in enumerate(rows):
        if n:
            eng.set_permanence(td.staircase_permanence(C, want))
        _same(htm.predicted_input(), want, (name, "votes"))
        for mv, mb in pairs:
            x, words = encode(want, mv, mb), td.encode_words(want, mv, mb, W)
            for call in (1, 2):
                _same(htm.predicted_bits(mv, mb), x, (name, mv, mb, f"predicted_bits call {call}"))
            for call in (1, 2):
                _poke(eng, bank, ones)
                eng.encode_votes(mv, mb, bank, R, r)
                got = _peek(eng, bank, R * W).reshape(R, W)
                _same(got[r], words, (name, mv, mb, f"row words, call {call}"))
                assert (got[[0, 2]] == 0xFFFFFFFF).all(), (name, mv, mb, "a neighbouring row was written")


def test_votes_above_4096_decode_to_the_definitions_value():
    """votes -> value on the device (htm_predicted_value: k_pin + k_decode_votes): three fields at unaligned offsets (101, 131
    and 97 bits from offsets 0, 101 and 232), the middle one periodic, over staircase votes from 0 to 8 192 with many ties."""
    from bithtm_amd.encoders import ScalarEncoder, ScalarField
    shape = td.SHAPES[-1]
    I, C, K = shape
    enc = ScalarEncoder([ScalarField(0.0, 100.0, 101, 7), ScalarField(-5.0, 5.0, 131, 21, periodic=True), ScalarField(0.0, 1.0, 97, 5)], input_dim=I)
    rows = td.chain_rows(shape)
    htm = _model(shape, 0.0, td.staircase_permanence(C, rows[0]))
    _set(htm.engine, np.ones((C, K), bool))
    for n, want in enumerate(rows):
        if n:
            htm.engine.set_permanence(td.staircase_permanence(C, want))
        assert want.max() > 4096 and np.bincount(want).max() > 8
        _same(htm.predicted_input(), want, (n, "votes"))
        bucket, score = enc.decode(want)
        value, got_score = htm.predicted_value(enc)
        _same(got_score, score, (n, "score"))
        assert (bucket >= 0).all() and np.array_equal(value, enc.value_of(bucket)), (n, value, enc.value_of(bucket))


@pytest.mark.parametrize("shape", [s for s in td.SHAPES if s[2] > 32], ids=[i for i, s in zip(td.SHAPE_IDS, td.SHAPES) if s[2] > 32])
def test_the_record_counts_columns_predicted_in_the_second_word(shape):
    """rec_column_bits makes the same two-word test as role_pin: after importing a prediction that sits in cell 32 alone (then cell
    31, then the last cell), a one-step run(learning=False, record=ALL) reports every predicted column in predicted_columns_before."""
    I, C, K = shape
    thr, perm = td.permanence_case(shape, "seeded-0.0")
    htm = _model(shape, thr, perm)
    cols = dict(td.column_sets(C))["third"]
    bank = _bank(2, I, 3)
    for cell in (32, 31, K - 1):
        pred = td.prediction(C, K, cols, [cell])
        _set(htm.engine, pred)
        _same(htm.predicted_input(), votes_of(perm, thr, pred), (cell, "votes"))
        rec = htm.run(bank, 1, learning=False, record=ALL)
        assert rec.predicted_columns_before[0] == pred.any(axis=1).sum() == len(cols), (cell, rec.predicted_columns_before[0], len(cols))
