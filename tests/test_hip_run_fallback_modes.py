"""The resume fallback of a batched run together with the run's modes.  A run(continuing=True) leaves the Spatial Pooler one
step ahead; where the next run() on the bank finds the pipelined schedule gone -- it passes pipeline=False, or another model
with a stream of its own has appeared on the device -- it finishes that step in the form the run before began it and goes on
unpipelined.  Here that call is recorded, carries reset bits and (where the schedule lets a decoding call go ahead at all)
decodes the predicted input: every field of the three calls' records and the state they leave against a twin that takes the
same 46 steps one by one with reset() and process()."""
import functools
import gc

import numpy as np
import pytest

from test_hip_run_record import ALL, _assert_record, _bank
from test_hip_sequence_reset import RESETS, _expected

SHAPE = (300, 1024, 16, 64)                         # input_dim, column_dim, cell_dim, active_columns
CHUNKS = (20, 17, 9)
SEED = 5


def _model():
    import bithtm_amd as B
    I, Cn, K, k = SHAPE
    np.random.seed(SEED)                            # (the SP's permanences are drawn from NumPy's global stream)
    return B.HierarchicalTemporalMemory(I, Cn, K, seed=SEED, active_columns=k)


@functools.lru_cache(maxsize=None)
def _stepwise():
    """The 46 steps on a twin, one by one (host-fed steps compute what every schedule of a batched run computes): the record
    fields, the votes after each step, the state at the end.  Computed once and left alone."""
    bank = _bank(8, SHAPE[0], 7)
    twin = _model()
    counters, cols, preds, votes = [], [], [], []
    for t in range(sum(CHUNKS)):
        c, a, p = _expected(twin, [bank[t % 8]], RESETS, t)
        counters.append(c), cols.append(a), preds.append(p), votes.append(twin.predicted_input())
    state = twin.state_dict()
    out = (np.concatenate(counters), np.concatenate(cols), np.concatenate(preds), np.stack(votes))
    for a in out + tuple(state.values()):
        a.setflags(write=False)
    return bank, out, state


@pytest.mark.gpu
@pytest.mark.parametrize("cause", ["pipeline_false", "second_model"])
@pytest.mark.parametrize("lean, decode", [("2", True), ("1", True), ("0", False)], ids=["two-launch", "three-launch", "four-launch"])
def test_recorded_reset_decoding_run_through_the_resume_fallback(lean, decode, cause, monkeypatch):
    monkeypatch.setenv("BITHTM_LEAN", lean)
    from bithtm_amd.engine import HtmError
    bank, (counters, cols, preds, votes), state = _stepwise()
    gc.collect()                                    # (no other model alive: one with a stream of its own takes the pipelined schedule away)
    fields = ALL + ("predicted_input",) if decode else ALL
    htm = _model()
    parts = [htm.run(bank, CHUNKS[0], continuing=True, record=fields, resets=RESETS)]
    ahead = htm.engine.run_plan(CHUNKS[0], continuing=True)["pipelined"]
    print(f"BITHTM_LEAN={lean} {cause}: the first call was pipelined and left the Spatial Pooler ahead: {ahead}")
    if ahead:
        with pytest.raises(HtmError, match="ahead"):            # ... so the second call takes the fallback
            htm.process(bank[0])
    other = None
    if cause == "second_model":
        other = _model()                            # a second live handle with a stream of its own
        other.process(bank[0])
        assert not htm.engine.run_plan(CHUNKS[1])["pipelined"]
        parts.append(htm.run(bank, CHUNKS[1], record=fields, resets=RESETS))
    else:
        parts.append(htm.run(bank, CHUNKS[1], pipeline=False, record=fields, resets=RESETS))
    parts.append(htm.run(bank, CHUNKS[2], record=fields, resets=RESETS))
    start = 0
    for i, (rec, n) in enumerate(zip(parts, CHUNKS)):
        part = slice(start, start + n)
        _assert_record(rec, (counters[part], cols[part], preds[part]), what=f"call {i}")
        assert np.array_equal(rec.step_index, np.arange(start, start + n)), f"call {i}"
        if decode:
            assert np.array_equal(rec.predicted_input, votes[part]), f"call {i}"
        start += n
    assert counters[:, 3].max() > 0 and (not decode or votes.any())        # (the stretch predicts something)
    got = htm.state_dict()
    assert got.keys() == state.keys()
    for key in state:
        assert np.array_equal(got[key], state[key]), key
    del other
