"""Closed-loop forecasting without a GPU: the oracle's own step composed with the reference's votes expression and encode()
against the recorded run of the unmodified reference (tests/golden/generate_forecast.py), encode() on hand-made votes, and the
C ABI of htm_encode_votes / htm_set_run_feedback (declared, exported, bound, NULL checks that need no device)."""

import copy
import os
import re

import numpy as np
import pytest

from forecast_fixture import CASES, FIXTURE, encode, oracle_closed_loop, trained_oracle, unpack_rows, votes_of

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def trained():
    rec = dict(np.load(FIXTURE))
    return rec, trained_oracle(rec)


@pytest.mark.parametrize("case", range(len(CASES)), ids=[f"min{a}-max{b}" for a, b in CASES])
def test_oracle_closed_loop_reproduces_the_reference(trained, case):
    import refdiff
    rec, (ora, tm) = trained
    sp_o = ora.spatial_pooler
    assert refdiff.digest(votes_of(sp_o.permanence, sp_o.params.permanence_threshold, tm.cell_prediction)) == rec["seed_votes_digest"][case]
    assert [tuple(c) for c in rec["cases"].tolist()] == CASES
    min_votes, max_bits = CASES[case]
    steps, I = int(rec["steps"]), int(rec["input_dim"])
    rows, votes, cols = oracle_closed_loop(copy.deepcopy(ora), tm, steps, min_votes, max_bits)
    assert np.array_equal(rows, unpack_rows(rec["rows"][case], I))
    assert [refdiff.digest(v) for v in votes] == rec["votes_digest"][case].tolist()
    assert np.array_equal(cols, rec["active_column"][case])


def test_fixture_holds_sustained_and_empty_cases():
    rec = dict(np.load(FIXTURE))
    bits = [unpack_rows(r, int(rec["input_dim"])).sum(axis=1) for r in rec["rows"]]
    assert bits[0].min() > 0 and bits[1].min() > 0 and (bits[1] <= 10).all() and (bits[0] <= 18).all()
    assert bits[2].max() > 18 and bits[2][-1] == 0           # (uncapped: an over-full row, then nothing is predicted any more)


def test_encode_on_hand_made_votes():
    from bithtm_amd.networks import encode_votes
    for enc in (encode, encode_votes):
        v = np.array([0, 3, 1, 3, 2, 3, 1, 0, 2], np.int32)
        assert enc(v, 1, 0).tolist() == (v >= 1).tolist()
        assert enc(v, 2, 0).tolist() == (v >= 2).tolist()
        # ties at the cut-off go to the lower index: three 3s, then the first of the two 2s
        assert np.flatnonzero(enc(v, 1, 4)).tolist() == [1, 3, 4, 5]
        assert np.flatnonzero(enc(v, 1, 2)).tolist() == [1, 3]
        assert np.flatnonzero(enc(v, 1, 6)).tolist() == [1, 2, 3, 4, 5, 8]
        # more room than candidates: the threshold decides; fewer than min_votes is never set
        assert np.flatnonzero(enc(v, 2, 100)).tolist() == [1, 3, 4, 5, 8]
        assert np.flatnonzero(enc(v, 3, 5)).tolist() == [1, 3, 5]
        assert not enc(v, 4, 2).any() and not enc(np.zeros(37, np.int32), 1, 5).any() and not enc(np.zeros(37, np.int32), 1, 0).any()
        # input_dim that is no multiple of 32, the last input included
        w = np.zeros(45, np.int32)
        w[[44, 31, 32, 0]] = [5, 5, 5, 1]
        assert np.flatnonzero(enc(w, 1, 2)).tolist() == [31, 32]
        assert np.flatnonzero(enc(w, 1, 3)).tolist() == [31, 32, 44]
        assert np.flatnonzero(enc(w, 1, 0)).tolist() == [0, 31, 32, 44]
        with pytest.raises((AssertionError, ValueError)):
            enc(v, 0, 0)
        with pytest.raises((AssertionError, ValueError)):
            enc(v, 1, -1)


def test_header_declares_and_library_binds_the_forecast_abi():
    from bithtm_amd import _lib
    header = open(os.path.join(ROOT, "include", "bithtm_hip.h")).read()
    assert re.search(r"int htm_encode_votes\(htm_handle \*h, int32_t min_votes, int32_t max_bits, uint32_t \*device_bank, int32_t bank_rows, "
                     r"int32_t row\);", header)
    assert re.search(r"int htm_set_run_feedback\(htm_handle \*h, uint32_t \*device_bank, int32_t n_inputs, int32_t min_votes, int32_t max_bits\);",
                     header)
    assert "#define BITHTM_ABI_VERSION 4" in header
    assert len(_lib.EXPORTS["htm_encode_votes"][1]) == 6 and len(_lib.EXPORTS["htm_set_run_feedback"][1]) == 5
    lib = _lib.load()
    assert lib.htm_abi_version() == 4
    assert lib.htm_encode_votes(None, 1, 0, None, 1, 0) == -1
    assert lib.htm_set_run_feedback(None, None, 0, 1, 0) == -1


def test_python_surface():
    import bithtm_amd as B
    for cls in (B.HierarchicalTemporalMemory, B.InferenceView, B.ModelGroup):
        assert callable(cls.forecast)
    assert callable(B.HierarchicalTemporalMemory.predicted_bits) and callable(B.InferenceView.predicted_bits)
