"""Predicted-input decoding without a GPU: the oracle against a recorded lock-step run of the unmodified reference
(tests/golden/generate_predicted_input.py) -- the votes of every step from the oracle's own state, with the formula the
reference's objects define -- and the C ABI of htm_predicted_input / htm_set_run_predicted_input (declared, exported, argument
checks that need no device)."""

import os
import re
from types import SimpleNamespace

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FIXTURE = os.path.join(ROOT, "tests", "golden", "predicted_input.npz")


def votes_of(permanence, threshold, cell_prediction):
    """(pp.permanence[tm_state.cell_prediction.any(axis=1)] >= pp.permanence_threshold).sum(axis=0)"""
    return (permanence[np.asarray(cell_prediction).any(axis=1)] >= threshold).sum(axis=0).astype(np.int32)


def fixture_inputs(rec):
    """The inputs of the recorded run, step by step (refdiff.make_inputs, pattern_index)."""
    import refdiff
    I, patterns = int(rec["input_dim"]), int(rec["patterns"])
    bank, rng = refdiff.make_inputs(int(rec["seed"]) + 1, patterns, I, float(rec["density"]))
    for t in range(int(rec["steps"])):
        yield bank[refdiff.pattern_index(t, patterns, 0.0, rng)] ^ (rng.rand(I) < float(rec["noise"]))


def test_oracle_replays_the_reference_votes():
    """Every step's votes, from the oracle's permanences and cell predictions, give the reference's digests; and each step's
    votes dotted with the next input give the sum of the next step's overlaps over the columns it predicted."""
    import refdiff
    from oracle import HTMOracle
    rec = dict(np.load(FIXTURE))
    seed, I, C, K, k = (int(rec[f]) for f in ("seed", "input_dim", "column_dim", "cell_dim", "active_columns"))
    resets = set(rec["resets"].tolist())
    assert resets and not rec["learning"].all()
    np.random.seed(seed)
    ora = HTMOracle(I, C, K, active_columns=k, seed=seed)
    assert refdiff.digest(ora.spatial_pooler.permanence) == rec["permanence_digest"]
    sp_o = ora.spatial_pooler
    empty = SimpleNamespace(cell_prediction=np.zeros((C, K), bool), cell_activation=np.zeros((C, K), bool), winner_cell=None,
                            distal_state=None)
    prev = None
    for t, x in enumerate(fixture_inputs(rec)):
        learning = bool(rec["learning"][t])
        if t in resets:
            sp = sp_o.step(x, learning=learning)
            tm = ora.temporal_memory.step(sp.active_column, learning=learning, prev_state=empty)
        else:
            sp, tm = ora.step(x, learning=learning)
            if prev is not None:
                votes, pred = prev
                assert int(votes.astype(np.int64) @ x) == int(np.asarray(sp.overlaps)[pred].sum()), t
        votes = votes_of(sp_o.permanence, sp_o.params.permanence_threshold, tm.cell_prediction)
        assert refdiff.digest(votes) == rec["votes_digest"][t], f"step {t}: votes differ from the reference's"
        assert int(votes.sum()) == int(rec["votes_total"][t])
        prev = (votes, np.asarray(tm.cell_prediction).any(axis=1))
    assert (rec["votes_total"] > 0).sum() > len(rec["votes_total"]) // 2


def test_header_declares_and_library_exports_the_decoding_abi():
    from bithtm_amd import _lib
    header = open(os.path.join(ROOT, "include", "bithtm_hip.h")).read()
    assert re.search(r"int htm_predicted_input\(htm_handle \*h, int32_t \*host_dst\);", header)
    assert re.search(r"int htm_set_run_predicted_input\(htm_handle \*h, int32_t \*device_votes\);", header)
    assert "#define BITHTM_ABI_VERSION 4" in header
    assert "htm_predicted_input" in _lib.EXPORTS and "htm_set_run_predicted_input" in _lib.EXPORTS


def test_decoding_entry_points_check_their_arguments():
    """NULL handles: HTM_ERR_ARGUMENT, without a device."""
    from bithtm_amd import _lib
    lib = _lib.load()
    assert lib.htm_abi_version() == 4
    assert lib.htm_predicted_input(None, None) == -1
    assert lib.htm_set_run_predicted_input(None, None) == -1


def test_record_field_and_run_record_attribute():
    """CPU: "predicted_input" is a record field of its own, ordered after the others, and RunRecord carries it."""
    from bithtm_amd import RunRecord
    from bithtm_amd.networks import _record_fields
    assert _record_fields(("predicted_input", "counters")) == ("counters", "predicted_input")
    assert _record_fields("predicted_input") == ("predicted_input",)
    votes = np.arange(6, dtype=np.int32).reshape(2, 3)
    rec = RunRecord(np.arange(2), predicted_input=votes)
    assert rec.fields == ("predicted_input",) and rec.predicted_input is votes and rec.active_columns is None
    assert rec.active_column is None and rec.anomaly_score is None
