"""Sequence resets without a GPU: the oracle against a recorded lock-step run of the unmodified reference with resets in its
own idiom, `tm.last_state = tm.get_empty_state()` (tests/golden/generate_lockstep_reset.py), and the C ABI of htm_reset /
htm_set_run_resets (declared, exported, argument checks that need no device)."""

import os
import re
from types import SimpleNamespace

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden")


def test_oracle_replays_the_reference_with_resets():
    """Every field of every step and the store at every check give the reference's digests, the oracle stepping with the
    empty state as prev_state where the reference was reset."""
    import refdiff
    from oracle import HTMOracle
    rec = refdiff.load_lockstep(os.path.join(GOLDEN, "lockstep_reset.npz"))
    seed, I, C, K, steps = (int(rec[k]) for k in ("seed", "input_dim", "column_dim", "cell_dim", "steps"))
    resets = set(rec["resets"].tolist())
    assert {1, 40, 41} <= resets                                # (a reset at step 1, two consecutive ones)
    assert any(not rec["learning"][t] for t in resets)         # (and resets on steps with learning off)
    np.random.seed(seed)
    ora = HTMOracle(I, C, K, active_columns=round(C * 0.02), seed=seed)
    assert refdiff.digest(ora.spatial_pooler.permanence) == rec["permanence_digest"]
    bank, rng = refdiff.make_inputs(seed + 1, int(rec["patterns"]), I, float(rec["density"]))
    names, store_names = [str(n) for n in rec["step_field_names"]], [str(n) for n in rec["store_field_names"]]
    stores = dict(zip(rec["store_steps"].tolist(), rec["store_digest"]))
    empty = SimpleNamespace(cell_prediction=np.zeros((C, K), bool), cell_activation=np.zeros((C, K), bool), winner_cell=None,
                            distal_state=None)
    for t in range(steps):
        x = bank[refdiff.pattern_index(t, int(rec["patterns"]), 0.0, rng)] ^ (rng.rand(I) < float(rec["noise"]))
        learning = bool(rec["learning"][t])
        if t in resets:
            sp = ora.spatial_pooler.step(x, learning=learning)
            tm = ora.temporal_memory.step(sp.active_column, learning=learning, prev_state=empty)
            assert not tm.active_column_bursting.size or tm.active_column_bursting.all(), t
        else:
            sp, tm = ora.step(x, learning=learning)
        fields = refdiff.step_fields(sp, tm)
        assert list(fields) == names
        for n, a, want in zip(names, fields.values(), rec["step_digest"][t]):
            assert refdiff.digest(a) == want, f"step {t}: {n} differs from the reference's"
        if t in stores:
            fields = refdiff.oracle_store_fields(ora)
            for n, a, want in zip(store_names, fields.values(), stores[t]):
                assert refdiff.digest(a) == want, f"step {t}: store field {n} differs from the reference's"
    assert ora.temporal_memory.S == int(rec["segments"])


def test_header_declares_and_library_exports_the_reset_abi():
    from bithtm_amd import _lib
    header = open(os.path.join(ROOT, "include", "bithtm_hip.h")).read()
    assert re.search(r"int htm_reset\(htm_handle \*h\);", header)
    assert re.search(r"int htm_set_run_resets\(htm_handle \*h, const uint32_t \*device_bits, int32_t n_inputs\);", header)
    assert "#define BITHTM_ABI_VERSION 4" in header
    assert "htm_reset" in _lib.EXPORTS and "htm_set_run_resets" in _lib.EXPORTS


def test_reset_entry_points_check_their_arguments():
    """NULL handles: HTM_ERR_ARGUMENT, without a device."""
    from bithtm_amd import _lib
    lib = _lib.load()
    assert lib.htm_abi_version() == 4
    assert lib.htm_reset(None) == -1
    assert lib.htm_set_run_resets(None, None, 0) == -1
