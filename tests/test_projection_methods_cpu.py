"""The oracle's PredictiveProjection.update / .process (oracle/htm_oracle.py) against the unmodified reference, on the
adversarial cases of tests/projection_method_cases.py -- without a device and without the reference: what the reference
computed is recorded in tests/golden/projection_methods.npz (tests/golden/generate_projection_methods.py).  Every case's
precondition -- the proof, on the oracle alone, that the case reaches the path it is named for -- is asserted here, and so
are the argument checks PredictiveProjection makes before it touches an engine."""

import os
import sys

import numpy as np
import pytest

import projection_method_cases as pc

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden"))
import generate_projection_methods as gen  # noqa: E402  (input_digests / trace_digests: pure NumPy; the reference is imported by main() only)

FIXTURE = np.load(gen.PATH)
RECORDED = [str(n) for n in FIXTURE["cases"]]


def test_every_recordable_case_is_in_the_fixture():
    assert RECORDED == [n for n in pc.CASE_NAMES if pc.build(n).record]
    assert len(RECORDED) == len(pc.CASE_NAMES) >= 38


@pytest.mark.parametrize("name", RECORDED)
def test_the_case_is_the_one_that_was_recorded(name):
    """The builders are deterministic: the store, the first State and every argument of every call hash to what the recorder
    saw; the arguments kept in the fixture are the case's."""
    case = pc.build(name)
    assert np.array_equal(gen.input_digests(case), FIXTURE[f"{name}/inputs"])
    for i, call in enumerate(case.calls):
        for k in ("active", "learning", "winner"):
            if f"{name}/call{i}/{k}" in FIXTURE.files:
                assert np.array_equal(FIXTURE[f"{name}/call{i}/{k}"], call[k])
        for k in ("activation", "punish", "output_learning"):
            if f"{name}/call{i}/{k}" in FIXTURE.files:
                assert np.array_equal(np.unpackbits(FIXTURE[f"{name}/call{i}/{k}"])[:case.N].astype(np.bool_), call[k])


@pytest.mark.parametrize("name", RECORDED)
def test_oracle_gives_every_recorded_value(name):
    """After every call: seg_cell, seg_nsyn, segcount and the canonical synapses (permanences by their bits); after every
    process: every State field.  Exactly the reference's."""
    tr, _ = pc.oracle_trace(name)
    names, dig = gen.trace_digests(pc.build(name), tr)
    assert names == [str(n) for n in FIXTURE["field_names"]]
    want = FIXTURE[f"{name}/digests"]
    assert dig.shape == want.shape
    bad = np.argwhere(dig != want)
    assert len(bad) == 0, [(int(i), names[j]) for i, j in bad[:8]]
    assert len(tr[-1].store["seg_cell"]) == int(FIXTURE[f"{name}/segments"])


@pytest.mark.parametrize("name", pc.CASE_NAMES)
def test_the_case_reaches_the_path_it_is_named_for(name):
    pc.check_preconditions(name)


def test_learn_comes_before_grow_before_punish_on_one_row():
    """The order of projections.py:284-293 on a row that is in both sets, spelled out by hand for one synapse of each kind."""
    from oracle import TMParams, TemporalMemoryOracle
    p = TMParams(permanence_increment=0.02, permanence_decrement=0.03, permanence_punishment=0.07, segment_activation_threshold=2,
                 segment_matching_threshold=2, segment_sampling_synapses=4)
    c = pc.Case("by_hand", 64, 8, p, 8, 5)
    c.put_rows([9], [np.array([1, 2, 3, 4])], [np.array([0.06, 0.04, 0.5, 0.02], dtype=np.float32)])
    st = c.start([1, 2, 3])
    o = pc.fresh_oracle(c)
    punish = np.zeros(64, dtype=np.bool_)
    punish[9] = True
    o.update(st, np.isin(np.arange(64), [1, 2, 3, 40]), [9], punish, winner_input=np.array([40]))
    f32, f64 = np.float32, np.float64
    want = {1: f32(f64(f32(f64(f32(0.06)) + 0.02)) - 0.07),         # learned, then punished: stays (punished first it would be pruned)
            3: f32(f64(f32(f64(f32(0.5)) + 0.02)) - 0.07),
            40: f32(f64(f32(0.21)) - 0.07)}                          # grown by the learning step, active, punished
    # cell 2: 0.04 + 0.02 - 0.07 < 0, pruned by the two together; cell 4 (inactive): 0.02 - 0.03 < 0, pruned by learning
    got = {int(c_): o.perm[0][i] for i, c_ in enumerate(o.presyn[0]) if c_ >= 0}
    assert sorted(got) == sorted(want) and o.seg_nsyn[0] == 3
    assert all(got[k].view(np.int32) == want[k].view(np.int32) for k in want)


# ---- the argument checks of bithtm_amd.PredictiveProjection, made before an engine exists

def _projection(N=2048):
    import bithtm_amd as B
    return B.PredictiveProjection(N, segment_capacity=1024, segment_slots=32)


def _state(N, S=0):
    from types import SimpleNamespace
    return SimpleNamespace(prediction=np.zeros(N), segment_potential=np.zeros(S, np.int64), matching_segment=np.zeros(0, np.int64),
                           matching_segment_activation=np.zeros(0, np.int64), matching_segment_active=np.zeros(0, np.bool_),
                           max_jittered_potential=np.zeros(N, np.float32), matching_segment_jittered_potential=np.zeros(0, np.float32))


@pytest.mark.parametrize("learning,text", [([5, 9, 9, 30], "cell 9"), ([3, 2048], "2048"), ([-1, 4], "-1")],
                         ids=["repeated", "too-large", "negative"])
def test_update_refuses_bad_learning_output_before_any_engine_exists(learning, text):
    proj = _projection()
    z = np.zeros(2048, dtype=np.bool_)
    with pytest.raises(ValueError, match=text):
        proj.update(_state(2048), z, np.array(learning), z)
    assert proj._engine is None


@pytest.mark.parametrize("what", ["winner_input-repeated", "winner_input-range", "mask-length", "too-many-learning-cells"])
def test_update_refuses_other_bad_arguments_before_any_engine_exists(what):
    N = 65536 if what == "too-many-learning-cells" else 2048
    proj = _projection(N)
    z = np.zeros(N, dtype=np.bool_)
    kw = dict(prev_state=_state(N), input_activation=z, learning_output=np.array([1, 2]), output_punishment=z)
    if what == "winner_input-repeated":
        kw["winner_input"] = np.array([7, 8, 7])
    elif what == "winner_input-range":
        kw["winner_input"] = np.array([7, N])
    elif what == "mask-length":
        kw["output_punishment"] = np.zeros(N - 1, dtype=np.bool_)
    else:
        kw["learning_output"] = np.arange(pc.COUNT_LIMIT)
    with pytest.raises(ValueError):
        proj.update(**kw)
    assert proj._engine is None


@pytest.mark.parametrize("active,text", [([4, 7, 4], "cell 4"), ([0, 2048], "2048"), ([-3], "-3")], ids=["repeated", "too-large", "negative"])
def test_process_refuses_bad_active_input_before_any_engine_exists(active, text):
    proj = _projection()
    with pytest.raises(ValueError, match=text):
        proj.process(np.array(active))
    assert proj._engine is None
    with pytest.raises(ValueError):
        pc.fresh_oracle(pc.build("layout_1")).process(np.array([4, 7, 4]))
