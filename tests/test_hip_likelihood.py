"""Anomaly likelihood on the device (AnomalyLikelihood; htm_likelihood_*) against its definition,
bithtm_amd/likelihood.py.  Every comparison is exact: the likelihoods as their uint64 bit patterns, the exported state entry for
entry.  The stand-alone door (update_counts) runs the geometry cases of tests/likelihood_cases.py without stepping a model; the
model tests hold run(likelihood=), group.run(likelihood=) and group.tick(likelihood=) to the definition applied to the same
calls' counters, and the models themselves to the same calls without likelihood=."""
import numpy as np
import pytest

import likelihood_cases as cases
from likelihood_cases import P_SMALL, SIZES, SPLITS, SPLIT_IDS, as_kwargs
from live_tick_cases import EAGER, EAGER_IDS, SMALL
from test_hip_live_tick import _group, _model, _setenv
from test_hip_model_group import _banks, _same_state


# rows per bank: a sequence short enough that the small model learns it within the 60 scored steps (from its third pass on columns
# are predicted and the bursting count moves), and that divides 30, so two runs of 30 steps read the rows one run of 60 reads
ROWS = 10


def _bits(x):
    return np.ascontiguousarray(x, dtype=np.float64).view(np.uint64)


def _same_likelihood_state(lk, states, what=""):
    got, want = lk.state_dict(), cases.stacked_state(states)
    for key in want:
        assert got[key].dtype == want[key].dtype and np.array_equal(got[key], want[key]), (what, key)


def _update_in_calls(lk, active, bursting, splits):
    parts, at = [], 0
    for n in splits:
        parts.append(lk.update_counts(active[:, at:at + n], bursting[:, at:at + n], device=0))
        at += n
    return np.concatenate(parts, axis=1)


# ---- the stand-alone door: every split x B, a different stream per member
@pytest.mark.gpu
@pytest.mark.parametrize("B", SIZES)
@pytest.mark.parametrize("name,pname,splits", SPLITS, ids=SPLIT_IDS)
def test_update_counts_equals_the_definition(name, pname, splits, B):
    import bithtm_amd as Bm
    params = cases.PARAMS[pname]
    active, bursting = cases.member_streams(B, sum(splits), seed=len(name))
    want, states = cases.reference(params, active, bursting)
    lk = Bm.AnomalyLikelihood(B, **as_kwargs(params))
    got = _update_in_calls(lk, active, bursting, splits)
    assert got.shape == want.shape and got.dtype == np.float64
    wrong = np.argwhere(_bits(got) != _bits(want))
    assert not len(wrong), (name, B, len(wrong), wrong[:5].tolist(), [(got[i, j], want[i, j]) for i, j in wrong[:5]])
    _same_likelihood_state(lk, states, name)


@pytest.mark.gpu
@pytest.mark.parametrize("stream", cases.STREAMS)
def test_every_stream_alone_equals_the_definition(stream):
    """B = 1 (the record pointer goes by value): each stream under each parameter set, in ragged calls."""
    import bithtm_amd as Bm
    for pname, splits in (("P_small", [3, 1, 16, 17, 40]), ("P_small", [cases.CHUNK + 1]), ("P_every", [1, 1, 62, 3, 64, 200]),
                          ("P_wide", [14, 1, 600])):
        params = cases.PARAMS[pname]
        for seed in (0, 1):
            active, bursting = cases.stream(stream, sum(splits), seed)
            want, states = cases.reference(params, active[None], bursting[None])
            lk = Bm.AnomalyLikelihood(1, **as_kwargs(params))
            got = _update_in_calls(lk, active[None], bursting[None], splits)
            assert np.array_equal(_bits(got), _bits(want)), (stream, pname, seed)
            _same_likelihood_state(lk, states, (stream, pname))
    # a one-dimensional call of one stream gives a one-dimensional answer
    lk = Bm.AnomalyLikelihood(**as_kwargs(P_SMALL))
    active, bursting = cases.stream(stream, 20)
    assert np.array_equal(_bits(lk.update_counts(active, bursting, device=0)), _bits(cases.reference(P_SMALL, active[None], bursting[None])[0][0]))


# ---- a model
def _defined(rec, splits=None):
    """The definition over a RunRecord's counters."""
    return cases.reference(P_SMALL, rec.active_columns[None].astype(np.int64), rec.bursting_columns[None].astype(np.int64), splits)


def _same_counters(a, b, what):
    from bithtm_amd.engine import RECORD_COUNTERS
    assert np.array_equal(a.step_index, b.step_index), what
    for name in RECORD_COUNTERS:
        assert np.array_equal(getattr(a, name), getattr(b, name)), (what, name)


def _pair(seed):
    m, twin = _model(SMALL, seed), _model(SMALL, seed)
    twin.engine.set_permanence(m.engine.get_permanence())
    return m, twin


@pytest.mark.gpu
def test_a_run_with_a_likelihood_equals_the_definition_over_its_counters():
    import bithtm_amd as Bm
    bank = _banks(1, ROWS, SMALL[0], 5, density=0.1)[0]
    m, twin = _pair(11)
    lk = Bm.AnomalyLikelihood(1, **as_kwargs(P_SMALL))
    rec = m.run(bank, 60, likelihood=lk)
    plain = twin.run(bank, 60, record=True)
    _same_counters(rec, plain, "scored against plain")                 # the model is untouched by the scoring
    _same_state(m, twin, "scored against plain")
    assert plain.anomaly_likelihood is None and rec.anomaly_likelihood.shape == (60,) and rec.anomaly_likelihood.dtype == np.float64
    want, states = _defined(rec)
    assert np.array_equal(_bits(rec.anomaly_likelihood), _bits(want[0]))
    assert (want[0][:7] == 0.5).all() and len(set(want[0][7:].tolist())) > 3          # (the comparison is of something)
    assert np.array_equal(rec.log_likelihood, Bm.likelihood.log_likelihood(want[0]))
    _same_likelihood_state(lk, states)
    # two runs of 30 steps equal one run of 60, with other fields recorded beside the counters
    m2, _ = _pair(11)
    lk2 = Bm.AnomalyLikelihood(1, **as_kwargs(P_SMALL))
    first = m2.run(bank, 30, likelihood=lk2, record=("active_column",))
    second = m2.run(bank, 30, likelihood=lk2)
    assert first.active_column.shape == (30, SMALL[3]) and first.active_columns is not None
    assert np.array_equal(_bits(np.concatenate([first.anomaly_likelihood, second.anomaly_likelihood])), _bits(want[0]))
    _same_likelihood_state(lk2, states)
    # the model's reset leaves the likelihood's state alone
    m2.reset()
    _same_likelihood_state(lk2, states)
    # an inference view gives its own stream's likelihood
    view, lkv = m.inference_view(), Bm.AnomalyLikelihood(1, **as_kwargs(P_SMALL))
    recv = view.run(bank, 40, likelihood=lkv)
    want_v, states_v = _defined(recv)
    assert np.array_equal(_bits(recv.anomaly_likelihood), _bits(want_v[0]))
    _same_likelihood_state(lkv, states_v)
    with pytest.raises(ValueError, match="one stream"):
        m.run(bank, 1, likelihood=Bm.AnomalyLikelihood(2))
    assert m.run(bank, 0, likelihood=lk).anomaly_likelihood.shape == (0,)


# ---- groups
@pytest.mark.gpu
@pytest.mark.parametrize("B", [3, 5])
def test_a_group_run_with_a_likelihood_equals_every_members_solo_run(B):
    import bithtm_amd as Bm
    banks = _banks(B, ROWS, SMALL[0], 7, density=0.1)
    group, twins, _ = _group(SMALL, B)
    plain_group, _, _ = _group(SMALL, B)
    lk = Bm.AnomalyLikelihood(B, **as_kwargs(P_SMALL))
    recs = group.run(banks, 60, likelihood=lk)
    plain = plain_group.run(banks, 60, record=True)
    states = []
    for i, t in enumerate(twins):
        solo_lk = Bm.AnomalyLikelihood(1, **as_kwargs(P_SMALL))
        solo = t.run(banks[i], 60, likelihood=solo_lk)
        _same_counters(recs[i], solo, f"member {i}")
        _same_counters(recs[i], plain[i], f"member {i} against the run without likelihood=")
        want, st = _defined(solo)
        assert np.array_equal(_bits(recs[i].anomaly_likelihood), _bits(solo.anomaly_likelihood)), i
        assert np.array_equal(_bits(recs[i].anomaly_likelihood), _bits(want[0])), i
        _same_state(group.models[i], t, f"member {i}")
        _same_state(group.models[i], plain_group.models[i], f"member {i} against the run without likelihood=")
        states += st
    _same_likelihood_state(lk, states)
    assert len({r.anomaly_likelihood.tobytes() for r in recs}) == B                    # (every member its own stream)
    # resets: the models' leave the likelihood alone; the likelihood's own restart only the flagged streams
    group.reset()
    group.models[0].reset()
    _same_likelihood_state(lk, states)
    mask = np.arange(B) % 2 == 0
    lk.reset(mask)
    more = group.run(banks, 20, likelihood=lk)
    for i, t in enumerate(twins):
        t.reset()
        solo = t.run(banks[i], 20, record=True)
        _same_counters(more[i], solo, f"member {i} after the resets")
        if mask[i]:
            want = _defined(solo)[0][0]
        else:
            both = cases.reference(P_SMALL, np.concatenate([recs[i].active_columns, solo.active_columns])[None].astype(np.int64),
                                   np.concatenate([recs[i].bursting_columns, solo.bursting_columns])[None].astype(np.int64))[0][0]
            want = both[60:]
        assert np.array_equal(_bits(more[i].anomaly_likelihood), _bits(want)), (i, bool(mask[i]))
    assert lk.state_dict()["t"].tolist() == [20 if f else 80 for f in mask]
    # the state's round trip: an object loaded from state_dict() continues as the original does
    saved = lk.state_dict()
    other = Bm.AnomalyLikelihood(B, **as_kwargs(P_SMALL))
    other.load_state_dict(saved)                    # (not bound yet: applied when it is)
    active, bursting = cases.member_streams(B, 25, seed=3)
    a, b = lk.update_counts(active, bursting), other.update_counts(active, bursting, device=0)
    assert np.array_equal(_bits(a), _bits(b))
    x, y = lk.state_dict(), other.state_dict()
    assert all(np.array_equal(x[k], y[k]) for k in x) and x["t"].tolist() == [45 if f else 105 for f in mask]
    other.load_state_dict(saved)                    # (bound: imported at once)
    z = other.state_dict()
    assert all(np.array_equal(z[k], saved[k]) for k in saved)
    with pytest.raises(ValueError, match="streams"):
        group.run(banks, 1, likelihood=Bm.AnomalyLikelihood(B + 1))
    with pytest.raises(ValueError, match="streams"):
        group.tick(banks[:, 0], likelihood=Bm.AnomalyLikelihood(B + 1))


@pytest.mark.gpu
@pytest.mark.parametrize("env", EAGER, ids=EAGER_IDS)
@pytest.mark.parametrize("B", [3, 5])
def test_scored_ticks_equal_the_scored_run(B, env, monkeypatch):
    """60 scored ticks against group.run(likelihood=) over the same rows, and against 60 ticks without likelihood=."""
    import bithtm_amd as Bm
    _setenv(env, monkeypatch)
    banks = _banks(B, ROWS, SMALL[0], 7, density=0.1)
    ran, _, _ = _group(SMALL, B)
    ticked, _, _ = _group(SMALL, B)
    plain, _, _ = _group(SMALL, B)
    lk_run, lk_tick = (Bm.AnomalyLikelihood(B, **as_kwargs(P_SMALL)) for _ in range(2))
    recs = ran.run(banks, 60, likelihood=lk_run)
    want = np.stack([r.anomaly_likelihood for r in recs])
    got = np.zeros_like(want)
    for n in range(60):
        rows = banks[:, n % ROWS]
        tick = ticked.tick(rows, likelihood=lk_tick, predicted_input=n % 7 == 3)
        bare = plain.tick(rows, predicted_input=n % 7 == 3)
        assert tick.anomaly_likelihood.shape == (B,) and tick.anomaly_likelihood.dtype == np.float64 and bare.anomaly_likelihood is None
        got[:, n] = tick.anomaly_likelihood
        for i in range(B):
            assert tick.bursting_columns[i] == recs[i].bursting_columns[n] == bare.bursting_columns[i], (n, i)
            assert tick.active_columns[i] == recs[i].active_columns[n] and tick.step_index[i] == bare.step_index[i] == n
        if tick.predicted_input is not None:
            assert np.array_equal(tick.predicted_input, bare.predicted_input)
    assert np.array_equal(_bits(got), _bits(want))
    x, y = lk_run.state_dict(), lk_tick.state_dict()
    assert all(np.array_equal(x[k], y[k]) for k in x)
    for i in range(B):
        _same_state(ticked.models[i], ran.models[i], f"member {i}: ticks against the run")
        _same_state(ticked.models[i], plain.models[i], f"member {i}: ticks against ticks without likelihood=")


@pytest.mark.gpu
def test_the_example_prints_the_likelihood_column_only_when_asked():
    """example.py --batched_report: with --likelihood every line gains the step's likelihood -- one stream over all epochs, equal
    to the definition over the printed bursting counts -- and without it the output is what it was."""
    import io
    import re
    from bithtm_amd import example
    from bithtm_amd.likelihood import define
    args = ["--epochs", "16", "--input_patterns", "30", "--input_dim", "200", "--column_dim", "2048", "--cell_dim", "8", "--batched_report"]
    outs = []
    for extra in ([], ["--likelihood"]):
        np.random.seed(3)
        out = io.StringIO()
        example.main(args + extra, out=out)
        outs.append(out.getvalue().splitlines()[:-1])              # (the last line is the wall time)
    plain, scored = outs
    assert len(plain) == len(scored) == 480 and not any("likelihood" in x for x in plain)
    assert [x.split(", anomaly likelihood: ")[0] for x in scored] == plain
    bursting = np.array([int(re.search(r"bursting columns: +(\d+)", x).group(1)) for x in plain])
    correct = np.array([int(re.search(r"correct columns: +(\d+)", x).group(1)) for x in plain])
    want, _ = define(bursting + correct, bursting)                 # NuPIC's defaults: probation ends at step 388
    got = [x.split(", anomaly likelihood: ")[1] for x in scored]
    assert got == [f"{v:.6f}" for v in want] and set(got[:387]) == {"0.500000"} and set(got[387:]) != {"0.500000"}
    with pytest.raises(SystemExit, match="--batched_report"):
        example.main(args[:-1] + ["--likelihood"], out=io.StringIO())


@pytest.mark.gpu
def test_a_scored_group_run_crosses_pool_growth_and_the_object_outlives_the_group():
    """Members on streams of their own with default-sized pools and inputs that never repeat (tests/test_hip_model_group.py's growth
    case): between two batches of the scored run every member is re-created -- its old handle destroyed with its stream, its record
    buffers new -- and the likelihood goes on through the new handles; then the group and its models go, and the object continues
    through a handle of its own.  All of it equals the definition over the run's counters followed by the further counts."""
    import gc
    import weakref
    import bithtm_amd as Bm
    from test_hip_model_group import _group as _plain_group
    size, B, steps = (1000, 2048, 32, None), 3, 400
    group, twins, _ = _plain_group(size, B)
    first = [weakref.ref(m.engine) for m in group.models]               # (weak: the old handles must really go)
    cap0 = group.models[0].engine.segment_capacity
    assert len({m.engine.stream_handle() for m in group.models}) == B   # (streams of their own: the group's is member 0's)
    inputs = _banks(B, steps, size[0], 8)
    lk = Bm.AnomalyLikelihood(B, **as_kwargs(P_SMALL))
    recs = group.run(inputs, steps, likelihood=lk)
    gc.collect()
    assert all(r() is None for r in first) and group.models[0].engine.segment_capacity > cap0
    active = np.stack([r.active_columns for r in recs]).astype(np.int64)
    bursting = np.stack([r.bursting_columns for r in recs]).astype(np.int64)
    want, states = cases.reference(P_SMALL, active, bursting)
    assert np.array_equal(_bits(np.stack([r.anomaly_likelihood for r in recs])), _bits(want))
    _same_likelihood_state(lk, states)
    for i, t in enumerate(twins):                                       # the models are what they are without likelihood=
        t.run(inputs[i], steps)
        _same_state(group.models[i], t, f"member {i}")
    del group, twins, t, recs
    gc.collect()
    more_a, more_b = cases.member_streams(B, 70, seed=5)
    got = lk.update_counts(more_a, more_b)                              # (no model left: through the object's own handle)
    both, states = cases.reference(P_SMALL, np.concatenate([active, more_a], axis=1), np.concatenate([bursting, more_b], axis=1))
    assert np.array_equal(_bits(got), _bits(both[:, steps:]))
    _same_likelihood_state(lk, states)
