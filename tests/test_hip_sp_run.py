"""Batched stand-alone Spatial Pooler runs (include/bithtm_hip.h: htm_sp_run): SpatialPooler.run over a
device bank against the same steps taken one by one with process() and against the oracle -- every record field and the whole
state left behind, bit for bit --; how calls compose; what recording costs; graph reuse; device-side noise; the hand-over to
TemporalMemory.run; the refusals; and that a fused model beside it is untouched.

Shapes (input_dim, column_dim, active_columns): (33, 257, 5) -- two input words with one live bit in the second, one column in
the second 256-block, overlaps of at most 33 so that ties across the k-th place are the rule; (777, 3000, 60) -- nothing a
multiple of 32 or 256; (100, 2048, 300) -- k above 256: two record blocks, the second partly idle."""

import ctypes as C
import gc
from types import SimpleNamespace

import numpy as np
import pytest

from oracle import SpatialPoolerOracle
from oracle.htm_oracle import topk_is_unambiguous

pytestmark = pytest.mark.gpu

SHAPES = [(33, 257, 5), (777, 3000, 60), (100, 2048, 300)]
SHAPE_IDS = ["33x257x5", "777x3000x60", "100x2048x300"]
ALL = ("active_column", "active_overlap", "active_boosted")
ROWS, STEPS = 7, 150                # (7 rows: co-prime to the 16-step graph span, so rows and parities mix)


def _inputs(I, seed=11):
    return np.random.RandomState(seed).rand(ROWS, I) < 0.2


def _poolers(I, Cn, k, count=2, seed=1, **kw):
    import bithtm_amd as B
    out = []
    for _ in range(count):
        np.random.seed(seed)                    # (the permanences are drawn from NumPy's global stream)
        out.append(B.SpatialPooler(I, Cn, k, **kw))
    return out


def _assert_same_sp(a, b, what=""):
    """Permanence rows, duty cycle, step index (the binding's and the device's)."""
    assert np.array_equal(a.proximal_projection.permanence.view(np.int64), b.proximal_projection.permanence.view(np.int64)), what
    assert np.array_equal(a.boosting.duty_cycle.view(np.int32), b.boosting.duty_cycle.view(np.int32)), what
    assert a._engine.steps == b._engine.steps and a._engine.info().step_index == b._engine.info().step_index == a._engine.steps, what


def _assert_same_step(a, b, x, what=""):
    """One more process(x) on both: the three State fields (the overlap reads every mask row, so this also compares the masks)."""
    sa, sb = a.process(x), b.process(x)
    assert np.array_equal(sa.active_column, sb.active_column), what
    assert np.array_equal(sa.overlaps, sb.overlaps), what
    assert np.array_equal(sa.boosted_overlaps.view(np.int64), sb.boosted_overlaps.view(np.int64)), what


def _assert_same_record(r, s, what=""):
    assert r.fields == s.fields and np.array_equal(r.step_index, s.step_index), what
    for f in r.fields:
        x, y = getattr(r, f), getattr(s, f)
        assert x.dtype == y.dtype and x.shape == y.shape, (what, f)
        assert np.array_equal(x.view(np.int64) if x.dtype == np.float64 else x, y.view(np.int64) if y.dtype == np.float64 else y), (what, f)


def _assert_record_is(rec, states, start, k, what=""):
    """`rec` (all three fields) against the States of process() / the oracle's steps."""
    n = len(states)
    assert rec.fields == ALL and np.array_equal(rec.step_index, start + np.arange(n)) and rec.step_index.dtype == np.int64
    assert rec.active_column.dtype == np.int32 and rec.active_overlap.dtype == np.int32 and rec.active_boosted.dtype == np.float64
    assert rec.active_column.shape == rec.active_overlap.shape == rec.active_boosted.shape == (n, k)
    for i, st in enumerate(states):
        cols = np.asarray(st.active_column)
        assert np.array_equal(rec.active_column[i], cols), (what, i)
        assert np.array_equal(rec.active_overlap[i], np.asarray(st.overlaps)[cols]), (what, i)
        assert np.array_equal(rec.active_boosted[i].view(np.int64), np.asarray(st.boosted_overlaps)[cols].view(np.int64)), (what, i)


@pytest.mark.parametrize("eager", [False, True], ids=["graph", "eager"])
@pytest.mark.parametrize("learning", [True, False], ids=["learning", "frozen"])
@pytest.mark.parametrize("shape", SHAPES, ids=SHAPE_IDS)
def test_run_equals_stepwise(shape, learning, eager, monkeypatch):
    """run(inputs, 150) == 150 process() calls: permanences, duty cycle, step index, and the State of the step after."""
    if eager:
        monkeypatch.setenv("BITHTM_EAGER_BELOW", "1000000")
    I, Cn, k = shape
    inputs = _inputs(I)
    sp, twin = _poolers(I, Cn, k)
    assert sp.run(inputs, STEPS, learning=learning) is None
    for t in range(STEPS):
        twin.process(inputs[t % ROWS], learning=learning)
    assert (sp._engine.graph_count() == 0) == eager
    _assert_same_sp(sp, twin)
    _assert_same_step(sp, twin, inputs[STEPS % ROWS])
    _assert_same_sp(sp, twin, "after the next step")


@pytest.mark.parametrize("shape", SHAPES, ids=SHAPE_IDS)
def test_run_equals_the_oracle(shape):
    """150 steps, learning off on every seventh: runs of the matching lengths and flags, all three record fields, the final
    permanences and duty cycle against the oracle.  On (33, 257, 5) the lower-index-first policy must have decided a step."""
    I, Cn, k = shape
    inputs = _inputs(I)
    sp, = _poolers(I, Cn, k, 1)
    ora = SpatialPoolerOracle(I, Cn, k, permanence=sp.proximal_projection.permanence.copy())
    flags = [t % 7 != 3 for t in range(STEPS)]
    want = [ora.step(inputs[t % ROWS], learning=flags[t]) for t in range(STEPS)]
    t = 0
    while t < STEPS:
        n = 1
        while t + n < STEPS and flags[t + n] == flags[t]:
            n += 1
        rec = sp.run(inputs, n, learning=flags[t], record=ALL)
        _assert_record_is(rec, want[t:t + n], t, k, f"steps {t}..{t + n - 1}")
        t += n
    assert np.array_equal(sp.proximal_projection.permanence.view(np.int64), ora.permanence.view(np.int64))
    assert np.array_equal(sp.boosting.duty_cycle.view(np.int32), ora.duty_cycle.view(np.int32))
    if shape == SHAPES[0]:
        assert any(not topk_is_unambiguous(w.boosted_overlaps, k) for w in want)


@pytest.mark.parametrize("shape", SHAPES, ids=SHAPE_IDS)
def test_calls_compose_and_records_belong_to_their_call(shape):
    I, Cn, k = shape
    inputs = _inputs(I)
    sp, one = _poolers(I, Cn, k)
    whole = one.run(inputs, STEPS, record=ALL)
    parts, at = [], 0
    for n in (40, 0, 1, 109):
        rec = sp.run(inputs, n, record=ALL)
        assert len(rec) == n and np.array_equal(rec.step_index, at + np.arange(n)) and rec.active_column.shape == (n, k)
        parts.append(rec)
        at += n
    assert np.array_equal(whole.step_index, np.arange(STEPS))
    for f in ALL:
        joined = np.concatenate([getattr(p, f) for p in parts])
        assert joined.tobytes() == getattr(whole, f).tobytes() and joined.shape == getattr(whole, f).shape, f
    assert (np.diff(whole.active_column, axis=1) > 0).all()                     # ascending
    _assert_same_sp(sp, one)
    only, ref = sp.run(inputs, 9, record="active_overlap"), one.run(inputs, 9, record=ALL)
    assert only.fields == ("active_overlap",) and only.active_column is None and only.active_boosted is None
    assert np.array_equal(only.active_overlap, ref.active_overlap) and np.array_equal(only.step_index, STEPS + np.arange(9))
    first = sp.run(inputs, 5, record=True)
    assert first.fields == ("active_column",) and np.array_equal(first.active_column, one.run(inputs, 5, record=ALL).active_column)


def _launches(sp, inputs, steps, **kw):
    eng = sp._ensure_engine()
    eng.profile(True)
    out = sp.run(inputs, steps, **kw)
    prof = eng.profile_read()
    eng.profile(False)
    return {name: cnt for name, (_, cnt) in prof.items() if cnt}, out       # (a name stays listed, with 0, once it was launched)


@pytest.mark.parametrize("shape", SHAPES, ids=SHAPE_IDS)
def test_recording_changes_nothing_and_costs_no_launch(shape):
    I, Cn, k = shape
    inputs = _inputs(I)
    rec, plain = _poolers(I, Cn, k)
    rec.run(inputs, 60, record=ALL)
    plain.run(inputs, 60)
    rec.run(inputs, 30, learning=False, record=ALL)
    plain.run(inputs, 30, learning=False)
    _assert_same_sp(rec, plain)
    _assert_same_step(rec, plain, inputs[90 % ROWS])
    with_rec, _ = _launches(rec, inputs, 10, record=ALL)
    without, _ = _launches(plain, inputs, 10)
    assert with_rec == without and with_rec["sp_run_tail"] == 10, (with_rec, without)
    with_rec, _ = _launches(rec, inputs, 10, learning=False, record=ALL)
    without, _ = _launches(plain, inputs, 10, learning=False)
    assert sum(with_rec.values()) == sum(without.values()) + 10, (with_rec, without)
    assert with_rec["sp_run_tail"] == 10 and "sp_run_tail" not in without and "sp_learn" not in without
    assert {n: c for n, c in with_rec.items() if n != "sp_run_tail"} == without
    _assert_same_sp(rec, plain)


def test_graphs_are_captured_once():
    I, Cn, k = SHAPES[1]
    inputs = _inputs(I)
    sp, = _poolers(I, Cn, k, 1)
    sp.run(inputs, STEPS)
    eng = sp._engine
    g = eng.graph_count()
    assert g > 0
    sp.run(inputs, STEPS)
    assert eng.graph_count() == g
    sp.run(inputs, STEPS, record=ALL)
    g_rec = eng.graph_count()
    assert g_rec > g
    before = {f: eng._record_bufs["sp_" + f][0] for f in ALL}
    sp.run(inputs, 4 * STEPS, record=ALL)                       # (more steps than the buffers held: other buffers)
    assert all(eng._record_bufs["sp_" + f][0] != before[f] for f in ALL)
    assert eng.graph_count() == g_rec
    sp.run(inputs, STEPS, learning=False)
    assert eng.graph_count() > g_rec


@pytest.mark.parametrize("shape", SHAPES, ids=SHAPE_IDS)
def test_noise_equals_the_explicit_bank(shape):
    """run(noise=0.05) in fills of 32 steps (the ring of 34 rows wraps) == the run over the 150 rows flipped on the host."""
    from bithtm_amd.networks import flip_noise
    I, Cn, k = shape
    inputs = _inputs(I)
    noisy, explicit = _poolers(I, Cn, k)
    noisy.noise_chunk = 32
    rows = np.stack([inputs[t % ROWS] ^ flip_noise(9, t, I, 0.05) for t in range(STEPS)])
    assert (rows != np.stack([inputs[t % ROWS] for t in range(STEPS)])).any()
    got = noisy.run(inputs, STEPS, record=ALL, noise=0.05, noise_seed=9)
    want = explicit.run(rows, STEPS, record=ALL)
    _assert_same_record(got, want)
    _assert_same_sp(noisy, explicit)
    _assert_same_step(noisy, explicit, inputs[0])


def test_zero_noise_is_the_run_without_noise():
    I, Cn, k = SHAPES[1]
    inputs = _inputs(I)
    zero, plain = _poolers(I, Cn, k)
    for sp in (zero, plain):                    # (both handles exist before either steps: the same select form on both)
        sp._ensure_engine()
    a, _ = _launches(zero, inputs, 10, noise=0.0, noise_seed=3)
    b, _ = _launches(plain, inputs, 10)
    assert a == b
    zero.run(inputs, STEPS, noise=0.0)
    plain.run(inputs, STEPS)
    assert zero._engine.graph_count() == plain._engine.graph_count() > 0
    _assert_same_sp(zero, plain)


def test_record_hands_over_to_tm_run():
    import bithtm_amd as B
    from test_hip_tm_run import _assert_same_tm
    I, Cn, k = SHAPES[1]
    inputs = _inputs(I)
    sp, = _poolers(I, Cn, k, 1)
    rec = sp.run(inputs, 64, record=True)
    tm, twin = B.TemporalMemory(Cn, 8, seed=5), B.TemporalMemory(Cn, 8, seed=5)
    tm.run(rec.active_column, 64)
    for row in rec.active_column:
        twin.process(SimpleNamespace(active_column=row))
    _assert_same_tm(tm, twin)
    assert tm._engine.info().segments > 0


def test_refusals():
    import bithtm_amd as B
    from bithtm_amd import _lib as L
    from bithtm_amd.engine import HtmError
    from test_hip_run_record import _twins
    from test_hip_sequence_reset import _assert_same_state
    I, Cn, k = SHAPES[1]
    inputs = _inputs(I)
    # a handle with a Temporal Memory; its fused pooler
    htm, htm_twin = _twins(I, Cn, 8, active_columns=k)
    for m in (htm, htm_twin):
        m.run(inputs, 5)
    eng = htm.engine
    bank = eng.upload_bank(inputs)
    with pytest.raises(HtmError, match=r"\(-4\).*use htm_run"):
        eng.sp_run(bank, ROWS, 4)
    with pytest.raises(ValueError, match=r"call its run\(\)"):
        htm.spatial_pooler.run(inputs, 4)
    assert eng.steps == 5 and eng.info().step_index == 5
    for m in (htm, htm_twin):
        m.run(inputs, 20)
    _assert_same_state(htm, htm_twin)
    # a Spatial Pooler's own handle: a wrong struct_bytes, no buffer, n_inputs = 0, a null bank, n_steps < 0
    sp, twin = _poolers(I, Cn, k)
    sp.run(inputs, 5)
    eng = sp._engine
    bank = eng.upload_bank(inputs)
    buf = eng.device_buffer(4 * 4 * k)
    rec = L.HtmSpRunRecord()
    rec.struct_bytes, rec.active_column = C.sizeof(L.HtmSpRunRecord) - 1, buf
    assert eng.lib.htm_sp_run(eng.h, C.c_void_p(bank), ROWS, 4, 1, 1, C.byref(rec)) == -1
    assert b"struct_bytes" in eng.lib.htm_last_error(eng.h)
    rec.struct_bytes, rec.active_column = C.sizeof(L.HtmSpRunRecord), None
    assert eng.lib.htm_sp_run(eng.h, C.c_void_p(bank), ROWS, 4, 1, 1, C.byref(rec)) == -1
    assert b"no record buffer" in eng.lib.htm_last_error(eng.h)
    with pytest.raises(HtmError, match=r"\(-1\).*n_inputs"):
        eng.sp_run(bank, 0, 4)
    with pytest.raises(HtmError, match=r"\(-1\).*n_steps"):
        eng.sp_run(bank, ROWS, -1)
    with pytest.raises(HtmError, match=r"\(-1\).*null bank"):
        eng.sp_run(None, ROWS, 4)
    eng.lib.hipFree(C.c_void_p(buf))
    assert eng.steps == 5 and eng.info().step_index == 5 and eng.sp_run(bank, ROWS, 0) is None and eng.steps == 5
    for t in range(5):
        twin.process(inputs[t % ROWS])
    _assert_same_sp(sp, twin)
    got = sp.run(inputs, 30, record=ALL)
    _assert_record_is(got, [twin.process(inputs[t % ROWS]) for t in range(5, 35)], 5, k, "after the refusals")
    _assert_same_sp(sp, twin)

    # a plug-in pooler steps on the host
    class Projection(B.DenseProjection):
        pass
    np.random.seed(3)
    plug = B.SpatialPooler(I, Cn, k, proximal_projection=Projection(I, Cn))
    np.random.seed(3)
    plug_twin = B.SpatialPooler(I, Cn, k, proximal_projection=Projection(I, Cn))
    plug.process(inputs[0])
    plug_twin.process(inputs[0])
    with pytest.raises(ValueError, match=r"call process\(\)"):
        plug.run(inputs, 4)
    for t in range(1, 4):
        a, b = plug.process(inputs[t]), plug_twin.process(inputs[t])
        assert np.array_equal(a.active_column, b.active_column) and np.array_equal(a.overlaps, b.overlaps)


def test_a_fused_model_beside_it_is_untouched():
    """A fused model's run() interleaved with sp.run on another handle of the same device: the state of a twin that never had
    the neighbour (the handle registry and the exchange mode are shared per process)."""
    from test_hip_run_record import _twins
    I, Cn, k = SHAPES[1]
    inputs = _inputs(I)
    twin = _twins(I, Cn, 8, active_columns=k)[0]                # (alone on the device: the other of the pair is gone at once)
    gc.collect()
    twin.run(inputs, 64)
    twin.run(inputs, 64)
    twin_state = twin.state_dict()
    del twin
    gc.collect()
    htm = _twins(I, Cn, 8, active_columns=k)[0]
    gc.collect()
    htm.run(inputs, 64)
    sp, alone = _poolers(I, Cn, k)
    rec = sp.run(inputs, 40, record=ALL)
    htm.run(inputs, 64)
    got = htm.state_dict()
    for key in twin_state:
        assert np.array_equal(np.asarray(got[key]), np.asarray(twin_state[key])), key
    del htm
    gc.collect()
    _assert_same_record(rec, alone.run(inputs, 40, record=ALL))     # (and the pooler's run is that of a pooler alone)
    _assert_same_sp(sp, alone)
