"""CPU: the pure pieces of the host-side batched-run loop -- the size rule of a device-side batch (networks.batch_steps), the loop
that cuts a call into batches (networks._batches) and the constructor of a State that never was on a device (_Lazy._eager).
The expected sizes are written out as the expressions the six run loops each had before they shared the rule."""

import numpy as np
import pytest

from bithtm_amd.networks import SpatialPooler, TemporalMemory, _batches, batch_steps


def single(left, free, k, cap=None):
    """HierarchicalTemporalMemory.run / TemporalMemory.run / ModelGroup.run: max(1, min(left, free // (2 k) - 1)), then the
    caller's cap (noise_chunk)."""
    n = max(1, min(left, free // (2 * k) - 1))
    return n if cap is None else min(n, cap)


def stacked(left, chunk, free, k, period, S):
    """RegionStack.run: min(chunk, left), then per level min(n, max(S, (free // (2 k) - 1) * period // S * S))."""
    n = min(chunk, left)
    return min(n, max(S, (free // (2 * k) - 1) * period // S * S))


@pytest.mark.parametrize("k", [1, 5, 40])
def test_batch_size_around_the_free_segment_edges(k):
    # free segments 0, just below / at / above 2 k, and at the next multiples, where the quotient steps
    for free in (0, 1, 2 * k - 1, 2 * k, 2 * k + 1, 4 * k - 1, 4 * k, 4 * k + 1, 6 * k, 1000 * k + 3):
        for left in (1, 2, 7, 10 ** 6):
            want = single(left, free, k)
            assert batch_steps(left, free, 2 * k) == want, (left, free, k)
            assert want >= 1                                # (the run gets on even with a full pool)
    assert batch_steps(50, 0, 2 * k) == 1 and batch_steps(50, 2 * k, 2 * k) == 1 and batch_steps(50, 4 * k, 2 * k) == 1
    assert batch_steps(50, 6 * k, 2 * k) == 2 and batch_steps(1, 6 * k, 2 * k) == 1


def test_batch_size_with_a_cap_below_and_above_the_rule():
    k, free = 5, 400                                        # the rule alone: 400 // 10 - 1 = 39
    assert batch_steps(100, free, 2 * k) == 39
    for cap in (1, 4, 38, 39, 40, 1024):
        for left in (1, 20, 39, 100):
            assert batch_steps(left, free, 2 * k, cap=cap) == single(left, free, k, cap), (left, cap)
    assert batch_steps(100, free, 2 * k, cap=4) == 4 and batch_steps(100, free, 2 * k, cap=1024) == 39
    # no pool to look at (a fixed capacity, a forecast): the steps left, or the cap
    assert batch_steps(100) == 100 and batch_steps(100, cap=16) == 16 and batch_steps(3, cap=16) == 3 and batch_steps(1) == 1


@pytest.mark.parametrize("S,period", [(1, 1), (4, 1), (4, 2), (4, 4), (6, 3)])
def test_batch_size_rounds_to_the_strides_product(S, period):
    k = 3
    for free in (0, 5, 6, 7, 12, 30, 31, 66, 600):
        for chunk, left in ((S, S), (4 * S, 8 * S), (64 * S, 16 * S), (16 * S, 64 * S)):
            want = stacked(left, chunk, free, k, period, S)
            got = batch_steps(batch_steps(left, cap=chunk), free, 2 * k, period=period, multiple=S)
            assert got == want, (free, chunk, left)
            assert got % S == 0 and got >= S
    if S == 4 and period == 1:
        assert batch_steps(64, 66, 2 * k, period=1, multiple=4) == 8        # (66 // 6 - 1) = 10 level-0 steps -> 8
        assert batch_steps(64, 0, 2 * k, period=1, multiple=4) == 4         # a full pool: one window all the same
    if S == 4 and period == 4:
        assert batch_steps(64, 30, 2 * k, period=4, multiple=4) == 16       # 4 steps of the top level = 16 inputs


def test_batches_cut_a_call_as_the_loops_did():
    # a forecast: chunks of the cap, nobody looks at a pool
    assert list(_batches(10, cap=4)) == [(0, 4), (4, 4), (8, 2)]
    assert list(_batches(0, cap=4)) == [] and list(_batches(3)) == [(0, 3)]


def test_batches_sizes_with_a_growing_pool():
    answers = [400, 70, 0, 400, 400]                        # what the look before each batch finds free
    free, looks = iter(answers), []

    def pools():
        looks.append(None)
        return [(next(free), 10, 1)]
    got = list(_batches(60, pools, cap=20))
    assert len(looks) == len(got) == 5                      # (one look per batch, made before it)
    want, done = [], 0
    for f in answers:
        if done >= 60:
            break
        n = single(60 - done, f, 5, 20)
        want.append((done, n))
        done += n
    assert got == want == [(0, 20), (20, 6), (26, 1), (27, 20), (47, 13)]
    # two pools (a stack's levels): the smaller budget wins, in multiples of the strides' product
    got = list(_batches(32, lambda: [(600, 6, 1), (30, 6, 4)], cap=64, multiple=4))
    assert got == [(0, 16), (16, 16)]


def test_eager_state_holds_its_fields_and_never_asks_a_device():
    cols, ov, bo = np.array([3, 1, 2]), np.arange(5), np.linspace(0, 1, 5)
    st = SpatialPooler.State._eager(active_column=cols, overlaps=ov, boosted_overlaps=bo)
    assert type(st) is SpatialPooler.State and st._engine is None and st._step == -1
    assert st.active_column is cols and st.overlaps is ov and st.boosted_overlaps is bo
    st._materialize()                                       # (nothing to fetch)
    st.overlaps = ov + 1                                    # fields stay assignable, as on a State read from the device
    assert np.array_equal(st.overlaps, ov + 1) and "overlaps" not in st.__dict__
    with pytest.raises(AttributeError):
        st.no_such_field
    # the Temporal Memory's empty state is built the same way (networks.py:59-65)
    tm = TemporalMemory(16, 4)
    e = tm.get_empty_state()
    assert type(e) is TemporalMemory.State and e._engine is None and e._step == -1
    assert e.winner_cell is None and e.distal_state is None and e.cell_prediction.shape == (16, 4) and not e.cell_activation.any()
    assert e.active_cell[0].size == 0 and e.active_column_bursting.size == 0


class _FakeTM:
    """What _BatchedCall asks of a Temporal Memory: its engine's step index, input_dim and sticky-flag check, and _new_state."""

    def __init__(self, log, name, steps, column_dim, input_dim):
        from types import SimpleNamespace
        self.column_dim, self.name, self.log = column_dim, name, log
        self._engine = SimpleNamespace(steps=steps, input_dim=input_dim, check_capacity=lambda: log.append(("check", name)))

    def _new_state(self, cols):
        self.log.append(("state", self.name, cols))


def test_batched_call_keeps_first_steps_parts_and_runs_the_tail_in_order():
    from bithtm_amd.engine import RECORD_COUNTERS
    from bithtm_amd.networks import _BatchedCall
    log = []
    a, b = _FakeTM(log, "a", 7, 40, 9), _FakeTM(log, "b", 100, 40, 9)
    call = _BatchedCall([a, b], ("counters", "column_prediction"))
    a._engine.steps, b._engine.steps = 12, 105               # (the first step is the one the call started at)
    W = len(RECORD_COUNTERS)
    for n in (3, 2):                                        # two batches: 3 + 2 steps per member
        call.add([{"counters": np.full((n, W), n + i, np.int32), "column_prediction": np.full((n, 2), 1 + i, np.uint32)} for i in (0, 1)])
    recs = call.finish([5, 5], [4, 4])
    # the tail: every member's new last_state first, then every member's sticky flags
    assert log == [("state", "a", None), ("state", "b", None), ("check", "a"), ("check", "b")]
    assert [r.step_index.tolist() for r in recs] == [list(range(7, 12)), list(range(100, 105))]
    assert recs[0].active_columns.tolist() == [3, 3, 3, 2, 2] and recs[1].active_columns.tolist() == [4, 4, 4, 3, 3]
    assert recs[0].column_prediction.shape == (5, 40) and recs[0].column_prediction.dtype == np.bool_
    assert recs[0].column_prediction[:, 0].all() and not recs[0].column_prediction[:, 1].any()     # word 1 = bit 0 only
    assert recs[1].column_prediction[:, 1].all() and recs[0].active_column is None
    # without a record nothing is kept and None comes back per member; `columns`: the host-fed lists of the last step, and an
    # empty list leaves last_state alone (a run of 0 steps); `read`: records read after the flags were checked
    del log[:]
    call = _BatchedCall([a], None)
    call.add([{"counters": np.zeros((1, W), np.int32)}])
    assert call.finish([1], [4], columns=[]) == [None] and call.parts == [[]] and log == [("check", "a")]
    del log[:]
    cols = np.array([1, 2])
    call = _BatchedCall([a], ("active_column",))
    recs = call.finish([2], [3], columns=[cols], read=lambda: log.append("read") or [{"active_column": np.arange(6, dtype=np.int32).reshape(2, 3)}])
    assert log[0][:2] == ("state", "a") and log[0][2] is cols and log[1:] == [("check", "a"), "read"]
    assert recs[0].active_column.tolist() == [[0, 1, 2], [3, 4, 5]] and recs[0].step_index.tolist() == [12, 13]
    # a call of 0 steps with a record: empty arrays of the right widths
    r = _BatchedCall([a], ("counters", "active_column", "predicted_input")).finish([0], [4])[0]
    assert len(r) == 0 and r.active_column.shape == (0, 4) and r.predicted_input.shape == (0, 9) and r.active_columns.shape == (0,)
