"""GPU: the batched run's two-launch step with the winner list built in its LAST launch (k_last_handover, csrc/htm_handover_last.h)
wherever no winner of the step lacks a segment, and by block 0 of the first launch (k_first_handover, csrc/htm_handover.h) wherever
one does -- against process(), which steps through k_act_mid_rows and k_learn_scan_emit, and against the oracle.  Bit for bit:
everything compared is integers or floats rounded one by one.

Every run here takes BOTH paths and changes between them in both directions; each test asserts that from the oracle's per-step
allocation (a run that never leaves one path proves nothing).  Inputs: 300 bits, boosting off, four patterns cycled, 60 steps: the
model learns the cycle within five steps (no winner lacks a segment from then on) and falls back to bursting steps later on."""

import functools

import numpy as np
import pytest

from oracle import HTMOracle, SPParams, TMParams

pytestmark = pytest.mark.gpu

I, SEED, STEPS = 300, 61, 60
CHUNKS = (1, 2, 17, 40)                             # a streamed run's calls: 60 steps
SPP = SPParams(boost_intensity=0.0)
SMALL = TMParams(segment_activation_threshold=3, segment_matching_threshold=3, segment_sampling_synapses=5)
SHAPES = {"one-block": (256, 32, 5, SMALL),         # one activation block
          "ragged-last": (2048, 32, 41, None),      # 6 activation blocks, the last with one column
          "K8": (2048, 8, 41, None),                # 32 columns per block
          "K40": (1024, 40, 20, None),              # two words per column
          "two-passes": (2048, 40, 1100, None)}     # 2 200 slots: the list pass loops (2 048 slots per pass)
BANK = np.random.RandomState(62).rand(4, I) < 0.06


def _make(C, K, k, tmp, cap=None):
    from hip_impl import make_htm
    np.random.seed(SEED)
    perm = HTMOracle(I, C, K, active_columns=k, seed=SEED, sp_params=SPP, tm_params=tmp).spatial_pooler.permanence.copy()
    return lambda: make_htm(I, C, K, k, SEED, perm.copy(), sp_params=SPP, tm_params=tmp, segment_capacity=cap)


@functools.lru_cache(maxsize=None)
def _oracle(name, plan=((STEPS, True),), resets=None):
    """The oracle over the plan [(steps, learning)], once per shape and plan: (the model, per step: winners without a segment,
    active columns, winner cells in the reference's order, active cells)"""
    C, K, k, tmp = SHAPES[name]
    np.random.seed(SEED)
    ora = HTMOracle(I, C, K, active_columns=k, seed=SEED, sp_params=SPP, tm_params=tmp)
    un, cols, winners, cells, t = [], [], [], [], 0
    for n, learning in plan:
        for _ in range(n):
            o_sp, o_tm = ora.step(BANK[t % len(BANK)], learning=learning)
            lu = ora.temporal_memory.last_update
            # (the first step has no distal state: nothing is allocated and `last_update` is the step's before, or None)
            un.append(len(lu.unaccounted) if learning and lu is not None and t > 0 else 0)
            cols.append(o_sp.active_column.copy())
            winners.append(o_tm.winner_cell[0].astype(np.int64) * K + o_tm.winner_cell[1])
            cells.append(len(o_tm.active_cell[0]))
            t += 1
    return ora, un, cols, winners, cells


def _both_paths(un, learning=None):
    """From the oracle's allocation: at least 5 steps of each kind among the learning steps behind the first, and both changes"""
    kinds = [u > 0 for t, u in enumerate(un) if t > 0 and (learning is None or learning[t])]
    pairs = set(zip(kinds, kinds[1:]))
    assert kinds.count(True) >= 5 and kinds.count(False) >= 5, un
    assert (True, False) in pairs and (False, True) in pairs, un


def _digest(htm):
    st, d = htm.engine.read_store(), htm.engine.read_distal()
    info = htm.engine.check_capacity()              # (raises on any error bit: capacity, the work array, a fan-in that never completed)
    return (htm.engine.read_sp_fields()["active_column"], st["S"], st["seg_cell"], st["seg_nsyn"], st["segcount"], st["presyn"],
            st["perm"].view(np.int32), htm.temporal_memory.last_state.cell_prediction, htm.engine.read_duty_cycle().view(np.int32),
            d["matching_segment"], d["max_jittered_potential"].view(np.int32), d["segment_potential"],
            (info.new_segment_requests, info.recycled_segments, info.winner_cells, info.active_cells), _winners(htm))


def _same(a, b, what):
    for i, (x, y) in enumerate(zip(a, b)):
        assert np.array_equal(np.asarray(x), np.asarray(y)), f"{what}: field {i} of the digest differs"


def _winners(htm):
    """HTM_F_WINNER_CELL as the library returns it: in the list's order, not sorted"""
    from bithtm_amd import _lib as L
    eng = htm.engine
    return eng.read(L.F_WINNER_CELL, np.int32, eng.info().winner_cells).astype(np.int64)


def _twin(make, plan, resets=None):
    """process() step by step: (the model, per step its winner_cells and active_cells counters, per step its winner list)"""
    twin, counts, lists, t = make(), [], [], 0
    for n, learning in plan:
        for _ in range(n):
            if resets is not None and resets[t % len(resets)]:
                twin.reset()
            twin.process(BANK[t % len(BANK)], learning=learning)
            info = twin.engine.info()
            counts.append((info.winner_cells, info.active_cells))
            lists.append(_winners(twin))
            t += 1
    return twin, counts, lists


def _streamed(make, plan, lists, **kw):
    """`continuing` chunks of 1, 2, 17 and 40 steps, cut again where the plan changes `learning`; at every call boundary the winner
    list in order against the twin's of that step"""
    htm, chunks, t = make(), list(CHUNKS), 0
    for n, learning in plan:
        while n:
            take = min(n, chunks[0])
            n -= take
            chunks[0] -= take
            if not chunks[0]:
                chunks.pop(0)
            htm.run(BANK, take, learning=learning, continuing=n > 0, **kw)
            t += take
            assert np.array_equal(_winners(htm), lists[t - 1]), f"winner list behind step {t - 1}"
    return htm


def _check(name, plan=((STEPS, True),), resets=None, cap=None):
    from hip_impl import compare_store_with_oracle
    C, K, k, tmp = SHAPES[name]
    make = _make(C, K, k, tmp, cap)
    kw = {} if resets is None else dict(resets=resets)
    twin, counts, lists = _twin(make, plan, resets)
    want = _digest(twin)
    for mode in ("graph", "eager"):
        htm, got, t = make(), [], 0
        for n, learning in plan:
            rec = htm.run(BANK, n, learning=learning, use_graph=mode == "graph", record=("counters", "active_column"), **kw)
            got += [(int(rec.winner_cells[i]), int(rec.active_cells[i])) for i in range(n)]
            t += n
            assert np.array_equal(_winners(htm), lists[t - 1]), f"{mode}: winner list behind step {t - 1}"
            if resets is None:
                cols = _oracle(name, plan)[2]
                for i in range(n):
                    assert np.array_equal(np.asarray(rec.active_column[i]), cols[t - n + i]), f"{mode}: step {t - n + i}: active columns"
        for i, (x, y) in enumerate(zip(got, counts)):
            assert x == y, f"{mode}: step {i}: (winner_cells, active_cells) {x}, the twin's {y}"
        _same(_digest(htm), want, mode)
        if mode == "graph":
            graph = htm
    _same(_digest(_streamed(make, plan, lists, **kw)), want, "continuing")
    if resets is not None:
        return None
    ora, un, _, winners, cells = _oracle(name, plan)
    for i, (w, c) in enumerate(counts):
        assert (w, c) == (len(winners[i]), cells[i]), f"step {i}: the twin's counters and the oracle's"
        assert np.array_equal(lists[i], winners[i]), f"step {i}: the twin's winner list and the oracle's"
    compare_store_with_oracle(sum(n for n, _ in plan) - 1, ora, graph)
    o_d, d = ora.temporal_memory.prev_distal, graph.engine.read_distal()
    assert np.array_equal(d["matching_segment"], o_d.matching_segment) and np.array_equal(d["segment_potential"], o_d.segment_potential)
    assert np.array_equal(graph.temporal_memory.last_state.cell_prediction, ora.temporal_memory.prev_prediction)
    return un


@pytest.mark.parametrize("name", list(SHAPES))
def test_block_shapes_through_both_paths(name):
    un = _check(name)
    _both_paths(un)
    if name in ("ragged-last", "K8"):
        assert un[7] == 1                           # (one winner of 41 asks: one activation block raises its flag)
    if name != "two-passes":
        assert un[21] == SHAPES[name][2]            # (a fully bursting step in the middle of the run)


def test_learning_off_in_the_middle():
    """learning=False: nobody asks for a segment whatever the activation finds, block 0 does not wait, the list is the last launch's"""
    plan = ((20, True), (20, False), (20, True))
    un = _check("ragged-last", plan)
    _both_paths(un, [t < 20 or t >= 40 for t in range(STEPS)])


def test_sequence_resets_inside_the_run():
    """a reset empties the winner list and the distal state of the step before (k_tm_reset, in front of the step's first launch): the
    step behind it has no distal state, asks for nothing and its list is the last launch's"""
    resets = np.array([0, 0, 1, 0], bool)
    _check("ragged-last", resets=resets)
    _both_paths(_oracle("ragged-last")[1])          # (the run without resets takes both paths; with them every reset step adds a change)


@pytest.mark.parametrize("env", [{"BITHTM_SCAN_LARGE": "1"}, {"BITHTM_HANDOVER_LDS_CAP": "16"}], ids=["large-pool-form", "list-through-memory"])
def test_the_other_forms_of_the_two_launches(monkeypatch, env):
    """BITHTM_SCAN_LARGE=1: k_last_handover<E, 4, false>, the streaming scan that the learning and emit blocks join.
    BITHTM_HANDOVER_LDS_CAP=16: block 0's full path with its list beyond 16 entries going through memory."""
    for key, value in env.items():
        monkeypatch.setenv(key, value)
    un = _check("ragged-last")
    _both_paths(un)
    assert max(un) > 16


def test_a_fork_between_calls_and_a_view_after_the_run():
    C, K, k, tmp = SHAPES["ragged-last"]
    make = _make(C, K, k, tmp)
    un = _oracle("ragged-last")[1]
    _both_paths(un[:30])
    twin, _, lists = _twin(make, ((STEPS, True),))
    def alone(f, t0):
        """the fork goes on alone (a learning=False handle over its parent's weights), from the step it was taken at, before its
        parent steps on: against a twin of its own, stepped by process() to where the fork was taken"""
        ref = make()
        for t in range(t0):
            ref.process(BANK[t % 4])
        want = [np.asarray(ref.process(BANK[(t0 + i) % 4], learning=False)[0].active_column) for i in range(7)]
        got = f.run(BANK, 7, record=("active_column",))
        for i in range(7):
            assert np.array_equal(np.sort(np.asarray(got.active_column[i])), np.sort(want[i])), (t0, i)
        assert np.array_equal(f.temporal_memory.last_state.cell_prediction, ref.temporal_memory.last_state.cell_prediction), t0
        assert np.array_equal(_winners(f), _winners(ref)), t0
        f.engine.check_capacity()

    htm = make()
    htm.run(BANK, 18)                               # (17 had no winner without a segment: its list was written by the last launch)
    assert un[17] == 0
    fork = htm.fork()
    assert np.array_equal(_winners(fork), lists[17]) and np.array_equal(_winners(htm), lists[17])
    alone(fork, 18)
    htm.run(BANK, 4)                                # (21 is the fully bursting step: its list was written by block 0)
    assert un[21] > 0
    late = htm.fork()
    assert np.array_equal(_winners(late), lists[21])
    alone(late, 22)
    htm.run(BANK, 38)
    _same(_digest(htm), _digest(twin), "the parent of two forks")
    view, ref = htm.inference_view(), twin
    view.run(BANK, 5)
    want = _digest(twin)
    for i in range(5):
        ref.process(BANK[(STEPS + i) % 4], learning=False)
    assert np.array_equal(view.temporal_memory.last_state.cell_prediction, ref.temporal_memory.last_state.cell_prediction)
    _same(_digest(htm), want, "the parent after its view ran")


@pytest.mark.parametrize("first", ["run", "process"])
def test_a_host_fed_step_between_two_batched_calls(first):
    """process() reads the winners a batched call's last step left (its learning role grows synapses to them) and the batched call
    reads process()'s: around step 21, where the list changes hands twice"""
    C, K, k, tmp = SHAPES["ragged-last"]
    make = _make(C, K, k, tmp)
    un = _oracle("ragged-last")[1]
    twin, _, lists = _twin(make, ((STEPS, True),))
    htm, t = make(), 0
    # 20 | 1 | 1 | 38: the host-fed step is 20 (nothing asked before it, run-first) or 21 (the bursting step, process-first)
    calls = (("run", 20), ("process", 1), ("run", 1), ("process", 1), ("run", 37)) if first == "run" else \
            (("process", 1), ("run", 20), ("process", 1), ("run", 1), ("process", 1), ("run", 36))
    assert un[21] > 0 and un[20] == 0 and un[22] == 0
    for kind, n in calls:
        if kind == "run":
            htm.run(BANK, n)
        else:
            htm.process(BANK[t % 4])
        t += n
        assert np.array_equal(_winners(htm), lists[t - 1]), f"winner list behind step {t - 1} ({kind})"
    assert t == STEPS
    _same(_digest(htm), _digest(twin), first)
