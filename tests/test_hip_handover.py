"""GPU: the first launch of the batched run's two-launch step (k_first_handover, csrc/htm_handover.h) -- block 0 of the middle role
keeps the list of winners without a segment in LDS and issues its stores behind its last load -- against process(), which steps
through the launch's earlier form (k_act_mid_rows), and against the oracle.  Bit for bit: everything compared is integers or
floats rounded one by one.  More than 128 needed 1 024-blocks (the pairs beyond the LDS go through memory) are
tests/test_hip_pool_geometry.py's: alloc_many_blocks, two-launch, batched, runs this kernel."""

import numpy as np
import pytest

from oracle import HTMOracle, TMParams

pytestmark = pytest.mark.gpu

CHUNKS = (1, 2, 17, 40)                             # a streamed run's calls: 60 steps


def _digest(htm):
    st, d = htm.engine.read_store(), htm.engine.read_distal()
    info = htm.engine.check_capacity()
    return (htm.engine.read_sp_fields()["active_column"], st["S"], st["seg_cell"], st["seg_nsyn"], st["segcount"], st["presyn"],
            st["perm"].view(np.int32), htm.temporal_memory.last_state.cell_prediction, htm.engine.read_duty_cycle().view(np.int32),
            d["matching_segment"], d["max_jittered_potential"].view(np.int32), d["segment_potential"],
            (info.new_segment_requests, info.recycled_segments))


def _same(a, b, what):
    for i, (x, y) in enumerate(zip(a, b)):
        assert np.array_equal(np.asarray(x), np.asarray(y)), f"{what}: field {i} of the digest differs"


def _model(I, C, K, k, seed, cap, tmp=None):
    from hip_impl import make_htm
    np.random.seed(seed)
    ora = HTMOracle(I, C, K, active_columns=k, seed=seed, tm_params=tmp)
    perm = ora.spatial_pooler.permanence.copy()
    return ora, lambda: make_htm(I, C, K, k, seed, perm.copy(), tm_params=tmp, segment_capacity=cap)


def _run_modes(make, bank, plan):
    """plan: [(steps, learning)], 60 steps in all.  -> the models after a graph run, an eager run and a streamed run (`continuing`
    chunks of 1, 2, 17 and 40 steps, cut again where the plan changes `learning`: a stream ends there), the per-step winner
    columns of the graph run, and the process() twin"""
    assert sum(n for n, _ in plan) == sum(CHUNKS)
    out, cols = {}, []
    for mode in ("graph", "eager"):
        htm = make()
        for n, learning in plan:
            rec = htm.run(bank, n, learning=learning, use_graph=mode == "graph", record=("active_column",))
            if mode == "graph":
                cols += [np.asarray(rec.active_column[i]) for i in range(n)]
        out[mode] = htm
    htm, chunks = make(), list(CHUNKS)
    for n, learning in plan:
        while n:
            take = min(n, chunks[0])
            n -= take
            chunks[0] -= take
            if not chunks[0]:
                chunks.pop(0)
            htm.run(bank, take, learning=learning, continuing=n > 0)
    out["continuing"] = htm
    twin, t = make(), 0
    for n, learning in plan:
        for _ in range(n):
            twin.process(bank[t % len(bank)], learning=learning)
            t += 1
    return out, cols, twin


def _check(I, C, K, k, seed, bank, plan=((60, True),), cap=None, tmp=None):
    """-> the oracle's allocation per step [(unaccounted, recycled, fresh)]"""
    from hip_impl import compare_store_with_oracle
    ora, make = _model(I, C, K, k, seed, cap, tmp)
    out, cols, twin = _run_modes(make, bank, plan)
    want = _digest(twin)
    for mode, htm in out.items():
        _same(_digest(htm), want, mode)
    alloc, t = [], 0
    for n, learning in plan:
        for _ in range(n):
            o_sp, _ = ora.step(bank[t % len(bank)], learning=learning)
            assert np.array_equal(cols[t], o_sp.active_column), f"step {t}: active columns"
            lu = getattr(ora.temporal_memory, "last_update", None)
            alloc.append((len(lu.unaccounted), len(lu.recycled), len(lu.fresh)) if learning and lu is not None else (0, 0, 0))
            t += 1
    compare_store_with_oracle(t - 1, ora, out["graph"])
    o_d = ora.temporal_memory.prev_distal
    d = out["graph"].engine.read_distal()
    assert np.array_equal(d["matching_segment"], o_d.matching_segment) and np.array_equal(d["segment_potential"], o_d.segment_potential)
    assert np.array_equal(out["graph"].temporal_memory.last_state.cell_prediction, ora.temporal_memory.prev_prediction)
    return alloc


def _bank(I, rows, seed, density=0.06):
    return np.random.RandomState(seed).rand(rows, I) < density


@pytest.mark.parametrize("C,K,k", [(256, 32, 5),        # one activation block
                                   (2048, 32, 41),      # 6 activation blocks, the last with one column
                                   (2048, 8, 41),       # 32 columns per block
                                   (1024, 40, 20)],     # two words per column
                         ids=["one-block", "ragged-last", "K8", "K40"])
def test_block_shapes_from_scratch(C, K, k):
    """60 steps from scratch over non-repeating inputs: every column bursts and every winner asks for a segment"""
    alloc = _check(300, C, K, k, 61, _bank(300, 60, 62))
    # (5 winners grow rows of 5 synapses, below the matching threshold: the one-block shape recycles them step after step)
    assert max(a[0] for a in alloc) == k and sum(a[1] + a[2] for a in alloc) >= 50 * k


def test_more_activation_blocks_than_a_wave_has_lanes():
    C, K, k = 32768, 32, 655                        # 82 activation blocks
    alloc = _check(300, C, K, k, 63, _bank(300, 60, 64), cap=65536)
    assert max(a[0] for a in alloc) == k


def test_list_beyond_the_lds_capacity_goes_through_memory(monkeypatch):
    """BITHTM_HANDOVER_LDS_CAP (read when a handle is created): entries of the list past it are stored to memory and read back
    behind a barrier -- what a shape with more than 3 584 winners without a segment in one step does"""
    monkeypatch.setenv("BITHTM_HANDOVER_LDS_CAP", "16")
    alloc = _check(300, 2048, 32, 41, 65, _bank(300, 60, 66))
    assert min(a[0] for a in alloc[2:]) > 16, alloc       # (from the oracle: the forced capacity was exceeded)
    monkeypatch.setenv("BITHTM_HANDOVER_LDS_CAP", "0")
    _check(300, 256, 32, 5, 67, _bank(300, 60, 68))


def test_a_run_that_recycles_and_appends_in_one_step():
    """Low thresholds, heavy punishment, a walk that jumps between six patterns: rows die and the allocation takes the lowest dead
    ids first, then fresh ones -- in a pool that the run nearly fills"""
    I, C, K, k = 300, 512, 8, 20
    tmp = TMParams(permanence_punishment=0.25, segment_activation_threshold=7, segment_matching_threshold=7, segment_sampling_synapses=12)
    rng = np.random.RandomState(53)
    base, rows, cur = rng.rand(6, I) < 0.06, [], 0
    for _ in range(60):
        cur = int(rng.randint(6)) if rng.rand() < 0.5 else (cur + 1) % 6
        rows.append(base[cur])
    alloc = _check(I, C, K, k, 52, np.stack(rows), cap=512, tmp=tmp)
    assert [a for a in alloc if a[1] > 0 and a[2] > 0], alloc     # (the oracle itself recycled and appended in one step)
    assert [a for a in alloc if 0 < a[0] < k]                      # (... and steps in which only some winners asked)


def test_learning_off_stretches():
    """learning=False: nobody asks for a segment, the launch has no classification blocks"""
    _check(300, 2048, 32, 41, 69, _bank(300, 7, 70), plan=((13, True), (9, False), (21, True), (1, False), (16, True)))


def test_reset_and_checkpoint_between_runs(tmp_path):
    """run -> reset -> run and run -> load -> run against process(): the launch keeps no state of its own between steps (no slot or
    tag was added), so this holds it to the model's state as any run() / process() comparison does"""
    I, C, K, k = 300, 2048, 32, 41
    _, make = _model(I, C, K, k, 71, None)
    bank = _bank(I, 9, 72)
    htm, twin = make(), make()
    htm.run(bank, 23)
    for t in range(23):
        twin.process(bank[t % 9])
    htm.reset()
    twin.reset()
    htm.run(bank, 18)
    for t in range(23, 41):
        twin.process(bank[t % 9])
    _same(_digest(htm), _digest(twin), "after the reset")
    path = str(tmp_path / "model.npz")
    htm.save(path)
    htm.run(bank, 11)                               # (steps the checkpoint does not know of)
    htm.load(path)
    twin.load(path)
    t0 = htm.engine.steps
    htm.run(bank, 19)
    for t in range(t0, t0 + 19):
        twin.process(bank[t % 9])
    _same(_digest(htm), _digest(twin), "after the checkpoint")


def test_a_fork_and_a_view_stepped_after_their_parent():
    """learning=False handles of their own stepping through the launch (no classification blocks), and the parent after them"""
    I, C, K, k = 300, 2048, 32, 41
    _, make = _model(I, C, K, k, 73, None)
    bank = _bank(I, 9, 74)
    htm, twin = make(), make()
    htm.run(bank, 30)
    for t in range(30):
        twin.process(bank[t % 9])
    fork, view = htm.fork(), htm.inference_view()
    t0 = fork.engine.steps                          # (a run reads bank row (steps + i) % rows)
    got = fork.run(bank, 7, record=("active_column",))
    view.run(bank, 5)
    want = [np.asarray(twin.process(bank[(t0 + i) % 9], learning=False)[0].active_column) for i in range(7)]
    for i in range(7):
        assert np.array_equal(np.sort(np.asarray(got.active_column[i])), np.sort(want[i])), i
    assert np.array_equal(fork.temporal_memory.last_state.cell_prediction, twin.temporal_memory.last_state.cell_prediction)
    # the parent, stepped on after its fork and view ran, is where a model that never had them would be
    lone = make()
    lone.run(bank, 30)
    lone.run(bank, 12)
    htm.run(bank, 12)
    _same(_digest(htm), _digest(lone), "the parent after its fork")
