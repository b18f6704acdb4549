"""GPU: region stacks (bithtm_amd.RegionStack, htm_pack_columns) against the recorded two-level stack of
the unmodified reference (tests/golden/stack_two_level.npz) and against the chained oracles."""

import ctypes as C

import numpy as np
import pytest

import stack_fixture as sf

pytestmark = pytest.mark.gpu

RECORD = ("counters", "active_column", "column_prediction")


@pytest.fixture(scope="module")
def fx():
    return sf.load()


def make_stack(fx, stride, **kw):
    """The recorded stack on the device: level l with seed + l and the permanences the recorded reference drew."""
    from bithtm_amd import RegionStack
    levels = [(int(c), int(K), int(k)) for c, K, k in zip(fx["column_dim"], fx["cell_dim"], fx["active_columns"])]
    stack = RegionStack(int(fx["input_dim"]), levels, strides=[stride], seed=int(fx["seed"]), **kw)
    for l, m in enumerate(stack.levels):
        m.engine.set_permanence(sf.initial_permanence(fx, l))
    return stack


def rows_of(fx):
    """One bank row per recorded step (the 8 patterns cycled), and the reset flag of each row."""
    bank = sf.inputs(fx)
    steps = int(fx["steps"])
    return bank[np.arange(steps) % len(bank)], sf.schedule(fx)[1]


def learning_spans(fx):
    a, b, n = int(fx["learning_off"][0]), int(fx["learning_off"][1]), int(fx["steps"])
    return [(0, a, True), (a, b, False), (b, n, True)]


def final_states(stack):
    return [m.state_dict() for m in stack.levels]


def assert_same_states(got, want, what=""):
    assert len(got) == len(want)
    for l, (a, b) in enumerate(zip(got, want)):
        assert sorted(a) == sorted(b), (what, l)
        for key in a:
            x, y = np.asarray(a[key]), np.asarray(b[key])
            assert x.shape == y.shape and x.tobytes() == y.tobytes(), f"{what}: level {l}: state field {key} differs"


@pytest.fixture(scope="module")
def stepwise(fx):
    """RegionStack.process over both recorded runs, every digest checked against the reference's on the way ->
    {stride: per-level records in run()'s layout + the final state of every level}."""
    rows, reset = rows_of(fx)
    learning = sf.schedule(fx)[0]
    out = {}
    for stride in fx["strides"].tolist():
        stack = make_stack(fx, stride)
        rec = [dict(active_column=[], column_prediction=[], segments=[], step_index=[]) for _ in stack.levels]
        count = [0, 0]
        for t in range(len(rows)):
            if reset[t]:
                stack.reset()
            res = stack.process(rows[t], learning=bool(learning[t]))
            assert (res[1] is None) == bool((t + 1) % stride)
            for l, st in enumerate(res):
                if st is None:
                    continue
                sp, tm = st
                segments = stack.levels[l].engine.info().segments
                sf.check_step(fx, stride, l, count[l], sp, tm, segments)
                rec[l]["active_column"].append(np.asarray(sp.active_column))
                rec[l]["column_prediction"].append(np.asarray(tm.cell_prediction).any(axis=1))
                rec[l]["segments"].append(segments)
                count[l] += 1
        assert count == [len(rows), len(rows) // stride] and stack.steps == len(rows)
        out[stride] = dict(rec=rec, states=final_states(stack))
    return out


def test_process_reproduces_the_reference_at_both_levels_and_strides(stepwise):
    assert sorted(stepwise) == [1, 3]


def run_recorded_spans(stack, fx, calls, use_graph=True):
    """The recorded run through run(): the learning spans cut into calls of at most `calls` steps; -> per-level joined records."""
    rows, reset = rows_of(fx)
    parts = [[] for _ in stack.levels]
    for a, b, learn in learning_spans(fx):
        t = a
        while t < b:
            n = min(calls, b - t)
            recs = stack.run(rows, n, learning=learn, use_graph=use_graph, record=RECORD, resets=reset)
            for l, r in enumerate(recs):
                parts[l].append(r)
            t += n
    return parts


def assert_records_equal_stepwise(parts, want, stride):
    for l, rs in enumerate(parts):
        cols = np.concatenate([r.active_column for r in rs])
        pred = np.concatenate([r.column_prediction for r in rs])
        segs = np.concatenate([r.segments for r in rs])
        idx = np.concatenate([r.step_index for r in rs])
        w = want["rec"][l]
        assert np.array_equal(cols, np.array(w["active_column"])), f"level {l}: active_column"
        assert np.array_equal(pred, np.array(w["column_prediction"])), f"level {l}: column_prediction"
        assert np.array_equal(segs, np.array(w["segments"])), f"level {l}: segments"
        assert np.array_equal(idx, np.arange(len(idx))), f"level {l}: step_index"


@pytest.mark.parametrize("use_graph", [True, False], ids=["graph", "eager"])
@pytest.mark.parametrize("calls,chunk", [(10 ** 6, None), (24, None), (10 ** 6, 9)], ids=["one-call-per-span", "calls-of-24", "chunks-of-9"])
@pytest.mark.parametrize("stride", [1, 3])
def test_run_equals_process(fx, stepwise, stride, calls, chunk, use_graph):
    """run() -- as one call per learning span, as calls of 24 steps, and with chunks of 9 level-0 steps (a span of 120 steps is
    13 chunks and a shorter last one) -- gives process()'s records at every level and leaves every level in process()'s state."""
    stack = make_stack(fx, stride)
    if chunk:
        stack.chunk_steps = chunk
    parts = run_recorded_spans(stack, fx, calls, use_graph)
    if chunk:
        assert [n for n, _ in stack.last_run_chunks][-4:] == [9, 9, 9, 6]       # (the last span: 96 steps)
    assert_records_equal_stepwise(parts, stepwise[stride], stride)
    assert_same_states(final_states(stack), stepwise[stride]["states"], f"stride {stride}")
    assert stack.steps == int(fx["steps"])


def test_row_rotation_and_mixing_process_with_run(fx, stepwise):
    """A run() started when the upper level's step count is no multiple of the chunk's row count (after a few process() calls)
    reads its chunk bank from the right row on: equals stepwise.  And every level is at rest afterwards: process(),
    predicted_input() and state_dict() work on each."""
    rows, reset = rows_of(fx)
    stride = 3
    stack = make_stack(fx, stride)
    stack.chunk_steps = 30
    for t in range(21):                             # 21 level-0 steps: 7 upper steps, and a chunk of 9 upper rows follows
        stack.process(rows[t])
    assert stack.levels[1].engine.steps == 7
    assert stack.run(rows, 27) is None
    assert stack.levels[1].engine.steps == 16
    for m in stack.levels:
        assert m.predicted_input().shape == (m.engine.input_dim,)
        assert m.temporal_memory.last_state.cell_prediction.shape == (m.column_dim, m.cell_dim)
    for t in range(48, 120):                        # (the recorded run resets before step 48)
        if reset[t]:
            stack.reset()
        stack.process(rows[t])
    twin = make_stack(fx, stride)
    for t in range(120):
        if reset[t]:
            twin.reset()
        twin.process(rows[t])
    assert_same_states(final_states(stack), final_states(twin), "process + run + process")
    for l in range(2):
        assert stack.levels[l].engine.info().segments == stepwise[stride]["rec"][l]["segments"][120 // (stride if l else 1) - 1]


def test_graphs_are_reused_by_chunks_of_one_length(fx):
    rows, _ = rows_of(fx)
    stack = make_stack(fx, 3)
    stack.chunk_steps = 48
    stack.run(rows, 48 * 4 + 24)
    log = stack.last_run_chunks
    assert [n for n, _ in log] == [48, 48, 48, 48, 24]
    assert all(g > 0 for g in log[0][1])
    assert log[1][1] == log[2][1] == log[3][1], log          # (the second chunk may add the other step parity's graphs, once)


def test_resets_in_run(fx):
    from bithtm_amd import RegionStack
    rows, _ = rows_of(fx)
    stack = make_stack(fx, 3)
    flags = np.zeros(len(rows), dtype=bool)
    flags[[0, 30, 33]] = True
    bad = flags.copy()
    bad[31] = True
    with pytest.raises(ValueError):
        stack.run(rows, 60, resets=bad)             # a flagged row that is no multiple of the stride
    with pytest.raises(ValueError):
        stack.run(rows[:10], 30, resets=flags[:10])  # 10 rows cycled: not a multiple of the stride
    with pytest.raises(ValueError):
        stack.run(rows, 61)
    stack.chunk_steps = 12
    stack.run(rows, 60, resets=flags)
    stack.process(rows[60])
    with pytest.raises(ValueError):
        stack.reset()                               # in the middle of a window
    with pytest.raises(ValueError):
        stack.run(rows, 3)
    stack.process(rows[61]), stack.process(rows[62])
    twin = make_stack(fx, 3)
    for t in range(63):
        if flags[t]:
            twin.reset()
        twin.process(rows[t])
    assert_same_states(final_states(stack), final_states(twin), "resets= against reset() calls")
    assert isinstance(stack, RegionStack)


def test_save_and_load_in_mid_training(fx, stepwise, tmp_path):
    rows, reset = rows_of(fx)
    stack = make_stack(fx, 3)
    stack.run(rows, 60, resets=reset)
    path = str(tmp_path / "stack.npz")
    stack.save(path)
    other = make_stack(fx, 3)
    other.load(path)
    assert other.steps == 60
    for s in (stack, other):
        s.run(rows, 60, resets=reset)
    assert_same_states(final_states(other), final_states(stack), "after load")
    assert stack.levels[1].engine.info().segments == stepwise[3]["rec"][1]["segments"][39]
    with pytest.raises(ValueError):
        make_stack(fx, 1).load(path)                # other strides
    from bithtm_amd import RegionStack
    with pytest.raises(ValueError):
        RegionStack(int(fx["input_dim"]), [(1024, 8, 64), (128, 8, 16)], strides=[3]).load(path)      # other shapes


def test_of_refuses_what_needs_a_device(fx):
    import bithtm_amd as B
    from bithtm_amd import RegionStack
    from bithtm_amd.group import SharedStream
    stream = SharedStream(0)
    a = B.HierarchicalTemporalMemory(100, 256, 4, seed=1, stream=stream)
    b = B.HierarchicalTemporalMemory(256, 128, 4, seed=2, stream=stream)
    lone = B.HierarchicalTemporalMemory(256, 128, 4, seed=3)
    bank = np.random.RandomState(0).rand(6, 100) < 0.2
    stack = RegionStack.of([a, b], strides=[2])
    stack.run(bank, 12)
    assert (a.engine.steps, b.engine.steps, stack.steps) == (12, 6, 12)
    with pytest.raises(ValueError, match="stream"):
        RegionStack.of([a, lone])
    with pytest.raises(ValueError, match="view"):
        RegionStack.of([a, b.inference_view()])
    with pytest.raises(ValueError, match="column_dim"):
        RegionStack.of([b, a])
    a.run(bank, 4, continuing=True)
    with pytest.raises(ValueError, match="streamed"):
        RegionStack.of([a, b])
    a.run(bank, 4)


def test_default_sized_pool_grows_inside_a_run():
    """A run long enough to make level 0's default-sized pool grow (novel input throughout: every column bursts, 20 new segments
    per step, each with 20 synapses -- past the matching threshold, so it is not recycled) finishes, keeps every level on the
    stack's stream, and equals stepwise."""
    from bithtm_amd import RegionStack
    I, levels = 120, [(1024, 4, 20), (128, 4, 8)]
    rng = np.random.RandomState(3)
    bank = rng.rand(700, I) < 0.15                  # 700 different inputs: nothing repeats
    stacks = [RegionStack(I, levels, strides=[2], seed=9) for _ in range(2)]
    for s in stacks:
        for l, m in enumerate(s.levels):
            m.engine.set_permanence(np.random.RandomState(20 + l).randn(m.column_dim, m.engine.input_dim) * 0.1)
    run, step = stacks
    cap0, stream0 = run.levels[0].engine.segment_capacity, run.levels[0].engine.stream_handle()
    run.run(bank, 700)
    assert run.levels[0].engine.segment_capacity > cap0, "the pool did not have to grow: the test checks nothing"
    assert all(m.engine.stream_handle() == stream0 for m in run.levels)
    assert len(run.last_run_chunks) > 1
    for t in range(700):
        step.process(bank[t])
    want, got = final_states(step), final_states(run)
    for l in range(2):                              # (the pools may have grown to different capacities: compare what is in use)
        S = int(want[l]["tm_S"])
        assert int(got[l]["tm_S"]) == S
        for key in want[l]:
            x, y = np.asarray(got[l][key]), np.asarray(want[l][key])
            if key in ("tm_presyn", "tm_perm"):
                w = min(x.shape[1], y.shape[1])
                assert (x[:, w:] < 0).all() and (y[:, w:] < 0).all() and x[:, :w].tobytes() == y[:, :w].tobytes(), (l, key)
            elif key != "tm_slots":
                assert x.shape == y.shape and x.tobytes() == y.tobytes(), (l, key)


@pytest.mark.parametrize("input_dim,k,stride,n_rows,bank_rows,first_row", [
    (1000, 20, 1, 7, 7, 3),             # a width that is no multiple of 128, rotated
    (31, 5, 3, 4, 9, 7),                # one (padded) word row, rows wrapping round a larger bank
    (65536, 1311, 4, 5, 5, 0),          # the headline width: 8 KB of bitmap per block, 5 244 entries per row
    (300, 64, 2, 300, 300, 299)])       # more blocks than one wave of them
def test_pack_columns_alone(input_dim, k, stride, n_rows, bank_rows, first_row):
    """Random ascending lists into a bank: bit-equal to the NumPy contract, rows outside the written range untouched."""
    import bithtm_amd as B
    htm = B.HierarchicalTemporalMemory(input_dim, 64, 4, active_columns=4)
    eng = htm.engine
    lib, W = eng.lib, eng.words
    assert W == (input_dim + 127) // 128 * 4
    rng = np.random.RandomState(input_dim + k)
    lists = np.stack([np.sort(rng.choice(input_dim, k, replace=False)) for _ in range(n_rows * stride)]).astype(np.int32)
    want = rng.randint(0, 2 ** 32, size=(bank_rows + 2, W), dtype=np.uint64).astype(np.uint32)       # (a guard row on each side)
    d_lists, d_bank = C.c_void_p(), C.c_void_p()
    assert lib.hipMalloc(C.byref(d_lists), lists.nbytes) == 0 and lib.hipMalloc(C.byref(d_bank), want.nbytes) == 0
    try:
        assert lib.hipMemcpy(d_lists, lists.ctypes.data_as(C.c_void_p), lists.nbytes, 1) == 0
        assert lib.hipMemcpy(d_bank, want.ctypes.data_as(C.c_void_p), want.nbytes, 1) == 0
        inner = d_bank.value + 4 * W
        eng.pack_columns(d_lists.value, k, n_rows, stride, inner, bank_rows, first_row)
        assert not sf.pack_columns(lists, input_dim, stride, want[1:-1], first_row)
        eng.sync()
        got = np.empty_like(want)
        assert lib.hipMemcpy(got.ctypes.data_as(C.c_void_p), d_bank, want.nbytes, 2) == 0
        assert np.array_equal(got, want)
        assert eng.info().capacity_error == 0
        # the argument checks that need a handle
        for args in ((0, n_rows, stride, inner, bank_rows, 0), (k, -1, stride, inner, bank_rows, 0), (k, n_rows, 0, inner, bank_rows, 0),
                     (k, n_rows, stride, inner, 0, 0), (k, n_rows, stride, inner, bank_rows, bank_rows), (k, n_rows, stride, inner, bank_rows, -1)):
            assert lib.htm_pack_columns(eng.h, d_lists, *args[:3], C.c_void_p(args[3]), *args[4:]) == -1, args
        assert lib.htm_pack_columns(eng.h, None, k, 1, 1, C.c_void_p(inner), 1, 0) == -1
        if input_dim == 1000:
            # an id outside the range: the sticky bit, and nothing written outside the row
            lists[1, 3], lists[2, 0] = input_dim, -5
            assert lib.hipMemcpy(d_lists, lists.ctypes.data_as(C.c_void_p), lists.nbytes, 1) == 0
            eng.pack_columns(d_lists.value, k, n_rows, stride, inner, bank_rows, first_row)
            assert sf.pack_columns(lists, input_dim, stride, want[1:-1], first_row)
            eng.sync()
            assert lib.hipMemcpy(got.ctypes.data_as(C.c_void_p), d_bank, want.nbytes, 2) == 0
            assert np.array_equal(got, want)
            assert eng.info().capacity_error & 64
    finally:
        eng.sync()
        lib.hipFree(d_lists)
        lib.hipFree(d_bank)


def test_pack_columns_refuses_handles_it_cannot_serve():
    import bithtm_amd as B
    tm = B.TemporalMemory(64, 4)
    tm.process(type("S", (), {"active_column": np.array([1, 5])})())
    eng = tm._engine
    buf = C.c_void_p()
    assert eng.lib.hipMalloc(C.byref(buf), 4096) == 0
    try:
        assert eng.lib.htm_pack_columns(eng.h, buf, 1, 1, 1, buf, 1, 0) == -4        # HTM_ERR_STATE: no Spatial Pooler
        htm = B.HierarchicalTemporalMemory(100, 256, 4)
        bank = np.random.RandomState(0).rand(4, 100) < 0.2
        htm.run(bank, 4, continuing=True)
        if htm._streaming and htm.engine.run_plan(4)["pipelined"]:
            assert eng.lib.htm_pack_columns(htm.engine.h, buf, 1, 1, 1, buf, 1, 0) == -4    # ... a handle that is ahead
        htm.run(bank, 4)
        assert eng.lib.htm_pack_columns(htm.engine.h, buf, 1, 1, 1, buf, 1, 0) == 0
        htm.engine.sync()
    finally:
        eng.lib.hipFree(buf)


def test_full_size_stack_against_the_chained_oracles():
    """1 000 -> 65 536 x 32 -> 4 096 x 32, stride 2, 200 steps of run() with graph replay, against two chained oracles stepped
    from the seed (their overlap counted over the active inputs only: the same integers as the dense form, at a hundredth of
    the memory traffic of a 4 096 x 65 536 comparison per step)."""
    from bithtm_amd import RegionStack
    from hip_impl import compare_store_with_oracle
    I, levels, seed, steps = 1000, [(65536, 32, 1311), (4096, 32, 82)], 5, 200
    stack = RegionStack(I, levels, strides=[2], seed=seed)
    perms = []
    for l, m in enumerate(stack.levels):
        perms.append(np.random.RandomState(50 + l).randn(m.column_dim, m.engine.input_dim) * 0.1)
        m.engine.set_permanence(perms[l])
    ora = sf.OracleStack(I, levels, [2], seed, permanences=perms)
    del perms
    for o in ora.levels:
        sp = o.spatial_pooler
        sp.overlaps = lambda x, sp=sp: (sp.permanence[:, np.flatnonzero(x)] >= sp.params.permanence_threshold).sum(axis=1)
    bank = np.random.RandomState(6).rand(20, I) < 0.1
    recs = stack.run(bank, steps, record=("active_column", "counters"))
    want = [[], []]
    for t in range(steps):
        for l, st in enumerate(ora.process(bank[t % len(bank)])):
            if st is not None:
                want[l].append(st[0].active_column)
    for l in range(2):
        assert np.array_equal(recs[l].active_column, np.array(want[l])), f"level {l}: active columns"
        assert recs[l].segments[-1] == ora.levels[l].temporal_memory.S
        compare_store_with_oracle(steps, ora.levels[l], stack.levels[l])
    assert recs[0].predicted_columns.max() > 0      # (a learned stretch at the lower level)
