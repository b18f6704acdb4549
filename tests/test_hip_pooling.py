"""GPU: pooling links of region stacks (bithtm_amd.PoolingLink, RegionStack(links=), htm_pool_columns):
htm_pool_columns alone against the NumPy statement of its contract on every case of tests/pooling_cases.py, and pooled stacks
against the recorded chained reference (tests/golden/stack_pooled.npz) and against the stepwise process()."""

import numpy as np
import pytest

import pooling_cases as pc
import stack_fixture as sf
from test_hip_region_stack import assert_same_states, final_states, learning_spans, rows_of

pytestmark = pytest.mark.gpu

CASES = pc.cases()
GUARD = 64                                          # bytes of pattern behind every array the call writes


@pytest.fixture(scope="module")
def fx():
    with np.load(sf.PATH.replace("stack_two_level", "stack_pooled")) as z:
        return {k: z[k] for k in z.files}


def fixture_link(fx, stride):
    from bithtm_amd import PoolingLink
    return PoolingLink(stride, *[int(v) for v in fx["link"]])


def make_stack(fx, link, **kw):
    """The recorded stack on the device (level l with seed + l and the permanences the recorded reference drew), its link `link`:
    an int or a PoolingLink."""
    from bithtm_amd import RegionStack
    levels = [(int(c), int(K), int(k)) for c, K, k in zip(fx["column_dim"], fx["cell_dim"], fx["active_columns"])]
    stack = RegionStack(int(fx["input_dim"]), levels, links=[link], seed=int(fx["seed"]), **kw)
    for l, m in enumerate(stack.levels):
        m.engine.set_permanence(sf.initial_permanence(fx, l))
    return stack


def whole_state(stack):
    """The levels' states and, as one more entry, the stack's own (steps, links)."""
    own = {k: v for k, v in stack.state_dict().items() if k.startswith(("link", "stack_", "strides"))}
    return final_states(stack) + [own]


# ---- htm_pool_columns alone
@pytest.mark.parametrize("c", CASES, ids=[c.name for c in CASES])
def test_pool_columns_alone(c):
    """Bit-equal to the contract: the rows written, the rows not written, the guard bytes round the bank and behind the state
    arrays, the final state and the error bit."""
    import bithtm_amd as B
    htm = B.HierarchicalTemporalMemory(c.C, 64, 4, active_columns=4)       # (a handle per case: none outlives its test, and the error bit is sticky)
    eng = htm.engine
    lib, W, stride = eng.lib, eng.words, c.link.stride
    assert W == pc.bank_words(c.C)
    want = pc.replay(c)
    assert c.reaches(c, want), "the case does not reach the path it names"
    guard = np.full(GUARD, 0xA5, np.uint8)
    bank0 = np.concatenate([np.full((1, W), 0xDEADBEEF, np.uint32), want.before, np.full((1, W), 0xDEADBEEF, np.uint32)])
    colpred = pc.words_of(c.colpred)
    P0 = np.concatenate([c.persistence, np.zeros(-c.C % 16, np.uint8), guard])
    prev0 = np.concatenate([pc.words_of(c.prev[None])[0].view(np.uint8), np.zeros(-(4 * colpred.shape[1]) % 16, np.uint8), guard])
    window = (stride + 8) * 4 * W
    scratch_bytes = window * (c.batch_windows or c.windows)
    scratch0 = np.full(scratch_bytes + GUARD, 0xA5, np.uint8)
    ptrs = [eng.device_buffer(a.nbytes, np.ascontiguousarray(a)) for a in (c.lists, colpred, P0, prev0, scratch0, bank0)]
    d_lists, d_colpred, d_P, d_prev, d_scratch, d_bank = ptrs
    d_bits = None if c.resets is None else eng.upload_resets(c.resets)
    try:
        done = 0
        for n in c.calls:
            eng.pool_columns(c.link, d_lists + 4 * done * stride * c.k, c.k, d_colpred + 4 * done * stride * colpred.shape[1], n, d_P, d_prev, d_bits,
                             d_scratch, scratch_bytes, d_bank + 4 * W, c.bank_rows, (c.first_row + done) % c.bank_rows)
            done += n
        assert done == c.windows
        eng.sync()
        read = lambda ptr, like: eng.read_words(ptr, like.nbytes // 4, np.uint32).view(like.dtype).reshape(like.shape)
        bank, P, prev, scratch = read(d_bank, bank0), read(d_P, P0), read(d_prev, prev0), read(d_scratch, scratch0)
        assert np.array_equal(bank[1:-1], want.bank), "bank rows"
        assert (bank[[0, -1]] == 0xDEADBEEF).all(), "a guard row of the bank was written"
        untouched = sorted(set(range(c.bank_rows)) - {(c.first_row + r) % c.bank_rows for r in range(c.windows)})
        assert np.array_equal(bank[1:-1][untouched], want.before[untouched])
        assert np.array_equal(P[:c.C], want.persistence), "persistence"
        assert np.array_equal(np.unpackbits(prev[:4 * colpred.shape[1]], bitorder="little")[:c.C].astype(bool), want.prev), "prev"
        assert (P[-GUARD:] == 0xA5).all() and (prev[-GUARD:] == 0xA5).all() and (scratch[-GUARD:] == 0xA5).all(), "written out of bounds"
        assert bool(eng.info().capacity_error & 64) == want.bad
        assert eng.info().capacity_error & ~64 == 0
    finally:
        eng.sync()
        for p in ptrs:
            lib.hipFree(p)


# ---- the recorded stack
@pytest.fixture(scope="module")
def stepwise(fx):
    """RegionStack.process over both recorded runs, every digest checked against the reference's on the way ->
    {stride: the upper rows' bit counts seen, the final state of every level and of the link}."""
    rows, reset = rows_of(fx)
    learning = sf.schedule(fx)[0]
    out = {}
    for stride in fx["strides"].tolist():
        stack = make_stack(fx, fixture_link(fx, stride))
        count = [0, 0]
        for t in range(len(rows)):
            if reset[t]:
                stack.reset()
            res = stack.process(rows[t], learning=bool(learning[t]))
            assert (res[1] is None) == bool((t + 1) % stride)
            for l, st in enumerate(res):
                if st is None:
                    continue
                sf.check_step(fx, stride, l, count[l], st[0], st[1], stack.levels[l].engine.info().segments)
                count[l] += 1
        P, prev = stack.link_state(0)
        assert np.array_equal(P, fx[f"s{stride}_link_persistence"]) and np.array_equal(prev, fx[f"s{stride}_link_prev"])
        out[stride] = dict(states=whole_state(stack))
    return out


def test_process_reproduces_the_reference_at_both_levels_and_strides(stepwise):
    assert sorted(stepwise) == [1, 3]


def run_spans(stack, fx, calls, use_graph=True):
    rows, reset = rows_of(fx)
    for a, b, learn in learning_spans(fx):
        t = a
        while t < b:
            n = min(calls, b - t)
            stack.run(rows, n, learning=learn, use_graph=use_graph, resets=reset)
            t += n


@pytest.mark.parametrize("use_graph", [True, False], ids=["graph", "eager"])
@pytest.mark.parametrize("calls,chunk,scratch", [(10 ** 6, None, None), (24, None, None), (10 ** 6, 9, None), (10 ** 6, None, 2)],
                         ids=["one-call-per-span", "calls-of-24", "chunks-of-9", "batches-of-2-windows"])
@pytest.mark.parametrize("stride", [1, 3])
def test_run_equals_process(fx, stepwise, stride, calls, chunk, scratch, use_graph):
    """run() -- as one call per learning span, as calls of 24 steps, with chunks of 9 level-0 steps and with a scratch bound of two
    windows (a span of 120 steps: 60 or 20 batches) -- leaves every level and the link in process()'s state."""
    stack = make_stack(fx, fixture_link(fx, stride))
    if chunk:
        stack.chunk_steps = chunk
    if scratch:
        stack.pool_scratch_bytes = scratch * (stride + 8) * 4 * stack.levels[1].engine.words
    run_spans(stack, fx, calls, use_graph)
    if chunk:
        assert [n for n, _ in stack.last_run_chunks][-4:] == [9, 9, 9, 6]
    assert_same_states(whole_state(stack), stepwise[stride]["states"], f"stride {stride}")
    assert stack.steps == int(fx["steps"])
    assert stack.levels[0].engine.info().capacity_error == 0 and stack.levels[1].engine.info().capacity_error == 0


def test_mixing_process_with_run(fx):
    rows, reset = rows_of(fx)
    stack, twin = (make_stack(fx, fixture_link(fx, 3)) for _ in range(2))
    stack.chunk_steps = 30
    for t in range(21):
        stack.process(rows[t])
    assert stack.run(rows, 27) is None
    assert stack.link_state(0)[0].any()
    for t in range(48, 90):
        if reset[t]:
            stack.reset()
        stack.process(rows[t])
    stack.run(rows, 30, resets=reset)
    for t in range(120):
        if reset[t]:
            twin.reset()
        twin.process(rows[t])
    assert_same_states(whole_state(stack), whole_state(twin), "process + run + process + run")


def test_resets_in_run_against_reset_and_process(fx):
    rows, _ = rows_of(fx)
    stack, twin = (make_stack(fx, fixture_link(fx, 3)) for _ in range(2))
    flags = np.zeros(len(rows), dtype=bool)
    flags[[0, 30, 33]] = True
    stack.chunk_steps = 12
    stack.run(rows, 60, resets=flags)
    for t in range(60):
        if flags[t]:
            twin.reset()
        twin.process(rows[t])
    assert_same_states(whole_state(stack), whole_state(twin), "resets= against reset() calls")
    stack.process(rows[60])
    with pytest.raises(ValueError):
        stack.reset()                               # in the middle of a window


def test_save_and_load_in_mid_training(fx, tmp_path):
    from bithtm_amd import PoolingLink
    rows, reset = rows_of(fx)
    stack = make_stack(fx, fixture_link(fx, 3))
    stack.run(rows, 60, resets=reset)
    path = str(tmp_path / "stack.npz")
    stack.save(path)
    other = make_stack(fx, fixture_link(fx, 3))
    other.load(path)
    assert other.steps == 60 and np.array_equal(other.link_state(0)[0], stack.link_state(0)[0]) and stack.link_state(0)[0].any()
    for s in (stack, other):
        s.run(rows, 60, resets=reset)
    assert_same_states(whole_state(other), whole_state(stack), "after load")
    with pytest.raises(ValueError, match="link 0"):
        make_stack(fx, 3).load(path)                # a plain link of the same stride
    with pytest.raises(ValueError, match="link 0"):
        make_stack(fx, PoolingLink(3, decay=2)).load(path)
    plain = make_stack(fx, 3)
    plain.run(rows, 6)
    assert sorted(k for k in plain.state_dict() if k.startswith("link")) == ["link0_window"]
    plain.save(path)
    with pytest.raises(ValueError, match="link 0"):
        other.load(path)


def test_graphs_are_reused_by_chunks_of_one_length(fx):
    rows, _ = rows_of(fx)
    stack = make_stack(fx, fixture_link(fx, 3))
    stack.chunk_steps = 48
    stack.run(rows, 48 * 4 + 24)
    log = stack.last_run_chunks
    assert [n for n, _ in log] == [48, 48, 48, 48, 24]
    assert all(g > 0 for g in log[0][1])
    assert log[1][1] == log[2][1] == log[3][1], log


def test_a_plain_stack_beside_a_pooled_one_gives_the_results_it_gave():
    """The recorded plain stack (tests/golden/stack_two_level.npz) through run(), a pooled stack running between its calls."""
    plain_fx = sf.load()
    rows, reset = rows_of(plain_fx)
    alone, beside = (make_stack(plain_fx, 3) for _ in range(2))
    pooled = make_stack(plain_fx, fixture_link({"link": [1, 8, 1, 16, 96]}, 3))
    for a in range(0, 120, 30):
        alone.run(rows, 30, resets=reset)
    for a in range(0, 120, 30):
        pooled.run(rows, 30, resets=reset)
        beside.run(rows, 30, resets=reset)
    assert_same_states(whole_state(beside), whole_state(alone), "a plain stack beside a pooled one")
    lists = [np.asarray(plain_fx["s3_l0_lists"][t], dtype=np.int64) for t in range(120)]
    assert beside.levels[0].engine.info().segments == plain_fx["s3_l0_segments"][119]
    assert beside.levels[1].engine.info().segments == plain_fx["s3_l1_segments"][39] and len(lists) == 120


def test_the_degenerate_link_equals_the_plain_stack_state_for_state():
    from bithtm_amd import PoolingLink
    plain_fx = sf.load()
    rows, reset = rows_of(plain_fx)
    k = int(plain_fx["active_columns"][0])
    plain = make_stack(plain_fx, 1)
    pooled = make_stack(plain_fx, PoolingLink(1, active_weight=4, predicted_weight=4, decay=16, ceiling=16, union_bits=k))
    for s in (plain, pooled):
        s.run(rows, 96, resets=reset)
        for t in range(96, 120):
            if reset[t]:
                s.reset()
            s.process(rows[t])
    assert_same_states(final_states(pooled), final_states(plain), "decay >= ceiling, equal weights, union_bits = k, stride 1")
    assert plain.levels[1].engine.info().segments == plain_fx["s1_l1_segments"][119]


def test_of_takes_links():
    import bithtm_amd as B
    from bithtm_amd import PoolingLink, RegionStack
    from bithtm_amd.group import SharedStream
    stream = SharedStream(0)
    a = B.HierarchicalTemporalMemory(100, 256, 4, seed=1, stream=stream)
    b = B.HierarchicalTemporalMemory(256, 128, 4, seed=2, stream=stream)
    bank = np.random.RandomState(0).rand(6, 100) < 0.2
    stack = RegionStack.of([a, b], links=[PoolingLink(2)])
    assert stack.strides == [2] and stack.links == [PoolingLink(2, union_bits=2 * a.active_columns)]
    stack.run(bank, 12)
    assert (a.engine.steps, b.engine.steps, stack.steps) == (12, 6, 12) and stack.link_state(0)[0].any()
    with pytest.raises(ValueError, match="not both"):
        RegionStack.of([a, b], strides=[2], links=[2])
    with pytest.raises(ValueError, match="link 0.*union_bits"):
        RegionStack.of([a, b], links=[PoolingLink(union_bits=257)])
    plain = RegionStack.of([a, b], links=[2])
    assert plain.links == [2] and plain.strides == [2]
    with pytest.raises(ValueError, match="not a pooling link"):
        plain.link_state(0)
