"""GPU: stacks of model groups (bithtm_amd.GroupStack, htm_group_pack_columns, htm_group_pool_columns).
Both entries alone against the NumPy contract on every group case of tests/group_stack_cases.py, and GroupStack against solo
RegionStack twins fed each member's inputs: every level's state, every link's state and all records bit for bit."""

import numpy as np
import pytest

import group_stack_cases as gc
import pooling_cases as pc
import stack_fixture as sf
from bithtm_amd.networks import RECORD_COUNTERS
from test_hip_region_stack import assert_same_states, final_states

pytestmark = pytest.mark.gpu

GROUPS = gc.groups()
GUARD = 64                                          # bytes of pattern behind every array a call writes
I, LEVELS = 300, [(1024, 8, 64), (256, 8, 32)]
RECORD = ("counters", "active_column", "column_prediction")
SEEDS = [41, 7, 19]
STEPS = 48
COMPARED = RECORD_COUNTERS + ("active_column", "column_prediction")        # a RunRecord's arrays under RECORD


# ---- the entries alone
def _group_for(g):
    import bithtm_amd as B
    return B.ModelGroup.create(len(g.members), g.C, 64, 4, active_columns=4)       # (a group per case: the error bit is sticky)


def _read(eng, ptr, like):
    return eng.read_words(ptr, like.nbytes // 4, np.uint32).view(like.dtype).reshape(like.shape)


def _banks(eng, before_each, W):
    """Each member's bank between two guard rows -> (host arrays, device addresses of the arrays)."""
    host = [np.concatenate([np.full((1, W), 0xDEADBEEF, np.uint32), b, np.full((1, W), 0xDEADBEEF, np.uint32)]) for b in before_each]
    return host, [eng.device_buffer(a.nbytes, np.ascontiguousarray(a)) for a in host]


@pytest.mark.parametrize("g", GROUPS, ids=[g.name for g in GROUPS])
def test_group_pool_columns_alone(g):
    """Per member bit-equal to the contract: the rows written, the rows not written, the guard rows round every bank and the guard
    bytes behind the state arrays and the scratch, the final state, and the error bit in the offending member only."""
    group = _group_for(g)
    eng = group.models[0].engine
    W, stride, n = eng.words, g.link.stride, len(g.members)
    assert W == pc.bank_words(g.C)
    want = gc.replay(g)
    guard = np.full(GUARD, 0xA5, np.uint8)
    bank0, d_bank = _banks(eng, [w.before for w in want], W)
    colpred = [pc.words_of(c.colpred) for c in g.members]
    P0 = [np.concatenate([c.persistence, np.zeros(-c.C % 16, np.uint8), guard]) for c in g.members]
    prev0 = [np.concatenate([pc.words_of(c.prev[None])[0].view(np.uint8), np.zeros(-(4 * colpred[0].shape[1]) % 16, np.uint8), guard]) for c in g.members]
    window = (stride + 8) * 4 * W
    scratch_bytes = n * window * (g.batch_windows or g.windows)
    scratch0 = np.full(scratch_bytes + GUARD, 0xA5, np.uint8)
    up = lambda arrays: [eng.device_buffer(a.nbytes, np.ascontiguousarray(a)) for a in arrays]
    d_lists, d_colpred, d_P, d_prev = up([c.lists for c in g.members]), up(colpred), up(P0), up(prev0)
    d_scratch = eng.device_buffer(scratch0.nbytes, scratch0)
    bits = [None if c.resets is None else eng.upload_resets(c.resets) for c in g.members]
    ptrs = d_bank + d_lists + d_colpred + d_P + d_prev + [d_scratch]
    try:
        group.pool_columns(g.link, d_lists, g.k, d_colpred, g.windows, d_P, d_prev, None if all(b is None for b in bits) else bits, d_scratch, scratch_bytes,
                           [p + 4 * W for p in d_bank], g.bank_rows, [c.first_row for c in g.members])
        eng.sync()
        assert (_read(eng, d_scratch, scratch0)[-GUARD:] == 0xA5).all(), "written behind the scratch"
        for i, (c, w) in enumerate(zip(g.members, want)):
            bank, P, prev = _read(eng, d_bank[i], bank0[i]), _read(eng, d_P[i], P0[i]), _read(eng, d_prev[i], prev0[i])
            assert np.array_equal(bank[1:-1], w.bank), f"member {i} ({c.name}): bank rows"
            assert (bank[[0, -1]] == 0xDEADBEEF).all(), f"member {i}: a guard row of the bank was written"
            untouched = sorted(set(range(c.bank_rows)) - {(c.first_row + r) % c.bank_rows for r in range(c.windows)})
            assert np.array_equal(bank[1:-1][untouched], w.before[untouched]), f"member {i}: untouched rows"
            assert np.array_equal(P[:c.C], w.persistence), f"member {i} ({c.name}): persistence"
            assert np.array_equal(np.unpackbits(prev[:4 * colpred[i].shape[1]], bitorder="little")[:c.C].astype(bool), w.prev), f"member {i}: prev"
            assert (P[-GUARD:] == 0xA5).all() and (prev[-GUARD:] == 0xA5).all(), f"member {i}: written out of bounds"
            flags = group.models[i].engine.info().capacity_error
            assert bool(flags & 64) == w.bad and flags & ~64 == 0, f"member {i} ({c.name}): error bit {flags}"
    finally:
        eng.sync()
        for p in ptrs:
            eng.lib.hipFree(p)


@pytest.mark.parametrize("g", GROUPS, ids=[g.name for g in GROUPS])
def test_group_pack_columns_alone(g):
    group = _group_for(g)
    eng = group.models[0].engine
    W = eng.words
    want = gc.replay_pack(g)
    bank0, d_bank = _banks(eng, [w.before for w in want], W)
    d_lists = [eng.device_buffer(c.lists.nbytes, np.ascontiguousarray(c.lists)) for c in g.members]
    try:
        group.pack_columns(d_lists, g.k, g.windows, g.link.stride, [p + 4 * W for p in d_bank], g.bank_rows, [c.first_row for c in g.members])
        eng.sync()
        for i, (c, w) in enumerate(zip(g.members, want)):
            bank = _read(eng, d_bank[i], bank0[i])
            assert np.array_equal(bank[1:-1], w.bank), f"member {i} ({c.name}): bank rows"
            assert (bank[[0, -1]] == 0xDEADBEEF).all(), f"member {i}: a guard row of the bank was written"
            flags = group.models[i].engine.info().capacity_error
            assert bool(flags & 64) == w.bad and flags & ~64 == 0, f"member {i} ({c.name}): error bit {flags}"
    finally:
        eng.sync()
        for p in d_bank + d_lists:
            eng.lib.hipFree(p)


# ---- GroupStack against solo twins
def link_of(kind, stride):
    from bithtm_amd import PoolingLink
    return stride if kind == "plain" else PoolingLink(stride)


def inputs_for(n, input_dim=I, rows=16, seed=5):
    return np.random.RandomState(seed).rand(n, rows, input_dim) < 0.1


def set_permanences(levels, seed):
    """The Spatial Poolers' permanences of one stack's levels from `seed` (a model draws its own from NumPy's global stream when it
    is made, so two stacks made one after the other differ whatever their seeds: the twins here get theirs explicitly)."""
    for l, m in enumerate(levels):
        m.engine.set_permanence(np.random.RandomState(100 * seed + l).randn(m.column_dim, m.engine.input_dim) * 0.1)


def region_stack(input_dim, levels, seed, **kw):
    from bithtm_amd import RegionStack
    stack = RegionStack(input_dim, levels, seed=seed, **kw)
    set_permanences(stack.levels, seed)
    return stack


def group_stack(n, input_dim, levels, seeds, **kw):
    from bithtm_amd import GroupStack
    gs = GroupStack(n, input_dim, levels, seeds=seeds, **kw)
    for member, seed in zip(gs.members, seeds):
        set_permanences(member.levels, seed)
    return gs


def whole_state(stack):
    """A RegionStack's levels' states and, as one more entry, the stack's own (steps, links)."""
    own = {k: v for k, v in stack.state_dict().items() if k.startswith(("link", "stack_", "strides"))}
    return final_states(stack) + [own]


def assert_records(got, want, what):
    for l, (a, b) in enumerate(zip(got, want)):
        for f in ("step_index",) + COMPARED:
            x, y = np.asarray(getattr(a, f)), np.asarray(getattr(b, f))
            assert x.shape == y.shape and x.tobytes() == y.tobytes(), f"{what}: level {l}: record field {f} differs"


def assert_members(gs, twins, what):
    assert gs.steps == twins[0].steps
    for b, twin in enumerate(twins):
        assert_same_states(whole_state(gs.members[b]), whole_state(twin), f"{what}: member {b}")


def solo(links, inputs, steps=STEPS, levels=LEVELS, input_dim=I, seeds=SEEDS, record=RECORD, **kw):
    """The yardstick: one RegionStack per member, run alone over its rows -> (stacks, records per member)."""
    from bithtm_amd import RegionStack
    stacks = [region_stack(input_dim, levels, s, links=links) for s in seeds]
    return stacks, [s.run(x, steps, record=record, **kw) if steps else None for s, x in zip(stacks, inputs)]


@pytest.fixture(scope="module")
def twins():
    """Per link, computed once and left unchanged: the final states and the records of three solo RegionStacks after STEPS steps."""
    cache = {}

    def get(kind, stride):
        if (kind, stride) not in cache:
            stacks, recs = solo([link_of(kind, stride)], inputs_for(3))
            cache[(kind, stride)] = ([whole_state(s) for s in stacks], recs)
        return cache[(kind, stride)]
    return get


MODES = {"one-call": (STEPS, None, None, True), "eager": (STEPS, None, None, False), "calls-of-24": (24, None, None, True), "chunks-of-9": (STEPS, 9, None, True),
         "scratch-of-2-windows": (STEPS, None, 2, True)}
RUNS = [(kind, stride, mode) for kind, stride in (("plain", 1), ("plain", 3), ("pooled", 1), ("pooled", 3)) for mode in MODES
        if kind == "pooled" or mode != "scratch-of-2-windows"]          # (a plain link has no scratch)


@pytest.mark.parametrize("kind,stride,mode", RUNS, ids=[f"{k}-{s}-{m}" for k, s, m in RUNS])
def test_run_equals_three_solo_stacks(twins, kind, stride, mode):
    from bithtm_amd import GroupStack
    calls, chunk, scratch, use_graph = MODES[mode]
    states, recs = twins(kind, stride)
    inputs = inputs_for(3)
    gs = group_stack(3, I, LEVELS, SEEDS, links=[link_of(kind, stride)])
    if chunk:
        gs.chunk_steps = chunk
    if scratch:
        gs.pool_scratch_bytes = 3 * scratch * (stride + 8) * 4 * gs.groups[1].models[0].engine.words
    parts = [gs.run(inputs, calls, use_graph=use_graph, record=RECORD) for _ in range(STEPS // calls)]
    if chunk:
        assert gs.last_run_chunks == [9, 9, 9, 9, 9, 3]
    assert gs.steps == STEPS and len(gs) == 3
    for b in range(3):
        assert_same_states(whole_state(gs.members[b]), states[b], f"{kind} stride {stride}: member {b}")
        for l in range(2):
            for f in ("step_index",) + COMPARED:
                got = np.concatenate([np.asarray(getattr(p[b][l], f)) for p in parts])
                want = np.asarray(getattr(recs[b][l], f))
                assert got.shape == want.shape and got.tobytes() == want.tobytes(), f"member {b}, level {l}: record field {f} differs"
        if kind == "pooled":
            assert gs.link_state(0, b)[0].any() and np.array_equal(gs.link_state(0, b)[0], states[b][-1]["link0_persistence"])
    for g in gs.groups:
        assert all(m.engine.info().capacity_error == 0 for m in g.models)


def test_one_member_equals_a_region_stack(twins):
    from bithtm_amd import GroupStack
    states, recs = twins("pooled", 3)
    gs = group_stack(1, I, LEVELS, SEEDS[:1], links=[link_of("pooled", 3)])
    got = gs.run(inputs_for(3)[:1], STEPS, record=RECORD)
    assert_same_states(whole_state(gs.members[0]), states[0], "B = 1")
    assert_records(got[0], recs[0], "B = 1")


def test_members_at_different_step_indices_of_equal_parity():
    """Member 1's models have stepped alone twice (level 0) and four times (level 1) before the call: its rows of the chunk banks start
    elsewhere (first_rows differ between the members) and its level 0 reads other rows of its inputs."""
    from bithtm_amd import GroupStack
    inputs = inputs_for(3)
    links = [link_of("pooled", 3)]
    stacks, _ = solo(links, inputs, steps=0)
    gs = group_stack(3, I, LEVELS, SEEDS, links=links)
    extra = np.random.RandomState(9).rand(4, 1024) < 0.06
    for s in (stacks[1], gs.members[1]):
        for t in range(2):
            s.levels[0].process(inputs[1, t])
        for t in range(4):
            s.levels[1].process(extra[t])
    want = [s.run(x, STEPS, record=RECORD) for s, x in zip(stacks, inputs)]
    got = gs.run(inputs, STEPS, record=RECORD)
    assert gs.members[1].levels[1].engine.steps == 4 + STEPS // 3 and gs.members[0].levels[1].engine.steps == STEPS // 3
    assert_members(gs, stacks, "different step indices")
    for b in range(3):
        assert_records(got[b], want[b], f"member {b}")


@pytest.mark.parametrize("kind", ["plain", "pooled"])
def test_a_level_of_two_cell_words(kind):
    from bithtm_amd import GroupStack
    levels, inputs, links = [(512, 48, 48), (256, 8)], inputs_for(3), [link_of(kind, 3)]
    stacks, want = solo(links, inputs, levels=levels)
    gs = group_stack(3, I, levels, SEEDS, links=links)
    got = gs.run(inputs, STEPS, record=RECORD)
    assert_members(gs, stacks, f"512 x 48, {kind}")
    for b in range(3):
        assert_records(got[b], want[b], f"member {b}")


def test_three_levels_a_plain_link_then_a_pooled_one():
    from bithtm_amd import GroupStack, PoolingLink
    levels, links = [(512, 8), (256, 8), (128, 8)], [2, PoolingLink(2)]
    inputs = inputs_for(3, 100)
    stacks, want = solo(links, inputs, levels=levels, input_dim=100)
    gs = group_stack(3, 100, levels, SEEDS, links=links)
    gs.chunk_steps = 20
    got = gs.run(inputs, STEPS, record=RECORD)
    assert gs.last_run_chunks == [20, 20, 8]
    assert_members(gs, stacks, "three levels")
    assert [len(got[0][l].step_index) for l in range(3)] == [48, 24, 12]
    for b in range(3):
        assert_records(got[b], want[b], f"member {b}")
    with pytest.raises(ValueError, match="not a pooling link"):
        gs.link_state(0, 0)
    assert gs.link_state(1, 2)[0].any()


# ---- the recorded chained reference
@pytest.mark.parametrize("kind", ["plain", "pooled"])
def test_member_0_reproduces_the_recorded_reference(kind):
    """tests/golden/stack_two_level.npz and stack_pooled.npz at stride 3 (240 steps, resets at 48, 96, 99 and 168, learning off over
    120..144): member 0 with the fixture's seed and permanences beside two members of other seeds, the calls cut where the
    recording resets or switches learning (a group run takes no resets: GroupStack.reset between the calls)."""
    from bithtm_amd import GroupStack, PoolingLink
    fx = sf.load()
    if kind == "pooled":
        with np.load(sf.PATH.replace("stack_two_level", "stack_pooled")) as z:
            fx = {k: z[k] for k in z.files}
    stride = 3
    link = stride if kind == "plain" else PoolingLink(stride, *[int(v) for v in fx["link"]])
    levels = [(int(c), int(K), int(k)) for c, K, k in zip(fx["column_dim"], fx["cell_dim"], fx["active_columns"])]
    gs = group_stack(3, int(fx["input_dim"]), levels, [int(fx["seed"]), 5, 6], links=[link])
    for l, m in enumerate(gs.members[0].levels):
        m.engine.set_permanence(sf.initial_permanence(fx, l))
    bank = sf.inputs(fx)
    learning, reset = sf.schedule(fx)
    steps = int(fx["steps"])
    inputs = np.stack([bank, np.roll(bank, 1, axis=0), np.roll(bank, 2, axis=0)])
    cuts = sorted({0, steps} | set(np.flatnonzero(reset).tolist()) | set((np.flatnonzero(np.diff(learning.astype(int))) + 1).tolist()))
    parts = []
    for a, b in zip(cuts, cuts[1:]):
        if reset[a]:
            gs.reset()
        parts.append(gs.run(inputs, b - a, learning=bool(learning[a]), record=RECORD)[0])
    lists = np.concatenate([p[0].active_column for p in parts])
    assert lists.shape == (steps, levels[0][2])
    if kind == "plain":                             # (the pooled recording keeps digests of the lists only)
        assert np.array_equal(lists, fx[f"s{stride}_l0_lists"].astype(lists.dtype)), "level 0: active columns"
    for l in range(2):
        segs = np.concatenate([p[l].segments for p in parts])
        assert np.array_equal(segs, fx[f"s{stride}_l{l}_segments"]), f"level {l}: segments"
    if kind == "pooled":
        P, prev = gs.link_state(0, 0)
        assert np.array_equal(P, fx[f"s{stride}_link_persistence"]) and np.array_equal(prev, fx[f"s{stride}_link_prev"])


# ---- views
def test_views_of_a_trained_stack_against_full_copies():
    """Three streams over ONE copy of a trained stack's weights against three full copies of it after reset(), run as RegionStacks
    with learning=False."""
    from bithtm_amd import GroupStack, RegionStack
    links = [link_of("pooled", 3)]
    train = inputs_for(1, seed=2)[0]
    trained = region_stack(I, LEVELS, 3, links=links)
    trained.run(train, 96)
    state = trained.state_dict()
    inputs = np.stack([np.roll(train, b, axis=0) for b in range(3)])       # the trained cycle, each stream entering it elsewhere
    copies = []
    for b in range(3):
        c = RegionStack(I, LEVELS, links=links, seed=3)
        c.load_state_dict(state)
        c.reset()
        copies.append(c)
    want = [c.run(x, STEPS, learning=False, record=RECORD) for c, x in zip(copies, inputs)]
    views = GroupStack.views(trained, 3)
    with pytest.raises(ValueError, match="learning=False only"):
        views.run(inputs, STEPS, learning=True)
    got = views.run(inputs, STEPS, record=RECORD)
    for b in range(3):
        for l in range(2):
            for f in COMPARED:
                x, y = np.asarray(getattr(got[b][l], f)), np.asarray(getattr(want[b][l], f))
                assert x.tobytes() == y.tobytes(), f"view {b}, level {l}: record field {f} differs"
        assert all(np.array_equal(x, y) for x, y in zip(views.link_state(0, b), copies[b].link_state(0)))
    assert all(r[0].correct_columns.sum() > 0 for r in got), "nothing was predicted: the views did not read trained weights"
    assert_same_states(whole_state(trained)[:2], [{k[3:]: v for k, v in state.items() if k.startswith(f"l{l}_")} for l in range(2)], "the trained stack")


# ---- process(), adopted stacks, growth, checkpoints
def test_process_and_run_mixed():
    from bithtm_amd import GroupStack
    inputs = inputs_for(3, rows=60)
    links = [link_of("pooled", 3)]
    stacks, _ = solo(links, inputs, steps=0)
    gs = group_stack(3, I, LEVELS, SEEDS, links=links)
    for t in range(9):
        out = gs.process(inputs[:, t])
        assert (out[1] is None) == bool((t + 1) % 3) and out[0].anomaly_score.shape == (3,)
    gs.run(inputs, 27)
    for t in range(36, 42):
        gs.process(inputs[:, t])
    with pytest.raises(ValueError):
        gs.process(inputs[0, 0])
    gs.process(inputs[:, 42])
    with pytest.raises(ValueError, match="multiples of 3"):
        gs.run(inputs, 3)                           # in the middle of a window
    for t in (43, 44):
        gs.process(inputs[:, t])
    gs.reset(np.array([False, True, False]))
    gs.run(inputs, 15)
    for b, s in enumerate(stacks):
        for t in range(60):
            if t == 45 and b == 1:
                s.reset()
            s.process(inputs[b, t])
    assert_members(gs, stacks, "process + run + process + reset + run")


def test_adopted_stacks_continue_alone():
    from bithtm_amd import GroupStack, RegionStack
    from bithtm_amd.group import SharedStream
    import bithtm_amd as B
    inputs = inputs_for(3, rows=40)
    links = [link_of("pooled", 2)]
    twins_, _ = solo(links, inputs, steps=0)
    stream = SharedStream(0)
    adopted = []
    for seed in SEEDS:
        models, below = [], I
        for l, (c, K, k) in enumerate(LEVELS):
            models.append(B.HierarchicalTemporalMemory(below, c, K, active_columns=k, seed=seed + l, stream=stream))
            below = c
        set_permanences(models, seed)
        adopted.append(RegionStack.of(models, links=links))
    for s, t, x in zip(adopted, twins_, inputs):
        s.run(x, 8)
        t.run(x, 8)
    gs = GroupStack.of(adopted)
    assert gs.steps == 8
    gs.run(inputs, 16)
    gs.process(inputs[:, 24])
    gs.process(inputs[:, 25])
    for s, t, x in zip(adopted, twins_, inputs):
        t.run(x, 16)
        t.process(x[24])
        t.process(x[25])
        assert s.steps == t.steps == 26
        s.run(x, 14)                                # ... and each goes on alone from there
        t.run(x, 14)
    for b in range(3):
        assert_same_states(whole_state(adopted[b]), whole_state(twins_[b]), f"adopted stack {b}")
    with pytest.raises(ValueError, match="stepped alone"):
        gs.run(inputs, 2)                           # (the group stack's own count stands at 26)
    assert GroupStack.of(adopted).steps == 40
    other = region_stack(I, LEVELS, 1, links=links)
    other.run(inputs[0], 40)
    with pytest.raises(ValueError, match="another stream"):
        GroupStack.of(adopted + [other])
    with pytest.raises(ValueError, match="steps"):
        GroupStack.of(adopted[:2] + [RegionStack.of(other.levels, links=links)])


def test_default_sized_pools_grow_inside_a_run():
    from bithtm_amd import GroupStack, RegionStack
    inp, levels = 120, [(1024, 4, 20), (128, 4, 8)]
    bank = np.random.RandomState(3).rand(2, 700, inp) < 0.15          # 700 different inputs per member: nothing repeats
    gs = group_stack(2, inp, levels, [9, 30], strides=[2])
    solos = [region_stack(inp, levels, s, strides=[2]) for s in (9, 30)]
    cap0 = gs.groups[0].models[0].engine.segment_capacity
    gs.run(bank, 700)
    assert gs.groups[0].models[0].engine.segment_capacity > cap0, "the pools did not have to grow: the test checks nothing"
    assert len(gs.last_run_chunks) > 1 and sum(gs.last_run_chunks) == 700
    for b, s in enumerate(solos):
        s.run(bank[b], 700)
        want, got = final_states(s), final_states(gs.members[b])
        for l in range(2):                          # (the pools may have grown to different capacities: compare what is in use)
            assert int(got[l]["tm_S"]) == int(want[l]["tm_S"])
            for key in want[l]:
                x, y = np.asarray(got[l][key]), np.asarray(want[l][key])
                if key in ("tm_presyn", "tm_perm"):
                    w = min(x.shape[1], y.shape[1])
                    assert (x[:, w:] < 0).all() and (y[:, w:] < 0).all() and x[:, :w].tobytes() == y[:, :w].tobytes(), (b, l, key)
                elif key != "tm_slots":
                    assert x.shape == y.shape and x.tobytes() == y.tobytes(), (b, l, key)


def test_state_dict_round_trip_and_a_region_stack_loads_a_member():
    from bithtm_amd import GroupStack, RegionStack
    inputs = inputs_for(3)
    links = [link_of("pooled", 3)]
    gs = group_stack(3, I, LEVELS, SEEDS, links=links)
    gs.run(inputs, 24)
    states = gs.state_dict()
    assert len(states) == 3 and int(states[1]["stack_steps"]) == 24
    other = group_stack(3, I, LEVELS, SEEDS, links=links)       # (a dictionary holds no seed: the loader is made with the member's, as a RegionStack's is)
    for member in other.members:
        set_permanences(member.levels, 77)
    other.load_state_dict(states)
    assert other.steps == 24
    alone = RegionStack(I, LEVELS, links=links, seed=SEEDS[2])
    alone.load_state_dict(states[2])
    gs.run(inputs, 24)
    other.run(inputs, 24)
    alone.run(inputs[2], 24)
    for b in range(3):
        assert_same_states(whole_state(other.members[b]), whole_state(gs.members[b]), f"after load: member {b}")
    assert_same_states(whole_state(alone), whole_state(gs.members[2]), "a RegionStack that loaded member 2")
    with pytest.raises(ValueError, match="one per member"):
        other.load_state_dict(states[:2])
    with pytest.raises(ValueError):
        group_stack(3, I, LEVELS, SEEDS, links=[3]).load_state_dict(states)


def test_a_region_stack_and_a_model_group_beside_a_group_stack_end_as_without_it():
    import bithtm_amd as B
    from bithtm_amd import GroupStack, RegionStack
    inputs = inputs_for(3)
    links = [link_of("pooled", 3)]

    def others():
        group = B.ModelGroup.create(3, I, 1024, 8, active_columns=64, seeds=[1, 2, 3])
        for m, seed in zip(group.models, (1, 2, 3)):
            set_permanences([m], seed)
        return region_stack(I, LEVELS, 11, links=[3]), group
    alone_stack, alone_group = others()
    beside_stack, beside_group = others()
    gs = group_stack(3, I, LEVELS, SEEDS, links=links)
    for _ in range(2):
        alone_stack.run(inputs[0], 24)
        alone_group.run(inputs, 24)
    for _ in range(2):
        gs.run(inputs, 24)
        beside_stack.run(inputs[0], 24)
        gs.process(inputs[:, 0])
        beside_group.run(inputs, 24)
        gs.process(inputs[:, 1])
        gs.process(inputs[:, 2])
    assert_same_states(whole_state(beside_stack), whole_state(alone_stack), "a plain RegionStack beside a GroupStack")
    assert_same_states([m.state_dict() for m in beside_group.models], [m.state_dict() for m in alone_group.models], "a ModelGroup beside a GroupStack")
