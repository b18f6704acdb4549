"""GPU: the stand-alone PredictiveProjection methods (`process` / `update`; htm_tm_scan / htm_tm_update) with the arguments a
caller's own TemporalMemory.process may pass and the fused step never forms -- the cases of tests/projection_method_cases.py.

Every case loads its exported store into a device projection (Engine.import_tm_state) and makes the same calls through
bithtm_amd.PredictiveProjection as the oracle did (tests/test_projection_methods_cpu.py pins that oracle to the unmodified
reference and proves that each case reaches its path).  Everything is compared EXACTLY: seg_cell, seg_nsyn, segcount, the
canonical synapses of the whole store with permanences as bit patterns, every State field of every process, htm_info's
counters, and capacity_error == 0 wherever the oracle ran out of nothing.  Each case runs once on one handle."""

from types import SimpleNamespace

import numpy as np
import pytest

import projection_method_cases as pc

pytestmark = pytest.mark.gpu


def engine_state(case, eng):
    """The case's exported state in the engine's length: per-cell arrays padded to whole words of cells."""
    n = eng.column_dim * eng.cell_dim
    st = dict(case.state0)

    def padded(a, fill=0):
        a = np.asarray(a).reshape(-1)
        out = np.full(n, fill, dtype=a.dtype)
        out[:len(a)] = a
        return out
    for f in ("segcount", "prev_prediction", "prev_activation", "max_jittered_potential", "prediction"):
        st[f] = padded(st[f])
    return st


class DeviceTarget:
    """bithtm_amd.PredictiveProjection behind the interface projection_method_cases.replay drives."""

    def __init__(self, case):
        import bithtm_amd as B
        p = case.params
        self.case = case
        self.proj = B.PredictiveProjection(case.N, segment_capacity=case.capacity or 4096, segment_slots=case.slots,
                                           **{f: getattr(p, f) for f in p.__dataclass_fields__})
        self.proj.cell_dim, self.proj.seed = case.cell_dim, case.seed
        self.eng = self.proj._ensure_engine()
        self.eng.import_tm_state(engine_state(case, self.eng))
        self.first_state = B.PredictiveProjection.State({f: np.asarray(case.state0[f]) for f in pc.STATE_FIELDS})
        self.infos = []

    def process(self, active, return_jittered_potential_info=True):
        return self.proj.process(active, return_jittered_potential_info=return_jittered_potential_info)

    def get_jittered_potential_info(self, st):
        return self.proj.get_jittered_potential_info(st)

    def update(self, prev, activation, learning, punish, winner, output_learning, eps, raises):
        from bithtm_amd.engine import CapacityError
        kw = dict(winner_input=winner, output_learning=output_learning, epsilon=eps)
        if raises == "capacity":
            with pytest.raises(CapacityError):
                self.proj.update(prev, activation, learning, punish, **kw)
            return True
        self.proj.update(prev, activation, learning, punish, **kw)
        return False

    def snapshot(self):
        st = self.eng.read_store()
        info = self.eng.info()
        self.infos.append(SimpleNamespace(segments=info.segments, requests=info.new_segment_requests, recycled=info.recycled_segments,
                                          appended=info.appended_segments, capacity_error=info.capacity_error))
        return pc.store_snapshot(st["seg_cell"], st["presyn"], st["perm"], st["seg_nsyn"], st["segcount"][:self.case.N])


def same_state(name, i, got, want):
    for f, w in want.items():
        g = np.asarray(got[f])
        if w.dtype == np.float32:
            assert g.dtype == np.float32 and np.array_equal(g.view(np.int32), w.view(np.int32)), (name, i, f)
        else:
            assert g.shape == w.shape and np.array_equal(g, w), (name, i, f, np.flatnonzero(np.asarray(g != w).reshape(-1))[:8])


def same_store(name, i, got, want, but_rows=()):
    S = len(want["seg_cell"])
    assert len(got["seg_cell"]) == S, (name, i, "segments", len(got["seg_cell"]), S)
    keep = np.ones(S, dtype=np.bool_)
    keep[np.asarray(but_rows, dtype=np.int64)] = False
    assert np.array_equal(got["seg_cell"], want["seg_cell"]), (name, i, "seg_cell", np.flatnonzero(got["seg_cell"] != want["seg_cell"])[:8])
    assert np.array_equal(got["segcount"], want["segcount"]), (name, i, "segcount")
    bad = np.flatnonzero((got["seg_nsyn"] != want["seg_nsyn"]) & keep)
    assert len(bad) == 0, (name, i, "seg_nsyn", bad[:8], got["seg_nsyn"][bad[:8]], want["seg_nsyn"][bad[:8]])
    assert np.array_equal(got["syn_count"][keep], want["syn_count"][keep]), (name, i, "valid synapses per row")
    gk, wk = np.repeat(keep, got["syn_count"]), np.repeat(keep, want["syn_count"])
    row = np.repeat(np.arange(S), want["syn_count"])[wk]
    for f in ("syn_presyn", "syn_perm_bits"):
        g, w = got[f][gk], want[f][wk]
        assert np.array_equal(g, w), (name, i, f, "first rows that differ", np.unique(row[g != w])[:8], int((g != w).sum()))


def run_case(name):
    case = pc.build(name)
    want, _ = pc.oracle_trace(name)
    dev = DeviceTarget(case)
    got = pc.replay(case, target=dev)
    assert len(got) == len(want) == len(dev.infos)
    for i, (g, w, info) in enumerate(zip(got, want, dev.infos)):
        overflow = bool(g.raised)
        if w.state is not None:
            same_state(name, i, g.state, w.state)
        same_store(name, i, g.store, w.store, but_rows=getattr(case, "overflow_rows", ()) if overflow else ())
        assert info.segments == len(w.store["seg_cell"]), (name, i)
        if w.op == "update" and w.last is not None:
            assert (info.requests, info.recycled, info.appended) == (len(w.last.unaccounted), len(w.last.recycled), len(w.last.fresh)), (name, i)
        assert (info.capacity_error != 0) == (overflow or any(x.raised for x in got[:i])), (name, i, info.capacity_error)
    return dev, got, want


@pytest.mark.parametrize("name", [n for n in pc.CASE_NAMES if n.startswith("learn_punish")])
def test_a_segment_that_learns_and_is_punished_learns_first(name):
    """projections.py:284-293: the learning update (with its growth), then the punishment, on the same row.  The case's rows
    that are in both sets hold active synapses with permanence p in [0, 0.1] (increment 0.02, punishment 0.07): learn then
    punish gives f32(f32(p + 0.02) - 0.07), pruned iff negative (p < 0.05); punish then learn prunes every p < 0.07 (the
    synapses with 0.05 <= p < 0.07 are missing, the others are f32(f32(p - 0.07) + 0.02)); learning alone leaves f32(p + 0.02)
    and prunes no active synapse; punishment alone leaves f32(p - 0.07) on active synapses and keeps every inactive one, which
    learning lowers by 0.03 and prunes below that.  The `grow` case adds synapses at 0.21 in the learning step that the
    punishment must lower to f32(0.21f - 0.07).  So a wrong order, a lost update or a row written by two work items at once
    changes counts or bit patterns of these rows; the case runs once, nothing is repeated to catch a race."""
    run_case(name)


@pytest.mark.parametrize("name", [n for n in pc.CASE_NAMES if n.startswith("multi_learning")])
def test_every_cell_of_a_column_learns_and_allocation_recycles_and_appends(name):
    run_case(name)


@pytest.mark.parametrize("name", [n for n in pc.CASE_NAMES if n.startswith("winners_")])
def test_winner_input_of_every_size_inside_and_outside_the_activation(name):
    run_case(name)


@pytest.mark.parametrize("name", ["connected_257", "connected_600", "connected_4097"])
def test_segments_connected_to_most_winners_grow_all_the_absent_ones(name):
    """A learning segment that lacks fewer of the previous winners than it may add grows exactly the absent ones (the reference
    takes min(n_add, absent), projections.py:125-127), also with more than 256 winners; growth that ends on the last slot
    raises nothing."""
    run_case(name)


def test_a_row_that_needs_one_more_slot_raises_and_leaves_the_rest_as_the_oracle():
    """segment_slots 512, a row of 483 synapses that grows 30: update raises CapacityError; every other row, the counts and
    the counters are the oracle's, the row itself keeps its 483 synapses and gains the 29 that fit."""
    dev, got, want = run_case("connected_capacity")
    row = pc.build("connected_capacity").overflow_rows[0]
    assert got[0].raised and got[0].store["seg_nsyn"][row] == 512 and want[0].store["seg_nsyn"][row] == 513


@pytest.mark.parametrize("name", [n for n in pc.CASE_NAMES if n.startswith("layout_")])
def test_cell_layouts(name):
    run_case(name)


@pytest.mark.parametrize("name", ["layout_3", "layout_4", "layout_7"])
def test_padding_bits_of_active_words_are_ignored(name):
    """htm_tm_scan directly: bits of `active_words` beyond a column's cells (33 and 48 cells in two words) and beyond
    output_dim (1 000 cells in 32 words) are set -- the States and the store must be the oracle's all the same."""
    case = pc.build(name)
    want, _ = pc.oracle_trace(name)
    dev = DeviceTarget(case)
    eng, scan = dev.eng, dev.eng.tm_scan
    K, C = eng.cell_dim, eng.column_dim
    wpc = eng.cell_words // C
    pad = np.zeros((C, 32 * wpc), dtype=np.bool_)
    pad[:, K:] = True
    if C * K > case.N:
        flat = np.zeros(C * K, dtype=np.bool_)
        flat[case.N:] = True
        pad[:, :K] |= flat.reshape(C, K)
    assert pad.any()
    extra = np.packbits(pad.reshape(C * wpc, 32), axis=1, bitorder="little").view(np.uint32).reshape(-1)
    eng.tm_scan = lambda words: scan(np.asarray(words, dtype=np.uint32) | extra)
    got = pc.replay(case, target=dev)
    for i, (g, w) in enumerate(zip(got, want)):
        if w.state is not None:
            same_state(name, i, g.state, w.state)
        same_store(name, i, g.store, w.store)
    eng.check_capacity()


@pytest.mark.parametrize("name", [n for n in pc.CASE_NAMES if n.startswith("process_")])
def test_process_on_its_own(name):
    run_case(name)


def test_earlier_and_repeated_prev_states():
    run_case("prev_states")


@pytest.mark.parametrize("name", [n for n in pc.CASE_NAMES if n.startswith("epsilon_")])
def test_epsilon_with_several_best_matching_segments_per_cell(name):
    run_case(name)


@pytest.mark.parametrize("name", [n for n in pc.CASE_NAMES if n.startswith("count_")])
def test_65535_learning_cells_in_one_call(name):
    run_case(name)


def _words(eng, cells):
    from bithtm_amd.engine import bool_to_words
    m = np.zeros(eng.column_dim * eng.cell_dim, dtype=np.bool_)
    m[cells] = True
    return bool_to_words(m.reshape(eng.column_dim, eng.cell_dim)).reshape(eng.column_dim, -1)


@pytest.mark.parametrize("shape", ["2048x32", "1024x64"])
def test_65536_learning_cells_are_refused_and_the_handle_stays_usable(shape):
    """One call with 65 536 learning cells or more: ValueError from PredictiveProjection.update, HTM_ERR_ARGUMENT from
    htm_tm_update, before anything is enqueued; the valid call that follows gives the oracle's result."""
    from bithtm_amd.engine import HtmError
    name = f"count_{shape}"
    case = pc.build(name)
    want, _ = pc.oracle_trace(name)
    dev = DeviceTarget(case)
    call = case.calls[0]
    before = dev.snapshot()
    with pytest.raises(ValueError, match="65536"):
        dev.proj.update(dev.first_state, call["activation"], np.arange(case.N), call["punish"], winner_input=call["winner"])
    ww = _words(dev.eng, np.arange(case.N))
    with pytest.raises(HtmError, match="learning cells"):
        dev.eng.tm_update(np.arange(dev.eng.column_dim), ww, ww & 0, None)
    same_store(name, "refused", dev.snapshot(), before)
    got = pc.replay(case, target=dev)
    for i, (g, w) in enumerate(zip(got, want)):
        if w.state is not None:
            same_state(name, i, g.state, w.state)
        same_store(name, i, g.store, w.store)
    dev.eng.check_capacity()


def test_refused_arguments_enqueue_nothing_and_the_next_valid_call_is_the_oracles():
    """Repeated or out-of-range ids in learning_output / winner_input / active_input (ValueError naming the cell); through the C
    entry more listed columns than active_columns, a repeated column, a column out of range (HTM_ERR_ARGUMENT); a view
    handle (HTM_ERR_STATE).  The store is untouched after all of them, and the case then runs as if nothing had been asked."""
    from bithtm_amd.engine import HtmError
    name = "layout_1"
    case = pc.build(name)
    want, _ = pc.oracle_trace(name)
    dev = DeviceTarget(case)
    call, eng = case.calls[0], dev.eng
    before = dev.snapshot()
    L = call["learning"]
    for bad, text in ((np.r_[L[:3], L[2], L[3:]], f"cell {L[2]}"), (np.r_[L, case.N], str(case.N)), (np.r_[-1, L], "-1")):
        with pytest.raises(ValueError, match=text):
            dev.proj.update(dev.first_state, call["activation"], bad, call["punish"], winner_input=call["winner"])
    with pytest.raises(ValueError, match=f"cell {call['winner'][1]}"):
        dev.proj.update(dev.first_state, call["activation"], L, call["punish"], winner_input=np.r_[call["winner"], call["winner"][1]])
    with pytest.raises(ValueError, match="cell 5"):
        dev.proj.process(np.array([5, 9, 5]))
    with pytest.raises(ValueError):
        dev.proj.process(np.array([case.N]))
    C = eng.column_dim
    ww = _words(eng, L)
    cols = np.flatnonzero(ww.any(axis=1))
    for bad_cols in (np.r_[cols[:-1], cols[0]], np.r_[cols[:-1], C], np.r_[cols[:-1], -1]):
        with pytest.raises(HtmError, match="column"):
            eng.tm_update(bad_cols, ww[cols], ww[cols] & 0, None)
    too_many = np.arange(C + 1) % C
    with pytest.raises(HtmError, match="active_columns"):
        eng.tm_update(too_many, np.ones((C + 1, ww.shape[1]), np.uint32), np.zeros((C + 1, ww.shape[1]), np.uint32), None)
    import bithtm_amd as B
    parent = B.HierarchicalTemporalMemory(64, 256, 8, active_columns=8)             # (a view needs a parent with both layers)
    view = parent.inference_view()
    one = np.ones((1, 1), dtype=np.uint32)
    with pytest.raises(HtmError, match="view"):
        view._engine.tm_update(np.array([3]), one, one & 0, None)
    del view, parent
    same_store(name, "refused", dev.snapshot(), before)
    got = pc.replay(case, target=dev)
    for i, (g, w) in enumerate(zip(got, want)):
        if w.state is not None:
            same_state(name, i, g.state, w.state)
        same_store(name, i, g.store, w.store)
    eng.check_capacity()


@pytest.mark.parametrize("how", ["mask-from-caller", "mask-built-by-the-library"])
def test_the_c_entry_with_unordered_columns_and_the_default_mask(how):
    """htm_tm_update directly: `columns` in a shuffled order with their words shuffled alike, and punish_words NULL ("every cell
    of a column not listed") against the same mask spelled out -- both must give the oracle's store for that mask."""
    name = "layout_1"
    case = pc.build(name)
    dev = DeviceTarget(case)
    eng, call = dev.eng, case.calls[0]
    K = eng.cell_dim
    listed = np.unique(call["learning"] // K)
    punish = np.ones((eng.column_dim, K), dtype=np.bool_)
    punish[listed] = False
    o = pc.fresh_oracle(case)
    o.update(o.prev_distal, call["activation"], call["learning"], punish.reshape(-1), winner_input=call["winner"])
    real = eng.tm_update
    order = np.random.RandomState(5).permutation(len(listed))
    seen = []

    def shuffled(cols, ww, uw, pw):
        assert np.array_equal(cols, listed)
        seen.append(pw is None)
        return real(np.asarray(cols)[order], np.asarray(ww)[order], np.asarray(uw)[order], pw)
    eng.tm_update = shuffled
    dev.proj.update(dev.first_state, call["activation"], call["learning"], None if how == "mask-built-by-the-library" else punish.reshape(-1),
                    winner_input=call["winner"])
    assert seen == [how == "mask-built-by-the-library"]
    same_store(name, how, dev.snapshot(), pc.oracle_snapshot(o))
    eng.check_capacity()
