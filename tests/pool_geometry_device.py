"""Device-side helpers of the pool-geometry tests (tests/test_hip_pool_geometry.py: solo handles; tests/test_hip_group_geometry.py:
model groups and inference-view groups): a case of tests/pool_geometry_cases.py loaded into a device model, and the comparison of
one step with the oracle's record of it.  Not collected by pytest; imports the device library only inside its functions."""

import numpy as np

import pool_geometry_cases as pg
from projection_method_cases import store_snapshot


def device_model(case, state=None, capacity=None, seed=None, params=None, empty=False):
    """The case on the device: its permanence, duty cycle and exported state.  The environment is the caller's (set before this).
    A pool has at least 64 slots per row (htm_create): the cases of 32 slots keep every row within 32 synapses (their precondition)
    in a pool of 64, which is what the scan's one-chunk path is for.
    `capacity`: another segment_capacity than the case's (the members of a group need one in common); `seed`: another Temporal
    Memory seed; `params`: other TMParams; `empty`: no duty cycle and no state are loaded (an empty twin: zero duty cycles, an empty
    store, step index 0 -- its first step is the caller's)."""
    from bithtm_amd import _lib as L
    from hip_impl import make_htm
    htm = make_htm(case.I, case.C, case.K, case.k, case.seed if seed is None else seed, case.permanence.copy(), None, params or case.params,
                   segment_capacity=case.capacity if capacity is None else capacity, segment_slots=max(64, case.slots))
    eng = htm.engine
    if not empty:
        eng.write(L.F_DUTY_CYCLE, case.duty0, np.float32)
        eng.import_tm_state(case.state0 if state is None else state)
    return htm, eng


def same_store(what, got, want):
    S = len(want["seg_cell"])
    assert len(got["seg_cell"]) == S, (what, "segments", len(got["seg_cell"]), S)
    for f in ("seg_cell", "segcount", "seg_nsyn", "syn_count"):
        bad = np.flatnonzero(got[f] != want[f])
        assert len(bad) == 0, (what, f, bad[:8], got[f][bad[:8]], want[f][bad[:8]])
    row = np.repeat(np.arange(S), want["syn_count"])
    for f in ("syn_presyn", "syn_perm_bits"):
        bad = got[f] != want[f]
        assert not bad.any(), (what, f, "first rows that differ", np.unique(row[bad])[:8], int(bad.sum()))


def compare_step(case, eng, r, h_sp, h_tm, what, store=True):
    """Everything the docstring of tests/test_hip_pool_geometry.py lists, for the step of oracle record r."""
    from hip_impl import compare_with_oracle
    compare_with_oracle(what, r.sp, r.tm, h_sp, h_tm, case.K)
    od, d = r.tm.distal_state, eng.read_distal()
    assert np.array_equal(d["segment_potential"], od.segment_potential), (what, "segment_potential",
                                                                          np.flatnonzero(d["segment_potential"] != od.segment_potential)[:8])
    got, want = d["max_jittered_potential"].view(np.int32), od.max_jittered_potential.view(np.int32)
    assert np.array_equal(got, want), (what, "max_jittered_potential: cells", np.flatnonzero(got != want)[:8])
    assert np.array_equal(d["matching_segment_jittered_potential"].view(np.int32), od.matching_segment_jittered_potential.view(np.int32)), what
    info = eng.check_capacity()                      # (CapacityError is a failure: every case fits its pool)
    assert info.segments == r.S, (what, info.segments, r.S)
    alloc = (info.new_segment_requests, info.recycled_segments, info.appended_segments)
    assert alloc == (len(r.last.unaccounted), len(r.last.recycled), len(r.last.fresh)), (what, alloc)
    cnt1, cnt2 = eng.read_recyclable_counts()
    want1, want2 = pg.recount(r.nsyn, case.params.segment_matching_threshold)
    assert np.array_equal(cnt1, want1), (what, "recyclable counts per 1 024 ids: blocks", np.flatnonzero(cnt1 != want1)[:8],
                                         cnt1[cnt1 != want1][:8], want1[cnt1 != want1][:8])
    assert np.array_equal(cnt2, want2), (what, "recyclable counts per 2^20 ids", cnt2, want2)
    if store and r.store is not None:
        st = eng.read_store()
        same_store(what, store_snapshot(st["seg_cell"], st["presyn"], st["perm"], st["seg_nsyn"], st["segcount"]), r.store)


def compare_sp_weights(eng, r, what):
    """The Spatial Pooler's permanences (float64) and duty cycles (float32) by their bits, as hip_impl.compare_store_with_oracle."""
    got, want = eng.get_permanence().view(np.int64), r.perm.view(np.int64)
    assert np.array_equal(got, want), (what, "SP permanence: columns", np.unique(np.nonzero(got != want)[0])[:8])
    got, want = eng.read_duty_cycle().view(np.int32), r.duty.view(np.int32)
    assert np.array_equal(got, want), (what, "duty cycle: columns", np.flatnonzero(got != want)[:8])


def last_states(htm):
    """(sp State, tm State) of the model's last completed step, whoever enqueued it (the model, a batched run or a group)."""
    eng = htm.engine
    return type(htm.spatial_pooler).State(eng, eng.steps), htm.temporal_memory.last_state
