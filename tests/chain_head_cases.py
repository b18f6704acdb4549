"""Cases for the winner rows' update (tests/test_hip_winner_rows.py: role_sp_row with its increments and threshold in registers):
a small model, its inputs, the oracle's record of every step
(computed once per process and shared, left unchanged by the tests) and the comparison of a device model with it.
tests/test_chain_head_cases_cpu.py proves that each case reaches the path it is for.  Not collected by pytest; imports the device
library only inside its functions."""

from types import SimpleNamespace

import numpy as np

from oracle import HTMOracle, SPParams, TMParams

# calls of a batched run whose ends are compared field by field (30 steps in all; every call's last step takes the plan of a
# call's end, every other step the steady two-launch step)
CHUNKS = (1, 2, 3, 5, 8, 11)

ROWS = {
    # role_sp_row: I not a multiple of 128 (one partial wave), the padded tail (130: two elements into the second 128), the
    # bench's width (four full passes of a 256-thread block); defaults: increments 0.03 : 0.015 and threshold 0
    "rows_i100": dict(I=100, C=512, K=8, k=20, seed=3),
    "rows_i130": dict(I=130, C=512, K=8, k=20, seed=4),
    "rows_i1024": dict(I=1024, C=512, K=8, k=20, seed=5),
    # a threshold above zero and increments that are not 2 : 1 (0.07 - 0.013 and -0.013 as float64 sums; permanences drawn around
    # the threshold so that bits cross it both ways)
    "rows_i130_thr": dict(I=130, C=512, K=8, k=20, seed=6,
                          sp=dict(permanence_mean=0.05, permanence_std=0.05, permanence_threshold=0.05, permanence_increment=0.07,
                                  permanence_decrement=0.013)),
}

_built, _traces = {}, {}


def build(name):
    if name not in _built:
        spec = dict(steps=30, noise=0.03, patterns=4, density=0.12, sp={}, tm={})
        spec.update(ROWS[name])
        sp_params, tm_params = SPParams(**spec["sp"]), TMParams(**spec["tm"])
        rng = np.random.RandomState(spec["seed"])
        permanence = sp_params.permanence_mean + sp_params.permanence_std * rng.randn(spec["C"], spec["I"])
        pats = rng.rand(spec["patterns"], spec["I"]) < spec["density"]
        # one bank row per step (a batched run reads row t % steps at step t): the patterns cycled, each showing with noise of its own
        bank = np.stack([pats[t % len(pats)] ^ (rng.rand(spec["I"]) < spec["noise"]) for t in range(spec["steps"])])
        _built[name] = SimpleNamespace(name=name, I=spec["I"], C=spec["C"], K=spec["K"], k=spec["k"], seed=spec["seed"], steps=spec["steps"],
                                       sp_params=sp_params, tm_params=tm_params, permanence=permanence, bank=bank)
    return _built[name]


def oracle_trace(name):
    """(records, oracle): one record per step -- sp / tm (the States), last (the oracle's last_update), S, new (winner cells without
    a matching segment in the state before) -- and the oracle as the last step left it."""
    if name not in _traces:
        case = build(name)
        ora = HTMOracle(case.I, case.C, case.K, active_columns=case.k, seed=case.seed, sp_params=case.sp_params, tm_params=case.tm_params,
                        permanence=case.permanence.copy())
        tm, out = ora.temporal_memory, []
        for t in range(case.steps):
            o_sp, o_tm = ora.step(case.bank[t], learning=True)
            out.append(SimpleNamespace(t=t, sp=o_sp, tm=o_tm, last=tm.last_update, S=tm.S))
        _traces[name] = (out, ora)
    return _traces[name]


def alloc_counts(r):
    """(winner cells without a segment, recycled ids, fresh ids) of the step of record r; the first step has no state before it."""
    return (0, 0, 0) if r.last is None else (len(r.last.unaccounted), len(r.last.recycled), len(r.last.fresh))


def device_model(case, capacity=None):
    from hip_impl import make_htm
    return make_htm(case.I, case.C, case.K, case.k, case.seed, case.permanence.copy(), case.sp_params, case.tm_params,
                    segment_capacity=capacity)


def compare_step(case, htm, r, h_sp, h_tm, what):
    """Active columns, overlaps, cell activation and prediction, winner cells, matching segments with their potentials
    (hip_impl.compare_with_oracle), max_jittered_potential and the matching segments' jittered potential by their bits, the
    allocation's counts, a clean capacity check -- of the step of oracle record r."""
    from hip_impl import compare_with_oracle
    eng = htm.engine
    compare_with_oracle(what, r.sp, r.tm, h_sp, h_tm, case.K)
    od, d = r.tm.distal_state, eng.read_distal()
    assert np.array_equal(d["segment_potential"], od.segment_potential), (what, "segment_potential")
    got, want = d["max_jittered_potential"].view(np.int32), od.max_jittered_potential.view(np.int32)
    assert np.array_equal(got, want), (what, "max_jittered_potential: cells", np.flatnonzero(got != want)[:8])
    assert np.array_equal(d["matching_segment_jittered_potential"].view(np.int32), od.matching_segment_jittered_potential.view(np.int32)), what
    info = eng.check_capacity()
    assert info.segments == r.S, (what, info.segments, r.S)
    alloc = (info.new_segment_requests, info.recycled_segments, info.appended_segments)
    assert alloc == alloc_counts(r), (what, alloc, alloc_counts(r))


def host_fed(name, capacity=None):
    """The case step by step through process(), compared after every step; the whole store, permanences and duty cycles at the end."""
    from hip_impl import compare_store_with_oracle
    case, (tr, ora) = build(name), oracle_trace(name)
    htm = device_model(case, capacity)
    for r in tr:
        h_sp, h_tm = htm.process(case.bank[r.t], learning=True)
        compare_step(case, htm, r, h_sp, h_tm, (name, "process", r.t))
    compare_store_with_oracle((name, "process"), ora, htm)


def batched(name, capacity=None):
    """The case through htm.run in the default, two-launch schedule (graph replay).  One call over all steps with a record: after
    every step the active columns, the predicted columns and the counters -- bursting columns, active cells, winner cells, segments,
    new segments -- are the oracle's; then the store.  A second model takes the steps in calls of CHUNKS steps: after every call every
    field of compare_step."""
    from hip_impl import compare_store_with_oracle
    from pool_geometry_device import last_states
    from bithtm_amd.engine import RECORD_COUNTERS
    case, (tr, ora) = build(name), oracle_trace(name)
    assert sum(CHUNKS) >= case.steps
    htm = device_model(case, capacity)
    plan = htm.engine.run_plan(case.steps)
    assert plan["hip_graph"] and plan["pipelined"] and not plan["scan_large"], plan
    rec = htm.run(case.bank, case.steps, learning=True, record=("counters", "active_column", "column_prediction"))
    got = np.stack([getattr(rec, f) for f in RECORD_COUNTERS], axis=1)
    prev = np.zeros(case.C, bool)
    for r in tr:
        pred = r.tm.cell_prediction.any(axis=1)
        want = [len(r.sp.active_column), int(r.tm.active_column_bursting.sum()), int(prev.sum()), int(pred.sum()), len(r.tm.active_cell[0]),
                len(r.tm.winner_cell[0]), r.S, alloc_counts(r)[0]]
        assert got[r.t].tolist() == want, (name, "run", r.t, got[r.t].tolist(), want)
        assert np.array_equal(np.sort(rec.active_column[r.t]), np.sort(r.sp.active_column)), (name, "run", r.t, "active columns")
        assert np.array_equal(rec.column_prediction[r.t], pred), (name, "run", r.t, "predicted columns")
        prev = pred
    compare_step(case, htm, tr[-1], *last_states(htm), (name, "run", "end"))
    compare_store_with_oracle((name, "run"), ora, htm)
    htm = device_model(case, capacity)
    done = 0
    for n in CHUNKS:
        n = min(n, case.steps - done)
        if n == 0:
            break
        htm.run(case.bank, n, learning=True)
        done += n
        compare_step(case, htm, tr[done - 1], *last_states(htm), (name, "run in calls", done - 1))
    compare_store_with_oracle((name, "run in calls"), ora, htm)
