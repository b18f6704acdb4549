"""GPU: model groups and inference-view groups (htm_group_step / htm_group_run: kgrp_middle, kgrp_tail, kgrp_learn, kgrp_scan,
kgrp_scan_shared -- bithtm_amd/csrc/htm_group.h, group_enqueue_step) on the group plans of tests/group_geometry_cases.py: members of ONE
launch in different size-dependent forms of the allocation, the classification, the sparse clear and the scan, each held to its own
oracle record.  tests/test_group_geometry_cpu.py proves on the oracle what each plan reaches, that no two members could pass with
each other's state, and that the expectations are the oracle's that tests/golden/pool_geometry.npz pins to the reference.

Learning groups: every plan under the three forms of the group's last launches (FORMS), stepped by group.process (the eager
htm_group_step; every member compared after every step) and by one group.run with records (replayed as a hipGraph; compared at the
end, and the records' step_index, active_column, bursting_columns and new_segments with the trace); then every member takes one
more step ALONE and is compared again -- the group must leave nothing behind that a solo launch reads (hints, fan counters, match
bits).  Compared EXACTLY per member: everything pool_geometry_device.compare_step lists (every field of compare_with_oracle, the
whole segment_potential, max_jittered_potential by its bits, the store, htm_info's allocation counters, the recyclable counts
against a recount, check_capacity) and the Spatial Pooler's permanences and duty cycles by their bits (kgrp_tail's and
kgrp_middle's role_sp_row: both row placements).

View groups: every view plan under five forms of the scan (VIEW_FORMS), stepped by group.process and, from fresh views, by one
recorded group.run; every view held to its oracle in the SP and TM fields of compare_with_oracle (prediction bits and the matching
rows' potentials and activations among them), the whole segment_potential, the bits of max_jittered_potential and of the matching
rows' jittered potentials, and its duty cycles; the parent's store and permanences byte-identical before and after.

Nothing is skipped, repeated to catch a race, or run on a mutated kernel.  No two forms here take the same launches, so the product
is run in full: 12 plans x 3 forms x 2 modes, 4 view plans x 5 forms (the four asked for, whose default turns out to scan inside
kgrp_tail, and kgrp_scan's small form, which no other view form would launch)."""

from types import SimpleNamespace

import numpy as np
import pytest

import group_geometry_cases as gg
import pool_geometry_cases as pg
from pool_geometry_device import compare_sp_weights, compare_step, device_model, last_states

pytestmark = pytest.mark.gpu

ALL = ("counters", "active_column", "column_prediction")
# the last launches of a learning group step: kgrp_tail (learning role + scan + permanence rows); kgrp_learn + kgrp_scan in the large
# form, the permanence rows in kgrp_middle; the same two launches in the small form
FORMS = {"fused-tail": {}, "scan-large": {"BITHTM_SCAN_LARGE": "1"}, "learn+scan": {"BITHTM_FUSE_TM": "0"}}
# a view group's scan, per member: role_scan inside kgrp_tail (the default; no permanence rows with learning off), kgrp_scan in the small
# and the large form; for all members of a chunk: kgrp_scan_shared with M = min(16, B) members per chunk, and with 2
VIEW_FORMS = {"per-member": {}, "per-member-unfused": {"BITHTM_FUSE_TM": "0"}, "per-member-large": {"BITHTM_SCAN_LARGE": "1"}, "shared": {"BITHTM_SHARED_SCAN": "1"},
              "shared-M2": {"BITHTM_SHARED_SCAN": "1", "BITHTM_SHARED_SCAN_MEMBERS": "2"}}
MODES = ("process", "run")
# the launches each form must make, by the names the engine's profile keeps them under (member 0's handle: group_enqueue_step)
LAUNCHES = {"fused-tail": {"group:tm_learn+tm_scan+sp_learn"}, "scan-large": {"group:tm_learn", "group:tm_scan_large"}, "learn+scan": {"group:tm_learn", "group:tm_scan"},
            "per-member": {"group:tm_learn+tm_scan"}, "per-member-unfused": {"group:tm_learn", "group:tm_scan"}, "per-member-large": {"group:tm_learn", "group:tm_scan_large"},
            "shared": {"group:tm_learn", "group:tm_scan_shared"}, "shared-M2": {"group:tm_learn", "group:tm_scan_shared"}}
TAILS = set().union(*LAUNCHES.values())


def _form_of(env, forms):
    return next(fid for fid, e in forms.items() if e == env)


def _plan(name):
    return gg.mixed_plan() if name == "mixed" else gg.learning_plan(name)


def _compare(m, htm, r, what):
    """Member m after the step of its record r: compare_step as the solo tests use it (the thresholds are the member's own: an
    empty twin may have other ones than its case), then the Spatial Pooler's rows."""
    h_sp, h_tm = last_states(htm)
    compare_step(SimpleNamespace(K=m.case.K, params=m.params), htm.engine, r, h_sp, h_tm, what)
    compare_sp_weights(htm.engine, r, what)


def _members_on_the_device(plan, what):
    """Every member as the plan says it joins the group: the case imported (member 3: under its own seed), member 1 two learning
    steps on, an empty twin after its one step with learning off -- each step taken alone compared like any other."""
    from hip_impl import compare_with_oracle
    models = []
    for i, m in enumerate(plan.members):
        case, bank = m.case, m.case.bank()
        htm, eng = device_model(case, capacity=plan.capacity, seed=m.seed, params=m.params, empty=m.kind == "empty")
        if m.kind == "empty":
            h_sp, h_tm = htm.process(case.patterns[case.first], learning=False)
            compare_with_oracle((what, i, "first"), m.first[0], m.first[1], h_sp, h_tm, case.K)
            assert eng.info().segments == 0
        for r in m.alone:
            htm.process(bank[r.t % len(bank)], learning=True)
            _compare(m, htm, r, (what, i, "alone before", r.t))
        assert eng.steps == m.trace[0].t
        models.append(htm)
    return models


@pytest.mark.parametrize("name,env,mode", [pytest.param(n, env, mode, id=f"{n}-{fid}-{mode}") for n in pg.SMALL + ["mixed"]
                                           for fid, env in FORMS.items() for mode in MODES])
def test_members_in_different_forms_of_one_launch_each_equal_their_oracle(name, env, mode, monkeypatch):
    """What a group-only fault would change (tests/test_group_geometry_cpu.py asserts each premise):
      * a member's state read from tab[0] or tab[y +- 1], in any role: no two members of a plan share an expected state -- the store, S,
        the winners or matching_segment of that member differ at once;
      * kgrp_middle's match bits zeroed by member 0's S, or a grid sized for one member cutting another's rows short: the empty twin
        (S = 0, appending from id 0) and member 1 (a larger S than member 0's) keep stale bits or lose rows -- the next step's
        classification, which every plan's step alone behind the group runs, differs;
      * the speculation bound n_spec taken from another member than the smallest (the twin's hint is 0 while alloc_many_blocks and
        classify_words alone would speculate over 1 024 blocks and more): rows past the twin's S are scanned as if they existed --
        matching_segment, the per-cell maxima or a capacity flag differ;
      * thresholds, punishment or seed read through another member's Dev (the mixed plan: matching threshold 8 beside 4, punishment
        0.3 beside 0.01; member 3's seed): the recyclable counts, the punished rows' permanences, the winners or the grown
        synapses differ;
      * role_sp_row of kgrp_tail / kgrp_middle reading another member's bank row (member 1 is at another row of its bank than the
        others in the same launch) or writing half a float64: the permanences differ by their bits;
      * a hint, fan counter or match bit left behind by the group: the step each member then takes alone differs."""
    import bithtm_amd as B
    plan = _plan(name)
    for key, value in env.items():
        monkeypatch.setenv(key, value)
    what = (plan.name, mode)
    models = _members_on_the_device(plan, what)
    group = B.ModelGroup(models)
    n = plan.n_group
    e0 = models[0].engine
    if "BITHTM_SCAN_LARGE" in env:
        assert e0.run_plan(n)["scan_large"]
    banks = np.stack([m.case.bank() for m in plan.members])
    if mode == "process":
        e0.profile(True)                            # (the eager path; a profiled handle would not replay graphs)
        for t in range(n):
            X = np.stack([banks[i][m.trace[t].t % banks.shape[1]] for i, m in enumerate(plan.members)])
            rec = group.process(X, learning=True)
            assert rec.step_index.tolist() == [m.trace[t].t for m in plan.members]
            for i, (m, htm) in enumerate(zip(plan.members, models)):
                _compare(m, htm, m.trace[t], (what, "member", i, "group step", t))
        launched = e0.profile_read()
        e0.profile(False)
        assert set(launched) & TAILS == LAUNCHES[_form_of(env, FORMS)] and launched["group:tm_mid"][1] == n, (what, sorted(launched))
    else:
        assert e0.run_plan(n)["hip_graph"], "the group run would launch eagerly"
        recs = group.run(banks, n, learning=True, record=ALL)
        for i, (m, htm, rec) in enumerate(zip(plan.members, models, recs)):
            tr = m.trace[:n]
            assert htm.engine.steps == tr[-1].t + 1
            assert rec.step_index.tolist() == [r.t for r in tr], (what, i, rec.step_index)
            assert np.array_equal(rec.active_column, np.stack([r.sp.active_column for r in tr])), (what, i, "active_column")
            assert rec.bursting_columns.tolist() == [int(r.tm.active_column_bursting.sum()) for r in tr], (what, i, rec.bursting_columns)
            assert rec.new_segments.tolist() == [len(r.last.recycled) + len(r.last.fresh) for r in tr], (what, i, rec.new_segments)
            assert np.array_equal(rec.column_prediction, np.stack([r.tm.cell_prediction.any(axis=1) for r in tr])), (what, i, "column_prediction")
            _compare(m, htm, tr[-1], (what, "member", i, "end of the run"))
    for i, (m, htm) in enumerate(zip(plan.members, models)):       # one more step, alone
        r = m.trace[n]
        htm.process(banks[i][r.t % banks.shape[1]], learning=True)
        _compare(m, htm, r, (what, "member", i, "alone behind the group"))


def _weights(m):
    st = m.engine.read_store()
    return m.engine.get_permanence().tobytes(), {k: np.asarray(v).tobytes() for k, v in st.items()}


def _compare_view(case, view, r, what):
    from hip_impl import compare_with_oracle
    h_sp, h_tm = last_states(view)
    compare_with_oracle(what, r.sp, r.tm, h_sp, h_tm, case.K)
    od, d = r.tm.distal_state, view.engine.read_distal()
    assert np.array_equal(d["segment_potential"], od.segment_potential), (what, "segment_potential", np.flatnonzero(d["segment_potential"] != od.segment_potential)[:8])
    got, want = d["max_jittered_potential"].view(np.int32), od.max_jittered_potential.view(np.int32)
    assert np.array_equal(got, want), (what, "max_jittered_potential: cells", np.flatnonzero(got != want)[:8])
    assert np.array_equal(d["matching_segment_jittered_potential"].view(np.int32), od.matching_segment_jittered_potential.view(np.int32)), (what, "jittered potentials")
    assert np.array_equal(view.engine.read_duty_cycle().view(np.int32), r.duty.view(np.int32)), (what, "duty cycle")
    view.engine.check_capacity()


@pytest.mark.parametrize("name,B,env", [pytest.param(n, b, env, id=f"{n}-B{b}-{fid}") for n, b in gg.VIEW_PLANS for fid, env in VIEW_FORMS.items()])
def test_views_of_one_crafted_store_each_equal_their_oracle(name, B, env, monkeypatch):
    """ModelGroup.views over the crafted rows as imported (nothing learns: every ROW_KINDS x ROW_SIZES row is scanned by every view
    that shows its source pattern), view i on inputs of its own, one view on an all-zero input.
      * kgrp_scan_shared's chunk loop ending at 32 slots, or its `valid` mask off by one: rows of 33, 63 and 64 synapses are short
        (match_pot, matching_segment); a slot past a row's count read as cell 0: a potential too large;
      * potential and connected count packed into one word carrying into each other, or `>` for `>=` at either threshold or at
        f32(threshold): match_act / match_active of the rows at A, A - 1 and on the threshold differ, then prediction bits;
      * a member's accumulator, bitmap (s_bits + m * cw), act words, thresholds, seed or step read from its neighbour, in a chunk of 16,
        5, 2 or 1: views that show different inputs differ in matching_segment and the maxima; the jitter key is the member's own step;
      * the second cell word (cell_dim 48) or the last partial word of match bits (S = 70 003) dropped: matching rows are missing;
      * a member without any hit in a 16-row group taking its neighbour's `if (hit)` / `__any(matching)` branch: rows appear or vanish;
      * anything written into the shared store or the parent's permanences: the parent's bytes differ."""
    import bithtm_amd as Bm
    plan, T = gg.view_plan(name, B), gg.VIEW_STEPS
    case = plan.case
    for key, value in env.items():
        monkeypatch.setenv(key, value)
    parent, eng = device_model(case)
    if "BITHTM_SCAN_LARGE" in env:
        assert eng.run_plan(T)["scan_large"]
    before = _weights(parent)
    group = Bm.ModelGroup.views(parent, B)
    group.models[0].engine.profile(True)
    for t in range(T):
        rec = group.process(plan.shown[:, t])
        assert rec.step_index.tolist() == [eng.steps + t] * B
        for i, v in enumerate(group.models):
            _compare_view(case, v, plan.trace[i][t], (plan.name, "process", "view", i, "step", t))
    launched = group.models[0].engine.profile_read()
    group.models[0].engine.profile(False)
    assert set(launched) & TAILS == LAUNCHES[_form_of(env, VIEW_FORMS)] and launched["group:tm_mid"][1] == T, (plan.name, sorted(launched))
    assert _weights(parent) == before
    del group
    group = Bm.ModelGroup.views(parent, B)                # fresh views: as after a reset, at the parent's step index
    assert eng.run_plan(T)["hip_graph"], "the group run would launch eagerly"
    recs = group.run(plan.bank, T, record=ALL)
    for i, (v, rec) in enumerate(zip(group.models, recs)):
        tr = plan.trace[i]
        assert rec.step_index.tolist() == [eng.steps + t for t in range(T)], (plan.name, i, rec.step_index)
        assert np.array_equal(rec.active_column, np.stack([r.sp.active_column for r in tr])), (plan.name, i, "active_column")
        assert np.array_equal(rec.column_prediction, np.stack([r.tm.cell_prediction.any(axis=1) for r in tr])), (plan.name, i, "column_prediction")
        assert rec.bursting_columns.tolist() == [int(r.tm.active_column_bursting.sum()) for r in tr], (plan.name, i, rec.bursting_columns)
        assert rec.new_segments.tolist() == [0] * T and rec.segments.tolist() == [int(case.state0["S"])] * T
        _compare_view(case, v, tr[-1], (plan.name, "run", "view", i, "end"))
    assert _weights(parent) == before
