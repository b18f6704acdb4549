"""The group plans of tests/group_geometry_cases.py without a device: every precondition that makes
tests/test_hip_group_geometry.py mean what it says, proved on the oracle alone.  A precondition that does not hold is a failure.

  * the expectations are the pinned oracle's: member 0's records are pg.oracle_trace's, member 1's are the same trace two steps on;
  * members never share an expected state: at every group step any two members differ in a compared array, and every NumPy mutant
    that hands member i the expectation of member j is caught (a kernel that read tab[0], or tab[y +- 1], fails on the device);
  * phase-shifted plans: at the first group step members 0 and 1 (and the empty twin) are in different size-dependent forms --
    FORMS says which, per case, from the oracle's last_update;
  * the empty twin stays small enough for the group's speculation bound to be 0;
  * the mixed plan keeps the three cases' own preconditions at the common capacity, and has a punishing member beside members
    that do not punish;
  * view plans: what the scans reach (potential 64, M, M - 1, activation A, A - 1, a permanence on f32(threshold) and one ulp below, a
    row of 33 synapses, an owner cell >= 32, the last partial word) and how the members of one launch differ (a 16-row group
    that matches in one member of a chunk and not in another; a row that matches in two members of a chunk at different
    potentials).

Three statements of the plans' specification cannot hold and are replaced by what the oracle shows (each where it is asserted):
an empty twin appends k rows per step, which is under 64 only for k < 64; the mixed plan's empty twin grows min(16, 8 winners) = 8
synapses per row; with P = 2 patterns two of five views see the same inputs, and no input of scan_rows_* leaves a view without a
matching row."""

import numpy as np
import pytest

import group_geometry_cases as gg
import pool_geometry_cases as pg

SCAN_SEGS = 64                  # bithtm_amd/csrc/htm_dev.h: rows per block iteration of the scan; n_spec = min(hint / SCAN_SEGS, blocks) & ~63
GRP_SHARED_MMAX = 16            # bithtm_amd/csrc/htm_group.h


def test_the_constants_are_the_library_s():
    import os
    import re
    root = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "bithtm_amd", "csrc")
    dev, grp, eng = (open(os.path.join(root, f)).read() for f in ("htm_dev.h", "htm_group.h", "htm_engine.hip"))
    assert int(re.search(r"#define SCAN_SEGS (\d+)", dev).group(1)) == SCAN_SEGS
    assert int(re.search(r"#define GRP_SHARED_MMAX (\d+)", grp).group(1)) == GRP_SHARED_MMAX
    assert "f.spec = std::min(lo / SCAN_SEGS, h0->sz.scan_blocks) & ~63;" in eng


def _plans():
    return [gg.learning_plan(n) for n in pg.SMALL] + [gg.mixed_plan()]


@pytest.mark.parametrize("name", pg.SMALL)
def test_the_expectations_are_the_pinned_oracle_s(name):
    """Member 0's and member 1's records are pg.oracle_trace's (which tests/test_pool_geometry_cpu.py holds to the recorded
    reference), step for step; the steps past the case's own stay within the device's rows of 64 slots and the plan's capacity."""
    plan, tr = gg.learning_plan(name), pg.oracle_trace(name)
    n = len(tr)
    assert plan.n_group == n - 2 >= 1 and len(plan.full) == n + 1
    for a, b in zip(plan.full, tr):
        assert a.t == b.t and a.S == b.S and not gg.differing(gg.expectation(a), gg.expectation(b))
    m0, m1, m2, m3 = plan.members
    assert [r.t for r in m0.trace] == list(range(1, plan.n_group + 2)) and [r.t for r in m1.alone] == [1, 2]
    assert [r.t for r in m1.trace] == list(range(3, plan.n_group + 4)) and len(m2.trace) == len(m3.trace) == plan.n_group + 1
    for m in plan.members:
        assert len(m.trace) == plan.n_group + 1
        for r in m.trace:
            assert r.slots <= 64 and r.nsyn.max() <= 64 and r.S <= plan.capacity, (name, m.kind, r.t, r.slots, r.S)
    assert m3.seed != m0.seed


def test_members_never_share_an_expected_state():
    """At every group step (and the step alone behind it) any two members differ in S, the winner cells, matching_segment or the
    store -- so does every mutant: member i compared with member j's expectation is reported, with its own it is not."""
    for plan in _plans():
        for t in range(plan.n_group + 1):
            ex = [gg.expectation(m.trace[t]) for m in plan.members]
            for i, want in enumerate(ex):
                assert gg.differing(want, want) == []
                for j, other in enumerate(ex):
                    if i != j:
                        assert gg.differing(other, want), (plan.name, t, "member", i, "could pass with the state of member", j)


def _ids(x):
    return np.asarray(x, dtype=np.int64).tolist()


def _forms_block_edges(m0, m1, m2):
    assert _ids(m0.recycled) == [0, 1023, 1024] and len(m0.fresh) == 0, "member 0 does not recycle across the 1 024-id block edge"
    assert len(m1.recycled) == 0 and len(m1.fresh) == 8 and m1.fresh[0] > 3072, "member 1 does not only append"


def _forms_exact_cut(m0, m1, m2):
    assert len(m0.recycled) >= 39 and len(np.unique(m0.recycled >> 10)) == 6, "member 0's cut does not fall in the sixth block"
    assert len(m1.recycled) == 0 and len(m1.fresh) == 48


def _forms_many_blocks(m0, m1, m2):
    assert len(np.unique(m0.recycled >> 10)) > 128, "member 0's needed blocks fit NEED_LDS"
    assert len(m1.recycled) == 0 and len(m1.fresh) == 176, "member 1 needs a block"
    assert len(m2.recycled) == 0 and _ids(m2.fresh) == list(range(176)), "the empty twin does not append from id 0"


def _forms_stay_dead(m0, m1, m2):
    assert len(m0.recycled) == 0 and _ids(m0.fresh) == [1023, 1024], "member 0 does not append across the block edge"
    assert _ids(m1.recycled) == [1023, 1024] and len(m1.fresh) == 0, "member 1 does not recycle the rows that stayed dead"
    assert _ids(m2.fresh) == [0, 1]


def _forms_after_death(m0, m1, m2):
    assert len(m0.punished) == 7 and _ids(m0.recycled) == [2000, 2001, 2002, 2003], "member 0 does not punish rows to death"
    assert len(m1.punished) == 0 and len(m1.recycled) == 5 and len(m1.fresh) == 3, "member 1 does not recycle the rest and append"


def _forms_classify(m0, m1, m2):
    assert len(m0.learning) > 100 and len(m0.punished) > 100 and len(m1.learning) > 100 and len(m1.punished) > 100
    assert not np.intersect1d(np.r_[m0.learning, m0.punished] >> 5, np.r_[m1.learning, m1.punished] >> 5).size, "members 0 and 1 classify the same words"
    assert (np.r_[m0.learning, m0.punished] >> 5).max() == (70003 - 1) >> 5, "member 0 does not classify the last, partial word"
    assert len(m2.learning) == 0 and len(m2.punished) == 0 and len(m2.fresh) == 64


def _forms_scan_rows(m0, m1, m2):
    cover = np.arange(16) * 16 + 5
    assert _ids(m0.learning) == _ids(cover) and len(m0.punished) == 0, "member 0: a crafted row is on the work list (not the plain scan)"
    listed = np.union1d(m1.learning, m1.punished)
    assert len(np.setdiff1d(listed, cover)) > 100 and len(m1.punished) > 50 and len(m1.learning) > 10, "member 1: the crafted rows are not listed (no SELF form)"
    assert len(m2.learning) == 0 and _ids(m2.fresh) == list(range(16))


# which size-dependent forms members 0, 1 (and 2) are in at the FIRST group step, from the oracle's last_update of that step
FORMS = {
    "alloc_block_edges_1": _forms_block_edges, "alloc_block_edges_1023": _forms_block_edges, "alloc_exact_cut_minus1": _forms_exact_cut,
    "alloc_exact_cut_equal": _forms_exact_cut, "alloc_exact_cut_plus1": _forms_exact_cut, "alloc_many_blocks": _forms_many_blocks,
    "alloc_stay_dead": _forms_stay_dead, "alloc_after_death": _forms_after_death, "classify_words": _forms_classify,
    "scan_rows_k32": _forms_scan_rows, "scan_rows_k48": _forms_scan_rows,
}


@pytest.mark.parametrize("name", pg.SMALL)
def test_members_0_and_1_are_in_different_forms_at_the_first_group_step(name):
    assert list(FORMS) == pg.SMALL
    plan = gg.learning_plan(name)
    m0, m1, m2, m3 = (m.trace[0].last for m in plan.members)
    FORMS[name](m0, m1, m2)
    assert len(m2.recycled) == 0 and len(m2.learning) == 0 and len(m2.punished) == 0 and m2.fresh[0] == 0, "the empty twin does not append from id 0"
    # (member 3: the allocation does not depend on the seed -- the same ids as member 0 -- and the draws do)
    assert _ids(m3.recycled) == _ids(m0.recycled) and _ids(m3.fresh) == _ids(m0.fresh)
    a, b = plan.members[0].trace[0], plan.members[3].trace[0]
    assert {"syn_presyn", "winner"} & set(gg.differing(gg.expectation(a), gg.expectation(b))), "the second seed draws what the first drew"


def test_the_empty_twin_stays_small():
    """0 < S at the end of every plan, and S <= k rows per step taken (every active column bursts without a match: one appended row
    each) -- under 64 rows per step wherever k < 64, as the plans' specification puts it; classify_words (k = 64) and
    alloc_many_blocks (k = 176) append k.  What the bound is for holds everywhere: the twin's segment count, which is its hint, keeps the
    group's speculation bound min(lo / SCAN_SEGS, blocks) & ~63 at 0, while member 0's alone is not 0 in the five cases of 4 096 rows and more."""
    nonzero = []
    for plan in _plans():
        twin = next(m for m in plan.members if m.kind == "empty")
        steps = plan.n_group + 1
        S, k = twin.trace[-1].S, twin.case.k
        assert 0 < S <= k * steps, (plan.name, S)
        assert k >= 64 or S < 64 * steps, (plan.name, S)
        assert all((r.S // SCAN_SEGS) & ~63 == 0 for r in twin.trace), (plan.name, "the twin's hint lets the group speculate")
        if (int(plan.members[0].case.state0["S"]) // SCAN_SEGS) & ~63:
            nonzero.append(plan.name)
    assert nonzero == ["alloc_exact_cut_minus1", "alloc_exact_cut_equal", "alloc_exact_cut_plus1", "alloc_many_blocks", "classify_words"]


def test_the_mixed_plan_keeps_its_cases_and_mixes_punishment():
    plan = gg.mixed_plan()
    assert plan.n_group == 3 and [m.kind for m in plan.members] == ["case", "case", "case", "empty"]
    for name, m in zip(gg.MIXED, plan.members):
        case, tr = pg.build(name), pg.oracle_trace(name)
        assert m.case is case and plan.capacity >= case.capacity and m.trace[-1].S <= plan.capacity
        for a, b in zip(m.trace, tr):                # (the oracle knows no capacity: the first three records are the case's own trace)
            assert a.S == b.S and not gg.differing(gg.expectation(a), gg.expectation(b))
        for fn in case.checks:
            fn(case, m.trace[:3])
        pg.check_preconditions(name)
    twin = plan.members[3]
    assert (twin.params.segment_activation_threshold, twin.params.segment_matching_threshold, twin.params.segment_sampling_synapses) == (9, 8, 16)
    assert all(m.params.segment_matching_threshold == 4 for m in plan.members[:3])
    assert len({m.params.permanence_punishment for m in plan.members}) == 2 and len({int(m.case.state0["S"]) for m in plan.members[:3]}) == 3
    # the twin's rows: one synapse to each of the k = 8 previous winner cells -- min(16, 8), where the specification says 16 (a step
    # has one winner per bursting column: 8) -- which is exactly its own matching threshold (alive) and twice the others'
    for r in twin.trace:
        assert len(r.last.fresh) == 8 and (r.nsyn[r.last.fresh] == 8).all() and twin.params.segment_matching_threshold == 8
        assert pg.recount(r.nsyn, 8)[0].sum() == 0 and pg.recount(r.nsyn, 9)[0].sum() == r.S
    punishing = [[len(m.trace[t].last.punished) > 0 for m in plan.members] for t in range(plan.n_group)]
    assert any(any(row) and not all(row) for row in punishing), "no step at which one member punishes and another does not"


# ------------------------------------------------------------------------------------------ views

def _chunks(B, M):
    return [list(range(lo, min(lo + M, B))) for lo in range(0, B, M)]


@pytest.mark.parametrize("name,B", gg.VIEW_PLANS)
def test_views_differ_wherever_their_inputs_differ(name, B):
    """At every step: views that show different inputs differ in a compared array, and so does every such mutant; views with the
    same inputs so far are equal (P = 2: views 0 and 2 -- a plan of five views over two patterns cannot avoid it).  Hence a scan that
    took every member's state from tab[0] fails (some view shows another input than view 0 at every step), and one that took it from
    tab[y + 1] or tab[y - 1] fails too (views 0, 1 and 2 -- a pattern, the all-zero input, a pattern -- differ at every step)."""
    plan = gg.view_plan(name, B)
    assert gg.ZERO_VIEW == 1 and (plan.pattern[1] == -1).all() and (plan.pattern[B - 1] == 0).all() and not plan.shown[1].any()
    for i in set(range(B)) - {1, B - 1}:
        assert plan.pattern[i].tolist() == [(i + t) % plan.case.P for t in range(gg.VIEW_STEPS)]
    for t in range(gg.VIEW_STEPS):
        ex = [gg.view_expectation(plan.trace[i][t]) for i in range(B)]
        for i in range(B):
            assert gg.differing(ex[i], ex[i]) == []
            for j in range(B):
                if plan.pattern[i, t] != plan.pattern[j, t]:
                    assert gg.differing(ex[j], ex[i]), (plan.name, t, "view", i, "could pass with the state of view", j)
                if np.array_equal(plan.pattern[i, :t + 1], plan.pattern[j, :t + 1]):
                    assert not gg.differing(ex[j], ex[i]), (plan.name, t, i, j)
        assert (plan.pattern[:, t] != plan.pattern[0, t]).any() and gg.differing(ex[1], ex[0]) and gg.differing(ex[2], ex[1])
    assert len({plan.pattern[i].tobytes() for i in range(B)}) == min(B, plan.case.P + 2)
    assert np.array_equal(plan.bank[:, (1 + np.arange(gg.VIEW_STEPS)) % gg.VIEW_STEPS], plan.shown) and int(plan.case.state0["step_index"]) == 1


@pytest.mark.parametrize("name", ["scan_rows_k32", "scan_rows_k48"])
def test_the_view_scans_reach_every_threshold(name):
    plan = gg.view_plan(name, 5)
    case, st = plan.case, plan.case.state0
    M, A = case.params.segment_matching_threshold, case.params.segment_activation_threshold
    thr = np.float32(case.params.permanence_threshold)
    below = np.nextafter(thr, np.float32(0.0))
    seen = set()
    for i in range(plan.B):
        for r in plan.trace[i]:
            d = r.tm.distal_state
            pot, m, act = d.segment_potential, d.matching_segment, d.matching_segment_activation
            active_cell = np.r_[r.tm.cell_activation.reshape(-1), False]
            hit = active_cell[np.where(st["presyn"] >= 0, st["presyn"], case.N)]
            bits = st["perm"].view(np.int32)
            seen |= {what for what, ok in (
                ("potential 64", ((st["seg_nsyn"] == 64) & (pot == 64)).any()), ("potential M", (pot == M).any()), ("potential M - 1", (pot == M - 1).any()),
                ("activation A", (act == A).any()), ("activation A - 1", (act == A - 1).any()),
                ("on the threshold", (hit[m] & (bits[m] == thr.view(np.int32))).any()), ("an ulp below", (hit[m] & (bits[m] == below.view(np.int32))).any()),
                ("33 synapses", ((st["seg_nsyn"][m] == 33) & (pot[m] == 33)).any()),
                ("owner cell >= 32", (st["seg_cell"][m] % case.K >= 32).any())) if ok}
            # every crafted row is scanned, as imported, by every view that shows its source pattern
            if plan.pattern[i][r.t - 1] == 0:
                want = pg.oracle_trace(name)[0].tm.distal_state.segment_potential
                assert np.array_equal(pot[list(case.kinds)], want[list(case.kinds)]), (name, i, r.t)
    want = {"potential 64", "potential M", "potential M - 1", "activation A", "activation A - 1", "on the threshold", "an ulp below", "33 synapses"}
    assert seen >= want | ({"owner cell >= 32"} if case.K > 32 else set()), (name, want - seen)
    sizes = {n for n, _, _ in case.kinds.values()}
    kinds = {k for _, k, _ in case.kinds.values()}
    assert sizes == set(pg.ROW_SIZES) and kinds == set(pg.ROW_KINDS)


def test_a_view_of_classify_words_matches_in_the_last_partial_word():
    plan = gg.view_plan("classify_words", 5)
    S = int(plan.case.state0["S"])
    assert S % 32 and any((r.tm.distal_state.matching_segment >> 5).max() == (S - 1) >> 5 for i in range(5) for r in plan.trace[i])
    # ... and here a view is left without a matching row while others have more than a thousand (no input of scan_rows_* does that:
    # every pattern, and the all-zero input, activates all cells of columns that crafted or cover rows listen to)
    counts = np.array([[len(plan.trace[i][t].tm.distal_state.matching_segment) for i in range(5)] for t in range(gg.VIEW_STEPS)])
    assert ((counts.min(axis=1) == 0) & (counts.max(axis=1) > 1000)).sum() >= 4, counts


@pytest.mark.parametrize("name,B", gg.VIEW_PLANS)
def test_the_members_of_one_launch_differ_row_group_by_row_group(name, B):
    """Per step and for both chunkings (min(16, B) members and 2): some group of 16 rows (one wave's) holds a matching row in one
    member of a chunk and none in another -- `if (hit)` and `__any(matching...)` are taken per member.  In scan_rows_k48 and
    classify_words some row matches in two members of one chunk at different potentials (the accumulators are the member's own): a
    row that a pattern's view sees in full and the all-zero view (columns 0 .. k - 1: some of the pattern's) in part.  scan_rows_k32
    has no such row, and the test says so: its all-zero view matches the crafted rows alone, at their full potentials."""
    plan = gg.view_plan(name, B)
    S = int(plan.case.state0["S"])
    groups = (S + 15) // 16
    thr = plan.case.params.segment_matching_threshold
    for M in (min(GRP_SHARED_MMAX, B), 2):
        two_potentials = False
        for t in range(gg.VIEW_STEPS):
            mixed = False
            for chunk in _chunks(B, M):
                pots = np.stack([plan.trace[i][t].tm.distal_state.segment_potential for i in chunk])
                match = pots >= thr
                per_group = np.stack([np.bincount(np.flatnonzero(row) >> 4, minlength=groups) > 0 for row in match])
                mixed |= bool((per_group.any(axis=0) & ~per_group.all(axis=0)).any())
                both = match.sum(axis=0) >= 2
                lo = np.where(match, pots, 1 << 30).min(axis=0)
                hi = np.where(match, pots, -1).max(axis=0)
                two_potentials |= bool((both & (lo != hi)).any())
            assert mixed, (plan.name, M, t, "every 16-row group matches in all members of its chunk or in none")
        assert two_potentials == (name != "scan_rows_k32"), (plan.name, M, "a row that matches in two members of a chunk at different potentials", two_potentials)
