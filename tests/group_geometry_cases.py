"""Group plans over the hand-built pools of tests/pool_geometry_cases.py: which members one ModelGroup (bithtm_amd/group.py;
htm_group_*, bithtm_amd/csrc/htm_group.h) steps together, and what the oracle says each of them must hold after every step.  Shared by
tests/test_group_geometry_cpu.py (every precondition, on the oracle alone) and tests/test_hip_group_geometry.py (the device).

The group path sizes every launch for member 0 and takes the members' state from tab[blockIdx.y]; it takes the scan form from the
LARGEST segment hint of the members and the scan's speculation bound from the SMALLEST (group_form, htm_engine.hip).  A plan
therefore puts members into DIFFERENT size-dependent forms in one launch: htm_group_create wants equal input_dim, column_dim,
cell_dim, active_columns, segment_capacity, segment_slots and step parity, and nothing else.

Phase-shifted plans, one per name in pg.SMALL (the 2^20-row cases are out of reach: about a gigabyte per member), four members:
  0  the case as imported;
  1  the same case two of its learning steps further (taken alone before the group exists: the parity stays equal);
  2  an empty twin -- the case's shape, permanence, duty cycle and parameters, no store, one learning=False step of
     patterns[case.first] taken alone (as Case.finish): its segment hint is 0, so the group's speculation bound is 0 while every grid is
     sized for the full pool;
  3  the case as imported under a second Temporal Memory seed (the seed keys the jitter and the growth draws: the same store,
     other draws).
The group takes len(case.steps) - 2 steps (member 1's trace ends there: one step for every small case); then every member takes
one more step alone.  Each member's bank is case.bank(): the step with index i shows row i % 4, so member 1 reads another row of
the same bank than the others in the same launch, and the steps past the case's own show patterns[case.first] again (nothing was
learnt for it at the first step, which had learning off: every column bursts without a match).

The mixed plan: alloc_block_edges_1 (S = 3 073), alloc_block_edges_1023 (S = 3 071), alloc_after_death (punishment 0.3) -- which share
the frame k = 8, P = 4, K = 32, 32 slots -- and an empty twin whose thresholds are pg.CLS (9 / 8 / 16) where the others have pg.ALLOC, at
one common segment_capacity: three group steps, one more alone.  Members of one launch then differ in matching and activation
threshold, sampling size, punishment and pool size.

View plans: ModelGroup.views(parent, B) over scan_rows_k32, scan_rows_k48 and classify_words as imported, B = 5 (and B = 17 for
scan_rows_k48: one chunk of GRP_SHARED_MMAX = 16 members and a chunk of one), six steps with learning off.  View i shows pattern
(i + t) % P at step t; view B - 1 shows pattern 0 at every step, view 1 an all-zero input (every overlap 0: the top-k policy takes
columns 0 .. k - 1; it shares a chunk with view 0 at every chunk size).  A view's oracle is pg.fresh_oracle(case) after a sequence
reset, stepped with learning=False.  With P = 2 patterns some views necessarily see the same inputs (views 0 and 2): such views
must be equal; views that show different inputs at a step must differ at it.

Every expectation comes from the oracle that tests/golden/pool_geometry.npz pins to the reference (pg.replay: the first
len(case.steps) records of member 0 ARE pg.oracle_trace's; tests/test_group_geometry_cpu.py asserts it).

Pure NumPy; nothing here touches a device."""

from types import SimpleNamespace

import numpy as np

import pool_geometry_cases as pg
from oracle import TMParams

SECOND_SEED = 7919          # member 3's Temporal Memory seed is the case's plus this
VIEW_STEPS = 6
ZERO_VIEW = 1               # the view that sees an all-zero input: in the chunk of view 0 whatever the chunk size
MIXED = ("alloc_block_edges_1", "alloc_block_edges_1023", "alloc_after_death")
VIEW_PLANS = (("scan_rows_k32", 5), ("scan_rows_k48", 5), ("scan_rows_k48", 17), ("classify_words", 5))
_plans = {}


def member(kind, case, trace, alone=(), seed=None, params=None, first=None):
    """kind: "case" | "shifted" | "empty" | "seed".  alone: the records of the steps the member takes alone before the group exists;
    trace: the group's steps, then one more alone; first: an empty twin's (sp, tm) States of its learning=False step."""
    return SimpleNamespace(kind=kind, case=case, trace=list(trace), alone=list(alone), seed=case.seed if seed is None else seed,
                           params=params or case.params, first=first)


def empty_member(case, params, n):
    _, o_sp, o_tm = pg.empty_oracle(case, params)
    return member("empty", case, pg.replay(case, n=n, empty=params), params=params, first=(o_sp, o_tm))


def learning_plan(name):
    """The phase-shifted plan of one small case."""
    key = ("shift", name)
    if key not in _plans:
        case = pg.build(name)
        n_group = len(case.steps) - 2
        assert n_group >= 1
        full = pg.replay(case, n=2 + n_group + 1)
        members = [member("case", case, full[:n_group + 1]),
                   member("shifted", case, full[2:], alone=full[:2]),
                   empty_member(case, case.params, n_group + 1),
                   member("seed", case, pg.replay(case, n=n_group + 1, seed=case.seed + SECOND_SEED), seed=case.seed + SECOND_SEED)]
        _plans[key] = SimpleNamespace(name=name, members=members, n_group=n_group, capacity=case.capacity + 2 * case.k, full=full)
    return _plans[key]


def mixed_plan():
    if "mixed" not in _plans:
        cases = [pg.build(n) for n in MIXED]
        frame = {(c.I, c.C, c.K, c.k, c.P, c.slots, len(c.steps), c.first) for c in cases}
        assert len(frame) == 1 and all(np.array_equal(c.permanence, cases[0].permanence) for c in cases)
        n_group = len(cases[0].steps)
        members = [member("case", c, pg.replay(c, n=n_group + 1)) for c in cases]
        members.append(empty_member(cases[0], TMParams(**pg.CLS), n_group + 1))
        _plans["mixed"] = SimpleNamespace(name="mixed", members=members, n_group=n_group, capacity=max(c.capacity for c in cases) + cases[0].k)
    return _plans["mixed"]


def oracle_reset(tm):
    """A sequence reset (networks.py:57-65): no predictions, no active cells, no winners, no distal state; the store and the step
    index stay."""
    tm.prev_prediction = np.zeros((tm.column_dim, tm.cell_dim), dtype=np.bool_)
    tm.prev_activation = np.zeros((tm.column_dim, tm.cell_dim), dtype=np.bool_)
    tm.prev_winner = np.zeros(0, dtype=np.int64)
    tm.prev_distal = None


def view_plan(name, B):
    """shown[i][t]: view i's input at group step t; bank[i]: the same rows where a batched run looks for them (the step with
    index s reads row s % VIEW_STEPS; the views start at the parent's step index); trace[i][t]: the view's expected States."""
    key = ("view", name, B)
    if key not in _plans:
        case = pg.build(name)
        T, P = VIEW_STEPS, case.P
        s0 = int(case.state0["step_index"])
        pattern = np.array([[(i + t) % P for t in range(T)] for i in range(B)])
        pattern[B - 1] = 0
        shown = case.patterns[pattern]
        shown[ZERO_VIEW] = False
        pattern[ZERO_VIEW] = -1
        bank = np.zeros_like(shown)
        bank[:, (s0 + np.arange(T)) % T] = shown
        traces = {}
        for i in range(B):
            history = pattern[i].tobytes()
            if history not in traces:                # (views with the same inputs have the same oracle: computed once)
                ora = pg.fresh_oracle(case)
                store = pg.oracle_snapshot(ora.temporal_memory)
                oracle_reset(ora.temporal_memory)
                recs = []
                for t in range(T):
                    o_sp, o_tm = ora.step(shown[i][t], learning=False)
                    recs.append(SimpleNamespace(t=t + 1, sp=o_sp, tm=o_tm, duty=ora.spatial_pooler.duty_cycle.copy()))
                after = pg.oracle_snapshot(ora.temporal_memory)
                assert all(np.array_equal(store[f], after[f]) for f in store), "a step with learning off changed the store"
                traces[history] = recs
        _plans[key] = SimpleNamespace(name=f"{name}-B{B}", case=case, B=B, pattern=pattern, shown=shown, bank=bank,
                                      trace=[traces[pattern[i].tobytes()] for i in range(B)])
    return _plans[key]


# ------------------------------------------------------------------------------------------ what a mix-up of members would change

def expectation(r):
    """The arrays of one record by which members are told apart (each is compared on the device)."""
    out = dict(S=np.int64(r.S), winner=np.stack(r.tm.winner_cell), matching_segment=r.tm.distal_state.matching_segment)
    out.update(r.store)
    return out


def view_expectation(r):
    d = r.tm.distal_state
    return dict(active_column=r.sp.active_column, overlaps=r.sp.overlaps, winner=np.stack(r.tm.winner_cell), matching_segment=d.matching_segment,
                segment_potential=d.segment_potential, cell_prediction=r.tm.cell_prediction,
                max_jittered_potential=d.max_jittered_potential.view(np.int32))


def differing(got, want):
    """The names of the arrays in which `got` is not `want`: what the device tests' comparisons would report."""
    return [f for f in want if np.shape(got[f]) != np.shape(want[f]) or not np.array_equal(got[f], want[f])]
