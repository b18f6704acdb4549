"""Hand-built segment pools for the FUSED step (htm_step / htm_run): every size- and layout-dependent form of the middle launch
(allocation in block 0, classification in blocks 1..n_cls), of the learning role's sparse clear and of the scan, reached
exactly, at the smallest pool at which it exists.  Shared by tests/test_pool_geometry_cpu.py (every precondition; the oracle
against the recorded reference), tests/golden/generate_pool_geometry.py (the recorder) and tests/test_hip_pool_geometry.py
(the device against the oracle).

A case is: a shape and TMParams; a block-structured proximal permanence (disjoint input groups: the columns A_j = {c : c mod P
== j, c < k * P} are connected to the bits of group j alone, so pattern j makes exactly A_j active whatever the boost factors
are -- the precondition asserts it at every step); a segment store written row by row into the oracle; a first State (one
learning=False step over that store) exported with it; at least three further learning steps (the first step after an import
clears the per-cell maxima densely: the sparse clear runs from the second on); and a PRECONDITION on the oracle alone
(last_update and the exported state) that proves the case reaches the path it is named for.  A precondition that does not hold
is a failure.

How a step's need is set: every active column bursts unless a crafted "cover" row -- owned by one of its cells, with synapses on
cells that the previous step certainly activated (all cells of a column that burst without a match) -- makes it predicted.  The
patterns of the allocation cases never recur, so a bursting column has no matching segment and needs exactly one new one.  All
other rows are inert: alive, owned by and connected to cells of columns no pattern activates.

Conventions (as tests/projection_method_cases.py): no growth-priority tie across a cut (the recorder asserts it); active-column
lists ascending.  Rows of 32 slots unless stated: no row ever holds more than 32 synapses (check_preconditions asserts after every
step that the oracle's rows have not widened).
The device's pool has 64 slots at least (htm_create), so these cases run there in rows of 64 that stay within their first chunk.

Which case crosses which threshold, and the constant it comes from (bithtm_amd/csrc/htm_tm_kernels.h unless named) -- if a
constant moves, the case moves with it:
  * 1 024 ids per recyclable count (`recyc_cnt`, `>> 10`): alloc_block_edges_{1,1023} (dead rows at 0, 1023, 1024, 2047, S-1;
    S = 3 073 and 3 071), alloc_stay_dead (fresh ids 1 023, 1 024), alloc_exact_cut_* (the cut inside a block of 20).
  * NEED_LDS = BS / 2 = 128 needed blocks in LDS (role_mid runs with BS = 256), more through d.recyc_need: alloc_many_blocks
    (170 needs over 151 blocks of one or two dead rows; S = 180 001).
  * `grown >= match_thr` at binding, `grown < match_thr` for fresh ids: alloc_stay_dead (2 winners, threshold 3) against every
    other allocation case (grown = min(sample, k) >= threshold).
  * role_learn's count change when a row crosses the threshold: alloc_after_death (punishment 0.3 on permanences 0.1).
  * classification, one row per thread up to (same_launch ? 2 : 8) * n_cls * 256 rows, n_cls <= kClassifyBlocks = 384
    (htm_engine.hip; 786 432 rows, 196 608 in the two-launch schedule, fewer where lean2_classify_blocks is smaller), the word
    form above, `by_xcd` for n_cls % 8 == 0 and n_cls >= 256: classify_words (S = 70 003, also under
    BITHTM_CLASSIFY_WORDS_ABOVE=0), natural_2p20_* (S = 2^20 + 3 000 > 786 432).
  * sparse clear per row up to 8 * nblk * BS rows, nblk <= kLearnBlocks = 256 blocks of RB = 512 threads (1 048 576), per word
    above: natural_2p20_*.
  * 2^20 ids per second-level count (`recyc_cnt2`, nb2 = 2): natural_2p20_hi (no recyclable row below 2^20: the first range is
    skipped) and natural_2p20_both.
  * the streaming scan above scan_large_above = 294 912 rows (htm_engine.hip, scan_pool_is_large): natural_2p20_*; every small
    case under BITHTM_SCAN_LARGE=1.
  * the scan's one-chunk path (rows of at most 32 slots), the loop for a lane's third and later hits (64 slots, 8 lanes per row:
    eight hits in a lane when all 64 synapses are active), the second cell word (cell_dim 48): scan_rows_k32, scan_rows_k48 --
    by the plain forms at step 1 (no crafted row is on the work list), and by the SELF form inside the learning role at steps 2 and 3,
    where the crafted rows are on the work list while their presynaptic cells are active again (the precondition asserts, among the
    listed rows, potentials 64, M and M - 1, activations A and A - 1, permanences on f32(threshold) and one ulp below after the
    update).  In every other case the rows on the work list have potential 0 in the step that lists them: their patterns never recur.

natural_2p20_* rests on the oracle alone (no recorded reference: the reference's store at 2^20 rows is out of reach of a unit
test); the oracle's allocation rule is pinned by the small cases.

Pure NumPy; nothing here touches a device."""

from types import SimpleNamespace

import numpy as np

from oracle import HTMOracle, TMParams, TemporalMemoryOracle
from projection_method_cases import store_snapshot

GROUP_BITS = 16


class Case:
    def __init__(self, name, k, n_patterns, params, seed, K=32, slots=32, column_dim=None, record=True):
        self.name, self.k, self.P, self.K, self.params, self.slots, self.seed = name, int(k), int(n_patterns), int(K), params, int(slots), int(seed)
        need = self.k * self.P + 32
        self.C = int(column_dim or (need + 63) // 64 * 64)
        assert self.C >= need
        self.I = max(64, self.P * GROUP_BITS)
        self.N = self.C * self.K
        self.record = record
        self.A = [np.arange(self.k, dtype=np.int64) * self.P + j for j in range(self.P)]
        self.quiet_columns = np.arange(self.k * self.P, self.C, dtype=np.int64)
        self.quiet = self.cells_of(self.quiet_columns)
        self.permanence = np.full((self.C, self.I), -0.5, dtype=np.float64)
        self.patterns = np.zeros((self.P, self.I), dtype=np.bool_)
        for j in range(self.P):
            self.permanence[self.A[j], j * GROUP_BITS:(j + 1) * GROUP_BITS] = 0.5
            self.patterns[j, j * GROUP_BITS:(j + 1) * GROUP_BITS] = True
        self.ora = self.new_oracle()
        self.tm = self.ora.temporal_memory
        self.rng = np.random.RandomState(seed)
        self.first, self.steps = 0, []
        self.uncovered = {}            # step -> the columns that burst without a match (every cell active after it)
        self.checks = []
        self.state0 = None

    def new_oracle(self):
        ora = HTMOracle(self.I, self.C, self.K, active_columns=self.k, seed=self.seed, tm_params=self.params, permanence=self.permanence.copy())
        ora.temporal_memory = TemporalMemoryOracle(self.C, self.K, self.params, seed=self.seed, slots=self.slots)
        return ora

    def cells_of(self, columns):
        return (np.asarray(columns, dtype=np.int64)[:, None] * self.K + np.arange(self.K)).reshape(-1)

    # ---- the store
    def fill_inert(self, S):
        """Rows 0..S-1 alive and inert: matching threshold + (0, 1, 2) synapses on quiet cells, quiet owners."""
        o, M, q = self.tm, self.params.segment_matching_threshold, self.quiet
        assert o.S == 0 and self.slots >= M + 2 and len(q) >= M + 2 + 8
        o._ensure_rows(S)
        ids = np.arange(S, dtype=np.int64)
        n = M + ids % 3
        idx = ((ids * 13) % (len(q) - (M + 2)))[:, None] + np.arange(M + 2)
        valid = np.arange(M + 2) < n[:, None]
        o.presyn[:S, :M + 2] = np.where(valid, q[idx], -1)
        o.perm[:S, :M + 2] = np.where(valid, (0.3 + (ids % 7) * 0.05)[:, None].astype(np.float32), np.float32(-1.0))
        o.seg_cell[:S] = q[(ids * 5) % len(q)]
        o.seg_nsyn[:S] = n
        o.segcount[:] = np.bincount(o.seg_cell[:S], minlength=self.N)
        o.S = S

    def set_row(self, s, owner, cells, perms):
        o = self.tm
        cells = np.asarray(cells, dtype=np.int64)
        assert s < o.S and len(np.unique(cells)) == len(cells) <= self.slots
        o.segcount[o.seg_cell[s]] -= 1
        o.segcount[owner] += 1
        o.seg_cell[s], o.seg_nsyn[s] = owner, len(cells)
        o.presyn[s], o.perm[s] = -1, -1.0
        o.presyn[s, :len(cells)] = cells
        o.perm[s, :len(cells)] = np.broadcast_to(np.asarray(perms, dtype=np.float32), cells.shape)

    def kill(self, ids):
        """Rows with fewer synapses than the matching threshold (0, 1, .. in turn): recyclable."""
        o, M = self.tm, self.params.segment_matching_threshold
        for i, s in enumerate(ids):
            keep = i % M
            o.presyn[s, keep:], o.perm[s, keep:], o.seg_nsyn[s] = -1, -1.0, keep
        return np.asarray(ids, dtype=np.int64)

    def pick(self, cells, n):
        return np.sort(self.rng.permutation(cells)[:n])

    def prev_cells(self, t):
        """Cells certainly active after step t - 1 (0: the first, learning=False step, where every active column bursts)."""
        return self.cells_of(self.A[self.first] if t == 1 else self.uncovered[t - 1])

    def plan(self, t, pattern, need, ids=(), perm=0.6):
        """Step t (1-based) shows `pattern` and needs `need` new segments: the other k - need columns get a cover row each (at `ids`)
        that predicts one of their cells (perm 0.3: unconnected -- the column bursts and the row's cell wins as the best match)."""
        assert t == len(self.steps) + 1
        self.steps.append(int(pattern))
        A, n_cov, act = self.A[pattern], self.k - need, self.params.segment_activation_threshold
        assert len(ids) == n_cov
        prev = self.prev_cells(t) if n_cov else None
        for i, s in enumerate(ids):
            self.set_row(s, A[i] * self.K + i % self.K, self.pick(prev, act + 1), perm)
        self.uncovered[t] = A[n_cov:]

    def finish(self):
        """The first State: one learning=False step over the crafted store; everything a replay starts from."""
        self.store0 = self.tm.export_state() if self.record else None      # (the crafted store before any step: what the recorder loads)
        o_sp, _ = self.ora.step(self.patterns[self.first], learning=False)
        assert np.array_equal(o_sp.active_column, self.A[self.first])
        self.state0 = self.tm.export_state()
        self.duty0 = self.ora.spatial_pooler.duty_cycle.copy()
        assert len(self.steps) >= 3 and self.tm.slots == self.slots
        self.capacity = int(self.state0["S"]) + self.k * len(self.steps) + 64
        return self

    def check(self, fn):
        self.checks.append(fn)

    def bank(self):
        """The pattern bank of one batched run: row t is the input of the step with index t (0: the first step, already taken)."""
        return self.patterns[[self.first] + self.steps]


def fresh_oracle(case):
    ora = case.new_oracle()
    ora.spatial_pooler.duty_cycle = case.duty0.copy()
    ora.temporal_memory.import_state(case.state0)
    return ora


def recount(nsyn, match_thr):
    """The recyclable counts a pool with these synapse counts must have: per 1 024 ids, per 2^20 ids."""
    S = len(nsyn)
    nb = (S + 1023) >> 10
    dead = np.flatnonzero(np.asarray(nsyn) < match_thr)
    return np.bincount(dead >> 10, minlength=nb).astype(np.int32), np.bincount(dead >> 20, minlength=(nb + 1023) >> 10).astype(np.int32)


def oracle_snapshot(tm):
    S = tm.S
    return store_snapshot(tm.seg_cell[:S], tm.presyn[:S], tm.perm[:S], tm.seg_nsyn[:S], tm.segcount)


def empty_oracle(case, params=None):
    """An empty twin of the case: its shape, permanence and parameters (or `params`), no store, and -- as Case.finish -- one
    learning=False step of patterns[case.first], whose duty cycle is therefore the case's.  Returns (oracle, sp State, tm State)."""
    params = params or case.params
    ora = HTMOracle(case.I, case.C, case.K, active_columns=case.k, seed=case.seed, tm_params=params, permanence=case.permanence.copy())
    ora.temporal_memory = TemporalMemoryOracle(case.C, case.K, params, seed=case.seed, slots=case.slots)
    o_sp, o_tm = ora.step(case.patterns[case.first], learning=False)
    assert np.array_equal(o_sp.active_column, case.A[case.first]) and np.array_equal(ora.spatial_pooler.duty_cycle, case.duty0)
    return ora, o_sp, o_tm


def replay(case, stores=None, n=None, offset=0, seed=None, empty=None):
    """The case's steps on a fresh oracle, one record per step: sp / tm (the States), last (the oracle's last_update), nsyn (the
    synapse counts after the step), store (store_snapshot; at the steps `stores` names, default all), perm / duty (the Spatial
    Pooler's permanences and duty cycles after the step).  The step with index i shows row i % (1 + len(case.steps)) of case.bank(),
    as a batched run over that bank does: the case's own steps, then -- `n` steps in all, default len(case.steps) -- the bank again.
    `offset`: the records of the first `offset` steps are left out (a member that took them alone); `seed`: another Temporal Memory
    seed over the same imported state (the jitter and the growth draws differ, the store does not); `empty`: TMParams of an empty
    twin (empty_oracle) instead of the case's store."""
    ora = fresh_oracle(case) if empty is None else empty_oracle(case, empty)[0]
    tm = ora.temporal_memory
    if seed is not None:
        tm.seed = int(seed)
    bank = case.bank()
    out = []
    for t in range(1, (len(case.steps) if n is None else n) + 1):
        assert tm.step_index == t
        o_sp, o_tm = ora.step(bank[t % len(bank)], learning=True)
        keep = stores is None or t in stores
        out.append(SimpleNamespace(t=t, sp=o_sp, tm=o_tm, last=tm.last_update, nsyn=tm.seg_nsyn[:tm.S].copy(), S=tm.S, slots=tm.slots,
                                   store=oracle_snapshot(tm) if keep else None, perm=ora.spatial_pooler.permanence.copy(),
                                   duty=ora.spatial_pooler.duty_cycle.copy()))
    return out[offset:]


# ------------------------------------------------------------------------------------------ allocation

ALLOC = dict(segment_activation_threshold=4, segment_matching_threshold=4, segment_sampling_synapses=8)


def _needs_check(needs):
    def check(case, tr):
        for r, n in zip(tr, needs):
            assert len(r.last.unaccounted) == n == len(r.last.recycled) + len(r.last.fresh), (case.name, r.t, len(r.last.unaccounted), n)
    return check


def alloc_block_edges(rem):
    """S = 3 072 + rem - 1024 * (rem > 1): dead rows at the first and last id of 1 024-blocks and at S - 1.  Step 1 needs 3 and takes
    0, 1023, 1024; step 2 needs 5: 2047, S - 1, then appends S, S + 1, S + 2."""
    S = 3073 if rem == 1 else 3071
    assert S % 1024 == rem
    c = Case(f"alloc_block_edges_{rem}", 8, 4, TMParams(**ALLOC), seed=100 + rem)
    c.fill_inert(S)
    dead = c.kill([0, 1023, 1024, 2047, S - 1])
    needs = [3, 5, 8]
    c.plan(1, 1, 3, ids=[100, 101, 102, 1500, 1501])
    c.plan(2, 2, 5, ids=[2046, 2048, 5])
    c.plan(3, 3, 8)
    c.finish()
    c.check(_needs_check(needs))

    def check(case, tr):
        assert np.array_equal(tr[0].last.recycled, dead[:3]) and len(tr[0].last.fresh) == 0
        assert np.array_equal(tr[1].last.recycled, dead[3:]) and np.array_equal(tr[1].last.fresh, [S, S + 1, S + 2])
        if rem == 1023:
            assert len(np.unique(tr[1].last.fresh >> 10)) == 2, "the appended ids do not cross a 1 024 boundary"
        else:
            assert (S - 1) % 1024 == 0, "S - 1 is not the only row of its block"
        assert len(tr[2].last.recycled) == 0 and len(tr[2].last.fresh) == 8
    c.check(check)
    return c


def alloc_exact_cut(delta):
    """40 dead rows in 6 blocks, the last block holding 20 of them; step 1 needs 40 + delta: the cut `rank < n_r` falls inside that
    block (-1), on its last dead row (0), or one past it (+1: one id is appended)."""
    c = Case(f"alloc_exact_cut_{ {-1: 'minus1', 0: 'equal', 1: 'plus1'}[delta]}", 48, 4, TMParams(**ALLOC), seed=110 + delta)
    S = 6100
    c.fill_inert(S)
    per_block = [4, 3, 5, 4, 4, 20]
    ids = np.concatenate([b * 1024 + np.sort(c.rng.permutation(1024 if b < 5 else S - 5 * 1024)[:n]) for b, n in enumerate(per_block)])
    dead = c.kill(ids)
    R = len(dead)
    assert R == 40
    needs = [R + delta, 5, 48]
    free = np.setdiff1d(np.arange(200, 900), dead)
    c.plan(1, 1, needs[0], ids=free[:48 - needs[0]])
    c.plan(2, 2, needs[1], ids=free[100:100 + 43])
    c.plan(3, 3, needs[2])
    c.finish()
    c.check(_needs_check(needs))

    def check(case, tr):
        n_r = min(R, R + delta)
        assert np.array_equal(tr[0].last.recycled, dead[:n_r]) and len(tr[0].last.fresh) == max(delta, 0)
        assert len(np.unique(dead[-20:] >> 10)) == 1, "the last 20 dead rows are not in one block"
        if delta < 0:
            assert tr[1].last.recycled[0] == dead[-1] and len(tr[1].last.fresh) == 4, "the row left over by the cut is not taken next"
        else:
            assert len(tr[1].last.recycled) == 0
    c.check(check)
    return c


def alloc_many_blocks():
    """S = 180 001 (176 blocks), one dead row in every block and a second one in every eighth; 176 active columns, 170 of them
    bursting without a match at step 1: the recycled ids lie in more than NEED_LDS = 128 blocks."""
    c = Case("alloc_many_blocks", 176, 4, TMParams(**ALLOC), seed=120, K=16, column_dim=1024)
    S = 180001
    c.fill_inert(S)
    nb = (S + 1023) >> 10
    ids = [b * 1024 + int(c.rng.randint(min(1024, S - b * 1024))) for b in range(nb)]
    ids += [b * 1024 + ((i - b * 1024 + 311) % 1000) for b, i in zip(range(nb), ids) if b % 8 == 3]
    dead = c.kill(np.unique(ids))
    assert len(dead) == nb + 22
    needs = [170, 176, 176]
    c.plan(1, 1, 170, ids=np.setdiff1d(np.arange(5000, 5100), dead)[:6])
    c.plan(2, 2, 176)
    c.plan(3, 3, 176)
    c.finish()
    c.check(_needs_check(needs))

    def check(case, tr):
        assert S >= 170000 and len(np.unique(dead >> 10)) >= 160 and np.bincount(dead >> 10).max() <= 2
        assert len(tr[0].last.unaccounted) >= 150
        assert len(np.unique(tr[0].last.recycled >> 10)) > 128, "the needed blocks fit NEED_LDS"
        assert np.array_equal(tr[0].last.recycled, dead[:170])
        assert np.array_equal(tr[1].last.recycled, dead[170:]) and len(tr[1].last.fresh) == 176 - (len(dead) - 170)
    c.check(check)
    return c


def alloc_stay_dead():
    """2 active columns, matching threshold 3: a bound row grows min(sample, 2) = 2 synapses and stays recyclable.  S0 = 1 023:
    step 1 appends 1023 and 1024 (two blocks), steps 2 and 3 recycle exactly those."""
    c = Case("alloc_stay_dead", 2, 4, TMParams(segment_activation_threshold=3, segment_matching_threshold=3, segment_sampling_synapses=8), seed=130)
    c.fill_inert(1023)
    c.plan(1, 1, 2)
    c.plan(2, 2, 2)
    c.plan(3, 3, 2)
    c.finish()
    c.check(_needs_check([2, 2, 2]))

    def check(case, tr):
        assert np.array_equal(tr[0].last.fresh, [1023, 1024]) and len(np.unique(tr[0].last.fresh >> 10)) == 2
        assert np.array_equal(tr[1].last.recycled, [1023, 1024]) and np.array_equal(tr[2].last.recycled, [1023, 1024])
        assert all(len(r.last.fresh) == 0 for r in tr[1:]) and tr[2].S == 1025
        assert (tr[0].nsyn[[1023, 1024]] == 2).all(), "the bound rows did not grow exactly two synapses"
    c.check(check)
    return c


def alloc_after_death():
    """Permanence 0.1, punishment 0.3: rows alive at import (ids 10..16, block 0) match the first State, are owned by columns that
    step 1 leaves inactive, and are punished below the matching threshold; the dead rows that exist at import lie in block 1.
    Step 1 takes four of those; step 2 must take the newly dead rows first.  Row 16 keeps four inactive synapses and survives."""
    c = Case("alloc_after_death", 8, 4, TMParams(permanence_punishment=0.3, **ALLOC), seed=140)
    S = 3000
    c.fill_inert(S)
    old_dead = c.kill(np.arange(2000, 2011))
    first = c.cells_of(c.A[0])
    victims = np.arange(10, 17)
    for i, s in enumerate(victims):
        n_quiet = (0, 2, 0, 1, 3, 0, 4)[i]
        c.set_row(s, c.quiet[40 + i], np.r_[c.pick(first, 5), c.pick(c.quiet[:64], n_quiet)], 0.1)
    needs = [4, 8, 8]
    c.plan(1, 1, 4, ids=[500, 501, 502, 503])
    c.plan(2, 2, 8)
    c.plan(3, 3, 8)
    c.finish()
    c.check(_needs_check(needs))

    def check(case, tr):
        M = case.params.segment_matching_threshold
        assert (case.state0["seg_nsyn"][victims] >= M).all() and np.isin(victims, case.state0["matching_segment"]).all()
        assert np.isin(victims, tr[0].last.punished).all()
        assert np.array_equal(tr[0].last.recycled, old_dead[:4])
        assert (tr[0].nsyn[victims[:-1]] < M).all() and tr[0].nsyn[victims[-1]] == 4 and (tr[0].nsyn[victims[:-1]] > 0).any()
        assert np.array_equal(tr[1].last.recycled, np.r_[victims[:-1], old_dead[4:6]]), "step 2 does not take the rows that died at step 1 first"
        assert victims.max() >> 10 < old_dead.min() >> 10
    c.check(check)
    return c


# ------------------------------------------------------------------------------------------ classification

CLASSES = ("active", "best", "not_best", "punished", "other")
CLS = dict(segment_activation_threshold=9, segment_matching_threshold=8, segment_sampling_synapses=16)


def class_rows(c, t, pattern, groups):
    """Step t shows `pattern`; the rows at `groups` (name -> ids) match the State before it, one class each in turn:
      active    owned by cell 0 of a column of the pattern's first 3/8, 12 connected synapses: the cell is predicted, the row learns;
      other     cell 1 of such a column, 10 unconnected synapses: the column is predicted by cell 0 -- neither learns nor is punished;
      best      cell 2 of a column of the next half, 14 unconnected synapses, one per column: the column bursts, cell 2 wins, the row learns;
      not_best  cells 2 and 3 of those columns, 10 synapses: matching, not the best;
      punished  a quiet owner: its column is inactive.
    The last eighth of the columns burst without a match (8 new segments at k = 64)."""
    assert t == len(c.steps) + 1
    c.steps.append(int(pattern))
    A, K, k = c.A[pattern], c.K, c.k
    P, B = A[:3 * k // 8], A[3 * k // 8:7 * k // 8]
    c.uncovered[t] = A[7 * k // 8:]
    prev = c.prev_cells(t)
    order = ("active", "punished", "best", "other", "not_best")
    count = dict.fromkeys(order, 0)
    for ids in groups.values():
        for i, s in enumerate(ids):
            cls = order[i % 5]
            if cls == "best" and count["best"] >= len(B):
                cls = "not_best"
            j = count[cls]
            count[cls] += 1
            if cls == "active":
                c.set_row(s, P[j % len(P)] * K, c.pick(prev, 12), 0.6)
            elif cls == "other":
                c.set_row(s, P[j % len(P)] * K + 1, c.pick(prev, 10), 0.3)
            elif cls == "best":
                c.set_row(s, B[j] * K + 2, c.pick(prev, 14), 0.3)
            elif cls == "not_best":
                c.set_row(s, B[j % len(B)] * K + 2 + j % 2, c.pick(prev, 10), 0.3)
            else:
                c.set_row(s, c.quiet[(7 * j) % len(c.quiet)], c.pick(prev, 11), (0.3, 0.6)[j % 2])
    assert count["best"] == len(B) and count["active"] >= len(P), (c.name, t, count)


def classes_of(case, prev, r):
    """The class of every row that matched the State `prev` (its matching_segment), by the oracle's decisions at step record r."""
    m = np.asarray(prev["matching_segment"], dtype=np.int64)
    active = np.asarray(prev["matching_segment_active"], dtype=np.bool_)
    learn, pun = np.isin(m, r.last.learning), np.isin(m, r.last.punished)
    col = case.state0["seg_cell"][m] // case.K
    bursting = np.zeros(case.C, dtype=np.bool_)
    bursting[r.sp.active_column] = r.tm.active_column_bursting[:, 0]
    cls = np.where(learn & active, 0, np.where(learn, 1, np.where(pun, 3, np.where(bursting[col], 2, 4))))
    assert not (learn & pun).any()
    return m, cls


def _class_check(groups, min_rows):
    def check(case, tr):
        m, cls = classes_of(case, case.state0, tr[0])
        n = np.bincount(cls, minlength=5)
        assert n.min() >= min_rows, (case.name, dict(zip(CLASSES, n.tolist())))
        for name, ids in groups.items():
            assert np.isin(ids, m).all(), (case.name, name, "a crafted row does not match")
            mine = cls[np.searchsorted(m, ids)]
            assert np.isin(mine, (0, 1)).any() and (mine == 3).any(), (case.name, name, "no learning or no punished row")
        assert len(tr[0].last.unaccounted) == case.k // 8
    return check


def classify_words():
    """S = 70 003 (2 188 words of match bits, the last of 19 rows; not a multiple of 256 words).  Rows that match the first State:
    40 consecutive fully set words, single rows at bit 0 and at bit 31 of words in every residue class mod 8 of their 128-byte
    line, five rows of the last, partial word -- all five classes at every position.  Steps 2 and 3 classify further runs."""
    c = Case("classify_words", 64, 4, TMParams(**CLS), seed=150)
    S = 70003
    c.fill_inert(S)
    nwords = (S + 31) // 32
    groups = dict(bit0=np.array([((16 + x) * 32 + 5) * 32 for x in range(8)]), bit31=np.array([((24 + x) * 32 + 20) * 32 + 31 for x in range(8)]),
                  last_word=np.array([69984, 69990, 69995, 70001, 70002]), run=np.arange(1100 * 32, 1140 * 32))
    assert S % 32 != 0 and nwords % 256 != 0 and groups["last_word"].min() >> 5 == nwords - 1
    assert sorted(set(((g >> 5) >> 5) & 7 for g in groups["bit0"])) == list(range(8)) == sorted(set(((g >> 5) >> 5) & 7 for g in groups["bit31"]))
    class_rows(c, 1, 1, groups)
    class_rows(c, 2, 2, dict(run=np.arange(1500 * 32 + 7, 1540 * 32 + 7), single=np.array([31, 32, 63, 64, 2047 * 32])))
    class_rows(c, 3, 3, dict(run=np.arange(2100 * 32, 2140 * 32)))
    c.finish()
    c.check(_class_check(groups, 20))

    def check(case, tr):
        bits = np.zeros(nwords * 32, dtype=np.bool_)
        bits[case.state0["matching_segment"]] = True
        words = bits.reshape(nwords, 32)
        assert words[1100:1140].all() and not words[1099].any() and not words[1140].any()
        for g in np.r_[groups["bit0"], groups["bit31"]]:
            assert words[g >> 5].sum() == 1
        for r in tr[1:]:
            assert len(r.last.learning) > 100 and len(r.last.punished) > 100, (case.name, r.t, "later steps classify nothing")
    c.check(check)
    return c


# ------------------------------------------------------------------------------------------ scan rows

ROW_SIZES = (1, 7, 8, 9, 31, 32, 33, 63, 64)
ROW_KINDS = ("all_active", "at_threshold", "ulp_below", "potential_at", "potential_short", "activation_at", "activation_short",
             "at_threshold_after", "ulp_below_after", "drops_short")


def permanence_that_becomes(target, delta):
    """A float32 p with f32(f64(p) + delta) == target exactly (projections.py:102-107: float64 sum, float32 store)."""
    p = np.float32(np.float64(target) - delta)
    for q in [p] + [f(p, n) for n in range(1, 64) for f in (_up, _down)]:
        if np.float32(np.float64(q) + delta) == target:
            return q
    raise AssertionError((target, delta))


def _up(p, n):
    for _ in range(n):
        p = np.nextafter(p, np.float32(2.0))
    return p


def _down(p, n):
    for _ in range(n):
        p = np.nextafter(p, np.float32(-1.0))
    return p


def scan_rows(K):
    """segment_slots 64, matching threshold 7, activation threshold 9; cell_dim 32 and 48 (a second cell word).  Rows of 1, 7, 8, 9, 31,
    32, 33, 63 and 64 synapses at the first and last id and on both sides of every 16-row (so every 64-row) boundary of 2 101 rows:
    every synapse on an active cell; connected synapses exactly at f32(threshold) and one ulp below; potential at the matching
    threshold and one short; activation at the activation threshold and one short.  Their active synapses lie on the cells of the
    first 8 columns of pattern 0 (the source columns: no row that could predict them, so they burst, every cell active, at every
    step); their owners are cells of the other 8 columns of pattern 0 (rows of at most 33 synapses: they may learn and grow) or quiet
    cells (punished).  The first State comes from pattern 1; steps 0, 0, 0:
      step 1  nothing matches the first State but 16 unconnected cover rows: the crafted rows are scanned as imported, none of them
              on the work list (the plain forms of the scan);
      step 2  they match the State of step 1, learn or are punished, and are scanned by the wave that rewrote them (the SELF form
              where the learning role and the scan share a launch) against the same source cells -- with potentials 64, M and M - 1
              (`drops_short`: a punished row of M active synapses, one at permanence 0.005, pruned), activations A and A - 1, and
              permanences that the update itself puts exactly on f32(threshold) and one ulp below (`*_after`);
      step 3  the same again over the rewritten rows."""
    # (punishment 0.04: with the default 0.01 no float32 above 0.5 is taken to one ulp below f32(0.5) by the float64 subtraction)
    p = TMParams(permanence_punishment=0.04, segment_activation_threshold=9, segment_matching_threshold=7, segment_sampling_synapses=16)
    c = Case(f"scan_rows_k{K}", 16, 2, p, seed=160 + K, K=K, slots=64)
    S = 2101
    c.first = 1
    c.fill_inert(S)
    M, Aa = p.segment_matching_threshold, p.segment_activation_threshold
    thr = np.float32(p.permanence_threshold)
    below = np.nextafter(thr, np.float32(0.0))
    d = c.tm.d
    after = {(True, "at_threshold_after"): permanence_that_becomes(thr, d.learn_active), (True, "ulp_below_after"): permanence_that_becomes(below, d.learn_active),
             (False, "at_threshold_after"): permanence_that_becomes(thr, d.punish_active), (False, "ulp_below_after"): permanence_that_becomes(below, d.punish_active)}
    src, own = c.A[0][:8], c.A[0][8:]
    source = c.cells_of(src)
    ids = np.arange(S)
    special = ids[(ids % 16 == 0) | (ids % 16 == 15) | (ids == S - 1)]
    cover = np.arange(16) * 16 + 5
    kinds, alone = {}, {}           # alone: the one learning row of each `*_after` kind that gets a column of its own (see below)
    for i, s in enumerate(special):
        n, kind = ROW_SIZES[i % 9], ROW_KINDS[(i // 9) % len(ROW_KINDS)]
        learns = n <= 33 and i % 2 == 0 and kind != "drops_short"
        h = {"potential_at": min(n, M), "potential_short": min(n, M - 1), "drops_short": min(n, M)}.get(kind, n)
        perms = np.full(n, 0.6, dtype=np.float32)
        if kind == "at_threshold":
            perms[:] = thr
        elif kind == "ulp_below":
            perms[:] = below
        elif kind == "activation_at":
            perms[min(n, Aa):] = 0.3
        elif kind == "activation_short":
            perms[min(n, Aa - 1):] = 0.3
        elif kind in ("at_threshold_after", "ulp_below_after"):
            perms[:] = after[(learns, kind)]
        elif kind == "drops_short":
            perms[0] = 0.005
        cells = np.r_[c.rng.permutation(source)[:h], c.rng.permutation(c.quiet)[:n - h]]
        # a learning row is owned by one of two cells of the first six owner columns: an active row predicts its cell and learns.  A row
        # whose permanences reach the threshold only by learning is unconnected before, so it learns only as the best match of a
        # bursting column: the last two owner columns hold one such row each and nothing else
        owner = own[(i // 2) % 6] * K + (i // 16) % 2 if learns else c.quiet[(11 * i) % len(c.quiet)]
        if learns and kind.endswith("_after") and n >= 31 and kind not in alone:
            alone[kind] = int(s)
            owner = own[6 + len(alone) - 1] * K + 3
        c.set_row(s, owner, cells, perms)
        kinds[int(s)] = (n, kind, learns)
    # step 1 shows pattern 0 over the untouched rows: every column bursts (its cover row matches the first State unconnected: no new
    # segment, so the rows of one synapse -- recyclable -- are still there when the step's scan runs) and every cell is active
    c.plan(1, 0, 0, ids=cover, perm=0.3)
    c.steps += [0, 0]
    c.finish()
    c.kinds = kinds
    assert len(alone) == 2

    def of_kind(kind, least=0):
        return np.array([s for s, (n, k_, _) in kinds.items() if k_ == kind and n >= least])

    def check(case, tr):
        st, d1 = case.state0, tr[0].tm.distal_state               # the scan of step 1: the crafted rows as they were imported
        pot = d1.segment_potential
        m, act, m_active = d1.matching_segment, d1.matching_segment_activation, d1.matching_segment_active
        assert tr[0].tm.active_column_bursting.all() and len(tr[0].last.unaccounted) == 0 and len(tr[0].last.punished) == 0
        assert np.array_equal(tr[0].last.learning, cover), "a crafted row is on the work list of step 1"
        assert np.array_equal(tr[0].nsyn[special], st["seg_nsyn"][special]), "a crafted row changed before its scan"
        assert (pot[special] > 0).all() and (pot[np.setdiff1d(ids, np.r_[special, cover])] == 0).all()
        for b in range(16, S, 16):
            assert pot[b - 1] > 0 and pot[b] > 0
        assert pot[0] > 0 and pot[S - 1] > 0
        assert set(st["seg_nsyn"][special].tolist()) == set(ROW_SIZES)
        assert ((st["seg_nsyn"] == 64) & (pot == 64)).any(), "no row with eight hits in every lane"
        assert (pot == M).any() and (pot == M - 1).any() and (act == Aa).any() and (act == Aa - 1).any()
        hit = np.isin(st["presyn"], source)
        bits = st["perm"].view(np.int32)
        assert (hit & (bits == thr.view(np.int32))).any() and (hit & (bits == below.view(np.int32))).any()
        assert np.isin(of_kind("at_threshold", Aa), m[m_active]).all() and not np.isin(of_kind("ulp_below", Aa), m[m_active]).any()
        assert K <= 32 or (source % K >= 32).any()
        # steps 2 and 3: the rows on the work list are scanned against cells that are active again (the SELF form)
        for r in tr[1:]:
            d2 = r.tm.distal_state
            assert r.tm.active_column_bursting[:8].all(), (case.name, r.t, "a source column is predicted: not all of its cells are active")
            listed = np.union1d(r.last.learning, r.last.punished)
            crafted = np.intersect1d(listed, special)
            assert len(np.intersect1d(r.last.learning, special)) > 10 and len(np.intersect1d(r.last.punished, special)) > 50, (case.name, r.t)
            p2 = d2.segment_potential[crafted]
            a2 = d2.matching_segment_activation[np.isin(d2.matching_segment, crafted)]
            assert set(st["seg_nsyn"][crafted].tolist()) >= set(ROW_SIZES[1:]), (case.name, r.t, "a row length is not on the work list")
            assert (p2 == 64).any() and (p2 == M).any() and (a2 == Aa).any() and (a2 == Aa - 1).any(), (case.name, r.t)
            if K > 32:
                rows = st["presyn"][crafted]
                assert (np.isin(rows, source) & (rows % K >= 32)).any()
        r, d2 = tr[1], tr[1].tm.distal_state
        assert np.isin(list(alone.values()), r.last.learning).all(), "a row alone in its column does not learn as the best match"
        listed = np.union1d(r.last.learning, r.last.punished)
        drops = of_kind("drops_short", M)
        assert len(drops) and np.isin(drops, r.last.punished).all() and (d2.segment_potential[drops] == M - 1).all() and (pot[drops] == M).all()
        assert (r.nsyn[of_kind("drops_short", M)] < st["seg_nsyn"][of_kind("drops_short", M)]).all() and (r.nsyn[drops] < M).any()
        start = np.r_[0, np.cumsum(r.store["syn_count"])]
        active2 = d2.matching_segment[d2.matching_segment_active]
        for kind, want, is_active in (("at_threshold_after", thr, True), ("ulp_below_after", below, False)):
            rows = np.intersect1d(of_kind(kind, Aa), listed)
            assert {kinds[int(s)][2] for s in rows} == {True, False}, (case.name, kind, "not both a learning and a punished row")
            for s in rows:
                got = r.store["syn_perm_bits"][start[s]:start[s + 1]]
                on = np.isin(r.store["syn_presyn"][start[s]:start[s + 1]], source)
                assert (got[on][:1] == want.view(np.int32)).all() and (got[on] == want.view(np.int32)).sum() >= Aa, (case.name, kind, s)
            assert np.isin(rows, active2).all() == is_active and np.isin(rows, active2).any() == is_active, (case.name, kind)
        assert all(x.slots == 64 for x in tr)
    c.check(check)
    return c


# ------------------------------------------------------------------------------------------ natural size

def natural_2p20(both):
    """S = 2^20 + 3 000 on 4 096 x 32 cells: above the row forms of the classification (786 432) and of the sparse clear (1 048 576),
    above the streaming scan's threshold (294 912), two second-level counts.  20 dead rows at ids >= 2^20 (`hi`: the first 2^20
    range has count 0 and is skipped; `both`: 8 more in blocks 3, 500 and 1 021); the four steps need 8 each.  Runs of 40 matching words
    below 2^20 near the top and across it, all five classes, for the classification of each of the four steps: the State before every
    step has per-cell maxima that the State after it has not (step 1 clears densely, steps 2, 3 and 4 sparsely, by words)."""
    c = Case(f"natural_2p20_{'both' if both else 'hi'}", 64, 5, TMParams(**CLS), seed=170 + both, column_dim=4096, record=False)
    top = 1 << 20
    S = top + 3000
    c.fill_inert(S)
    dead = top + 100 + np.sort(c.rng.permutation(2800)[:20])
    if both:
        dead = np.r_[3 * 1024 + np.arange(0, 300, 100), 500 * 1024 + np.arange(5, 305, 100), 1021 * 1024 + np.arange(1022, 1024), dead]
    dead = c.kill(np.unique(dead))

    def free(ids):
        return np.setdiff1d(ids, dead)
    groups = dict(run=np.arange(top - 64 * 32, top - 24 * 32), across=free(np.arange(top - 64, top + 64)), single=np.array([0, 31, top - 1, S - 1]))
    class_rows(c, 1, 1, groups)
    class_rows(c, 2, 2, dict(run=np.arange(top - 4000 * 32 + 3, top - 3960 * 32 + 3), high=free(np.arange(top + 2000, top + 2100))))
    class_rows(c, 3, 3, dict(run=np.arange(700000, 700000 + 40 * 32)))
    class_rows(c, 4, 4, dict(run=np.arange(300000 + 11, 300000 + 11 + 40 * 32), high=free(np.arange(top + 2500, top + 2600))))
    c.finish()
    c.stores = (1, 4)
    c.check(_class_check(groups, 5))

    def check(case, tr):
        assert tr[0].S > 8 * 384 * 256 and tr[0].S > 8 * 256 * 512 and ((tr[0].S + 1023) >> 10) > 1024
        rec = np.concatenate([r.last.recycled for r in tr])
        assert len(rec) == len(dead) and sum(len(r.last.fresh) for r in tr) > 0
        assert (tr[0].last.recycled >= top).all() != bool(both) and (dead >= top).all() != bool(both)
        prev = case.state0["max_jittered_potential"]
        for r in tr:                                  # (step 1: the dense clear; steps 2, 3, 4: the sparse one)
            now = r.tm.distal_state.max_jittered_potential
            assert ((prev > 0) & (now == 0)).sum() >= 20, (case.name, r.t, "no maximum that the clear of this step must remove")
            prev = now
    c.check(check)
    return c


# ------------------------------------------------------------------------------------------ the list

BUILDERS = {
    "alloc_block_edges_1": lambda: alloc_block_edges(1), "alloc_block_edges_1023": lambda: alloc_block_edges(1023),
    "alloc_exact_cut_minus1": lambda: alloc_exact_cut(-1), "alloc_exact_cut_equal": lambda: alloc_exact_cut(0),
    "alloc_exact_cut_plus1": lambda: alloc_exact_cut(1), "alloc_many_blocks": alloc_many_blocks, "alloc_stay_dead": alloc_stay_dead,
    "alloc_after_death": alloc_after_death, "classify_words": classify_words, "scan_rows_k32": lambda: scan_rows(32),
    "scan_rows_k48": lambda: scan_rows(48), "natural_2p20_hi": lambda: natural_2p20(False), "natural_2p20_both": lambda: natural_2p20(True),
}
CASE_NAMES = list(BUILDERS)
SMALL = [n for n in CASE_NAMES if not n.startswith("natural")]
LARGE = [n for n in CASE_NAMES if n.startswith("natural")]
_built, _traces = {}, {}


def build(name):
    """The case of that name, built once per process (the builders are deterministic)."""
    if name not in _built:
        _built[name] = BUILDERS[name]()
        assert _built[name].name == name
    return _built[name]


def oracle_trace(name):
    """replay(build(name)), computed once and shared by the tests of a process (left unchanged by them)."""
    if name not in _traces:
        case = build(name)
        _traces[name] = replay(case, stores=getattr(case, "stores", None))
    return _traces[name]


def release(name):
    """Forget a large case (its store and trace hold about a gigabyte)."""
    _built.pop(name, None)
    _traces.pop(name, None)


def check_preconditions(name):
    case, tr = build(name), oracle_trace(name)
    assert case.checks, f"{name}: a case without a precondition"
    for r, j in zip(tr, case.steps):
        assert np.array_equal(r.sp.active_column, case.A[j]), f"{name}: step {r.t}: the active columns are not the pattern's"
        assert r.sp.overlaps[case.A[j]].min() == GROUP_BITS and r.sp.overlaps.sum() == GROUP_BITS * case.k
    assert len(case.steps) >= 3 and len(tr) == len(case.steps)
    for fn in case.checks:
        fn(case, tr)
    for r in tr:                                     # the rows never widen (a device pool of 64 slots holds every case's rows)
        assert r.slots == case.slots and r.nsyn.max() <= case.slots, (name, r.t, r.slots, int(r.nsyn.max()))
    assert tr[-1].S <= case.capacity
