"""Adversarial calls of the stand-alone PredictiveProjection methods (`process` / `update`, projections.py:245-293; the C
entries htm_tm_scan / htm_tm_update), shared by tests/test_projection_methods_cpu.py (the oracle against the recorded
reference, and every case's precondition), tests/golden/generate_projection_methods.py (the recorder) and
tests/test_hip_projection_methods.py (the device against the oracle).

A case is a segment store written row by row into a TemporalMemoryOracle, a first State made by one `process`, and a list
of calls.  The arguments are the ones a caller's own TemporalMemory.process may legitimately pass and the fused step never
forms: punishment of learning cells, several learning cells per column, `winner_input` that is no subset of
`input_activation`, an earlier `prev_state`, other epsilons.  Every case carries a PRECONDITION, evaluated on the oracle
alone, that proves it reaches the path it is named for; a precondition that does not hold is a failure.

Conventions all cases keep, because the device and the reference agree only under them (both are documented with
PredictiveProjection.update):
  * `learning_output` is ascending: new segments are bound in the order of the list (projections.py:278-280), the device
    binds in ascending cell order;
  * `winner_input` holds distinct ids; the growth of one call never has a priority tie across its cut (the recorder
    asserts it: such ties are implementation-defined in the reference).

What a row can hold: segment_slots is at most 512, so a row "connected to all but m of the winners" exists for 257 winners
only; with 600 and 4 097 winners the rows hold 480 of them (as many as fit beside their other synapses), which still
leaves the growth search far fewer absent winners than its first estimate assumes.

The row that needs one slot more than segment_slots (case `connected_capacity`): `update` raises CapacityError; every
OTHER row, the counts and the counters are the oracle's; the row itself keeps the synapses it had and gains as many as fit.

Pure NumPy; nothing here touches a device."""

from types import SimpleNamespace

import numpy as np

from oracle import TMParams, TemporalMemoryOracle

STATE_FIELDS = ("prediction", "segment_potential", "matching_segment", "matching_segment_activation", "matching_segment_active",
                "max_jittered_potential", "matching_segment_jittered_potential")
COUNT_LIMIT = 65536            # learning cells of one update() call: fewer than this (the device packs two 16-bit counts)


def model_shape(N, cell_dim):
    """(columns, cells per column) of the oracle for a projection of N cells: the model's own when cell_dim divides N, else
    N columns of one cell (the projection lives in cell space; what a column is does not matter to it)."""
    return (N // cell_dim, cell_dim) if N % cell_dim == 0 else (N, 1)


class Case:
    def __init__(self, name, N, cell_dim, params, slots, seed, capacity=None):
        self.name, self.N, self.cell_dim, self.params, self.slots, self.seed = name, int(N), int(cell_dim), params, int(slots), int(seed)
        self.capacity = capacity
        self.ora = TemporalMemoryOracle(*model_shape(N, cell_dim), params, seed=seed, slots=slots)
        self.calls, self.checks, self.state0 = [], [], None
        self.record = True             # part of tests/golden/projection_methods.npz

    # ---- the store, row by row
    def put_rows(self, owners, rows, perms):
        o = self.ora
        S0, n = o.S, len(owners)
        o._ensure_slots(max([len(r) for r in rows] + [1]))
        o._ensure_rows(S0 + n)
        for i, (cell, r, pm) in enumerate(zip(owners, rows, perms)):
            s = S0 + i
            assert len(np.unique(r)) == len(r)
            o.seg_cell[s], o.seg_nsyn[s] = cell, len(r)
            o.presyn[s, :len(r)] = r
            o.perm[s, :len(r)] = np.asarray(pm, dtype=np.float32)
            o.segcount[cell] += 1
        o.S = S0 + n
        return np.arange(S0, S0 + n)

    def start(self, active, winners=None):
        """The first State ("p0": one process of `active`) and the exported store every replay starts from."""
        o = self.ora
        act = np.zeros(self.N, dtype=np.bool_)
        act[active] = True
        self.first_active = np.asarray(active, dtype=np.int64)
        o.prev_distal = o.process(active)
        o.prev_activation = act.reshape(o.column_dim, o.cell_dim)
        o.prev_prediction = (o.prev_distal.prediction > 1e-8).reshape(o.column_dim, o.cell_dim)
        o.prev_winner = None if winners is None else np.asarray(winners, dtype=np.int64)
        self.state0 = o.export_state()
        return o.prev_distal

    # ---- the calls (data only)
    def process(self, active, jitter=True, save=None):
        active = np.asarray(active, dtype=np.int64)
        assert len(np.unique(active)) == len(active), "repeated ids are refused (the reference counts them twice in the potential)"
        self.calls.append(dict(op="process", active=active, jitter=bool(jitter), save=save))

    def jitter(self, state):
        self.calls.append(dict(op="jitter", state=state))

    def update(self, prev, activation, learning, punish, winner=None, output_learning=None, eps=1e-8, raises=None):
        a = np.zeros(self.N, dtype=np.bool_)
        a[np.asarray(activation, dtype=np.int64)] = True
        pm = np.zeros(self.N, dtype=np.bool_)
        pm[np.asarray(punish, dtype=np.int64)] = True
        ol = None
        if output_learning is not None:
            ol = np.zeros(self.N, dtype=np.bool_)
            ol[np.asarray(output_learning, dtype=np.int64)] = True
        self.calls.append(dict(op="update", prev=prev, activation=a, learning=np.asarray(learning, dtype=np.int64), punish=pm,
                               winner=None if winner is None else np.asarray(winner, dtype=np.int64), output_learning=ol,
                               eps=float(eps), raises=raises))

    def check(self, fn):
        self.checks.append(fn)


def fresh_oracle(case):
    o = TemporalMemoryOracle(*model_shape(case.N, case.cell_dim), case.params, seed=case.seed, slots=case.slots)
    o.import_state(case.state0)
    return o


def store_snapshot(seg_cell, presyn, perm, nsyn, segcount):
    """The store as the tests compare it: owner, count, and the valid synapses of every row sorted by presynaptic id, the
    permanences as int32 bit patterns (oracle.canonical_synapses, vectorised)."""
    presyn = np.asarray(presyn, dtype=np.int64)
    perm = np.asarray(perm, dtype=np.float32)
    order = np.argsort(np.where(presyn >= 0, presyn, np.iinfo(np.int64).max), axis=1, kind="stable")
    ps, pm = np.take_along_axis(presyn, order, axis=1), np.take_along_axis(perm, order, axis=1)
    valid = ps >= 0
    return dict(seg_cell=np.asarray(seg_cell, dtype=np.int64), seg_nsyn=np.asarray(nsyn, dtype=np.int64),
                segcount=np.asarray(segcount, dtype=np.int64), syn_count=valid.sum(axis=1).astype(np.int64),
                syn_presyn=ps[valid], syn_perm_bits=np.ascontiguousarray(pm[valid]).view(np.int32).astype(np.int64))


def oracle_snapshot(o):
    S = o.S
    return store_snapshot(o.seg_cell[:S], o.presyn[:S], o.perm[:S], o.seg_nsyn[:S], o.segcount)


def state_fields(st):
    return {f: np.asarray(getattr(st, f)) for f in STATE_FIELDS}


def replay(case, target=None, before=False):
    """The case's calls on `target` (default: a fresh oracle; anything with the reference's process / update /
    get_jittered_potential_info and a `snapshot()`), one record per call:
      op, store (store_snapshot after the call), state (state_fields, process calls), last (the oracle's last_update, update
      calls), raised (update calls with `raises`), and with before=True the oracle's rows before an update (nsyn, presyn, perm)."""
    o = fresh_oracle(case) if target is None else None
    states = {"p0": o.prev_distal if o is not None else target.first_state}
    out = []
    for call in case.calls:
        rec = SimpleNamespace(op=call["op"], state=None, last=None, raised=None, before=None)
        if call["op"] == "process":
            st = o.process(call["active"]) if o is not None else target.process(call["active"], return_jittered_potential_info=call["jitter"])
            if call["save"]:
                states[call["save"]] = st
            if call["jitter"]:
                rec.state = state_fields(st)
            else:
                rec.state = {f: np.asarray(getattr(st, f)) for f in STATE_FIELDS[:5]}
        elif call["op"] == "jitter":
            st = states[call["state"]]
            if o is None:
                target.get_jittered_potential_info(st)
            rec.state = state_fields(st)
        else:
            prev = None if call["prev"] is None else states[call["prev"]]
            if o is not None:
                if before:
                    rec.before = SimpleNamespace(nsyn=o.seg_nsyn[:o.S].copy(), presyn=o.presyn[:o.S].copy(), perm=o.perm[:o.S].copy(), S=o.S)
                o.update(prev, call["activation"], call["learning"], call["punish"], winner_input=call["winner"],
                         output_learning=call["output_learning"], epsilon=call["eps"])
                rec.last = o.last_update if prev is not None else None
            else:
                rec.raised = target.update(prev, call["activation"], call["learning"], call["punish"], call["winner"],
                                           call["output_learning"], call["eps"], call["raises"])
        rec.store = oracle_snapshot(o) if o is not None else target.snapshot()
        out.append(rec)
    if o is not None:
        replay.last_oracle = o
    return out


# ------------------------------------------------------------------------------------------ building blocks

def pick(rng, N, n, must=(), exclude=()):
    """n distinct cells of [0, N), the cells `must` among them, none of `exclude`; ascending."""
    must = np.unique(np.asarray(must, dtype=np.int64))
    banned = np.zeros(N, dtype=np.bool_)
    banned[must] = True
    banned[np.asarray(exclude, dtype=np.int64)] = True
    rest = rng.permutation(np.flatnonzero(~banned))[:max(n - len(must), 0)]
    return np.sort(np.concatenate([must, rest]))


def random_rows(rng, n, N, pool, k_range, noise, perm_ranges):
    """n rows of k in k_range distinct presynaptic cells, each from `pool` with probability 1 - noise, and float32 permanences
    drawn from one of `perm_ranges` per row."""
    rows, perms = [], []
    for _ in range(n):
        k = int(rng.randint(k_range[0], k_range[1] + 1))
        n_pool = min(int(rng.binomial(k, 1.0 - noise)), len(pool))
        cand = np.concatenate([rng.permutation(pool)[:n_pool], rng.permutation(N)[:k]])
        _, first = np.unique(cand, return_index=True)
        cells = cand[np.sort(first)][:k]
        lo, hi = perm_ranges[int(rng.randint(len(perm_ranges)))]
        rows.append(cells)
        perms.append(rng.uniform(lo, hi, size=len(cells)).astype(np.float32))
    return rows, perms


def special_cells(N, K):
    """Cells where a layout goes wrong: the first and the last, the ends of the first column's words, the start of the last
    column (next to the padding of an engine laid out in whole words)."""
    s = {0, N - 1, min(K - 1, N - 1), min(K, N - 1), max(N - K, 0), min(31, N - 1), min(32, N - 1), max(N - 2, 0)}
    return np.array(sorted(s), dtype=np.int64)


def scenario(c, rng, n_active=60, n_seg=200, k_range=(4, 20), noise=0.3, n_owner_cells=100, specials=(),
             perm_ranges=((0.0, 0.15), (0.3, 0.9))):
    """A random store around one set of active cells: returns (active cells, owner cells, segment ids)."""
    N = c.N
    A = pick(rng, N, n_active, must=specials)
    owner_cells = pick(rng, N, n_owner_cells, must=specials)
    owners = owner_cells[rng.randint(len(owner_cells), size=n_seg)]
    owners[:len(specials)] = specials
    rows, perms = random_rows(rng, n_seg, N, A, k_range, noise, perm_ranges)
    for i in range(len(specials)):                     # the special cells are presynaptic too
        if specials[(i + 1) % len(specials)] not in rows[i]:
            rows[i][0] = specials[(i + 1) % len(specials)]
            _, first = np.unique(rows[i], return_index=True)
            keep = np.sort(first)
            rows[i], perms[i] = rows[i][keep], perms[i][keep]
    segs = c.put_rows(owners, rows, perms)
    return A, owner_cells, segs


def matching_owner_cells(o, st):
    return np.unique(o.seg_cell[st.matching_segment])


def usual_update(c, rng, st, A, owner_cells, n_unaccounted=10, winner=None, punish_learning=0.0, punish_others=0.5, specials=(),
                 eps=1e-8, prev="p0", activation=None, keep_out=(), keep_in=()):
    """One update in the general form: the owners of about half the matching segments learn (none of `keep_out`), with
    `n_unaccounted` cells that have no matching segment; the punishment covers the share `punish_learning` of the learning cells
    (only the learn-and-punish family and the special cells of the layouts: elsewhere no segment is in both sets, so that a
    family fails for its own reason), some other owners, and cells that own nothing."""
    o, N = c.ora, c.N
    mcells = matching_owner_cells(o, st)
    learn_m = np.setdiff1d(mcells[rng.rand(len(mcells)) < 0.5] if len(mcells) else mcells, keep_out)
    free = np.flatnonzero(st.max_jittered_potential < np.float32(eps))
    unacc = pick(rng, N, 0, must=rng.permutation(np.setdiff1d(free, specials))[:n_unaccounted])
    learning = np.unique(np.concatenate([learn_m, unacc, np.asarray(specials, dtype=np.int64), np.asarray(keep_in, dtype=np.int64)]))
    others = np.setdiff1d(owner_cells, learning)
    punish = np.unique(np.concatenate([others[rng.rand(len(others)) < punish_others], np.setdiff1d(rng.permutation(N)[:N // 16], learning)]))
    punish = np.unique(np.concatenate([punish, learning[rng.rand(len(learning)) < punish_learning], np.asarray(specials, dtype=np.int64)]))
    c.update(prev, A if activation is None else activation, learning, punish, winner=winner, eps=eps)
    return learning, punish


# ------------------------------------------------------------------------------------------ the families

def _overlap_check(min_both):
    def check(case, tr, ora):
        last = [r.last for r in tr if r.op == "update" and r.last is not None][0]
        both = np.intersect1d(last.learning, last.punished)
        assert len(both) >= min_both, f"{case.name}: {len(both)} segments both learn and are punished, want {min_both}"
    return check


def learn_punish(grow):
    """Family 1: a segment that both learns and is punished (256 columns x 8 cells, 300 segments).  increment 0.02,
    punishment 0.07, decrement 0.03: an ACTIVE synapse of permanence p ends at f32(f32(p + 0.02) - 0.07) -- pruned iff that
    is negative, i.e. p < 0.05; punished first it is pruned for p < 0.07, learning alone keeps it, punishment alone prunes
    p < 0.07 and leaves f32(p - 0.07).  An INACTIVE synapse ends at f32(p - 0.03) only under learning.  So every wrong order
    and every lost update changes bit patterns or counts of the rows that are in both sets.  grow: winner_input is a
    subset of the active cells, the learning step's new synapses (0.21) are active and the punishment lowers them to
    f32(0.21f - 0.07)."""
    c = Case(f"learn_punish_{'grow' if grow else 'plain'}", 2048, 8,
             TMParams(permanence_increment=0.02, permanence_decrement=0.03, permanence_punishment=0.07, segment_activation_threshold=6,
                      segment_matching_threshold=4, segment_sampling_synapses=12), slots=64, seed=11 + grow)
    rng = np.random.RandomState(100 + grow)
    A, owner_cells, _ = scenario(c, rng, n_active=60, n_seg=300, k_range=(4, 20), noise=0.3, n_owner_cells=120,
                                 perm_ranges=((0.0, 0.1), (0.03, 0.09), (0.3, 0.9)))
    st = c.start(A)
    W = rng.permutation(A)[:30] if grow else None
    usual_update(c, rng, st, A, owner_cells, winner=None if W is None else np.sort(W), punish_learning=0.5)
    c.process(np.unique(np.concatenate([A[::2], rng.permutation(c.N)[:30]])))
    c.check(_overlap_check(8))

    def both_prune(case, tr, ora):
        r = [r for r in tr if r.op == "update"][0]
        both = np.intersect1d(r.last.learning, r.last.punished)
        act = np.r_[case.calls[0]["activation"], False]
        ps, pm = r.before.presyn[both], r.before.perm[both]
        active = act[np.where(ps >= 0, ps, case.N)]
        assert (active & (pm >= 0.0) & (pm < 0.045)).any(), "no synapse that only the two updates together prune"
        assert (active & (pm > 0.052) & (pm < 0.068)).any(), "no synapse whose fate depends on the order of the two updates"
        assert (~active & (ps >= 0) & (pm < 0.029)).any(), "no synapse the learning step alone prunes"
        if grow:
            want = np.float32(np.float64(np.float32(0.21)) - 0.07).view(np.int32)
            assert (tr[0].store["syn_perm_bits"] == want).any(), "no grown synapse was punished"
    c.check(both_prune)
    return c


def multi_learning(K):
    """Family 2: every cell of several columns learns (32 of 32, 64 of 64), most of them without a matching segment; the store has
    dead segments in three 1 024-id blocks, fewer than the requests: recycling and appending happen in one call."""
    C = 96 if K == 32 else 40
    c = Case(f"multi_learning_k{K}", C * K, K, TMParams(segment_activation_threshold=4, segment_matching_threshold=3,
                                                       segment_sampling_synapses=8), slots=64, seed=21 + K, capacity=4096)
    rng = np.random.RandomState(200 + K)
    N = c.N
    full_cols = np.array([1, C // 2, C - 1])
    A, owner_cells, segs = scenario(c, rng, n_active=50, n_seg=2300, k_range=(3, 10), noise=0.3, n_owner_cells=400,
                                    specials=special_cells(N, K), perm_ranges=((0.2, 0.9),))
    o = c.ora
    dead = np.r_[np.arange(1000, 1050), np.arange(2100, 2112)]
    for s in dead:                                     # dead: fewer synapses than the matching threshold
        keep = int(rng.randint(0, 3))
        o.presyn[s, keep:], o.perm[s, keep:], o.seg_nsyn[s] = -1, -1.0, keep
    st = c.start(A)
    cells = np.unique(np.concatenate([(full_cols[:, None] * K + np.arange(K)).reshape(-1), rng.permutation(N)[:40], special_cells(N, K)]))
    punish = np.setdiff1d(np.unique(np.r_[rng.permutation(N)[:N // 8], owner_cells[::3]]), cells)
    c.update("p0", A, cells, punish, winner=np.sort(rng.permutation(A)[:20]))
    c.process(np.unique(np.concatenate([A[5:], rng.permutation(N)[:20]])))

    def check(case, tr, ora):
        last = tr[0].last
        assert len(last.recycled) > 0 and len(last.fresh) > 0, "recycling and appending must both happen"
        assert len(np.unique(last.recycled >> 10)) > 1, "recycled ids in one 1 024-block only"
        assert len(last.unaccounted) * 2 >= len(case.calls[0]["learning"]), "fewer than half the learning cells are unaccounted"
        assert len(last.learning) > 0, "no matching segment learns"
    c.check(check)
    return c


WINNER_SIZES = (None, 0, 1, 63, 64, 65, 255, 256, 257, 1000, 4096, 4097, 8192)
RELATIONS = ("disjoint", "subset", "overlapping")
SAMPLES = (1, 18, 32, 64, 1, 18, 32, 64, 1, 18, 64, 32, 64)        # per size: every width at small and at large sizes


def winner_sizes(i):
    """Family 3: `winner_input` of a given size -- None, empty, around the 64-lane chunks, the 256 staged candidates and the 4 096
    winners kept in LDS -- disjoint from the activation, inside it, or half of each; segment_sampling_synapses from SAMPLES
    (the three rank widths: up to 64, 128, 256 candidates)."""
    n_w, relation, sample = WINNER_SIZES[i], RELATIONS[i % 3], SAMPLES[i]
    c = Case(f"winners_{'none' if n_w is None else n_w}_{relation}_s{sample}", 16384, 32,
             TMParams(segment_activation_threshold=5, segment_matching_threshold=4, segment_sampling_synapses=sample), slots=128, seed=31 + i)
    rng = np.random.RandomState(300 + i)
    N = c.N
    A, owner_cells, _ = scenario(c, rng, n_active=80, n_seg=150, k_range=(4, 40), noise=0.2, n_owner_cells=90, perm_ranges=((0.15, 0.9),))
    st = c.start(A)
    W, activation = None, A
    if n_w is not None:
        outside = rng.permutation(np.setdiff1d(np.arange(N), A))
        if relation == "disjoint":
            W = outside[:n_w]
        elif relation == "subset":
            W = np.concatenate([rng.permutation(A)[:min(n_w, 40)], outside[:max(n_w - 40, 0)]])[:n_w]
            activation = np.union1d(A, W)
        else:
            W = outside[:n_w]
            activation = np.union1d(A, W[::2])
        W = np.sort(W)
    learning, _ = usual_update(c, rng, st, A, owner_cells, n_unaccounted=5, winner=W, activation=activation)
    c.process(np.unique(np.concatenate([A[::3], rng.permutation(N)[:40]]))[::-1])

    def check(case, tr, ora):
        call, r = case.calls[0], tr[0]
        w, act = call["winner"], call["activation"]
        assert (w is None) == (n_w is None) and (w is None or len(w) == n_w == len(np.unique(w)))
        if not n_w:
            assert r.store["syn_count"].sum() <= (r.before.presyn >= 0).sum(), "growth without winners"
            return
        inside = int(act[w].sum())
        assert {"disjoint": inside == 0, "subset": inside == n_w, "overlapping": 0 < inside < n_w or n_w == 1}[relation], (relation, inside)
        new = np.setdiff1d(r.store["syn_presyn"], r.before.presyn[r.before.presyn >= 0])
        assert len(np.intersect1d(new, w)) > 0 or len(r.last.fresh) > 0, "nothing grew"
        is_w = np.zeros(case.N + 1, dtype=np.bool_)
        is_w[w] = True
        before_w = is_w[np.where(r.before.presyn >= 0, r.before.presyn, case.N)].sum()
        assert is_w[r.store["syn_presyn"]].sum() > before_w, "no synapse to a winner was grown"
        if n_w >= 8192:                              # (4 097: the one winner past the 4 096 kept in LDS is read by every growing segment's search)
            late = np.zeros(case.N + 1, dtype=np.bool_)
            late[w[4096:]] = True
            assert late[r.store["syn_presyn"]].sum() > late[np.where(r.before.presyn >= 0, r.before.presyn, case.N)].sum(), \
                "no grown synapse to a winner beyond the first 4 096"
    c.check(check)
    return c


CONNECTED_MISSING = (0, 1, 10, 29, 30, 31)         # n_add = 30 below: {0, 1, 10, n_add - 1, n_add, n_add + 1}


def mostly_connected(n_w, overflow=False):
    """Family 4: learning segments already connected to most of the previous winners, few of their synapses active (hypothesis:
    the growth search gives up although winners are absent).  segment_slots 512, sampling 32, every such row has 2 active
    synapses: n_add = 30.  257 winners: rows that hold all but m of them, m in CONNECTED_MISSING, once as they are and once
    filled with other cells so that the growth ends exactly on slot 512.  600 / 4 097 winners: rows that hold 480, 470 and 450
    of them (482 synapses with the two active ones: growth ends exactly on the last slot).  overflow: one row that would
    need slot 513."""
    c = Case(f"connected_{'capacity' if overflow else n_w}", 16384, 32,
             TMParams(permanence_increment=0.1, permanence_decrement=0.001, segment_activation_threshold=2, segment_matching_threshold=2,
                      segment_sampling_synapses=32), slots=512, seed=41 + n_w + overflow, capacity=4096)
    rng = np.random.RandomState(400 + n_w + overflow)
    N, n_add = c.N, 30
    A = pick(rng, N, 40)
    W = pick(rng, N, n_w, exclude=A)
    rest = np.setdiff1d(np.arange(N), np.r_[A, W])
    rows, owners = [], pick(rng, N, 64, exclude=np.r_[A, W])
    plans = []                                        # (winners held, total synapses before the call)
    if overflow:
        plans = [(min(n_w, 481) - 31, 483), (n_w - 5 if n_w < 400 else 400, 0)]
    elif n_w <= 480:
        plans = [(n_w - m, 0) for m in CONNECTED_MISSING] + [(n_w - m, 512 - min(m, n_add)) for m in CONNECTED_MISSING]
    else:
        plans = [(480, 0), (470, 0), (450, 0), (480, 482), (300, 482), (40, 482)]
    for held, total in plans:
        row = np.concatenate([rng.permutation(A)[:2], rng.permutation(W)[:held]])
        if total:
            row = np.concatenate([row, rng.permutation(rest)[:total - len(row)]])
        rows.append(row)
    more_rows, more_perms = random_rows(rng, 40, N, A, (2, 30), 0.3, ((0.2, 0.9),))
    own = np.r_[owners[:len(rows)], owners[rng.randint(len(owners), size=40)]]
    c.put_rows(own, rows + more_rows, [np.full(len(r), 0.5, dtype=np.float32) for r in rows] + more_perms)
    st = c.start(A)
    learning = np.unique(np.r_[owners[:len(rows)], owners[len(rows)::2], pick(rng, N, 4, exclude=np.r_[A, W, owners])])
    punish = np.setdiff1d(np.unique(np.r_[owners[1::2], rng.permutation(N)[:200]]), learning)
    c.update("p0", A, learning, punish, winner=W, raises="capacity" if overflow else None)
    if not overflow:
        c.process(np.unique(np.concatenate([A[::2], W[::7]])))
    c.overflow_rows = np.array([0]) if overflow else np.zeros(0, dtype=np.int64)

    def check(case, tr, ora):
        r = tr[0]
        is_w = np.zeros(case.N + 1, dtype=np.bool_)
        is_w[W] = True
        n_plans = len(plans)
        assert np.isin(np.arange(n_plans), r.last.learning).all(), "a planned row does not learn"
        held = is_w[np.where(r.before.presyn[:n_plans] >= 0, r.before.presyn[:n_plans], case.N)].sum(axis=1)
        absent = n_w - held
        after = np.asarray(ora.seg_nsyn[:n_plans]).astype(np.int64) if overflow else r.store["seg_nsyn"][:n_plans]
        assert np.array_equal(after - r.before.nsyn[:n_plans], np.minimum(absent, n_add)), "growth is not min(absent, n_add)"
        if overflow:
            assert after[0] == 513 and after[1:].max() <= 512
        elif n_w == 257:
            assert ((absent > 0) & (absent < n_add)).any() and (absent == 0).any(), "hypothesis 2 is not reached"
            assert (after == 512).sum() >= 4, "no growth that ends on the last slot"
        else:
            assert (held >= 450).any() and (after == 512).sum() >= 3
    c.check(check)
    return c


def pc_classified(case, output_learning):
    """The matching segments of the case's first State that learn under `output_learning` (projections.py:264-268, epsilon 1e-8)."""
    o = fresh_oracle(case)
    d = o.prev_distal
    cell = o.seg_cell[d.matching_segment]
    best = np.abs(d.matching_segment_jittered_potential - d.max_jittered_potential[cell]) < np.float32(1e-8)
    return d.matching_segment[output_learning[cell] & (d.matching_segment_active | ((d.prediction[cell] < 1e-8) & best))]


LAYOUTS = ((600, 1), (2048, 8), (2048, 32), (33 * 40, 33), (48 * 40, 48), (64 * 32, 64), (96 * 20, 96), (1000, 32), (4097, 32))


def layout(N, K):
    """Family 5: cells per column 1, 8, 32, 33, 48, 64 (one and two words per column), 96 (laid out as flat words of 32) and
    output_dim 1 000 / 4 097 (a last word with padding); the first and last cell, the word ends and the cells next to the padding
    are active, learning, punished, owners and presynaptic."""
    c = Case(f"layout_n{N}_k{K}", N, K, TMParams(permanence_punishment=0.05, segment_activation_threshold=4, segment_matching_threshold=3,
                                                segment_sampling_synapses=10), slots=64, seed=51 + K + N)
    rng = np.random.RandomState(500 + N + K)
    sp = special_cells(N, K)
    A, owner_cells, _ = scenario(c, rng, n_active=40, n_seg=160, k_range=(3, 14), noise=0.25, n_owner_cells=60, specials=sp)
    st = c.start(A)
    usual_update(c, rng, st, A, owner_cells, n_unaccounted=8, winner=np.sort(np.unique(np.r_[rng.permutation(A)[:12], sp[::2], rng.permutation(N)[:10]])),
                 specials=sp)
    # output_learning of its own (projections.py:260-262 only builds it when the caller passes none): it classifies the matching
    # segments -- some learning cells are left out of it, some other owners are in -- while learning_output alone decides who
    # gets a new segment
    call = c.calls[-1]
    others = np.setdiff1d(owner_cells, np.r_[call["learning"], np.flatnonzero(call["punish"])])
    ol = np.union1d(np.setdiff1d(call["learning"], np.setdiff1d(call["learning"], sp)[::3]), others[:6])
    call["output_learning"] = np.isin(np.arange(N), ol)
    c.process(np.unique(np.r_[A[::2], sp, rng.permutation(N)[:20]]))
    c.update(None, A, sp, sp)                          # prev_state=None: nothing happens (projections.py:258-259)

    def check(case, tr, ora):
        call = case.calls[0]
        assert call["activation"][sp].all() and call["punish"][sp].all() and np.isin(sp, call["learning"]).all()
        mask = np.zeros(case.N, dtype=np.bool_)
        mask[call["learning"]] = True
        plain = pc_classified(case, mask)
        assert not np.array_equal(plain, tr[0].last.learning), "output_learning changes nothing"
        assert np.isin(sp, tr[0].before.presyn).all() and np.isin(sp, tr[0].store["seg_cell"]).all()
        assert all(np.array_equal(tr[2].store[f], tr[1].store[f]) for f in tr[1].store), "update(None, ...) changed the store"
    c.check(check)
    return c


def process_alone(matching, activation):
    """Family 6: process on its own -- no active input, every cell active, ids in descending order, two calls in a row
    (repeated ids are refused: tests/test_hip_projection_methods.py), a State asked for without
    its jitter and completed later, potentials of 512 = segment_slots; thresholds matching == activation, and matching 1."""
    c = Case(f"process_m{matching}_a{activation}", 2048, 8, TMParams(segment_activation_threshold=activation, segment_matching_threshold=matching,
                                                                  segment_sampling_synapses=12), slots=512, seed=61 + matching)
    rng = np.random.RandomState(600 + matching)
    N = c.N
    A, owner_cells, _ = scenario(c, rng, n_active=50, n_seg=120, k_range=(1, 16), noise=0.3, n_owner_cells=70, perm_ranges=((0.3, 0.7),))
    full = [rng.permutation(N)[:512], rng.permutation(N)[:512], rng.permutation(N)[:511]]
    full_owners = pick(rng, N, 3, exclude=owner_cells)
    c.put_rows(full_owners, full, [rng.uniform(0.3, 0.7, size=len(r)) for r in full])
    st = c.start(A)
    c.process(np.zeros(0, dtype=np.int64))
    c.process(np.arange(N), save="all")
    c.process(A[::-1])
    late = np.unique(np.r_[A[::2], rng.permutation(N)[:30]])
    c.process(late, jitter=False, save="late")
    c.jitter("late")
    usual_update(c, rng, st, A, owner_cells, winner=np.sort(rng.permutation(N)[:25]), prev="late", activation=late, keep_out=full_owners)
    c.process(A)

    def check(case, tr, ora):
        assert len(tr[0].state["matching_segment"]) == 0 and tr[0].state["segment_potential"].max() == 0
        assert tr[1].state["segment_potential"].max() == 512 and len(tr[1].state["matching_segment"]) > 60
        assert np.array_equal(tr[1].state["segment_potential"], tr[1].store["seg_nsyn"])
        m = tr[2].state
        assert (m["segment_potential"][m["matching_segment"]] == matching).any(), "no segment exactly at the matching threshold"
        assert (m["matching_segment_activation"] == activation).any() or matching == 1, "no segment exactly at the activation threshold"
        assert (m["matching_segment_activation"] == activation - 1).any() or matching == 1
    c.check(check)
    return c


def prev_states():
    """Family 7: an earlier State (three process calls back, the store grown in between) as prev_state; one State used for two
    updates (no segment of its matching set falls below the matching threshold in between); prev_state=None."""
    c = Case("prev_states", 2048, 8, TMParams(permanence_decrement=0.02, segment_activation_threshold=5, segment_matching_threshold=4,
                                             segment_sampling_synapses=14), slots=64, seed=71)
    rng = np.random.RandomState(700)
    N = c.N
    A, owner_cells, _ = scenario(c, rng, n_active=60, n_seg=200, k_range=(4, 18), noise=0.3, n_owner_cells=90, perm_ranges=((0.3, 0.9),))
    st = c.start(A)
    acts = [A]
    for i in range(3):
        W = np.sort(rng.permutation(acts[-1])[:20])
        usual_update(c, rng, st if i == 0 else c.ora.prev_distal, acts[-1], owner_cells, n_unaccounted=12, winner=W, prev=f"p{i}",
                     activation=acts[-1], punish_learning=0.0)
        nxt = np.unique(np.r_[acts[-1][::2], rng.permutation(N)[:35]])
        c.process(nxt, save=f"p{i + 1}")
        # (build time only: the case's own oracle follows the calls, so that the next update is chosen against a real State)
        call = c.calls[-2]
        c.ora.update(st if i == 0 else c.ora.prev_distal, call["activation"], call["learning"], call["punish"], winner_input=call["winner"])
        c.ora.prev_distal = c.ora.process(nxt)
        acts.append(nxt)
    W = np.sort(rng.permutation(A)[:20])
    learning0, punish0 = c.calls[0]["learning"], np.flatnonzero(c.calls[0]["punish"])
    c.update("p0", A, learning0, punish0, winner=W)                   # the State of three process calls earlier
    c.update("p0", A, learning0, punish0, winner=W)                   # ... and once more
    c.update(None, A, learning0, punish0, winner=W)
    c.process(A)

    def check(case, tr, ora):
        m0 = case.state0["matching_segment"]
        assert tr[5].store["seg_cell"].size > case.state0["seg_cell"].size + 20, "the store did not grow in between"
        for i in (5, 6, 7):
            assert (tr[i].store["seg_nsyn"][m0] >= case.params.segment_matching_threshold).all(), "a segment of the earlier matching set died"
        assert len(tr[6].last.learning) > 10 and len(np.unique(np.r_[tr[6].last.learning, tr[6].last.recycled])) == len(tr[6].last.learning) + len(tr[6].last.recycled)
        assert not np.array_equal(tr[6].store["syn_perm_bits"], tr[7].store["syn_perm_bits"]), "the second update changed nothing"
        assert all(np.array_equal(tr[8].store[f], tr[7].store[f]) for f in tr[7].store), "update(None, ...) changed the store"
    c.check(check)
    return c


def epsilons(eps):
    """Family 8: epsilon 1e-8, 0.3, 1.0 with several best-matching segments per cell: cells own four matching segments of one
    potential, whose jittered potentials differ by less than 1."""
    c = Case(f"epsilon_{eps}", 2048, 8, TMParams(segment_activation_threshold=9, segment_matching_threshold=4, segment_sampling_synapses=12),
             slots=64, seed=81)
    rng = np.random.RandomState(800)
    N = c.N
    A, owner_cells, _ = scenario(c, rng, n_active=50, n_seg=100, k_range=(4, 14), noise=0.3, n_owner_cells=60, perm_ranges=((0.3, 0.9),))
    twins = pick(rng, N, 25, exclude=owner_cells)
    rows = [np.r_[rng.permutation(A)[:6], rng.permutation(np.setdiff1d(np.arange(N), A))[:3]] for _ in range(100)]
    c.put_rows(np.repeat(twins, 4), rows, [rng.uniform(0.3, 0.9, size=9) for _ in rows])
    st = c.start(A)
    usual_update(c, rng, st, A, np.r_[owner_cells, twins], winner=np.sort(rng.permutation(A)[:20]), eps=eps, keep_in=twins[:20])
    c.process(A[::2])

    def check(case, tr, ora):
        n = np.bincount(ora.seg_cell[tr[0].last.learning], minlength=case.N)[twins[:20]]
        assert n.min() >= 1 and {1e-8: n.max() == 1, 0.3: 1 < n.max() and n.min() < 4, 1.0: n.min() == 4}[eps], (eps, n)
    c.check(check)
    return c


def count_limit(C, K, n_learning=COUNT_LIMIT - 1):
    """Family 9: 65 535 learning cells in one call (2 048 x 32 and 1 024 x 64: every cell but one), about half of them without a
    matching segment.  n_learning >= 65 536 is refused (tests/test_hip_projection_methods.py)."""
    c = Case(f"count_{C}x{K}_{n_learning}", C * K, K, TMParams(segment_activation_threshold=3, segment_matching_threshold=2,
                                                              segment_sampling_synapses=4), slots=64, seed=91 + K, capacity=80000)
    rng = np.random.RandomState(900 + K)
    N = c.N
    A = pick(rng, N, 64)
    o = c.ora
    owners = np.sort(rng.permutation(N)[:N // 2])
    S = len(owners)
    o._ensure_rows(S)
    o.seg_cell[:S], o.seg_nsyn[:S] = owners, 3
    o.presyn[:S, :3] = A[(np.arange(S)[:, None] * 7 + np.arange(3) * 5) % 64]         # three distinct active cells each
    o.perm[:S, :3] = rng.uniform(0.3, 0.9, size=(S, 3)).astype(np.float32)
    o.segcount[owners] = 1
    o.S = S
    c.start(A)
    learning = np.arange(N)[:n_learning] if n_learning < N else np.arange(N)
    c.update("p0", A, learning, np.setdiff1d(np.arange(N), learning), winner=A[::4])
    c.process(A[::2])
    c.record = n_learning < COUNT_LIMIT

    def check(case, tr, ora):
        if tr:
            assert abs(len(tr[0].last.unaccounted) - n_learning / 2) < 2 and len(tr[0].last.learning) > 30000
    c.check(check)
    return c


def all_case_names():
    names = ["learn_punish_plain", "learn_punish_grow", "multi_learning_k32", "multi_learning_k64"]
    names += [f"winners_{i}" for i in range(len(WINNER_SIZES))]
    names += ["connected_257", "connected_600", "connected_4097", "connected_capacity"]
    names += [f"layout_{i}" for i in range(len(LAYOUTS))]
    names += ["process_m5_a5", "process_m1_a3", "prev_states", "epsilon_1e-08", "epsilon_0.3", "epsilon_1.0",
              "count_2048x32", "count_1024x64"]
    return names


CASE_NAMES = all_case_names()
_built = {}


def build(name):
    """The case of that name, built once per process (the builders are deterministic)."""
    if name not in _built:
        if name.startswith("learn_punish"):
            c = learn_punish(name.endswith("grow"))
        elif name.startswith("multi_learning"):
            c = multi_learning(int(name.rsplit("k", 1)[1]))
        elif name.startswith("winners_"):
            c = winner_sizes(int(name.split("_")[1]))
        elif name == "connected_capacity":
            c = mostly_connected(257, overflow=True)
        elif name.startswith("connected_"):
            c = mostly_connected(int(name.split("_")[1]))
        elif name.startswith("layout_"):
            c = layout(*LAYOUTS[int(name.split("_")[1])])
        elif name.startswith("process_"):
            c = process_alone(*{"process_m5_a5": (5, 5), "process_m1_a3": (1, 3)}[name])
        elif name == "prev_states":
            c = prev_states()
        elif name.startswith("epsilon_"):
            c = epsilons(float(name.split("_")[1]))
        elif name.startswith("count_"):
            shape = name.split("_")[1].split("x")
            c = count_limit(int(shape[0]), int(shape[1]), int(name.split("_")[2]) if name.count("_") > 1 else COUNT_LIMIT - 1)
        else:
            raise KeyError(name)
        c.key = name
        _built[name] = c
    return _built[name]


_traces = {}


def oracle_trace(name):
    """replay(build(name)) on the oracle, computed once and shared by the tests of a process (left unchanged by them)."""
    if name not in _traces:
        _traces[name] = (replay(build(name), before=True), replay.last_oracle)
    return _traces[name]


def check_preconditions(name):
    case = build(name)
    tr, ora = oracle_trace(name)
    assert case.checks, f"{name}: a case without a precondition"
    for fn in case.checks:
        fn(case, tr, ora)
    overflow = any(call.get("raises") for call in case.calls)
    assert (ora.slots > case.slots) == overflow, f"{name}: rows of {ora.slots} slots, segment_slots is {case.slots}"
    assert case.slots % 64 == 0 and 64 <= case.slots <= 512 and ora.S <= (case.capacity or 4096)
    for r in tr:                                     # only the families named for it have a segment in both sets
        if r.last is not None and not name.startswith(("learn_punish", "layout_")):
            assert len(np.intersect1d(r.last.learning, r.last.punished)) == 0, f"{name}: a segment learns and is punished"

