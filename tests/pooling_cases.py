"""Shared by tests/test_pooling_cpu.py and tests/test_hip_pooling.py: the cases of htm_pool_columns, each named with the path it
reaches, the NumPy statement of the entry's contract (bank rotation, untouched rows, ids outside the range, resets; batches and
calls carry the state, so they do not show in it), the predicates that say which path a case reaches, the committed stream of the
model-level property and the chained oracles of a pooled stack.  Not collected by pytest.

The kernels' geometry the cases aim at (bithtm_amd/csrc/htm_pool.h): a scan block covers SCAN_BLOCK columns, a select thread
THREAD columns (16 snapshot bytes), a select block TRIP columns per trip."""

from types import SimpleNamespace

import numpy as np

from bithtm_amd.pooling import PoolingLink, PoolingState

SCAN_BLOCK, THREAD, WORD, TRIP = 256, 16, 32, 4096
DEFAULT = dict(active_weight=1, predicted_weight=8, decay=1, ceiling=16)


def words_of(bits):
    """bool[n, C] -> uint32[n, ceil(C / 32)], bit c of a row = bits[c] (the layout of a recorded column_prediction row)."""
    bits = np.asarray(bits, dtype=np.bool_)
    pad = np.zeros((bits.shape[0], (bits.shape[1] + 31) // 32 * 32), dtype=np.bool_)
    pad[:, :bits.shape[1]] = bits
    return np.packbits(pad, axis=1, bitorder="little").view(np.uint32)


def bank_words(C):
    return (C + 127) // 128 * 4


def pool_columns(link, C, lists, colpred, persistence, prev, resets, bank, first_row, snapshots=None):
    """htm_pool_columns in NumPy.  link: a resolved PoolingLink; lists int[n_rows * stride, k]; colpred bool[n_rows * stride, C];
    persistence uint8[C] and prev bool[C], changed in place; resets: bool[bank_rows] (a reset before the window that writes that
    bank row) or None; bank uint32[bank_rows, W] (W = C padded to 128 bits, in words), changed in place: row (first_row + r) %
    bank_rows = the link's row behind window r, pad bits 0, every other row as it was.  An id outside [0, C) counts for nothing.
    Returns whether such an id was met.  `snapshots`: a list that gets the persistence behind every window."""
    lists = np.asarray(lists, dtype=np.int64)
    n_rows = lists.shape[0] // link.stride
    bank_rows, W = bank.shape
    assert W == bank_words(C) and colpred.shape == (lists.shape[0], C)
    state = PoolingState(link, C)
    state.persistence, state.prev = persistence, prev
    bad = bool(((lists < 0) | (lists >= C)).any())
    for r in range(n_rows):
        row = (first_row + r) % bank_rows
        if resets is not None and resets[row]:
            state.reset()
        for s in range(r * link.stride, (r + 1) * link.stride):
            state.step(lists[s], colpred[s])
        bits = np.zeros(W * 32, dtype=np.bool_)
        bits[:C] = state.row()
        bank[row] = np.packbits(bits, bitorder="little").view(np.uint32)
        if snapshots is not None:
            snapshots.append(persistence.copy())
    return bad


def cut_of(P, union_bits):
    """How the select settles a snapshot: (cut value, columns at the cut that win, columns at the cut); (0, 0, 0) for an empty row."""
    P = np.asarray(P, dtype=np.int64)
    positive = int((P > 0).sum())
    take = min(union_bits, positive)
    if take == 0:
        return 0, 0, 0
    cut = int(np.sort(P)[::-1][take - 1])
    return cut, take - int((P > cut).sum()), int((P == cut).sum())


def stream(C, k, steps, seed, hit=0.6):
    """Synthetic lists and column predictions: ascending random lists; a step's prediction holds about `hit` of the next step's
    columns and as many others."""
    rng = np.random.RandomState(seed)
    lists = np.stack([np.sort(rng.choice(C, k, replace=False)) for _ in range(steps + 1)]).astype(np.int32)
    colpred = np.zeros((steps, C), dtype=np.bool_)
    for s in range(steps):
        nxt = lists[s + 1]
        colpred[s, nxt[rng.rand(k) < hit]] = True
        colpred[s, rng.choice(C, max(1, k // 2), replace=False)] = True
    return lists[:steps], colpred


def case(name, C, k, stride, windows, reaches, *, union_bits=None, bank_rows=None, first_row=0, resets=None, batch_windows=None, calls=None,
         lists=None, colpred=None, persistence=None, prev=None, seed=0, **params):
    """A case: the call's inputs, `reaches` (a predicate over the case and its replay), the batch (windows per batch the scratch is
    cut to; None: all) and `calls` (the windows of each call; None: one call)."""
    p = dict(DEFAULT)
    p.update(params)
    link = PoolingLink(stride=stride, union_bits=union_bits, **p).resolved(C, k)
    if lists is None:
        lists, colpred = stream(C, k, stride * windows, seed + C + k)
    bank_rows = windows if bank_rows is None else bank_rows
    flags = None
    if resets is not None:
        flags = np.zeros(bank_rows, dtype=np.bool_)
        flags[[(first_row + r) % bank_rows for r in resets]] = True
    return SimpleNamespace(name=name, C=C, k=k, link=link, windows=windows, lists=np.asarray(lists, dtype=np.int32), colpred=np.asarray(colpred, dtype=np.bool_),
                           persistence=np.zeros(C, np.uint8) if persistence is None else np.asarray(persistence, dtype=np.uint8),
                           prev=np.zeros(C, np.bool_) if prev is None else np.asarray(prev, dtype=np.bool_),
                           bank_rows=bank_rows, first_row=first_row, resets=flags, batch_windows=batch_windows, calls=calls or [windows], reaches=reaches)


def replay(c):
    """The contract over a case from a bank of a fixed pattern -> SimpleNamespace(bank, before, persistence, prev, bad, snapshots)."""
    W = bank_words(c.C)
    before = np.random.RandomState(c.C + c.windows).randint(0, 2 ** 32, size=(c.bank_rows, W), dtype=np.uint64).astype(np.uint32)
    bank, P, prev, snaps = before.copy(), c.persistence.copy(), c.prev.copy(), []
    bad = pool_columns(c.link, c.C, c.lists, c.colpred, P, prev, c.resets, bank, c.first_row, snaps)
    return SimpleNamespace(bank=bank, before=before, persistence=P, prev=prev, bad=bad, snapshots=snaps)


# ---- what a case reaches
def _blocks(c, r):
    return (bank_words(c.C) * 32 + SCAN_BLOCK - 1) // SCAN_BLOCK


def one_partial_word(c, r):
    return c.C % 32 != 0 and c.C < 64 and bank_words(c.C) == 4 and any(s[32:].any() for s in r.snapshots)


def two_scan_blocks(c, r):
    return _blocks(c, r) == 2 and c.C > SCAN_BLOCK and any((s[SCAN_BLOCK:] > 0).any() and (s[:SCAN_BLOCK] > 0).any() for s in r.snapshots) and bool(
        r.persistence[SCAN_BLOCK:].any() or r.prev[SCAN_BLOCK:].any())


def later_trips(c, r):
    rows = np.unpackbits(r.bank.view(np.uint8), axis=1, bitorder="little")
    return c.C > 2 * TRIP and c.C % THREAD != 0 and rows[:, 2 * TRIP:].any() and all(rows[:, t * TRIP:(t + 1) * TRIP].any() for t in range(2))


def bench_shape(c, r):
    return (c.C, c.k, c.link.stride, c.windows) == (65536, 1311, 1, 8) and c.link.union_bits == 2622


def ceiling_held(c, r):
    top = [(s == c.link.ceiling) for s in r.snapshots]
    return any((a & b).any() for a, b in zip(top, top[1:])) and c.link.ceiling < 255


def plain_link(c, r):
    lk = c.link
    return lk.decay >= lk.ceiling and lk.active_weight == lk.predicted_weight >= 1 and lk.union_bits >= c.k and lk.stride == 1


def predicted_only(c, r):
    return c.link.active_weight == 0 and any((s > 0).any() for s in r.snapshots) and any((s > 0).sum() < c.k for s in r.snapshots)


def active_only(c, r):
    return c.link.predicted_weight == 0 and all((s > 0).any() for s in r.snapshots)


def one_bit(c, r):
    rows = np.unpackbits(r.bank.view(np.uint8), axis=1, bitorder="little")
    return c.link.union_bits == 1 and (rows.sum(axis=1) == 1).all() and all(cut_of(s, 1)[2] > 1 for s in r.snapshots[:1])


def every_column(c, r):
    return c.link.union_bits == c.C and all(0 < (s > 0).sum() < c.C for s in r.snapshots)


def short_row(c, r):
    return c.link.union_bits < c.C and any(0 < (s > 0).sum() < c.link.union_bits for s in r.snapshots)


def _tie(c, r):
    """(columns at the cut of the last snapshot, how many of them win) of a case whose cut falls inside a tie."""
    s = r.snapshots[-1]
    cut, want, ties = cut_of(s, c.link.union_bits)
    return np.flatnonzero(s == cut), want, ties


def tie_inside(unit):
    def reaches(c, r):
        T, want, ties = _tie(c, r)
        return 0 < want < ties and T[want - 1] // unit == T[want] // unit and want >= 2
    return reaches


def tie_across(unit):
    def reaches(c, r):
        T, want, ties = _tie(c, r)
        return 0 < want < ties and T[want - 1] + 1 == T[want] and T[want] % unit == 0 and want >= 2 and T[0] // unit < T[want - 1] // unit
    return reaches


def reset_at(window):
    def reaches(c, r):
        row = (c.first_row + window) % c.bank_rows
        return c.resets is not None and bool(c.resets[row]) and (window == 0 or (r.snapshots[window - 1] > 0).any()) and (
            c.persistence.any() or window > 0)
    return reaches


def rotated(c, r):
    written = {(c.first_row + i) % c.bank_rows for i in range(c.windows)}
    return c.first_row != 0 and c.bank_rows > c.windows and (c.first_row + c.windows) > c.bank_rows and len(written) == c.windows


def three_batches_two_calls(c, r):
    return len(c.calls) == 2 and all(-(-n // c.batch_windows) == 3 for n in c.calls[:1]) and r.snapshots[c.calls[0] - 1].any()


def bad_id(c, r):
    return r.bad and (c.lists < 0).any() and (c.lists >= c.C).any()


def _tie_case(name, boundary, unit, inside=False):
    """One window over a preset persistence whose cut falls inside a group of equal values: above the cut 6 columns, at the cut
    columns on both sides of `boundary` (or, `inside`, within one unit), the quota ending right at the boundary."""
    C, k = 2 * TRIP + 37, 8
    P = np.zeros(C, dtype=np.uint8)
    above = np.array([1, 77, 300, 4097, 8200, C - 1])
    at = np.array([boundary + 3, boundary + 5, boundary + 9]) if inside else np.array([boundary - unit - 1, boundary - 3, boundary - 1, boundary, boundary + 2,
                                                                                       min(C - 2, boundary + unit + 1)])
    P[above], P[at] = 12, 6                          # one step with decay 1: 11 and 5
    want = 2 if inside else int(np.searchsorted(at, boundary))
    lists = np.array([[2, 9, 500, 900, 4100, 4200, 8000, 8100]])           # active columns elsewhere: 1 each, below the cut
    return case(name, C, k, 1, 1, tie_inside(unit) if inside else tie_across(unit), union_bits=len(above) + want, lists=lists,
                colpred=np.zeros((1, C), bool), persistence=P)


def _bad_case():
    C, k = 300, 6
    lists, colpred = stream(C, k, 6, 5)
    lists = lists.copy()
    lists[1, 2], lists[3, 0], lists[4, 5] = C, -5, 2 ** 31 - 1
    return case("an id outside the range", C, k, 2, 3, bad_id, lists=lists, colpred=colpred, bank_rows=5, first_row=1)


def cases():
    same = np.tile(np.arange(5, 21), (12, 1))       # the same 16 columns every step, predicted every step
    pred = np.zeros((12, 64), bool)
    pred[:, 5:21] = True
    out = [
        case("one partial word", 37, 5, 1, 4, one_partial_word),
        case("two scan blocks", 257, 16, 3, 5, two_scan_blocks, seed=1),
        case("the select's later trips", 2 * TRIP + 37, 64, 2, 3, later_trips, seed=1),
        case("the bench shape", 65536, 1311, 1, 8, bench_shape),
        case("ceiling reached and held", 64, 16, 1, 12, ceiling_held, lists=same, colpred=pred, active_weight=3, predicted_weight=5, ceiling=7),
        case("decay >= ceiling: the plain link", 300, 20, 1, 6, plain_link, active_weight=4, predicted_weight=4, decay=16, ceiling=16, union_bits=20),
        case("active_weight 0", 300, 20, 2, 5, predicted_only, active_weight=0),
        case("predicted_weight 0", 300, 20, 2, 5, active_only, predicted_weight=0),
        case("union_bits 1", 300, 20, 1, 4, one_bit, union_bits=1),
        case("union_bits C", 300, 20, 1, 4, every_column, union_bits=300),
        case("a short row", 300, 20, 1, 4, short_row, union_bits=290, decay=3, ceiling=9),
        _tie_case("ties inside one word", 64, WORD, inside=True),
        _tie_case("ties across a word boundary", 96, WORD),
        _tie_case("ties across a thread's boundary", 1040, THREAD),
        _tie_case("ties across a trip's boundary", 2 * TRIP, TRIP),
        _tie_case("ties across a scan block boundary", 3 * SCAN_BLOCK, SCAN_BLOCK),
        case("a reset at window 0", 300, 20, 2, 4, reset_at(0), resets=[0], persistence=np.full(300, 9), prev=np.ones(300, bool)),
        case("a reset at a middle window", 300, 20, 2, 5, reset_at(3), resets=[3], bank_rows=7, first_row=5),
        case("first_row != 0 with bank_rows > n_rows", 1000, 20, 1, 5, rotated, bank_rows=7, first_row=4),
        case("three batches, two calls", 257, 16, 2, 9, three_batches_two_calls, batch_windows=2, calls=[5, 4]),
        _bad_case(),
    ]
    assert len({c.name for c in out}) == len(out)
    return out


# ---- the model-level property (the issue's stream): 4 sequences of 8 random patterns, each shown 30 times in shuffled order
PROPERTY = dict(input_dim=300, column_dim=1024, cell_dim=8, active_columns=64, seed=3, sequences=4, length=8, density=0.1, stream_seed=7, epochs=30,
                link=dict(active_weight=1, predicted_weight=8, decay=1, ceiling=16, union_bits=160))


def property_stream():
    """(patterns bool[sequences, length, input_dim], order int[epochs, sequences]) from RandomState(stream_seed)."""
    p = PROPERTY
    rng = np.random.RandomState(p["stream_seed"])
    patterns = rng.rand(p["sequences"], p["length"], p["input_dim"]) < p["density"]
    order = np.stack([rng.permutation(p["sequences"]) for _ in range(p["epochs"])])
    return patterns, order


def property_figures():
    """The four figures of the last epoch over steps 4..7 of each sequence, on one oracle and the definition:
    dict(pooled_share, plain_share, same, different, plain_same, plain_different, reappears)."""
    from oracle import HTMOracle
    import stack_fixture as sf
    p = PROPERTY
    patterns, order = property_stream()
    np.random.seed(p["seed"])
    ora = HTMOracle(p["input_dim"], p["column_dim"], p["cell_dim"], active_columns=p["active_columns"], seed=p["seed"])
    C = p["column_dim"]
    state = PoolingState(PoolingLink(**p["link"]).resolved(C, p["active_columns"]), C)
    rows = {}                                       # (epoch, sequence) -> (pooled rows, plain rows) of its 8 steps
    for e, perm in enumerate(order):
        for q in perm:
            state.reset()
            pooled, plain = [], []
            for t in range(p["length"]):
                if t == 0:
                    sp = ora.spatial_pooler.step(patterns[q, t], learning=True)
                    tm = ora.temporal_memory.step(sp.active_column, learning=True, prev_state=sf._empty(C, p["cell_dim"]))
                else:
                    sp, tm = ora.step(patterns[q, t], learning=True)
                state.step(sp.active_column, tm.cell_prediction.any(axis=1))
                pooled.append(state.row())
                x = np.zeros(C, bool)
                x[sp.active_column] = True
                plain.append(x)
            rows[(e, int(q))] = (np.array(pooled), np.array(plain))
    last = p["epochs"] - 1
    out = {}
    for which, name in ((0, "pooled"), (1, "plain")):
        shares, same, diff = [], [], []
        for q in range(p["sequences"]):
            r = rows[(last, q)][which]
            for t in range(4, 8):
                shares.append((r[t] & r[t - 1]).sum() / max(1, r[t].sum()))
                same += [(r[t] & r[u]).sum() for u in range(4, 8) if u != t]
                diff += [(r[t] & rows[(last, o)][which][u]).sum() for o in range(p["sequences"]) if o != q for u in range(4, 8)]
        out[f"{name}_share"], out[f"{name}_same"], out[f"{name}_different"] = float(np.mean(shares)), float(np.mean(same)), float(np.mean(diff))
    out["reappears"] = float(np.mean([(rows[(last, q)][0][7] & rows[(last - 1, q)][0][7]).sum() / max(1, rows[(last - 1, q)][0][7].sum())
                                      for q in range(p["sequences"])]))
    return out


# ---- chained oracles through the definition
def pooled_oracles(input_dim, levels, links, seed, permanences=None):
    """stack_fixture.OracleStack whose links are ints or PoolingLinks: the reference's loop with the definition between the levels."""
    import stack_fixture as sf

    class Pooled(sf.OracleStack):
        def __init__(self):
            super().__init__(input_dim, levels, [k.stride if isinstance(k, PoolingLink) else k for k in links], seed, permanences)
            self.pool = {l: PoolingState(k.resolved(levels[l][0], levels[l][2]), levels[l][0]) for l, k in enumerate(links) if isinstance(k, PoolingLink)}

        def reset(self):
            super().reset()
            for p in self.pool.values():
                p.reset()

        def process(self, x, learning=True):
            out = [None] * len(self.levels)
            for l, ora in enumerate(self.levels):
                if self.pending[l]:
                    sp = ora.spatial_pooler.step(x, learning=learning)
                    tm = ora.temporal_memory.step(sp.active_column, learning=learning,
                                                  prev_state=sf._empty(ora.temporal_memory.column_dim, ora.temporal_memory.cell_dim))
                    self.pending[l] = False
                else:
                    sp, tm = ora.step(x, learning=learning)
                out[l] = (sp, tm)
                if l + 1 == len(self.levels):
                    break
                pool = self.pool.get(l)
                if pool is not None:
                    pool.step(sp.active_column, tm.cell_prediction.any(axis=1))
                else:
                    self.window[l][sp.active_column] = True
                if (self.steps + 1) % self.period[l + 1]:
                    break
                x = self.window[l].copy() if pool is None else pool.row()
                self.window[l][:] = False
                if l == 0:
                    self.upper_inputs.append(x)
            self.steps += 1
            return out
    return Pooled()
