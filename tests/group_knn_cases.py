"""The cases of the KNN classifier banks (bithtm_amd/knn.py's KNNBankDefinition, KNNClassifierBank, htm_knns_*):
per case the parameters, the streams, the bank's calls -- patterns [S, T, n], labels [S, T], learning flag -- and the path it reaches.
tests/test_group_knn_cpu.py holds the bank definition to one KNNDefinition per stream on every case and checks the paths;
tests/test_hip_group_knn.py holds the device to the definition on every one of them, bit for bit.

Shapes come from knn_cases.py: 256 x 8 with 8 pairs unless a case says otherwise."""
import functools

import numpy as np

import knn_cases as one
from bithtm_amd import _lib as L
from bithtm_amd.knn import KNNBankDefinition, KNNDefinition
from knn_cases import CHUNK, GLOBAL_SHAPE, QUERIES, SHAPE, SLOTS, TABLE_BYTES, WPC2_SHAPE, clustered, pattern

SCRATCH_BYTES, GRID_Y = L.KNNS_SCRATCH_BYTES, 65535
TABLE_2048_SHAPE = (2048, 8, 8)             # a table of 2 048 words: six fit a block's 48 KiB


# ---- twins of the header's host arithmetic (csrc/htm_knn_bank.h)
def table_words(shape):
    return shape[0] * ((shape[1] + 31) // 32)


def scratch_bytes(n, chunk, capacity, words):
    return n * chunk * (capacity * 2 + (0 if words * 4 <= TABLE_BYTES else words * 4))


def chunk_of(n, capacity, words):
    """The largest power of two <= CHUNK whose scratch fits the budget with n x chunk in a grid's y; 0: none."""
    chunk = CHUNK
    while chunk >= 1:
        if scratch_bytes(n, chunk, capacity, words) <= SCRATCH_BYTES and n * chunk <= GRID_Y:
            return chunk
        chunk //= 2
    return 0


def queries_of(words):
    if words * 4 <= TABLE_BYTES:
        return min(QUERIES, TABLE_BYTES // (words * 4))
    bitmap = (words + 31) // 32
    return min(QUERIES, TABLE_BYTES // (bitmap * 4)) if bitmap * 4 <= TABLE_BYTES else QUERIES


def distance_grid(counts, nq, words, n=None):
    """(x, y) of the bank's distance launch: the slot blocks of the largest count, the members' query groups."""
    n = len(counts) if n is None else n
    return -(-max(counts) // SLOTS), n * -(-nq // queries_of(words))


def shared_distance_grid(count, n_streams, n_steps, words):
    """... and of a shared bank's first chunk: one flat batch of n_streams x n_steps queries against one store."""
    nq = min(CHUNK, n_streams * n_steps)
    return -(-count // SLOTS), -(-nq // queries_of(words))


def params(labels=6, k=3, min_overlap=1, capacity=64, shape=SHAPE):
    return one.params(labels, k, min_overlap, capacity, shape)


def bank_definition(p, streams):
    return KNNBankDefinition(streams, p["labels"], p["k"], p["min_overlap"], p["capacity"], *p["shape"])


def call(index, words, labels, learning=True):
    """One call of a bank: index, words [S, T, n], labels [S, T] (None: nothing labelled)."""
    index, words = np.asarray(index, np.int32), np.asarray(words, np.uint32)
    labels = np.full(index.shape[:2], -1, np.int64) if labels is None else np.asarray(labels, np.int64)
    return dict(index=index, words=words, labels=labels, learning=learning)


def _streams(shape, S, T, seed, **kw):
    parts = [clustered(shape, T, seed + 31 * s, **kw) for s in range(S)]
    return np.stack([p[0] for p in parts]), np.stack([p[1] for p in parts]), np.stack([p[2] for p in parts])


def _hand(rows_per_stream, n=8):
    idx, wds = [], []
    for rows in rows_per_stream:
        i, w = zip(*[pattern(r, n) for r in rows])
        idx.append(i)
        wds.append(w)
    return np.asarray(idx, np.int32), np.asarray(wds, np.uint32)


def _q(cols, word=0b1):
    return [(c, word) for c in cols]


@functools.lru_cache(maxsize=None)
def case(name):
    """-> dict(params, streams, calls, refused: a call that must be refused behind them with every store unchanged (or None),
    source: the one-stream calls (knn_cases.call) that fill the store a shared bank reads (or None))."""
    def made(p, S, calls, refused=None, source=None):
        return dict(params=p, streams=S, calls=calls, refused=refused, source=source)
    if name == "counts-0-1-257":                    # stores of 0, 1 and 257 slots: an empty stream beside one past a block
        n = SLOTS + 1
        i, w, g = _streams(SHAPE, 3, n + 24, 1, centers=3)
        g[0, :] = -1
        g[1, 1:] = -1
        g[1, 0] = 4
        return made(params(k=5, capacity=n), 3, [call(i[:, :n], w[:, :n], g[:, :n]), call(i[:, n:], w[:, n:], None, False)])
    if name == "mixed-store":                       # tick-shaped calls (T = 1) in which some streams store and others do not
        i, w, g = _streams(SHAPE, 4, 10, 2, centers=2, labelled=0.5)
        g[3, :] = -1                                # (a stream that never stores)
        return made(params(k=2, capacity=16), 4, [call(i[:, t:t + 1], w[:, t:t + 1], g[:, t:t + 1]) for t in range(10)])
    if name == "chunk-plus-3":                      # one learning call of chunk + 3 steps, then the same steps asked frozen
        T = CHUNK + 3
        i, w, g = _streams(SHAPE, 2, T, 3, centers=3, labelled=0.6)
        return made(params(k=3, capacity=T), 2, [call(i, w, g), call(i, w, None, False)])
    if name == "capacity":                          # stream 1 filled exactly; one more in stream 1 alone refuses the whole call
        i, w, g = _streams(SHAPE, 3, 9, 4, centers=2)
        g[0, 2:] = -1
        g[2, :] = -1
        g[1, 5:] = -1                               # (stream 1 stores five: its capacity)
        more = np.full((3, 2), -1)
        more[1, 1], more[0, 0] = 3, 2               # (stream 0 has room for its one; stream 1 has none)
        return made(params(k=2, capacity=5), 3, [call(i[:, :5], w[:, :5], g[:, :5]), call(i[:, 5:7], w[:, 5:7], None, False)],
                    refused=call(i[:, 7:], w[:, 7:], more))
    if name == "ties":                              # k = 2: a vote tie in stream 0, a tie at the k-th overlap in stream 1, neither in stream 2
        stores = [[_q([0, 1, 2, 3, 4]), _q([0, 1, 2, 3, 20]), _q([40, 41])],          # labels 3, 1: one vote each, 1 wins; the nearest is labelled 3
                  [_q([0, 1, 2, 3]), _q([0, 1, 2, 50]), _q([0, 1, 2, 51])],           # overlaps 4, 3, 3: slot 1 beats slot 2
                  [_q([0, 1, 2, 3, 4, 5]), _q([0, 1, 30]), _q([0, 31, 32])]]
        asks = [[_q([0, 1, 2, 3, 4, 5])], [_q([0, 1, 2, 3, 4])], [_q([0, 1, 2, 3, 4, 5])]]
        si, sw = _hand(stores)
        qi, qw = _hand(asks)
        return made(params(k=2), 3, [call(si, sw, [[3, 1, 5], [0, 4, 5], [2, 2, 0]]), call(qi, qw, None, False)])
    if name == "wpc2":                              # two words per column, pairs with index -1, fewer pairs than max_pairs
        i, w, g = _streams(WPC2_SHAPE, 2, 30, 5, centers=2, n_pairs=12)
        i[0, 3, 2:4], i[1, 9, :] = -1, -1
        return made(params(k=3, shape=WPC2_SHAPE), 2, [call(i[:, :20], w[:, :20], g[:, :20]), call(i[:, 20:], w[:, 20:], None, False)])
    if name == "global-table":                      # the global-table form with 2 streams at 12 289 x 4; stream 1 stores nothing at first
        cols = np.concatenate([np.arange(0, 40), np.arange(GLOBAL_SHAPE[0] - 40, GLOBAL_SHAPE[0])])
        i, w, g = _streams(GLOBAL_SHAPE, 2, 40, 6, centers=3, columns=cols)
        for s, t in ((0, 0), (1, 33)):              # (the table's last word, stored and asked)
            if GLOBAL_SHAPE[0] - 1 not in i[s, t]:
                i[s, t, 0] = GLOBAL_SHAPE[0] - 1
        first = g[:, :25].copy()
        first[1, :] = -1
        return made(params(k=4, capacity=40, shape=GLOBAL_SHAPE), 2, [call(i[:, :25], w[:, :25], first), call(i[:, 25:33], w[:, 25:33], g[:, 25:33]),
                                                                      call(i[:, 33:], w[:, 33:], None, False)])
    if name == "small-chunk":                       # 1 100 streams: n x chunk fits a grid's y only at chunk 32; a call of 32 + 3 steps
        S, T = 1100, 35
        pi, pw, pg = clustered(SHAPE, 300, 7, centers=5, labelled=0.08)
        pick = np.random.default_rng(7).integers(0, 300, (S, T))          # (every stream draws its steps from the same 300 patterns)
        i, w, g = pi[pick], pw[pick], pg[pick]
        return made(params(k=2, capacity=T), S, [call(i, w, g), call(i[:, :3], w[:, :3], None, False)])
    if name in ("shared-9", "shared-2048"):         # frozen streams over a one-stream store: a last query group of one; six queries per block
        shape, S = (SHAPE, 9) if name == "shared-9" else (TABLE_2048_SHAPE, 7)
        n = SLOTS + 5
        si, sw, sg = clustered(shape, n, 8, centers=3)
        i, w, _ = _streams(shape, S, 2, 9, centers=3)
        i1, w1, _ = _streams(shape, S, 1, 10, centers=3)
        return made(params(k=3, capacity=n + 4, shape=shape), S, [call(i1, w1, None, False), call(i, w, None, False)], source=[one.call(si, sw, sg)])
    raise KeyError(name)


CASES = [
    ("counts-0-1-257", "stores of 0, 1 and 257 slots in one bank: the distance grid is sized by the largest, blocks past a stream's count leave"),
    ("mixed-store", "tick-shaped calls (T = 1) in which some streams store and others do not"),
    ("chunk-plus-3", "a call of chunk + 3 steps: two launches of the distance and select kernels; the case the split tests cut at every position"),
    ("capacity", "one stream past capacity: the whole call is refused and every store is unchanged"),
    ("ties", "a vote tie and a tie at the k-th overlap in different streams of one launch"),
    ("wpc2", "two words per column"),
    ("global-table", "the global-table form with 2 streams at 12 289 x 4, one of them empty at first"),
    ("small-chunk", "a stream count at which the chunk shrinks below 64"),
    ("shared-9", "the shared form with 9 streams: a last query group of one"),
    ("shared-2048", "the shared form with a table of 2 048 words: six queries per block"),
]
CASE_IDS = [c[0] for c in CASES]


def source_definition(c):
    """The one-stream definition a shared case's streams read, after its source calls (None for a case with own stores)."""
    if c["source"] is None:
        return None
    p = c["params"]
    d = KNNDefinition(p["labels"], p["k"], p["min_overlap"], p["capacity"], *p["shape"])
    for s in c["source"]:
        d.update(s["index"], s["words"], s["labels"], s["learning"])
    return d


def run_definition(c, calls=None):
    """The calls through the bank definition -> ([(best, votes) per call], the bank definition)."""
    src = source_definition(c)
    d = bank_definition(c["params"], c["streams"]) if src is None else KNNBankDefinition.shared(src, c["streams"])
    return [d.update(x["index"], x["words"], x["labels"], x["learning"]) for x in (c["calls"] if calls is None else calls)], d


@functools.lru_cache(maxsize=None)
def expected(name):
    return run_definition(case(name))


def store_arrays(d):
    """The bank definition's stores as the device exports them: (count int64 [S], pairs, labels, stamps concatenated in stream order)."""
    P = (d.source or d.defs[0]).max_pairs
    parts = [x.store_arrays() for x in d.defs]
    count = np.array(d.count, dtype=np.int64)
    if not parts:
        return count, np.zeros((0, P, 2), np.int32), np.zeros(0, np.int32), np.zeros(0, np.int64)
    return count, np.concatenate([p[0] for p in parts]), np.concatenate([p[1] for p in parts]), np.concatenate([p[2] for p in parts])


# ---- the model-level case: a group of three 256 x 8 members of equal weights over knn_cases.model_inputs(), member i PHASE rows ahead
# of member i - 1.  HIT_RATES: each member's share of later steps whose label is their pattern's number, computed by the definition over
# the ORACLE's states on the CPU (group_stream below; tests/test_group_knn_cpu.py recomputes them).
MEMBERS, PHASE = 3, 2
HIT_RATES = (35 / 36, 1.0, 35 / 36)


def member_inputs(i):
    inputs, labels, names = one.model_inputs()
    return np.roll(inputs, -PHASE * i, axis=0), np.roll(labels, -PHASE * i), np.roll(names, -PHASE * i)


@functools.lru_cache(maxsize=None)
def group_stream():
    """Per member: the oracle through its inputs and a definition over its states -> (best int32 [B, T, 5], votes int32 [B, T, labels],
    the bank definition whose streams are the members' definitions)."""
    from classifier_cases import pairs_of
    from oracle import HTMOracle
    m = one.MODEL
    bank = bank_definition(one.model_params(), MEMBERS)
    T = len(one.model_inputs()[0])
    best = np.zeros((MEMBERS, T, 5), np.int32)
    votes = np.zeros((MEMBERS, T, one.MODEL_PATTERNS), np.int32)
    for i in range(MEMBERS):
        inputs, labels, _ = member_inputs(i)
        ora = HTMOracle(m["input_dim"], m["column_dim"], m["cell_dim"], active_columns=m["active_columns"], seed=m["seed"], permanence=one.model_permanence())
        d = bank.defs[i]
        for t in range(T):
            sp = ora.spatial_pooler.step(inputs[t])
            tm = ora.temporal_memory.step(sp.active_column)
            index, words = pairs_of(tm.cell_activation, sp.active_column, m["cell_dim"])
            best[i, t], votes[i, t] = d.step(zip(index, words), labels[t])
    bank.total = T
    return best, votes, bank


def hit_rate(i, knn_label):
    _, labels, names = member_inputs(i)
    later = labels < 0
    return float((np.asarray(knn_label)[later] == names[later]).mean())
