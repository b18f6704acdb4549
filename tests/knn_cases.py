"""The cases of the KNN classifier (bithtm_amd/knn.py, KNNClassifier, htm_knn_*): parameters, the calls of each
case -- patterns, labels, learning flag -- the NumPy / definition side, and the path each case reaches.  tests/test_knn_cpu.py checks
that every case reaches the path it names; tests/test_hip_knn.py holds the device to the definition on every one of them, bit for bit.

Shapes are the smallest that reach the paths: models of 256 x 8 with 8 active columns and input_dim 64 (patterns of 8 pairs) unless a
case says otherwise."""
import functools

import numpy as np

from bithtm_amd import _lib as L
from bithtm_amd.knn import KNNDefinition, live_bits

CHUNK, SLOTS, QUERIES, TABLE_BYTES, BINS = L.KNN_CHUNK, L.KNN_SLOTS, L.KNN_QUERIES, L.KNN_TABLE_BYTES, L.KNN_BINS
SHAPE = (256, 8, 8)                         # column_dim, cell_dim, max_pairs
GLOBAL_SHAPE = (TABLE_BYTES // 4 + 1, 4, 8)   # the smallest table past the LDS budget: 12 289 columns of 4 cells (one word each)
NO_BITMAP_SHAPE = (TABLE_BYTES * 8 + 1, 4, 8)  # the smallest table whose presence bitmap (a bit per word) is past the budget too: 393 217 columns
WIDE_SHAPE = (128, 32, 64)                  # overlaps up to 2 048: the select's bins are two overlaps wide (shift 1)
WPC2_SHAPE = (64, 40, 16)                   # two words per column, the high one with 8 live bits


def params(labels=6, k=3, min_overlap=1, capacity=64, shape=SHAPE):
    return dict(labels=labels, k=k, min_overlap=min_overlap, capacity=capacity, shape=shape)


def definition(p):
    return KNNDefinition(p["labels"], p["k"], p["min_overlap"], p["capacity"], *p["shape"])


def call(index, words, labels, learning=True, raw=False):
    """One call: index int32 [T, n], words uint32 [T, n], labels int [T]; raw: the pairs hold what update_patterns would refuse
    (dead bits), so the GPU test hands them to enqueue() itself."""
    return dict(index=np.asarray(index, np.int32), words=np.asarray(words, np.uint32), labels=np.asarray(labels, np.int64), learning=learning, raw=raw)


def clustered(shape, T, seed, centers=4, n_pairs=None, labels=6, labelled=1.0, columns=None, bits=3):
    """T patterns around `centers` random centre patterns: each keeps a random number of its centre's pairs (a bit of a kept word
    sometimes dropped) and draws the rest elsewhere -- overlaps with many ties at every level.  -> (index [T, n], words [T, n], labels
    [T]: the centre's number modulo `labels`, -1 with probability 1 - labelled).  columns: the columns patterns are drawn from."""
    C, K, P = shape
    wpc = (K + 31) // 32
    n = P if n_pairs is None else n_pairs
    cols_per = n // wpc
    rng = np.random.default_rng(seed)
    columns = np.arange(C) if columns is None else np.asarray(columns)
    top = [min(32, K - w * 32) for w in range(wpc)]

    def word(w):
        return int(np.bitwise_or.reduce(1 << rng.integers(0, top[w], bits))) if top[w] > 0 else 0
    cent_cols = [rng.choice(columns, cols_per, replace=False) for _ in range(centers)]
    cent_words = [[[word(w) for w in range(wpc)] for _ in range(cols_per)] for _ in range(centers)]
    index = np.full((T, n), -1, np.int32)
    words = np.zeros((T, n), np.uint32)
    labs = np.full(T, -1, np.int64)
    for t in range(T):
        c = int(rng.integers(centers))
        keep = rng.permutation(cols_per)[:int(rng.integers(0, cols_per + 1))]
        used = set(int(cent_cols[c][j]) for j in keep)
        others = [int(x) for x in rng.permutation(columns) if int(x) not in used][:cols_per - len(keep)]
        row = [(int(cent_cols[c][j]), [x & ~(1 << int(rng.integers(0, 32))) if rng.random() < 0.3 else x for x in cent_words[c][j]]) for j in keep]
        row += [(col, [word(w) for w in range(wpc)]) for col in others]
        order = rng.permutation(len(row))
        for slot, r in enumerate(order):
            col, ws = row[r]
            for w in range(wpc):
                index[t, slot * wpc + w] = col * wpc + w
                words[t, slot * wpc + w] = ws[w] & ((1 << top[w]) - 1)
        if rng.random() < labelled:
            labs[t] = c % labels
    return index, words, labs


def pattern(pairs, n=8):
    """A hand-written pattern: [(index, word), ...] padded to n pairs with (-1, 0)."""
    pairs = list(pairs) + [(-1, 0)] * (n - len(pairs))
    return [i for i, _ in pairs], [w for _, w in pairs]


def hand(rows, labels, learning=True, n=8, raw=False):
    idx, wds = zip(*[pattern(r, n) for r in rows])
    return call(idx, wds, labels, learning, raw)


def _q(cols, word=0b1):
    return [(c, word) for c in cols]


@functools.lru_cache(maxsize=None)
def case(name):
    """-> (params, [calls], refused: a call that must be refused behind them with the store unchanged, or None)."""
    none = [-1]
    if name == "empty":
        i, w, _ = clustered(SHAPE, 5, 1)
        return params(), [call(i, w, none * 5, False), call(i, w, none * 5, True)], None
    if name == "one-slot":
        i, w, g = clustered(SHAPE, 6, 2, centers=1)
        return params(), [call(i[:1], w[:1], [4]), call(i[1:], w[1:], none * 5, False)], None
    if name == "around-k":                          # k = 3: stores of 2, 3 and 4 slots, each asked the same questions
        i, w, g = clustered(SHAPE, 12, 3, centers=2)
        ask = call(i[4:], w[4:], none * 8, False)
        return params(k=3), [call(i[:2], w[:2], g[:2]), ask, call(i[2:3], w[2:3], g[2:3]), ask, call(i[3:4], w[3:4], g[3:4]), ask], None
    if name == "block-plus-one":                    # 257 slots: the second block of the distance launch holds one
        i, w, g = clustered(SHAPE, SLOTS + 1 + 24, 4, centers=3)
        n = SLOTS + 1
        return params(k=5, capacity=n), [call(i[:n], w[:n], g[:n]), call(i[n:], w[n:], none * 24, False)], None
    if name == "blocks":                            # 600 slots in three blocks; ties at the k-th overlap on both sides of slot 256 and 512
        i, w, g = clustered(SHAPE, 600 + 40, 5, centers=2)
        return params(k=7, capacity=600), [call(i[:600], w[:600], g[:600]), call(i[600:], w[600:], none * 40, False)], None
    if name == "vote-tie":                          # two neighbours, labels 3 and 1, one vote each: 1 wins; the nearest is labelled 3
        store = [_q([0, 1, 2, 3, 4]), _q([0, 1, 2, 3, 20]), _q([40, 41])]
        return params(k=2), [hand(store, [3, 1, 5]), hand([_q([0, 1, 2, 3, 4, 5])], none, False)], None
    if name == "nearest-loses":                     # the nearest neighbour is labelled 0, the two behind it 2: the label is 2
        store = [_q([0, 1, 2, 3, 4, 5]), _q([0, 1, 2, 3, 30]), _q([0, 1, 2, 31, 32])]
        return params(k=3), [hand(store, [0, 2, 2]), hand([_q([0, 1, 2, 3, 4, 5])], none, False)], None
    if name == "min-overlap":                       # min_overlap 4: met exactly by the first query, missed by one by the second
        store = [_q([0, 1, 2, 3, 4])]
        return params(k=1, min_overlap=4), [hand(store, [2]), hand([_q([0, 1, 2, 3, 60]), _q([0, 1, 2, 61, 62])], none * 2, False)], None
    if name == "gate":                              # one call: a step never matches itself, and matches its twin stored before it
        a, b = _q([0, 1, 2, 3], 0b11), _q([8, 9, 10], 0b101)
        return params(k=1), [hand([a, a, b, a, b], [1, 2, 3, -1, 4])], None
    if name == "split-stream":                      # the stream tests split at every position
        i, w, g = clustered(SHAPE, 9, 6, centers=2, labelled=0.7)
        return params(k=2, capacity=16), [call(i, w, g)], None
    if name == "wpc2":                              # cell_dim 40: the high word's bits 8.. are no cells; dead pairs; short patterns
        i, w, g = clustered(WPC2_SHAPE, 30, 7, centers=2, n_pairs=12)
        i[3, 2:4], i[9, :] = -1, -1                 # (a dead column; a pattern with no live pair at all)
        return params(k=3, shape=WPC2_SHAPE), [call(i[:20], w[:20], g[:20]), call(i[20:], w[20:], none * 10, False)], None
    if name == "wpc2-dead-bits":                    # a stored and a query pair whose high word has bits at and above cell_dim
        hi = 0xFFFFFF81                              # cells 32 and 39 (bits 0 and 7) and 24 bits that are no cells
        store = [[(1, hi), (0, 0b1)], [(1, 0x80), (2, 0xFFFFFFFF)]]
        ask = [[(1, hi), (0, 0b1)], [(1, 0xFF00)], [(127, 0xFF), (128, 0xFF), (-5, 0xFF)]]       # (the last column; past the table; negative)
        return params(k=2, shape=WPC2_SHAPE), [hand(store, [1, 2], n=4, raw=True), hand(ask, none * 3, False, n=4, raw=True)], None
    if name == "global-table":                      # 12 289 columns of one word: the tables lie in the global scratch table
        cols = np.concatenate([np.arange(0, 40), np.arange(GLOBAL_SHAPE[0] - 40, GLOBAL_SHAPE[0])])
        i, w, g = clustered(GLOBAL_SHAPE, SLOTS + 9 + CHUNK + 5, 8, centers=3, columns=cols)
        for t in (0, SLOTS + 12):                   # (the table's last word, stored and asked)
            if GLOBAL_SHAPE[0] - 1 not in i[t]:
                i[t, 0] = GLOBAL_SHAPE[0] - 1
        n = SLOTS + 9
        return params(k=4, capacity=n + 8, shape=GLOBAL_SHAPE), [call(i[:n], w[:n], g[:n]), call(i[n:], w[n:], g[n:], False),
                                                                 call(i[n:n + 8], w[n:n + 8], g[n:n + 8])], None
    if name == "global-no-bitmap":                  # 393 217 columns: the global-table form without the presence bitmaps
        C = NO_BITMAP_SHAPE[0]
        cols = np.concatenate([np.arange(0, 40), np.arange(C - 40, C)])
        i, w, g = clustered(NO_BITMAP_SHAPE, 30 + 11, 13, centers=3, columns=cols)
        for t in (0, 33):
            if C - 1 not in i[t]:
                i[t, 0] = C - 1
        return params(k=3, shape=NO_BITMAP_SHAPE), [call(i[:30], w[:30], g[:30]), call(i[30:], w[30:], none * 11, False)], None
    if name in ("global-twin", "lds-twin"):         # the same streams, all below column 256, in both forms
        i, w, g = clustered((256, 4, 8), 40, 9, centers=3, labelled=0.6)
        shape = GLOBAL_SHAPE if name == "global-twin" else (256, 4, 8)
        return params(k=3, shape=shape), [call(i[:25], w[:25], g[:25]), call(i[25:], w[25:], g[25:], False)], None
    if name == "ragged-chunk":                      # 64 + 3 queries: the last chunk's one group of staged queries holds three
        i, w, g = clustered(SHAPE, 20 + CHUNK + 3, 10, centers=3)
        return params(k=3), [call(i[:20], w[:20], g[:20]), call(i[20:], w[20:], none * (CHUNK + 3), False), call(i[20:33], w[20:33], none * 13, False)], None
    if name == "capacity":                          # filled exactly; one more is refused and changes nothing
        i, w, g = clustered(SHAPE, 12, 11, centers=2)
        ask = call(i[6:], w[6:], none * 6, False)
        return params(k=2, capacity=5), [call(i[:3], w[:3], g[:3]), call(i[3:5], w[3:5], g[3:5]), ask], call(i[5:7], w[5:7], [-1, 3])
    if name == "two-level-bins":                    # overlaps up to 2 048 in bins of two: neighbours told apart inside the k-th bin
        i, w, g = clustered(WIDE_SHAPE, 60, 12, centers=2, bits=24)
        return params(k=4, shape=WIDE_SHAPE), [call(i[:40], w[:40], g[:40]), call(i[40:], w[40:], none * 20, False)], None
    raise KeyError(name)


CASES = [
    ("empty", "an empty store: every row (-1, 0, 0, -1, -1), no distance launch"),
    ("one-slot", "a store of one slot"),
    ("around-k", "stores of k - 1, k and k + 1 slots: fewer candidates than k, exactly k, and a k-th overlap to find"),
    ("block-plus-one", "a store one slot larger than one block's share of the distance launch; a learning call of five chunks"),
    ("blocks", "a store over three blocks, ties at the k-th overlap on both sides of a block boundary: the lower slots win"),
    ("vote-tie", "a vote tie between labels: the lower label wins"),
    ("nearest-loses", "the nearest neighbour's label loses the vote"),
    ("min-overlap", "min_overlap met exactly and missed by one"),
    ("gate", "inside one call a step does not match itself and matches its twin stored before it"),
    ("split-stream", "a call split at every position equals the one call"),
    ("wpc2", "two words per column; pairs with index -1; a pattern with no live pair; fewer pairs than max_pairs"),
    ("wpc2-dead-bits", "a high word with bits at and above cell_dim, an index past the table and a negative one: they count nothing"),
    ("global-table", "the global-table form (presence bitmaps in LDS) at the smallest shape past the LDS budget, two blocks and two chunks"),
    ("global-no-bitmap", "the global-table form at the smallest shape whose presence bitmap does not fit LDS either"),
    ("global-twin", "the global-table form over streams that fit the small shape"),
    ("lds-twin", "... and the same streams in the LDS form"),
    ("ragged-chunk", "a last chunk of three queries: the group of staged queries is not full"),
    ("capacity", "capacity filled exactly; one more labelled step is refused and changes nothing"),
    ("two-level-bins", "overlaps that outnumber the bins: the k-th overlap is found inside its bin"),
]
CASE_IDS = [c[0] for c in CASES]


def run_definition(p, calls, d=None):
    """The calls through the definition -> ([(best, votes) per call], the definition)."""
    d = definition(p) if d is None else d
    return [d.update(c["index"], c["words"], c["labels"], c["learning"]) for c in calls], d


@functools.lru_cache(maxsize=None)
def expected(name):
    p, calls, refused = case(name)
    return run_definition(p, calls)


def overlaps(d, index, words):
    """int [count]: the overlap of one pattern with every slot of the definition's store."""
    q = d._dense(zip(index, words))
    return np.array([sum(bin(w & s.get(i, 0)).count("1") for i, w in q.items()) for s in d._live], dtype=np.int64)


def select_twin(ov, labels_of, stamps, k, min_overlap, n_labels, shift):
    """The device's select over one query's overlaps, step for step in NumPy: the histogram of the candidates' bins, the k-th
    overlap's bin from the top, the overlaps inside it (shift > 0), then the walk in slot order that takes everything above the k-th
    overlap and the lowest slots at it -> (row [5], votes [labels], v, the tied slots at v, the tied slots taken)."""
    ov = np.asarray(ov, np.int64)
    key = np.where(ov >= min_overlap, ov, 0)
    cand = key > 0
    v, ties = 0, 0
    if cand.sum() > k:
        hist = np.bincount(key[cand] >> shift, minlength=BINS)
        assert len(hist) == BINS
        cum = 0
        for b in range(BINS - 1, -1, -1):
            if cum + hist[b] >= k:
                break
            cum += hist[b]
        v, above = b, cum
        if shift:
            inside = np.bincount(key[cand & ((key >> shift) == b)] & ((1 << shift) - 1), minlength=1 << shift)
            for low in range((1 << shift) - 1, -1, -1):
                if above + inside[low] >= k:
                    break
                above += inside[low]
            v = (b << shift) | low
        ties = k - above
    tied = np.flatnonzero(cand & (key == v)) if ties else np.zeros(0, np.int64)
    taken = np.concatenate([np.flatnonzero(cand & (key > v)), tied[:ties]]).astype(np.int64)
    votes = np.bincount(np.asarray(labels_of, np.int64)[taken], minlength=n_labels) if len(taken) else np.zeros(n_labels, np.int64)
    if not len(taken):
        return [-1, 0, 0, -1, -1], votes, v, tied, tied[:ties]
    first = taken[np.lexsort((taken, -key[taken]))][0]
    best = int(np.argmax(votes))
    return [best, int(votes[best]), int(key[first]), int(first), int(np.int64(stamps[first] & 0xFFFFFFFF).astype(np.int32))], votes, v, tied, tied[:ties]


# ---- the model-level case: six input patterns, repeated with flip noise, through a 256 x 8 model; the first LABELLED_EPOCHS passes
# are labelled with the pattern's number and stored, the later ones are asked.  HIT_RATE: the share of the later steps whose label is
# their pattern's number, computed by the definition over the ORACLE's states on the CPU (model_stream below; tests/test_knn_cpu.py
# recomputes it) -- the GPU test holds the device's record to that same stream, bit for bit.
MODEL = dict(input_dim=64, column_dim=256, cell_dim=8, active_columns=8, seed=5)
MODEL_PATTERNS, MODEL_EPOCHS, LABELLED_EPOCHS, MODEL_NOISE, MODEL_K = 6, 12, 6, 0.03, 3
HIT_RATE = 35 / 36                          # (one later step of 36 takes a neighbouring pattern's label)


def model_permanence():
    return np.random.RandomState(MODEL["seed"]).randn(MODEL["column_dim"], MODEL["input_dim"]) * 0.1


@functools.lru_cache(maxsize=None)
def model_inputs():
    """-> (inputs bool [T, input_dim]: the patterns' passes with every bit flipped with probability MODEL_NOISE, labels int [T]: the
    pattern's number in the labelled passes, -1 later, names int [T]: the pattern's number)."""
    rng = np.random.RandomState(17)
    base = rng.rand(MODEL_PATTERNS, MODEL["input_dim"]) < 0.15
    T = MODEL_PATTERNS * MODEL_EPOCHS
    names = np.arange(T) % MODEL_PATTERNS
    inputs = base[names] ^ (rng.rand(T, MODEL["input_dim"]) < MODEL_NOISE)
    labels = np.where(np.arange(T) < MODEL_PATTERNS * LABELLED_EPOCHS, names, -1)
    return inputs, labels, names


def model_params():
    return params(labels=MODEL_PATTERNS, k=MODEL_K, capacity=MODEL_PATTERNS * LABELLED_EPOCHS,
                  shape=(MODEL["column_dim"], MODEL["cell_dim"], MODEL["active_columns"]))


@functools.lru_cache(maxsize=None)
def model_stream():
    """The oracle through the inputs and the definition over its states -> (best int32 [T, 5], votes int32 [T, labels], the
    definition); computed once per process and shared."""
    from classifier_cases import pairs_of
    from oracle import HTMOracle
    m = MODEL
    inputs, labels, names = model_inputs()
    ora = HTMOracle(m["input_dim"], m["column_dim"], m["cell_dim"], active_columns=m["active_columns"], seed=m["seed"], permanence=model_permanence())
    d = definition(model_params())
    best = np.zeros((len(inputs), 5), np.int32)
    votes = np.zeros((len(inputs), MODEL_PATTERNS), np.int32)
    for t in range(len(inputs)):
        sp = ora.spatial_pooler.step(inputs[t])
        tm = ora.temporal_memory.step(sp.active_column)
        index, words = pairs_of(tm.cell_activation, sp.active_column, m["cell_dim"])
        best[t], votes[t] = d.step(zip(index, words), labels[t])
    return best, votes, d


def hit_rate(knn_label):
    inputs, labels, names = model_inputs()
    later = labels < 0
    return float((np.asarray(knn_label)[later] == names[later]).mean())


def live(index, word, shape):
    return live_bits(index, word, shape[1], shape[0])
