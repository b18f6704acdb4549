"""The KNN classifier's definition: plain sequential Python over integers.  The device object
(knn_classifier.KNNClassifier, htm_knn_*, csrc/htm_knn.h) equals it bit for bit.

NuPIC's KNNClassifier over active-cell patterns, with every quantity an integer: the patterns of labelled steps are stored, and a
later step is given the label most of its nearest stored patterns carry.

    pattern      as classifier.py has it: pairs (word index i, 32-bit word w) with distinct indices; only the live bits of w count
                 (live_bits: the cells of a column inside the table); a pair with i < 0 or w == 0 contributes nothing
    overlap      overlap(P, Q) = the sum of popcount(wP & wQ) over the indices present in both patterns
    store        slots 0 .. count - 1, each a pattern (padded to max_pairs pairs with (-1, 0)), a label and a stamp: the object's
                 running step total at the step that stored it.  Never overwritten; reset() empties it

One step with pattern P and label g (any g outside [0, labels) is no label), in this order:

    1. infer over the store as it is: the candidates are the slots with overlap(P, slot) >= min_overlap, the neighbours the first k
       of them by (overlap descending, slot ascending), votes[l] the neighbours labelled l; the result row is (label, votes,
       nearest_overlap, nearest_slot, nearest_step): the lowest label with the most votes and its votes, the first neighbour's
       overlap, slot and the low 32 bits of its stamp -- (-1, 0, 0, -1, -1) without a neighbour
    2. learn: with learning on and g a label, P goes into slot `count` with label g and stamp `total`; count += 1
    3. total += 1

A call whose labelled steps would take count past capacity is refused as a whole (ValueError), before any of its steps."""

import numpy as np

MAX_LABELS = 1024
MAX_K = 64
MAX_CAPACITY = 1 << 20
MAX_PAIRS = 2047                            # overlaps are kept in 16 bits: max_pairs * 32 <= 65 504
ROW = ("label", "votes", "nearest_overlap", "nearest_slot", "nearest_step")


def check_params(labels, k=1, min_overlap=1, capacity=4096):
    """-> (labels, k, min_overlap, capacity) as ints, or ValueError."""
    labels, k, min_overlap, capacity = int(labels), int(k), int(min_overlap), int(capacity)
    if not 1 <= labels <= MAX_LABELS:
        raise ValueError(f"labels must be in [1, {MAX_LABELS}], got {labels}")
    if not 1 <= k <= MAX_K:
        raise ValueError(f"k must be in [1, {MAX_K}], got {k}")
    if not 1 <= min_overlap <= 65535:
        raise ValueError(f"min_overlap must be in [1, 65535], got {min_overlap}")
    if not 1 <= capacity <= MAX_CAPACITY:
        raise ValueError(f"capacity must be in [1, 2^20] slots, got {capacity}")
    return labels, k, min_overlap, capacity


def live_bits(index, word, cell_dim, n_cols):
    """The bits of word `index` that are cells of a column below n_cols (cls_live_bits of csrc/htm_classifier.h)."""
    wpc = (cell_dim + 31) // 32
    index, word = int(index), int(word) & 0xFFFFFFFF
    if index < 0 or index // wpc >= n_cols:
        return 0
    top = cell_dim - (index % wpc) * 32
    return word if top >= 32 else word & ((1 << top) - 1)


def overlap(p, q):
    """Two patterns as {index: live word} -> the bits they share."""
    if len(q) < len(p):
        p, q = q, p
    return sum(bin(w & q.get(i, 0)).count("1") for i, w in p.items())


def is_label(g, labels):
    return 0 <= int(g) < labels


class KNNDefinition:
    """The sequential definition.  State: `slots` (the stored patterns as lists of (index, word) pairs, as they came), `labels_of`,
    `stamps`, `total`; count = len(slots)."""

    def __init__(self, labels, k=1, min_overlap=1, capacity=4096, column_dim=2048, cell_dim=32, max_pairs=40):
        self.labels, self.k, self.min_overlap, self.capacity = check_params(labels, k, min_overlap, capacity)
        self.column_dim, self.cell_dim, self.max_pairs = int(column_dim), int(cell_dim), int(max_pairs)
        self.slots, self._live, self.labels_of, self.stamps = [], [], [], []
        self.total = 0

    @property
    def count(self):
        return len(self.slots)

    def reset(self):
        self.slots, self._live, self.labels_of, self.stamps = [], [], [], []

    def _dense(self, pattern):
        out = {}
        for i, w in pattern:
            bits = live_bits(i, w, self.cell_dim, self.column_dim)
            if bits:
                out[int(i)] = bits
        return out

    def infer(self, pattern):
        """-> (the result row as a list of five ints, votes as a list of `labels` ints)."""
        p = self._dense(pattern)
        cands = []
        for s, q in enumerate(self._live):
            ov = overlap(p, q)
            if ov >= self.min_overlap:
                cands.append((-ov, s))
        cands.sort()
        near = cands[:self.k]
        votes = [0] * self.labels
        for _, s in near:
            votes[self.labels_of[s]] += 1
        if not near:
            return [-1, 0, 0, -1, -1], votes
        best = votes.index(max(votes))
        ov, s = -near[0][0], near[0][1]
        return [best, votes[best], ov, s, int(np.int64(self.stamps[s] & 0xFFFFFFFF).astype(np.int32))], votes

    def step(self, pattern, label=-1, learning=True):
        pattern = [(int(i), int(w) & 0xFFFFFFFF) for i, w in pattern]
        row, votes = self.infer(pattern)
        if learning and is_label(label, self.labels):
            if self.count >= self.capacity:
                raise ValueError(f"the store is full: capacity = {self.capacity} slots")
            self.slots.append(pattern)
            self._live.append(self._dense(pattern))
            self.labels_of.append(int(label))
            self.stamps.append(self.total)
        self.total += 1
        return row, votes

    def update(self, index, words, labels, learning=True, first_step=0):
        """Steps over arrays: index, words [T, n]; step i reads label (first_step + i) % len(labels) -> (best int32 [T, 5], votes
        int32 [T, labels]).  ValueError, with nothing done, for a call whose labelled steps do not fit the store."""
        T = len(index)
        mine = [int(labels[(first_step + t) % len(labels)]) for t in range(T)]
        stored = sum(is_label(g, self.labels) for g in mine) if learning else 0
        if self.count + stored > self.capacity:
            raise ValueError(f"the call would store {stored} patterns in a store of {self.count} of capacity = {self.capacity} slots")
        best = np.zeros((T, 5), dtype=np.int32)
        votes = np.zeros((T, self.labels), dtype=np.int32)
        for t in range(T):
            best[t], votes[t] = self.step(zip(index[t], words[t]), mine[t], learning)
        return best, votes

    def load_store(self, pairs, labels, stamps, total):
        """The inverse of store_arrays(): the store becomes these slots (pairs int [count, n, 2], labels [count], stamps [count]) and
        the step total `total` -- a state as the device object's load_state_dict takes it, without stepping through it."""
        if len(pairs) > self.capacity or not len(pairs) == len(labels) == len(stamps):
            raise ValueError(f"a store of at most capacity = {self.capacity} slots with a label and a stamp each, got {len(pairs)}, {len(labels)}, {len(stamps)}")
        self.slots = [[(int(i), int(w) & 0xFFFFFFFF) for i, w in p] for p in np.asarray(pairs).tolist()]
        self._live = [self._dense(p) for p in self.slots]
        self.labels_of, self.stamps, self.total = [int(g) for g in labels], [int(t) for t in stamps], int(total)

    def store_arrays(self):
        """The store as the device keeps it: (pairs int32 [count, max_pairs, 2] with unused pairs (-1, 0), labels int32 [count],
        stamps int64 [count])."""
        pairs = np.zeros((self.count, self.max_pairs, 2), dtype=np.int32)
        pairs[:, :, 0] = -1
        for s, pattern in enumerate(self.slots):
            for j, (i, w) in enumerate(pattern):
                pairs[s, j] = (i, np.uint32(w).view(np.int32))
        return pairs, np.asarray(self.labels_of, dtype=np.int32).reshape(-1), np.asarray(self.stamps, dtype=np.int64).reshape(-1)


class KNNBankDefinition:
    """`streams` independent KNNDefinitions with ONE step total: every update steps all of them by the same
    steps.  Stream i fed (patterns_i, labels_i) equals a KNNDefinition fed the same, row for row and store for store.  shared():
    frozen streams that infer over another definition's store."""

    def __init__(self, streams, labels, k=1, min_overlap=1, capacity=4096, column_dim=2048, cell_dim=32, max_pairs=40):
        self.streams = int(streams)
        if self.streams < 1:
            raise ValueError(f"streams must be at least 1, got {streams}")
        self.defs = [KNNDefinition(labels, k, min_overlap, capacity, column_dim, cell_dim, max_pairs) for _ in range(self.streams)]
        self.labels, self.capacity = self.defs[0].labels, self.defs[0].capacity
        self.source = None
        self.total = 0

    @classmethod
    def shared(cls, definition, streams):
        """`streams` frozen streams over `definition`'s store as it is at each call: every slot in [0, count) is seen, whatever its
        stamp.  They store nothing, learning is refused, and their own state is the step total."""
        d = definition
        bank = cls(streams, d.labels, d.k, d.min_overlap, d.capacity, d.column_dim, d.cell_dim, d.max_pairs)
        bank.defs, bank.source = [], d
        return bank

    @property
    def count(self):
        return [0] * self.streams if self.source is not None else [d.count for d in self.defs]

    def reset(self, streams=None):
        """Empty the stores `streams` (bool [streams]) names, or all of them; the total stays."""
        for i, d in enumerate(self.defs):
            if streams is None or streams[i]:
                d.reset()

    def update(self, index, words, labels=None, learning=True, first_step=0):
        """index, words [S, T, n], labels [S, R]: stream i's step t reads labels[i][(first_step + t) % R] -> (best int32 [S, T, 5],
        votes int32 [S, T, labels]).  ValueError, with every store unchanged, when ANY stream's labelled steps do not fit its store."""
        S, T = self.streams, len(index[0]) if len(index) else 0
        if len(index) != S or len(words) != S:
            raise ValueError(f"patterns of {S} streams, got {len(index)}")
        best = np.zeros((S, T, 5), dtype=np.int32)
        votes = np.zeros((S, T, self.labels), dtype=np.int32)
        if self.source is not None:
            if learning:
                raise ValueError("the streams read another definition's store: learning is refused")
            for i in range(S):
                for t in range(T):
                    best[i, t], votes[i, t] = self.source.infer([(int(a), int(w) & 0xFFFFFFFF) for a, w in zip(index[i][t], words[i][t])])
            self.total += T
            return best, votes
        if labels is None:                          # (nothing is labelled)
            labels = [[-1]] * S
        if len(labels) != S:
            raise ValueError(f"labels of {S} streams, got {len(labels)}")
        for i, d in enumerate(self.defs):
            mine = [int(labels[i][(first_step + t) % len(labels[i])]) for t in range(T)]
            stored = sum(is_label(g, self.labels) for g in mine) if learning else 0
            if d.count + stored > d.capacity:
                raise ValueError(f"stream {i}: the call would store {stored} patterns in a store of {d.count} of capacity = {d.capacity} slots")
        for i, d in enumerate(self.defs):
            d.total = self.total                    # (the one total: a stream's stamps are the bank's steps)
            best[i], votes[i] = d.update(index[i], words[i], labels[i], learning, first_step)
        self.total += T
        for d in self.defs:
            d.total = self.total
        return best, votes
