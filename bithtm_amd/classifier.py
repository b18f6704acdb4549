"""The SDR classifier's definition: plain sequential Python over integers.  The device object
(sdr_classifier.SDRClassifier, htm_classifier_*, csrc/htm_classifier.h) equals it bit for bit.

A softmax regression from the units (cells) of the pattern of step t to the bucket seen at step t + h, learned online, one weight
table per horizon h -- NuPIC's SDRClassifier with every sum an integer:

    W[h][u][b]   int32 in units of 2^-16, 0 at first, clamped to [-2^30, 2^30]
    pattern      pairs (word index i, 32-bit word w); bit j of w is unit (i // WPC) * K + (i % WPC) * 32 + j, K = cell_dim,
                 WPC = ceil(K / 32); a pair with w == 0 or i < 0 contributes nothing; the indices of one pattern are distinct
    a[b]         the sum of W[h][u][b] over the pattern's units
    e[b]         2^30 * exp(-(max a - a[b]) / 65536) by linear interpolation in EXP_TABLE (exp_q30); 0 from 32.0 on
    p[b]         (e[b] << 16) // sum e, in units of 2^-16

One step t with target bucket g (any g outside [0, buckets) is missing), in NuPIC's order: a reset empties the history; the pattern
enters it; every horizon infers (the lowest bucket with the largest a, and its p) over P_t with the weights as they are; then,
if learning is on, g is there and the history holds P_(t-h), W[h] moves by delta[b] = trunc(alpha_q * ((b == g) * 65536 - p'[b]) /
65536) on every unit of P_(t-h), p' being the softmax over P_(t-h) with the not yet updated weights."""

import math

import numpy as np

MAX_BUCKETS = 1024
MAX_HORIZONS = 8
MAX_HORIZON = 64
W_LIMIT = 1 << 30
EXP_ENTRIES = 2049
EXP_CUTOFF = 32 << 16                       # d from which e is 0

# EXP_TABLE[i] = round(2^30 * exp(-i / 64)), i in 0..2048: handed to the device as data
EXP_TABLE = np.array([int(round((1 << 30) * math.exp(-i / 64.0))) for i in range(EXP_ENTRIES)], dtype=np.int32)
_T = [int(x) for x in EXP_TABLE]


def exp_q30(d):
    """2^30 * exp(-d / 65536) for an integer d >= 0, by linear interpolation in the table; 0 for d >= 32 << 16."""
    if d >= EXP_CUTOFF:
        return 0
    i, f = d >> 10, d & 1023
    return _T[i] - (((_T[i] - _T[i + 1]) * f) >> 10)


def softmax(a):
    """The activations (ints) -> p (ints in units of 2^-16)."""
    m = max(a)
    e = [exp_q30(m - x) for x in a]
    z = sum(e)
    return [(x << 16) // z for x in e]


def delta_of(alpha_q, p, g):
    """The weight step of every bucket for target g under the distribution p: alpha_q * (onehot - p) / 65536 truncated toward 0."""
    out = []
    for b, pb in enumerate(p):
        x = alpha_q * ((65536 if b == g else 0) - pb)
        out.append((abs(x) >> 16) * (1 if x > 0 else -1 if x < 0 else 0))
    return out


def check_params(buckets, steps=(1,), alpha=0.001):
    """-> (buckets, steps as an ascending tuple, alpha_q), or ValueError."""
    buckets = int(buckets)
    if not 1 <= buckets <= MAX_BUCKETS:
        raise ValueError(f"buckets must be in [1, {MAX_BUCKETS}], got {buckets}")
    steps = tuple(int(s) for s in (steps if hasattr(steps, "__iter__") else (steps,)))
    if not 1 <= len(steps) <= MAX_HORIZONS or any(not 0 <= s <= MAX_HORIZON for s in steps) or any(a >= b for a, b in zip(steps, steps[1:])):
        raise ValueError(f"steps: 1 to {MAX_HORIZONS} ascending horizons in [0, {MAX_HORIZON}], got {steps}")
    alpha_q = int(round(float(alpha) * 65536))
    if not 1 <= alpha_q <= 65536:
        raise ValueError(f"alpha must round to 1..65536 in units of 2^-16, got {alpha}")
    return buckets, steps, alpha_q


def units_of(pattern, cell_dim):
    """The units of a pattern (a sequence of (index, word) pairs), in the pairs' order."""
    wpc = (cell_dim + 31) // 32
    out = []
    for i, w in pattern:
        i, w = int(i), int(w) & 0xFFFFFFFF
        if i < 0:
            continue
        for j in range(32):
            if (w >> j) & 1:
                out.append((i // wpc) * cell_dim + (i % wpc) * 32 + j)
    return out


def check_patterns(index, words, units, cell_dim):
    """Patterns as arrays index int [T, n], words uint32 [T, n] -> (int32, uint32) arrays, or ValueError: the indices of a step
    that are not negative are distinct and below units / cell_dim * WPC, and no word has a bit at or above cell_dim."""
    index, raw = np.asarray(index), np.asarray(words)
    if index.ndim != 2 or raw.shape != index.shape or index.dtype.kind not in "iu" or raw.dtype.kind not in "iu":
        raise ValueError(f"patterns: index int [T, n] and words uint32 [T, n], got {index.shape} {index.dtype} and {raw.shape} {raw.dtype}")
    if raw.size and (raw.astype(np.int64).min() < 0 or raw.astype(np.int64).max() > 0xFFFFFFFF):
        raise ValueError("patterns: a word does not fit 32 bits")
    wpc = (cell_dim + 31) // 32
    n_words = units // cell_dim * wpc
    index64 = index.astype(np.int64)
    if index.size and index64.max() >= n_words:
        raise ValueError(f"patterns: a word index is at or above {n_words}")
    words32 = raw.astype(np.uint32)
    live = index64 >= 0
    top = cell_dim - (index64 % wpc) * 32                    # bits of the word that are cells
    bad = live & (top < 32) & ((words32.astype(np.int64) >> np.clip(top, 0, 32)) != 0)
    if bad.any():
        raise ValueError(f"patterns: a word has a bit at or above cell_dim = {cell_dim}")
    for t in range(index.shape[0]):
        row = index64[t][live[t]]
        if np.unique(row).size != row.size:
            raise ValueError(f"patterns: step {t} names a word index twice")
    return np.ascontiguousarray(index64.astype(np.int32)), np.ascontiguousarray(words32)


class ClassifierDefinition:
    """The sequential definition.  State: the weights (sparse: {horizon index: {unit: int list [buckets]}}), the ring of the last
    max(steps) + 1 patterns (indexed by total step count modulo its length), `count` patterns since the last clearing, `total`."""

    def __init__(self, buckets, steps=(1,), alpha=0.001, units=2048, cell_dim=32, alpha_q=None):
        self.buckets, self.steps, self.alpha_q = check_params(buckets, steps, alpha if alpha_q is None else alpha_q / 65536.0)
        self.units, self.cell_dim = int(units), int(cell_dim)
        self.ring_len = max(self.steps) + 1
        self.weights = [dict() for _ in self.steps]
        self.ring = [[] for _ in range(self.ring_len)]
        self.count = 0
        self.total = 0

    def reset(self):
        self.count = 0

    def _row(self, h, u):
        return self.weights[h].get(u) or [0] * self.buckets

    def activation(self, h, units):
        a = [0] * self.buckets
        for u in units:
            row = self.weights[h].get(u)
            if row:
                a = [x + y for x, y in zip(a, row)]
        return a

    def step(self, pattern, target=-1, reset=False, learning=True, distribution=False):
        """One step -> (best int [H][2] as (bucket, p) pairs, the distributions int [H][buckets] or None)."""
        if reset:
            self.count = 0
        pattern = [(int(i), int(w) & 0xFFFFFFFF) for i, w in pattern]
        self.ring[self.total % self.ring_len] = pattern
        units = units_of(pattern, self.cell_dim)
        best, dist = [], []
        for h in range(len(self.steps)):
            a = self.activation(h, units)
            p = softmax(a)
            b = a.index(max(a))
            best.append((b, p[b]))
            dist.append(p)
        g = int(target)
        if learning and 0 <= g < self.buckets:
            for h, k in enumerate(self.steps):
                if k > self.count:                              # the history holds P_t .. P_(t - count)
                    continue
                past = units_of(self.ring[(self.total - k) % self.ring_len], self.cell_dim)
                delta = delta_of(self.alpha_q, softmax(self.activation(h, past)), g)
                for u in past:
                    row = self._row(h, u)
                    self.weights[h][u] = [max(-W_LIMIT, min(W_LIMIT, x + d)) for x, d in zip(row, delta)]
        self.count += 1
        self.total += 1
        return best, (dist if distribution else None)

    def update(self, index, words, targets, resets=None, learning=True, first_step=0):
        """Steps over arrays: index, words [T, n]; step i reads target and reset (first_step + i) % len(targets) ->
        (best int32 [T, H, 2], dist int32 [T, H, buckets])."""
        T = len(index)
        best = np.zeros((T, len(self.steps), 2), dtype=np.int32)
        dist = np.zeros((T, len(self.steps), self.buckets), dtype=np.int32)
        for t in range(T):
            r = (first_step + t) % len(targets)
            b, d = self.step(zip(index[t], words[t]), targets[r], bool(resets[r]) if resets is not None else False, learning, True)
            best[t], dist[t] = b, d
        return best, dist

    def dense_weights(self):
        """int32 [H, units, buckets]."""
        out = np.zeros((len(self.steps), self.units, self.buckets), dtype=np.int32)
        for h, table in enumerate(self.weights):
            for u, row in table.items():
                out[h, u] = row
        return out

    def load_dense_weights(self, w):
        w = np.asarray(w)
        assert w.shape == (len(self.steps), self.units, self.buckets)
        self.weights = [{int(u): [int(x) for x in w[h, u]] for u in np.flatnonzero(w[h].any(axis=1))} for h in range(len(self.steps))]

    def ring_arrays(self, max_pairs):
        """The ring as the device keeps it: int32 [ring_len, max_pairs, 2], unused pairs (-1, 0)."""
        out = np.zeros((self.ring_len, max_pairs, 2), dtype=np.int32)
        out[:, :, 0] = -1
        for s, pattern in enumerate(self.ring):
            for j, (i, w) in enumerate(pattern):
                out[s, j] = (i, np.uint32(w).view(np.int32))
        return out


class ClassifierBankDefinition:
    """A bank of n streams: n independent ClassifierDefinition objects of one config -- stream i fed
    (patterns_i, targets_i, resets_i) equals a one-stream object fed the same -- with one `total` for the object, since every call
    advances all streams by the same number of steps, and per stream its count, its ring and its weights.  weights="shared": every
    stream reads one weight table (`table`, a ClassifierDefinition whose weights are read where they lie, or a table of the bank's
    own); learning is refused; inference, rings and counts work as in an own-weights bank.  No arithmetic of its own."""

    def __init__(self, streams, buckets, steps=(1,), alpha=0.001, units=2048, cell_dim=32, alpha_q=None, weights="own", table=None):
        self.n = int(streams)
        if self.n < 1:
            raise ValueError(f"streams must be at least 1, got {streams}")
        if weights not in ("own", "shared"):
            raise ValueError(f"weights: 'own' or 'shared', got {weights!r}")
        self.shared = weights == "shared"
        self.members = [ClassifierDefinition(buckets, steps, alpha, units, cell_dim, alpha_q) for _ in range(self.n)]
        if self.shared:
            self.table = table if table is not None else ClassifierDefinition(buckets, steps, alpha, units, cell_dim, alpha_q)
            first = self.members[0]
            if (self.table.buckets, self.table.steps, self.table.units, self.table.cell_dim) != (first.buckets, first.steps, first.units, first.cell_dim):
                raise ValueError("the shared table was made with another config")
        elif table is not None:
            raise ValueError("table= goes with weights='shared'")
        self.total = 0

    def _attach(self):
        if self.shared:                                         # (read where it lies: the owner may have replaced its tables)
            for m in self.members:
                m.weights = self.table.weights

    def reset(self, streams=None):
        for i, m in enumerate(self.members):
            if streams is None or streams[i]:
                m.reset()

    def update(self, index, words, targets, resets=None, learning=True, first_step=0):
        """index, words [n, T, P]; targets [n, R]; resets [n, R] or None; step i reads target and reset (first_step + i) % R ->
        (best int32 [n, T, H, 2], dist int32 [n, T, H, buckets])."""
        if learning and self.shared:
            raise ValueError("the streams read one weight table: learning is refused")
        if len(index) != self.n or len(words) != self.n or len(targets) != self.n or (resets is not None and len(resets) != self.n):
            raise ValueError(f"the bank has {self.n} streams")
        self._attach()
        best, dist = [], []
        for i, m in enumerate(self.members):
            assert m.total == self.total
            b, d = m.update(index[i], words[i], targets[i], None if resets is None else resets[i], learning, first_step)
            best.append(b)
            dist.append(d)
        self.total += len(index[0])
        return np.stack(best), np.stack(dist)

    @property
    def counts(self):
        return [m.count for m in self.members]

    def dense_weights(self):
        """int32 [n, H, units, buckets] (shared: the one table, n times)."""
        self._attach()
        return np.stack([m.dense_weights() for m in self.members])

    def ring_arrays(self, max_pairs):
        """int32 [n, ring_len, max_pairs, 2]."""
        return np.stack([m.ring_arrays(max_pairs) for m in self.members])
