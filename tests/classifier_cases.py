"""Shared cases of the SDR classifier tests (tests/test_classifier_cpu.py, tests/test_hip_classifier.py, the launch-trace driver): the
parameter sets, pattern streams and call splits, each with the path it is there to reach -- the smallest shapes at which that path
can still go wrong.  tests/test_classifier_cpu.py asserts that every case reaches what it names.  Not collected by pytest.

The device splits a pattern's pairs 16 to a block (CLASSIFIER_PAIRS) and 4 waves to a block, a wave taking every fourth pair of its
block: pair counts 3, 4, 5 lie on either side of the wave boundary, 15, 16, 17 of the block boundary, 33 and 40 make three blocks meet
at the atomics and the ticket.  A lane takes 4 buckets, a wave pass 256: buckets 1, 3 (lanes beyond B inside one 16-byte load), 64, 65
(B_pad = 68) and 1024 (four passes)."""
import functools
from types import SimpleNamespace

import numpy as np

from bithtm_amd.classifier import EXP_CUTOFF, W_LIMIT, ClassifierDefinition

PAIRS, CHUNK = 16, 512                      # (bithtm_amd._lib.CLASSIFIER_PAIRS, CLASSIFIER_CHUNK; the CPU test holds them to the header)
EIGHT = (0, 1, 2, 3, 5, 8, 13, 64)


def params(buckets, steps, alpha_q, column_dim, cell_dim, max_pairs):
    return dict(buckets=buckets, steps=tuple(steps), alpha_q=alpha_q, column_dim=column_dim, cell_dim=cell_dim, max_pairs=max_pairs)


def stream(p, T, n_pairs, seed, bits=(1, 3), dead=0.15, missing=0.15, resets=0.0, full_words=False):
    """T steps of n_pairs pairs over p's geometry: distinct word indices per step, `bits` = (lo, hi) set cells per word (full_words:
    every cell of some words), a share `dead` of the pairs contributing nothing (index -1 or word 0), a share `missing` of the
    targets -1, a share `resets` of the steps behind a reset -> (index int32 [T, n], words uint32 [T, n], targets int32 [T], resets
    bool [T])."""
    rng = np.random.default_rng(seed)
    K = p["cell_dim"]
    wpc = (K + 31) // 32
    n_words = p["column_dim"] * wpc
    assert n_pairs <= n_words
    index = np.zeros((T, n_pairs), np.int32)
    words = np.zeros((T, n_pairs), np.uint32)
    for t in range(T):
        index[t] = rng.choice(n_words, n_pairs, replace=False)
        for j in range(n_pairs):
            top = min(32, K - (int(index[t, j]) % wpc) * 32)
            if full_words and rng.random() < 0.5:
                words[t, j] = (1 << top) - 1
            else:
                n = int(rng.integers(bits[0], bits[1] + 1))
                words[t, j] = sum(1 << int(b) for b in rng.choice(top, min(n, top), replace=False))
            r = rng.random()
            if r < dead / 2:
                index[t, j] = -1
            elif r < dead:
                words[t, j] = 0
    targets = rng.integers(0, p["buckets"], T).astype(np.int32)
    targets[rng.random(T) < missing] = -1
    return index, words, targets, rng.random(T) < resets


def definition(p):
    return ClassifierDefinition(p["buckets"], p["steps"], alpha_q=p["alpha_q"], units=p["column_dim"] * p["cell_dim"], cell_dim=p["cell_dim"])


def run_definition(p, index, words, targets, resets=None, learning=True, weights=None, splits=None):
    """The definition over the stream, in one call or in the calls of `splits` -> (best, dist, the definition object)."""
    d = definition(p)
    if weights is not None:
        d.load_dense_weights(weights)
    best, dist = [], []
    at = 0
    for n in (splits or [len(index)]):
        b, q = d.update(index[at:at + n], words[at:at + n], targets[at:at + n] if n else targets[:1],
                        None if resets is None else resets[at:at + n], learning) if n else (np.zeros((0, len(p["steps"]), 2), np.int32),
                                                                                          np.zeros((0, len(p["steps"]), p["buckets"]), np.int32))
        best.append(b)
        dist.append(q)
        at += n
    return np.concatenate(best), np.concatenate(dist), d


# ---- the streamed cases: (name, parameters, stream arguments, what the case is there to reach)
STREAMS = [
    ("B1-h0-K5", params(1, (0,), 66, 12, 5, 1), dict(T=6, n_pairs=1, seed=1, dead=0.0),
     "one bucket (p = 65536, delta 0), horizon 0, cell_dim 5 (bits above the cells masked), one pair with few bits"),
    ("B3-h1-wave", params(3, (1,), 66, 10, 32, 5), dict(T=24, n_pairs=5, seed=2),
     "lanes beyond B inside one load; 5 pairs: a wave takes a second pair; alpha_q 66: deltas of both signs"),
    ("B3-pairs3", params(3, (1,), 655, 10, 32, 3), dict(T=12, n_pairs=3, seed=3), "3 pairs: a wave without a pair"),
    ("B3-pairs4", params(3, (0, 1), 655, 10, 32, 4), dict(T=12, n_pairs=4, seed=4), "4 pairs: every wave exactly one"),
    ("B64-K64-h015", params(64, (0, 1, 5), 6554, 12, 64, 17), dict(T=20, n_pairs=17, seed=5, resets=0.15),
     "WPC = 2, three horizons, 17 pairs: a second block with one pair, resets that empty the history before it is 5 deep"),
    ("B65-pad", params(65, (1,), 65536, 24, 5, 15), dict(T=12, n_pairs=15, seed=6), "B_pad = 68: a 17th lane with one live bucket; alpha_q = 65536; 15 pairs"),
    ("B64-pairs16", params(64, (1,), 6554, 24, 32, 16), dict(T=10, n_pairs=16, seed=7), "16 pairs: one full block"),
    ("B1024-blocks", params(1024, (1,), 6554, 40, 32, 33), dict(T=6, n_pairs=33, seed=8, full_words=True, dead=0.05),
     "four passes of a wave over the buckets, three blocks at the atomics and the ticket, words with all 32 bits set"),
    ("h8-to-64", params(3, EIGHT, 655, 10, 32, 5), dict(T=70, n_pairs=5, seed=9), "eight horizons ending at 64: the ring 65 deep, P_(t-64) learned from in the last six steps"),
    ("narrow-call", params(8, (1, 2), 6554, 40, 32, 40), dict(T=12, n_pairs=7, seed=10),
     "a call with fewer pairs than max_pairs: the ring's rows padded with (-1, 0), the padded blocks contribute nothing"),
    ("alpha1", params(3, (1,), 1, 10, 32, 4), dict(T=10, n_pairs=4, seed=11, missing=0.0), "alpha_q = 1: |x| < 65536 for both signs, every delta truncates to 0"),
]
STREAM_IDS = [s[0] for s in STREAMS]


def streamed(name):
    _, p, args, _ = next(s for s in STREAMS if s[0] == name)
    return p, stream(p, **args)


# ---- the empty pattern: every pair dead -> a uniform p = 65536 // B
EMPTY = params(3, (0, 1), 6554, 10, 32, 4)


def empty_stream(T=4):
    return np.full((T, 4), -1, np.int32), np.zeros((T, 4), np.uint32), np.array([0, 1, 2, -1][:T], np.int32), np.zeros(T, bool)


# ---- weights set by import
CLAMP = params(3, (0,), 65536, 4, 32, 1)


def clamp_case(sign):
    """Every bucket of unit 0 at sign * (2^30 - 10): equal activations, p = 21845, so with alpha_q = 65536 the target's delta is
    +43691 and the others' -21845 -- one step meets the clamp at the upper (sign +1) or lower (sign -1) end."""
    w = np.zeros((1, 4 * 32, 3), np.int32)
    w[0, 0] = sign * (W_LIMIT - 10)
    return w, np.array([[0]], np.int32), np.array([[1]], np.uint32), np.array([1], np.int32)


D_EDGES = [1023, 1024, EXP_CUTOFF - 1, EXP_CUTOFF]
EDGES = params(2, (1,), 66, 4, 32, 1)


def edge_case():
    """Unit 32 * i (word i, bit 0) holds [0, -D_EDGES[i]]: step i's activations differ by exactly that d."""
    w = np.zeros((1, 4 * 32, 2), np.int32)
    for i, d in enumerate(D_EDGES):
        w[0, 32 * i] = (0, -d)
    return w, np.arange(4, dtype=np.int32)[:, None], np.ones((4, 1), np.uint32), np.full(4, -1, np.int32)


# ---- call splits (of the case's T steps); "short" has calls shorter than the ring
SPLITS = [("B64-K64-h015", [1] * 20), ("B64-K64-h015", [3, 2, 15]), ("h8-to-64", [30, 1, 39]), ("B3-h1-wave", [0, 5, 19])]
SPLIT_IDS = ["single-steps", "shorter-than-the-ring", "across-the-long-ring", "an-empty-call"]

# ---- frozen calls: 1, CHUNK and CHUNK + 1 steps behind a learned stretch
FROZEN = params(3, (0, 2), 6554, 10, 32, 4)
FROZEN_STEPS = [1, CHUNK, CHUNK + 1]

# ---- the definition's behaviour: 12 random patterns of 40 units over 2 048 units, 16 buckets, horizons (0, 1, 5)
PERIODIC = params(16, (0, 1, 5), 6554, 64, 32, 40)
PERIODIC_ALPHAS = [66, 655, 6554, 65536]


def periodic_stream(epochs=20, seed=12):
    rng = np.random.default_rng(seed)
    index = np.stack([rng.choice(64, 40, replace=False) for _ in range(12)]).astype(np.int32)
    words = (np.uint32(1) << rng.integers(0, 32, (12, 40)).astype(np.uint32)).astype(np.uint32)
    targets = rng.permutation(16)[:12].astype(np.int32)
    reps = lambda a: np.concatenate([a] * epochs)
    return reps(index), reps(words), reps(targets)


# ---- the model-level cases: a repeating sequence over one scalar field through a small model.  HIT_RATE: the 1-step hit rate of
# the last epoch of the definition run over the ORACLE's states on the CPU (model_stream below; tests/test_classifier_cpu.py
# recomputes it) -- the GPU test holds the device's record to that same bit-identical stream, not to a threshold of its own.
MODEL_SEQUENCE = [5.0, 40.0, 75.0, 20.0, 90.0, 55.0, 10.0, 65.0, 30.0, 85.0]
MODELS = {"128x4": dict(input_dim=64, column_dim=128, cell_dim=4, active_columns=8, seed=3, epochs=30),
          "128x64": dict(input_dim=64, column_dim=128, cell_dim=64, active_columns=8, seed=4, epochs=8)}
MODEL_STEPS = (1, 3)
MODEL_ALPHA = 0.1
HIT_RATE = {"128x4": (1.0, 1.0), "128x64": (1.0, 1.0)}     # per horizon of MODEL_STEPS, over the last pass


def model_encoder():
    from bithtm_amd.encoders import ScalarEncoder, ScalarField
    return ScalarEncoder([ScalarField(0.0, 100.0, 64, 9)])


def model_values(resets=False, missing=False):
    """-> (values float64 [10, 1], resets bool [10] or None): the sequence's rows; `resets`: a reset before every pass; `missing`: one
    value NaN (its row encodes no bit and has no target)."""
    v = np.array(MODEL_SEQUENCE, dtype=np.float64)[:, None]
    if missing:
        v[7, 0] = np.nan
    r = np.zeros(len(v), bool)
    r[0] = True
    return v, (r if resets else None)


def pairs_of(activation, active_column, cell_dim):
    """bool [C, K] and the step's ascending active columns -> the pattern the device captures: (index int32 [k * WPC], words uint32)."""
    wpc = (cell_dim + 31) // 32
    padded = np.zeros((activation.shape[0], wpc * 32), np.uint8)
    padded[:, :cell_dim] = activation
    dense = np.packbits(padded, axis=1, bitorder="little").view(np.uint32).reshape(-1)
    index = (np.asarray(active_column, np.int64)[:, None] * wpc + np.arange(wpc)).reshape(-1)
    return index.astype(np.int32), dense[index]


def model_permanence(m):
    return np.random.RandomState(m["seed"]).randn(m["column_dim"], m["input_dim"]) * 0.1


@functools.lru_cache(maxsize=None)
def model_stream(name, resets=False, missing=False):
    """The oracle through the model's `epochs` passes of the sequence and the definition over its states -> (best int32 [T, H, 2], dist,
    targets int32 [T]); computed once per process and shared."""
    from oracle import HTMOracle
    m = MODELS[name]
    enc = model_encoder()
    values, flags = model_values(resets, missing)
    bank, buckets = enc.encode(values), enc.bucket(values)[:, 0]
    ora = HTMOracle(m["input_dim"], m["column_dim"], m["cell_dim"], active_columns=m["active_columns"], seed=m["seed"], permanence=model_permanence(m))
    d = ClassifierDefinition(enc.fields[0].buckets, MODEL_STEPS, MODEL_ALPHA, units=m["column_dim"] * m["cell_dim"], cell_dim=m["cell_dim"])
    T = m["epochs"] * len(values)
    empty = SimpleNamespace(cell_prediction=np.zeros((m["column_dim"], m["cell_dim"]), bool), cell_activation=np.zeros((m["column_dim"], m["cell_dim"]), bool),
                            winner_cell=None, distal_state=None)        # (the oracle's sequence reset: a step from the empty state)
    best = np.zeros((T, len(MODEL_STEPS), 2), np.int32)
    dist = np.zeros((T, len(MODEL_STEPS), d.buckets), np.int32)
    for t in range(T):
        r = t % len(values)
        sp = ora.spatial_pooler.step(bank[r])
        tm = ora.temporal_memory.step(sp.active_column, prev_state=empty if flags is not None and flags[r] else None)
        index, words = pairs_of(tm.cell_activation, sp.active_column, m["cell_dim"])
        b, q = d.step(zip(index, words), buckets[r], bool(flags is not None and flags[r]), True, True)
        best[t], dist[t] = b, q
    return best, dist, np.tile(buckets, m["epochs"]).astype(np.int32)


def hit_rate(best, targets, horizon_index, horizon, period):
    """The share of the last `period` steps whose prediction for `horizon` steps ahead is the bucket seen then (the sequence repeats
    with `period`, and the stream is whole passes of it: the bucket `horizon` rows on)."""
    T = len(targets)
    assert T % period == 0
    want = np.array([targets[(t + horizon) % period] for t in range(T - period, T)])
    return float((best[T - period:, horizon_index, 0] == want).mean())
