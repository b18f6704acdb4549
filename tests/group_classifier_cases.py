"""Shared cases of the classifier-bank tests (tests/test_group_classifier_cpu.py, tests/test_hip_group_classifier.py, the launch-trace
driver): banks of n streams over the parameter sets and streams of tests/classifier_cases.py, each with the path it is there to reach.
tests/test_group_classifier_cpu.py asserts that every case reaches what it names.  Not collected by pytest.

The bank's kernels put the member on grid y beside the horizon (y = member * H + horizon; frozen: (member * n + step) * H + horizon)
and index everything a block touches by it: weights, ring, count, accumulator, ticket, delta, learn flag, targets, reset bits and
output rows.  A wrong index shows where neighbours differ: streams from different seeds, gates (learning, missing target, reset,
short history) that differ between members within ONE step, several blocks per (member, horizon) at the tickets."""
import functools
from types import SimpleNamespace

import numpy as np

from bithtm_amd.classifier import ClassifierBankDefinition, ClassifierDefinition
from classifier_cases import (CHUNK, EIGHT, MODEL_ALPHA, MODEL_SEQUENCE, MODEL_STEPS, MODELS, PAIRS, SPLITS, STREAMS,  # noqa: F401
                              definition, hit_rate, model_encoder, model_permanence, pairs_of, params, run_definition, stream)


def bank_stream(p, n, T, n_pairs, seed, **kw):
    """n streams of classifier_cases.stream from the seeds seed, seed + 101, ... -> (index int32 [n, T, P], words uint32 [n, T, P],
    targets int32 [n, T], resets bool [n, T])."""
    parts = [stream(p, T, n_pairs, seed + 101 * i, **kw) for i in range(n)]
    return tuple(np.stack([part[j] for part in parts]) for j in range(4))


def bank_definition(p, n, shared=False, table=None):
    return ClassifierBankDefinition(n, p["buckets"], p["steps"], alpha_q=p["alpha_q"], units=p["column_dim"] * p["cell_dim"], cell_dim=p["cell_dim"],
                                    weights="shared" if shared else "own", table=table)


def run_bank_definition(p, index, words, targets, resets=None, learning=True, splits=None, bank=None):
    """The bank definition over the streams, in one call or in the calls of `splits` -> (best [n, T, H, 2], dist [n, T, H, B], the bank)."""
    n, T = index.shape[:2]
    d = bank if bank is not None else bank_definition(p, n)
    best, dist, at = [], [], 0
    for k in (splits or [T]):
        if k:
            b, q = d.update(index[:, at:at + k], words[:, at:at + k], targets[:, at:at + k], None if resets is None else resets[:, at:at + k], learning)
        else:
            b, q = d.update(index[:, :0], words[:, :0], targets[:, :1], None if resets is None else resets[:, :1], learning)
        best.append(b)
        dist.append(q)
        at += k
    return np.concatenate(best, axis=1), np.concatenate(dist, axis=1), d


def run_singles(p, index, words, targets, resets=None, learning=True, weights=None):
    """n one-stream definitions, stream i fed (index[i], words[i], targets[i], resets[i]) -> (best, dist, the definitions)."""
    outs = [run_definition(p, index[i], words[i], targets[i], None if resets is None else resets[i], learning, None if weights is None else weights[i])
            for i in range(len(index))]
    return np.stack([o[0] for o in outs]), np.stack([o[1] for o in outs]), [o[2] for o in outs]


# ---- mixed gates: three streams, horizons (0, 2), max_pairs 40 -> three blocks per (member, horizon): neighbours' tickets and
# accumulators would collide under a wrong index.  Step MIXED_STEP holds, in ONE launch: member 0 learning at both horizons; member 1
# with a missing target AND reset at this step (its count goes to 1 whatever it was); member 2 reset one step before, so its history
# (count 1) is shorter than horizon 2 -- it learns at horizon 0 only.
MIXED = params(3, (0, 2), 6554, 10, 32, 40)
MIXED_STEP, MIXED_T = 6, 12


def mixed_stream():
    index, words, targets, resets = bank_stream(MIXED, 3, MIXED_T, 7, seed=21, resets=0.0, missing=0.1)
    s = MIXED_STEP
    resets[0, 1] = True
    targets[0, s] = 1
    targets[1, s], resets[1, s] = -1, True
    resets[2, s - 1] = True
    targets[2, s] = 2
    resets[:, s + 3] = (False, True, False)             # (later steps go on differing)
    return index, words, targets, resets


def gates(p, targets, resets, step):
    """Per member: (count before the step's pattern enters, after the step's own reset; per horizon, does the step learn)."""
    out = []
    for t_row, r_row in zip(targets, resets):
        count = 0
        for t in range(step):
            count = (0 if r_row[t] else count) + 1
        count = 0 if r_row[step] else count
        g = int(t_row[step])
        out.append((count, tuple(0 <= g < p["buckets"] and h <= count for h in p["steps"])))
    return out


# ---- the banked cases: (name, parameters, streams n, stream arguments, what the case is there to reach)
BANKS = [
    ("wide", params(1024, (1,), 6554, 8, 64, 16), 2, dict(T=4, n_pairs=16, seed=31, full_words=True, dead=0.05),
     "1 024 buckets: four bucket passes per wave; cell_dim 64: WPC = 2; one horizon: y = member"),
    ("narrow", params(1, (1,), 66, 6, 4, 1), 7, dict(T=6, n_pairs=1, seed=32, dead=0.0),
     "seven members of one bucket (B_pad 4: the members' rows of delta and accumulator are 4 and 8 words apart), cell_dim 4, one pair"),
    ("three-h015", params(64, (0, 1, 5), 6554, 12, 64, 17), 3, dict(T=14, n_pairs=17, seed=33, resets=0.2),
     "three members x three horizons, two blocks each, resets that differ between the members"),
]
BANK_IDS = [b[0] for b in BANKS]


def banked(name):
    _, p, n, args, _ = next(b for b in BANKS if b[0] == name)
    return p, n, bank_stream(p, n, **args)


# ---- frozen chunks: 16 members x 8 horizons = 128 rows per step, so a launch holds 65535 // 128 = 511 steps, not 512: T = 512
# crosses a chunk boundary, and the ring (65 deep) and the counts are carried over it per member.  One member: 1, CHUNK, CHUNK + 1.
FROZEN_BANK = params(3, EIGHT, 6554, 4, 32, 1)
FROZEN_N, FROZEN_T, FROZEN_LEARNED = 16, 512, 6
FROZEN_ONE_STEPS = [1, CHUNK, CHUNK + 1]


def chunk_steps(n, H):
    return min(CHUNK, 65535 // (n * H))


def frozen_stream(n, T, seed=41):
    """A learned stretch of FROZEN_LEARNED steps, then T frozen ones -> (learned stream, frozen stream)."""
    return (bank_stream(FROZEN_BANK, n, FROZEN_LEARNED, 1, seed, dead=0.0, missing=0.0),
            bank_stream(FROZEN_BANK, n, T, 1, seed + 7, dead=0.05, resets=0.01))


# ---- call splits of classifier_cases.SPLITS, over a bank of three streams of the named case
def split_bank(name):
    _, p, args, _ = next(s for s in STREAMS if s[0] == name)
    return p, bank_stream(p, 3, args["T"], args["n_pairs"], args["seed"] + 1000, **{k: v for k, v in args.items() if k not in ("T", "n_pairs", "seed")})


# ---- shared weights: four streams over one table of random weights
SHARED = params(8, (0, 2), 6554, 10, 32, 7)
SHARED_N, SHARED_T = 4, 9


def shared_case(seed=51):
    rng = np.random.default_rng(seed)
    w = rng.integers(-200000, 200000, (2, 10 * 32, 8)).astype(np.int32)
    return w, bank_stream(SHARED, SHARED_N, SHARED_T, 7, seed, resets=0.2)


# ---- the model level: groups of B members of one model (classifier_cases.MODELS), member i on MODEL_SEQUENCE rolled by i rows.
# GROUP_HIT_RATE: per member and horizon of MODEL_STEPS, the hit rate of the last pass of the definition over the ORACLE's states on the
# CPU (group_model_stream below; tests/test_group_classifier_cpu.py recomputes it); the GPU test holds the device's record to that same
# stream bit for bit.
# Members 2 and 5 have a NaN in row 7 (no bits, no target): that row is never a hit, 0.9 at best.  Every member of either model is held
# to the oracle (the streams are computed once per process and shared by the group sizes: seconds per member at 64 cells).
GROUP_SIZES = [1, 2, 7]
GROUP_EPOCHS = {"128x4": 30, "128x64": 8}
GROUP_HIT_RATE = {"128x4": [(1.0, 1.0), (1.0, 1.0), (0.9, 0.9), (1.0, 1.0), (1.0, 1.0), (0.9, 0.9), (1.0, 1.0)],
                  "128x64": [(1.0, 1.0), (1.0, 1.0), (0.9, 0.9), (1.0, 1.0), (1.0, 1.0), (0.9, 0.9), (1.0, 1.0)]}


def member_missing(i):
    return i in (2, 5)


def member_values(i, missing=False):
    """float64 [10, 1]: MODEL_SEQUENCE rolled by i rows; `missing`: row 7 NaN (it encodes no bit and has no target)."""
    v = np.roll(np.array(MODEL_SEQUENCE, dtype=np.float64), -i)[:, None].copy()
    if missing:
        v[7, 0] = np.nan
    return v


@functools.lru_cache(maxsize=None)
def group_model_stream(name, member, missing=False, reset_every=0):
    """The oracle through the model's passes of member `member`'s sequence and the definition over its states -> (best int32 [T, H, 2],
    dist, targets int32 [T]); `reset_every`: a sequence reset (of model and classifier history) before every step t > 0 with t %
    reset_every == 0.  Computed once per process and shared."""
    from oracle import HTMOracle
    m = MODELS[name]
    enc = model_encoder()
    values = member_values(member, missing)
    bank, buckets = enc.encode(values), enc.bucket(values)[:, 0]
    ora = HTMOracle(m["input_dim"], m["column_dim"], m["cell_dim"], active_columns=m["active_columns"], seed=m["seed"], permanence=model_permanence(m))
    d = ClassifierDefinition(enc.fields[0].buckets, MODEL_STEPS, MODEL_ALPHA, units=m["column_dim"] * m["cell_dim"], cell_dim=m["cell_dim"])
    T = GROUP_EPOCHS[name] * len(values)
    empty = SimpleNamespace(cell_prediction=np.zeros((m["column_dim"], m["cell_dim"]), bool), cell_activation=np.zeros((m["column_dim"], m["cell_dim"]), bool),
                            winner_cell=None, distal_state=None)
    best = np.zeros((T, len(MODEL_STEPS), 2), np.int32)
    dist = np.zeros((T, len(MODEL_STEPS), d.buckets), np.int32)
    for t in range(T):
        r = t % len(values)
        flag = bool(reset_every and t and t % reset_every == 0)
        sp = ora.spatial_pooler.step(bank[r])
        tm = ora.temporal_memory.step(sp.active_column, prev_state=empty if flag else None)
        index, words = pairs_of(tm.cell_activation, sp.active_column, m["cell_dim"])
        b, q = d.step(zip(index, words), buckets[r], flag, True, True)
        best[t], dist[t] = b, q
    return best, dist, np.tile(buckets, GROUP_EPOCHS[name]).astype(np.int32)
