"""Cases of the anomaly likelihood (bithtm_amd/likelihood.py is the definition; tests/test_likelihood_cpu.py and
tests/test_hip_likelihood.py run them): parameter sets, count streams and splits of T steps into calls, each with the path of
the definition and of the kernel (csrc/htm_likelihood.h) it reaches.  CHUNK is the kernel's steps per launch, read from the
binding.

Parameter sets, (learning_period, estimation_samples, history, averaging_window, reestimation_period):
  P_small  probation (8 steps), a re-estimate every 7 steps and a wrap of both rings, all within 60 steps; history < CHUNK, so a
           window's first step moves through the chunk itself
  P_every  an estimate at every step, the widest averaging window (64), and a window that never stops growing (no ring wrap)
  P_wide   a re-estimate every 4096 steps over the longest history: windows that span the carried ring and the chunk, and a ring
           that wraps once T > 16384
Streams ([T] active, [T] bursting), by name:
  bursting     every column bursting: q = 65536, the largest S2 (N * S2 = 2^60 at N = 16384)
  idle         active = 0: q = 0 by definition, never a division
  constant     one value throughout: var = 0 and the variance floor; with q = 0 also the mean floor
  alternating  0 and all bursting in turn: the largest variance, averages that round down
  binomial     seeded binomial(40, 0.1) bursting counts with a burst of 10 fully bursting steps: the realistic one
"""
import numpy as np

from bithtm_amd._lib import LIKELIHOOD_CHUNK as CHUNK
from bithtm_amd.likelihood import PARAMETERS

P_SMALL = (5, 3, 16, 4, 7)
P_EVERY = (0, 1, 16384, 64, 1)
P_WIDE = (10, 5, 16384, 10, 4096)
PARAMS = {"P_small": P_SMALL, "P_every": P_EVERY, "P_wide": P_WIDE}
STREAMS = ("bursting", "idle", "constant", "alternating", "binomial")
SIZES = (1, 3, 130)


def as_kwargs(p):
    return dict(zip(PARAMETERS, p))


def stream(name, T, seed=0):
    """(active int64[T], bursting int64[T]) of the named stream."""
    t = np.arange(T)
    if name == "bursting":
        return np.full(T, 32 + seed % 16), np.full(T, 32 + seed % 16)
    if name == "idle":
        return np.zeros(T, np.int64), np.zeros(T, np.int64)
    if name == "constant":
        return np.full(T, 48), np.full(T, 3 if seed % 2 else 0)
    if name == "alternating":
        return np.full(T, 37), np.where((t + seed) % 2, 37, 0)
    if name == "binomial":
        seed %= 7                                   # (seven variants: the reference of a large group is computed once per variant)
        rng = np.random.default_rng(1000 + seed)
        active = np.full(T, 40)
        bursting = rng.binomial(40, 0.1, T)
        at = T // 2 + seed % 5
        bursting[at:at + 10] = 40
        return active, bursting
    raise KeyError(name)


def member_streams(B, T, seed=0):
    """(active, bursting) int64 [B, T]: member i gets stream STREAMS[i % 5] with a seed of its own: neighbours always differ, and only the idle
    streams (active = 0 is one stream) repeat."""
    pairs = [stream(STREAMS[i % len(STREAMS)], T, seed + i) for i in range(B)]
    return np.stack([a for a, _ in pairs]).astype(np.int64), np.stack([b for _, b in pairs]).astype(np.int64)


# (name, parameter set, splits): the calls T = sum(splits) steps are cut into.  P_small's probation ends at t + 1 = 8 and it
# re-estimates at t + 1 = 8, 15, 22, ...; P_wide's at t + 1 = 15, 4111, 8207, 12303, 16399, ...
SPLITS = [
    ("ticks", "P_small", [1] * 60),                                     # the tick path: n_steps = 1, 60 launches
    ("ragged", "P_small", [3, 1, 16, 17, 40]),                          # no point / probation inside / a wrap inside a call
    ("on-points", "P_small", [7, 7, 1, 7, 14, 6]),                      # calls that begin (t = 7, 14) and end (t + 1 = 15, 22, 36) exactly on a point
    ("chunk", "P_small", [CHUNK]),
    ("chunk+1", "P_small", [CHUNK + 1]),                                # a second launch of one step
    ("2chunk+3", "P_small", [2 * CHUNK + 3]),
    ("every-chunk+1", "P_every", [CHUNK + 1]),                          # a point at every step, windows from step 0
    ("every-ragged", "P_every", [1, 1, 62, 3, 64, 200]),                # the averaging window fills at t = 63
    ("wide", "P_wide", [16385, 20000]),                                 # more than `history` per call; the ring wraps; N = 16384
    ("wide-on-points", "P_wide", [14, 1, 4096, 4095, 1]),               # a call that is exactly the first point; points at a call's last / first step
]
SPLIT_IDS = [name for name, _, _ in SPLITS]


def reference(params, active, bursting, splits=None):
    """The definition over [B, T] counts -> (float64 [B, T], the list of B LikelihoodStream end states)."""
    from bithtm_amd.likelihood import define
    out, states = [], []
    for a, b in zip(np.asarray(active, dtype=np.int64), np.asarray(bursting, dtype=np.int64)):
        key = (tuple(params), None if splits is None else tuple(splits), a.tobytes(), b.tobytes())
        if key not in _REFERENCES:                  # (computed once per distinct stream, shared and never changed)
            _REFERENCES[key] = define(a, b, splits=splits, **as_kwargs(params))
        L, st = _REFERENCES[key]
        out.append(L)
        states.append(st)
    return np.stack(out), states


_REFERENCES = {}


def stacked_state(states):
    """The definition's end states in the shape of AnomalyLikelihood.state_dict() (without "params")."""
    parts = [s.state() for s in states]
    return {k: np.stack([p[k] for p in parts]) for k in ("t", "mean", "std", "has_estimate", "q_ring", "a_ring")}
