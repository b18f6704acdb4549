"""Anomaly likelihood: how improbable the recent short-term average of a stream's raw anomaly score is under the distribution of
that stream's own recent history (NuPIC's anomaly likelihood, in integers wherever a sum is taken).

This file is the definition -- one stream, sequential, plain Python and NumPy -- that the device (csrc/htm_likelihood.h,
htm_likelihood_*, include/bithtm_hip.h) is held to bit for bit, as encoders.py is for the scalar encoder.

With t the number of scores the stream has seen before this one (t continues across calls):

    q_t = (bursting << 16) // active  if active > 0 else 0            integer, 0 .. 65536: the raw score in units of 2^-16
    a_t = sum(q[max(0, t+1-w) .. t]) // min(t+1, w)                   integer; w = averaging_window
    if t+1 >= probation and (t+1-probation) % reestimation_period == 0:          probation = learning_period + estimation_samples
        lo = max(learning_period, t+1-history); h = a[lo .. t]
        N, S1, S2 = len(h), sum(h), sum(x*x for x in h)               exact integers; N*S2 and S1*S1 <= 2^60
        mean = max(float64(S1) / float64(N), 1966.08)                 0.03 in units of 2^-16
        var  = max(float64(N*S2 - S1*S1) / float64(N*N), 1288490.1888)           0.0003 in units of 2^-32
        std  = sqrt(var)
    if no estimate yet: L_t = 0.5
    else:
        z = (float64(a_t) - mean) / std
        x = min(abs(z), 8.0) * 64.0; i = min(int(x), 511); f = x - float64(i)
        tail = TAIL[i] + f * (TAIL[i+1] - TAIL[i])
        L_t = tail if z < 0 else 1.0 - tail

The estimate made at step t applies to t itself and to every later step until the next one.  Every float64 operation is a
single IEEE operation (/, sqrt, *, +, -) in a fixed order, and the Gaussian tail is the table TAIL, built once here and handed
to the device as data: TAIL[i] = 0.5 * erfc((i / 64) / sqrt 2), linear interpolation between its 513 entries (error against
the tail itself <= (1/64)^2 / 8 * phi(1) = 7.385e-6).
"""

import math

import numpy as np

TAIL_ENTRIES = 513
TAIL = np.array([0.5 * math.erfc((i / 64.0) / math.sqrt(2.0)) for i in range(TAIL_ENTRIES)], dtype=np.float64)

MEAN_FLOOR = 1966.08                # 0.03 in units of 2^-16
VARIANCE_FLOOR = 1288490.1888       # 0.0003 in units of 2^-32
MAX_HISTORY = 16384
MAX_AVERAGING_WINDOW = 64
MAX_COUNT = 1 << 24                 # update_counts: 0 <= bursting <= active < 2^24

PARAMETERS = ("learning_period", "estimation_samples", "history", "averaging_window", "reestimation_period")


def check_params(learning_period=288, estimation_samples=100, history=8640, averaging_window=10, reestimation_period=100):
    """The five parameters as a tuple of ints in PARAMETERS order; ValueError for one outside its range."""
    p = tuple(int(x) for x in (learning_period, estimation_samples, history, averaging_window, reestimation_period))
    lp, es, hist, w, r = p
    if not 0 <= lp < 2 ** 31:
        raise ValueError(f"learning_period must be >= 0, got {lp}")
    if not 1 <= es < 2 ** 31:
        raise ValueError(f"estimation_samples must be >= 1, got {es}")
    if not 1 <= hist <= MAX_HISTORY:
        raise ValueError(f"history must be in [1, {MAX_HISTORY}], got {hist}")
    if not 1 <= w <= MAX_AVERAGING_WINDOW:
        raise ValueError(f"averaging_window must be in [1, {MAX_AVERAGING_WINDOW}], got {w}")
    if not 1 <= r < 2 ** 31:
        raise ValueError(f"reestimation_period must be >= 1, got {r}")
    return p


def check_counts(active, bursting):
    """(active, bursting) as int64 arrays of one shape; ValueError unless 0 <= bursting <= active < 2^24 everywhere."""
    active, bursting = np.asarray(active), np.asarray(bursting)
    if active.dtype.kind not in "iu" or bursting.dtype.kind not in "iu":
        raise ValueError("active and bursting are integer counts")
    active, bursting = active.astype(np.int64), bursting.astype(np.int64)
    if active.shape != bursting.shape:
        raise ValueError(f"active {active.shape} and bursting {bursting.shape} differ in shape")
    if active.size and not ((0 <= bursting) & (bursting <= active) & (active < MAX_COUNT)).all():
        raise ValueError("counts must satisfy 0 <= bursting <= active < 2^24")
    return active, bursting


def q_of(active, bursting):
    """The raw score of one step in units of 2^-16, an integer in [0, 65536]."""
    active, bursting = int(active), int(bursting)
    return (bursting << 16) // active if active > 0 else 0


def estimate(n, s1, s2):
    """(mean, std) of a window from its exact integer count, sum and sum of squares."""
    mean = max(float(s1) / float(n), MEAN_FLOOR)
    var = max(float(n * s2 - s1 * s1) / float(n * n), VARIANCE_FLOOR)
    return mean, math.sqrt(var)


def likelihood_of(a, mean, std, table=TAIL):
    """L of the short-term average `a` under the estimate (mean, std)."""
    z = (float(a) - mean) / std
    x = min(abs(z), 8.0) * 64.0
    i = min(int(x), 511)
    f = x - float(i)
    tail = float(table[i]) + f * (float(table[i + 1]) - float(table[i]))
    return tail if z < 0 else 1.0 - tail


def log_likelihood(likelihood):
    """NuPIC's log scale of a likelihood: log(1.0000000001 - L) / log(1e-10) (a derived value, formed on the host only)."""
    return np.log(1.0000000001 - np.asarray(likelihood, dtype=np.float64)) / math.log(1e-10)


class LikelihoodStream:
    """The state of one stream and its sequential update.  The state is what the device keeps per stream: t, the ring of the
    last averaging_window values of q and the ring of the last `history` values of a (both indexed by absolute step modulo
    their length, zero where nothing was written since the last reset), the current (mean, std) and whether there is one."""

    def __init__(self, **params):
        self.params = check_params(**params)
        self.reset()

    def reset(self):
        _, _, hist, w, _ = self.params
        self.t = 0
        self.q_ring = [0] * w                   # (Python ints: the sums below are exact whatever their size)
        self.a_ring = [0] * hist
        self.mean, self.std, self.has_estimate = 0.0, 0.0, 0
        self.estimates = 0                      # (how many estimates were made: the tests name the paths their cases reach)

    def update(self, active, bursting):
        """The likelihoods of len(active) further steps, float64."""
        active, bursting = check_counts(active, bursting)
        lp, es, hist, w, r = self.params
        probation = lp + es
        out = np.empty(len(active), dtype=np.float64)
        q_ring, a_ring = self.q_ring, self.a_ring
        for j, (n_active, n_bursting) in enumerate(zip(active.tolist(), bursting.tolist())):
            t = self.t
            q_ring[t % w] = q_of(n_active, n_bursting)
            count = min(t + 1, w)
            a = sum(q_ring[(t - m) % w] for m in range(count)) // count
            a_ring[t % hist] = a
            if t + 1 >= probation and (t + 1 - probation) % r == 0:
                lo = max(lp, t + 1 - hist)
                h = [a_ring[s % hist] for s in range(lo, t + 1)]
                self.mean, self.std = estimate(len(h), sum(h), sum(x * x for x in h))
                self.has_estimate = 1
                self.estimates += 1
            out[j] = likelihood_of(a, self.mean, self.std) if self.has_estimate else 0.5
            self.t = t + 1
        return out

    def state(self):
        return dict(t=np.int64(self.t), mean=np.float64(self.mean), std=np.float64(self.std), has_estimate=np.int32(self.has_estimate),
                    q_ring=np.array(self.q_ring, dtype=np.int32), a_ring=np.array(self.a_ring, dtype=np.int32))


def define(active, bursting, splits=None, **params):
    """The definition over one stream's counts, optionally cut into calls of `splits` steps (which changes nothing) ->
    (likelihood float64 [T], the LikelihoodStream after the last step)."""
    stream = LikelihoodStream(**params)
    active, bursting = check_counts(active, bursting)
    if splits is None:
        return stream.update(active, bursting), stream
    assert sum(splits) == len(active), (sum(splits), len(active))
    parts, at = [], 0
    for n in splits:
        parts.append(stream.update(active[at:at + n], bursting[at:at + n]))
        at += n
    return (np.concatenate(parts) if parts else np.zeros(0)), stream
