"""Cases of the live-tick tests (ModelGroup.tick / ModelGroup.reset; htm_live_tick, htm_live_reset) and the NumPy side of the
definition a tick is held to: ScalarEncoder.encode for the rows a tick steps on, ScalarEncoder.decode for the prediction it
returns, RunRecord's formulas for the derived counts.  Shared by tests/test_live_tick_cpu.py and tests/test_hip_live_tick.py.

Shapes (input_dim, column_dim, cell_dim, active_columns) -- the smallest at which each path can go wrong:
  (70, 128, 4, 8)       one 16-byte store per bank row, one cell word per column
  (300, 512, 48, 48)    two cell words per column, W = 12 words per row
  (1000, 2048, 32, None)  the reference shape, once, with B = 5
"""
import numpy as np

SMALL = (70, 128, 4, 8)
MID = (300, 512, 48, 48)
REFERENCE = (1000, 2048, 32, None)

EAGER = [{"BITHTM_EAGER_BELOW": "0"}, {"BITHTM_EAGER_BELOW": "64"}]
EAGER_IDS = ["graphs", "eager-below-64"]


def encoder_for(size, layout="default"):
    """The encoder layouts of the cases.
    input_dim 300: a periodic field of 260 bits, width 21, at offset 0 (longer than one 256-thread pass of the decode's prefix
                   sum; its windows wrap), a field of 37 bits, width 5, behind it (offset 260: it starts inside a 32-bit word and
                   crosses the next word boundary), three pad bits.
    input_dim 70:  one field of 70 bits.
    "sixteen":     sixteen fields one bit wide (the field cap), the rest of the row pad bits.
    input_dim 1000: two fields of 500 bits."""
    import bithtm_amd as B
    I = size[0]
    if layout == "sixteen":
        return B.ScalarEncoder([B.ScalarField(0.0, 4.0, 4, 1) for _ in range(16)], input_dim=I)
    if I == 300:
        return B.ScalarEncoder([B.ScalarField(0.0, 24.0, 260, 21, periodic=True), B.ScalarField(-1.0, 1.0, 37, 5)], input_dim=I)
    if I == 70:
        return B.ScalarEncoder([B.ScalarField(0.0, 10.0, 70, 9)], input_dim=I)
    if I == 1000:
        return B.ScalarEncoder([B.ScalarField(0.0, 100.0, 500, 21), B.ScalarField(0.0, 7.0, 500, 25, periodic=True)], input_dim=I)
    raise ValueError(size)


def field_ranges(enc):
    return [(f.minimum, f.maximum) for f in enc.fields]


def periodic_values(enc, B, rows, seed, period=10):
    """float64 [B, rows, F]: per member a sequence of `period` values per field, repeated -- something to learn -- each member's
    its own."""
    rng = np.random.RandomState(seed)
    base = np.empty((B, period, len(enc)))
    for j, (lo, hi) in enumerate(field_ranges(enc)):
        base[:, :, j] = lo + (hi - lo) * rng.rand(B, period)
    return base[:, np.arange(rows) % period]


def edge_values(enc):
    """float64 [n, F]: the values a tick must encode as the definition does -- NaN (missing), +-inf, minimum and maximum exactly,
    values far outside the range, and ordinary ones."""
    cols = []
    for lo, hi in field_ranges(enc):
        cols.append([np.nan, np.inf, -np.inf, lo, hi, lo - 1e12, hi + 1e300, -1e300, lo + 0.37 * (hi - lo), np.nextafter(hi, lo)])
    return np.array(cols, dtype=np.float64).T


def with_edges(values, enc, every=7):
    """`values` [B, rows, F] with edge values put in every `every`-th row (another one per member and occurrence): in one field,
    the others keeping what the sequence has there -- a row that is partly what the model expects -- and every third time in all
    fields at once."""
    out = values.copy()
    edges = edge_values(enc)
    F = values.shape[2]
    n = 0
    for r in range(3, values.shape[1], every):
        for i in range(values.shape[0]):
            if n % 3 == 2:
                out[i, r] = edges[n % len(edges)]
            else:
                out[i, r, n % F] = edges[n % len(edges), n % F]
            n += 1
    return out


def stream_values(enc, B, train, live, seed, period=10, jitter=0.01):
    """float64 [B, train + live, F]: `train` rows of each member's clean periodic sequence -- something it learns to predict --
    then `live` rows of the same sequence going on with a jitter of `jitter` times each field's range (rows that are mostly
    what the model expects) and the edge values of with_edges among them."""
    v = periodic_values(enc, B, train + live, seed, period)
    rng = np.random.RandomState(seed + 1)
    tail = v[:, train:].copy()
    for j, (lo, hi) in enumerate(field_ranges(enc)):
        tail[:, :, j] += jitter * (hi - lo) * rng.randn(B, live)
    v[:, train:] = with_edges(tail, enc)
    return v


# ---- the NumPy side of the definition
def encoded_rows(enc, values):
    """bool [..., input_dim]: the rows a tick steps on."""
    return enc.encode(values)


def decoded(enc, votes):
    """(bucket, score, value) of vote rows int [..., input_dim]: what a tick returns as predicted_bucket / _score / _value."""
    bucket, score = enc.decode(votes)
    return bucket, score, enc.value_of(bucket)


def derived(active, bursting, before):
    """(correct_columns, incorrect_columns, anomaly_score) by RunRecord's formulas."""
    active, bursting, before = (np.asarray(x) for x in (active, bursting, before))
    correct = active - bursting
    a = active.astype(np.float64)
    return correct, before - correct, np.where(a > 0, 1.0 - correct / np.maximum(a, 1.0), 0.0)
