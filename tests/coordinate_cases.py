"""Cases of the coordinate fields (bithtm_amd/encoders.py CoordinateField is the definition), shared by
tests/test_coordinate_cpu.py (every case reaches the path it names) and tests/test_hip_coordinate.py (the device gives the
definition's words).  A case is (input_dim, fields, rows): `fields` builds the encoder's fields, `rows` the float64 [n, columns]
values.  The select block of kcoord_bank has THREADS = 256 threads whatever the row's width; a candidate count N = (2r + 1)**2 at
or below the field's width takes no select at all."""
import numpy as np

THREADS = 256                                       # SCALAR_THREADS: kcoord_bank's block, and the bins of one histogram pass
TWO30 = 2.0 ** 30

# Ties exactly at the cut (seed 1, width 21, centres (13 t, -7 t)): 20 candidates above the cut and two AT it -- the lower index wins.
# (cx, cy, r, the tied candidate indices, their order)
TIES = ((140153, -75467, 8, (10, 54), 15934562),
        (565279, -304381, 8, (259, 269), 15373344),
        (26442, -14238, 20, (130, 722), 16494368),
        (63739, -34321, 20, (490, 1671), 16512015))
TIE_SEED, TIE_WIDTH = 1, 21

# the inputs of the overlap table of DESIGN.md section 28: seed 3, width 21, bits 400, 200 centres
OVERLAP = dict(seed=3, width=21, bits=400, centres=np.stack([1000 + 37 * np.arange(200), -500 + 11 * np.arange(200)], axis=-1))


def _coord(*args, **kw):
    from bithtm_amd import CoordinateField
    return CoordinateField(*args, **kw)


def _linear(*args, **kw):
    from bithtm_amd import ScalarField
    return ScalarField(*args, **kw)


def _rows(*rows):
    return np.array(rows, dtype=np.float64)


def _radii(radii, at=((0, 0), (-3, 7), (1000, -500), (-70001, -90001), (123456789, -987654321))):
    """One row per radius, the centres taken in turn: at 0, negative, mixed, far out."""
    return _rows(*[(at[i % len(at)][0], at[i % len(at)][1], r) for i, r in enumerate(radii)])


def _linear13():
    from bithtm_amd import ScalarField
    return [ScalarField(0.0, 10.0, 20 + j, 3 + j % 4, periodic=j % 3 == 0) for j in range(13)]


def _mixed():
    from bithtm_amd import CategoryField, HashedField, ScalarField
    return [ScalarField(0.0, 100.0, 61, 9), HashedField(0.0, 24.0, 97, 11, buckets=300, seed=5), CategoryField(4, 7, 30),
            _coord(333, 21, 9, resolution=(0.5, 2.0), origin=(10.0, -3.0), seed=6), ScalarField(-1.0, 1.0, 40, 5, periodic=True)]


def _mixed_rows():
    rng = np.random.RandomState(11)
    n = 24
    v = np.stack([rng.uniform(-5, 105, n), rng.uniform(0, 24, n), rng.randint(-1, 5, n).astype(np.float64), rng.uniform(-40, 40, n), rng.uniform(-40, 40, n),
                  rng.randint(0, 12, n).astype(np.float64), rng.uniform(-1, 1, n)], axis=-1)
    v[3, 0] = v[5, 1] = v[7, 3] = v[9, 4] = v[11, 5] = v[13, 6] = np.nan
    v[15] = np.nan
    return v


def _edge_rows():
    """x and y at 0, -0.0, below 0, and at both ends of +-2**30 with the first value outside; radii 0 to 3."""
    ends = (0.0, -0.0, -0.5, -1.0, -TWO30, -TWO30 - 1.0, np.nextafter(-TWO30, -np.inf), TWO30 - 1.0, TWO30 - 0.5, np.nextafter(TWO30, 0.0), TWO30, 1e300, -1e300)
    rows = [(e, 5.0, i % 4) for i, e in enumerate(ends)] + [(-5.0, e, (i + 1) % 4) for i, e in enumerate(ends)]
    return _rows(*rows, (-TWO30, TWO30 - 1.0, 3.0), (TWO30 - 1.0, -TWO30, 2.0))


CASES = {
    # ---- candidate counts (width 25: N = 1, 9 < width; N = 25 = width at r = 2; then the select)
    "r = 0 and N < width and N = width (no select)": (300, lambda: [_coord(280, 25, 20, seed=2)], lambda: _radii([0, 0.9, 1, 1.5, 2, 2.99, 0, 1, 2])),
    "N = width + 1 (width 24, r = 2: the smallest select)": (300, lambda: [_coord(290, 24, 5, seed=4)], lambda: _radii([2, 2, 2, 2, 2, 1, 3])),
    "N below and above the thread count (r = 3 .. 7: 49 .. 225; r = 8, 9, 11, 16: 289, 361, 529, 1089)":
        (400, lambda: [_coord(400, 25, 20, seed=2)], lambda: _radii([3, 4, 5, 6, 7, 7.5, 8, 8, 9, 11, 16, 20])),
    "r = 127 (65 025 candidates, 255 rounds of the block)": (512, lambda: [_coord(512, 41, 127, seed=9)], lambda: _radii([127, 126, 127.9])),
    "a radius above max_radius is clamped (to 20; +inf too)": (400, lambda: [_coord(400, 25, 20, seed=2)], lambda: _radii([20, 20.5, 21, 1000, 1e300, np.inf, 19.999])),
    "max_radius 0 (every radius is 0: one candidate)": (300, lambda: [_coord(300, 21, 0, seed=7)], lambda: _radii([0, 1, 5, np.inf, 0.5])),
    "width 1 and width 256 (the cut is the maximum; 256 winners of 289)": (1000, lambda: [_coord(300, 1, 12, seed=1), _coord(700, 256, 12, seed=2)],
                                                                          lambda: np.concatenate([_radii([8, 9, 12, 7, 0]), _radii([8, 12, 7, 9, 1])], axis=1)),
    # ---- ties and collisions
    "ties at the cut (two candidates of the cut's order, one slot: the lower index)":
        (400, lambda: [_coord(400, TIE_WIDTH, 20, seed=TIE_SEED)], lambda: _rows(*[(cx, cy, r) for cx, cy, r, _, _ in TIES])),
    "bits 16 with width 21 (winners collide)": (300, lambda: [_coord(16, 21, 10, seed=3)], lambda: _radii([0, 1, 2, 3, 8, 10])),
    "bits 1 (every winner is bit 0)": (300, lambda: [_coord(1, 5, 4, seed=3)], lambda: _radii([0, 4, np.nan])),
    # ---- values
    "a missing x, y, radius and a negative radius, each alone": (300, lambda: [_coord(300, 21, 6, seed=5)],
                                                                 lambda: _rows((np.nan, 2, 3), (1, np.nan, 3), (1, 2, np.nan), (1, 2, -1), (1, 2, -0.25), (1, 2, -np.inf), (np.inf, 2, 3),
                                                                               (1, -np.inf, 3), (1, 2, -0.0), (1, 2, 3), (np.nan, np.nan, np.nan))),
    "coordinates negative, at 0, and at both ends of +-2**30": (300, lambda: [_coord(300, 21, 3, seed=5)], _edge_rows),
    "a resolution and an origin per axis": (300, lambda: [_coord(300, 21, 6, resolution=(0.25, 3.0), origin=(100.5, -7.25), seed=8)],
                                            lambda: _rows((100.5, -7.25, 2), (100.49, -7.26, 2), (100.74, -4.26, 2), (100.75, -4.25, 2), (-1e6, 1e6, 6), (0.1 + 0.2, 0.3, 1))),
    # ---- table layout
    "an offset that is no multiple of 32, the field across several 128-bit stores": (1000, lambda: [_linear(0, 1, 45, 4), _coord(700, 33, 10, seed=2)],
                                                                                     lambda: np.concatenate([np.linspace(-0.1, 1.1, 8)[:, None], _radii([10, 9, 8, 3, 0, 10, 5, 7])], axis=1)),
    "a row wider than one pass of the storing loop (33 000 bits: 258 stores, 256 threads)":
        (33000, lambda: [_linear(0, 1, 32700, 40), _coord(290, 21, 10, seed=2)],
         lambda: np.concatenate([np.linspace(0, 1, 5)[:, None], _radii([10, 9, 8, 3, 0])], axis=1)),
    "linear + hashed + category + coordinate": (600, _mixed, _mixed_rows),
    "two coordinate fields with different seeds": (600, lambda: [_coord(300, 21, 9, seed=1), _coord(300, 21, 9, seed=2)],
                                                   lambda: np.concatenate([_radii([9, 4, 2, 0, np.nan, 3]), _radii([9, 4, 2, 0, 3, np.nan])], axis=1)),
    "sixteen entries ending in a coordinate group": (700, lambda: _linear13() + [_coord(200, 21, 9, seed=3)],
                                                     lambda: np.concatenate([np.random.RandomState(3).uniform(-1, 11, (6, 13)), _radii([9, 4, 2, 0, np.nan, 8.5])], axis=1)),
}


def encoder(name):
    from bithtm_amd import ScalarEncoder
    input_dim, fields, _ = CASES[name]
    return ScalarEncoder(fields(), input_dim)


def values(name):
    return np.ascontiguousarray(CASES[name][2](), dtype=np.float64)


def tie_rank(field, cx, cy, r):
    """(the cut's order, how many candidates lie above it, the indices of those at it) of one row that takes the select."""
    x, y = field.candidates(cx, cy, r)
    order = field.order(x, y)
    cut = np.sort(order)[-field.width]
    return int(cut), int((order > cut).sum()), np.flatnonzero(order == cut).tolist()


# ---- the model paths of tests/test_hip_coordinate.py: a vehicle's track over a coordinate field beside a linear one
def track_encoder(input_dim=300):
    """A speed field (linear) and a position field (coordinate) over `input_dim` bits; column 0 is the speed."""
    from bithtm_amd import ScalarEncoder, ScalarField
    return ScalarEncoder([ScalarField(0.0, 30.0, 60, 9), _coord(input_dim - 80, 21, 8, resolution=2.0, origin=(-50.0, -50.0), seed=4)], input_dim)


def track_values(n, seed, B=None, period=6, every=5):
    """float64 [B, n, 4] (or [n, 4]): (speed, x, y, radius) round a loop of `period` points per stream -- something to learn -- with
    a missing value or an out-of-range one in every `every`-th row."""
    rng = np.random.RandomState(seed)
    out = np.empty((B or 1, n, 4))
    for b in range(B or 1):
        loop = np.stack([rng.uniform(0, 30, period), rng.uniform(-200, 200, period), rng.uniform(-200, 200, period), rng.randint(1, 9, period).astype(np.float64)], axis=-1)
        out[b] = loop[np.arange(n) % period]
        for t in range(every - 1, n, every):
            c = (t // every + b) % 4
            out[b, t, c] = (np.nan, np.inf, 2.0 ** 31, -1.0)[c]     # (each is a missing value in its column; 2**31 is outside +-2**30)
    return out if B else out[0]
