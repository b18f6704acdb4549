"""Scalar streams: the NumPy definition of what htm_bank_encode and htm_decode_votes compute on the device (bithtm_amd/csrc/
htm_scalar.h).  The reference has no encoder: this module IS the definition, and the device is held to
it bit for bit.

A ScalarField maps a float64 value to one of `buckets` buckets and a bucket to a run of `width` consecutive bits of its
`bits` input bits (wrapping for a periodic field).  A ScalarEncoder lays 1 to 16 fields side by side in a model's input row.

    field.bucket(v):   t = (v - minimum) * scale            two separately rounded IEEE double operations
       non-periodic:   NaN t -> -1 (missing); else floor(t) clamped to [0, buckets - 1] IN DOUBLE, then converted
       periodic:       unless -2**31 <= t < 2**31 -> -1 (NaN and +-inf fail the comparison); else int64(floor(t)) mod buckets
    encode:            bucket b >= 0 sets the bits offset + (b + j) % bits, j < width; a missing value sets none
    decode(votes):     score[b] = sum of votes[offset + (b + j) % bits], j < width, b < buckets; the lowest b with the largest
                       score, or (-1, 0) where that score is 0 (votes are counts: never negative)
    value_of(b):       minimum + (b + 0.5) / scale, NaN for -1 -- on the host; the device never forms a value

Two further field kinds stand beside that linear one in the same row (bithtm_amd/csrc/htm_fields.h):

    CategoryField:     buckets = categories, minimum 0, scale 1; t = (v - 0.0) * 1.0; missing unless 0 <= floor(t) < categories
                       (an unknown id is missing, NOT clamped); bucket c sets the bits offset + c * width + j, j < width, so no
                       two categories share a bit; score[c] = the votes of those bits; value_of(c) = float(c)
    HashedField:       bucket(v) as a non-periodic ScalarField over `buckets` buckets; bucket b sets the bits offset + pos(b + j),
                       j < width, pos(i) = (htm_draw32(htm_stream_base(seed, 7, 0), i, 0) * bits) >> 32 for i < buckets + width
                       - 1 (positions may collide: a window may set fewer than `width` bits); G[i] = votes[offset + pos(i)],
                       score[b] = G[b] + ... + G[b + width - 1] (a collided bit counted once per j)
    Both decode to the lowest bucket with the largest score, (-1, 0) where that score is 0.

A coordinate field (bithtm_amd/csrc/htm_coord.h) reads THREE value columns -- x, y and a radius in cells:

    CoordinateField:   cell of an axis: t = (v - origin) * scale, scale = 1 / resolution; missing unless -2**30 <= t < 2**30 (NaN
                       and +-inf fail the comparison); else c = int32(floor(t))
                       radius: t = (v - 0.0) * 1.0; missing if NaN or t < 0; else r = int(min(floor(t), float(max_radius)))
                       candidates: the N = (2r + 1)**2 cells cx - r <= x <= cx + r, cy - r <= y <= cy + r, index
                       i = (y - (cy - r)) * (2r + 1) + (x - (cx - r));  order(x, y) = htm_draw24(htm_stream_base(seed, 8, 0), x, y),
                       bit(x, y) = (htm_draw32(htm_stream_base(seed, 8, 1), x, y) * bits) >> 32
                       the row gets offset + bit(p) of the min(width, N) candidates p of the largest order, ties at the cut to the
                       lower index; a row in which any of the three is missing gets no bit.  There is no decode: (-1, 0), NaN.

date_fields / date_values put a timestamp into such fields on the host (time of day, day of week, a weekend flag); geo_values
puts longitude, latitude and speed into the three columns of a coordinate field.
"""

import numpy as np

from . import _lib as L
from ._keyed import STREAM_COORDINATE, STREAM_FIELD_HASH, draw32

MAX_FIELDS = 16                                     # HTM_SCALAR_MAX_FIELDS
DECODE_MAX_BITS = 8192                              # HTM_DECODE_MAX_BITS: bits per field htm_decode_votes takes
HASHED_MAX_WIDTH = 256                              # HTM_HASHED_MAX_WIDTH: the positions of a hashed window live in the encode block's LDS
FIELD_LINEAR, FIELD_CATEGORY, FIELD_HASHED = 0, 1, 2        # htm_scalar_field.reserved & 3 (HTM_FIELD_CATEGORY, HTM_FIELD_HASHED)
FIELD_COORDINATE = 3                                # HTM_FIELD_COORDINATE: a group of three table entries, one per value column
COORD_MAX_RADIUS = 127                              # HTM_COORD_MAX_RADIUS: (2 * 127 + 1)**2 = 65 025 candidates at the most


class ScalarField:
    """One scalar of a stream: values in [minimum, maximum] over `bits` input bits, `width` of them set per value.
    buckets = bits for a periodic field (the window wraps round the field's end), else bits - width + 1;
    scale = buckets / (maximum - minimum), formed once here in float64 and handed to the device as that double."""

    kind, kind_code, seed = "linear", FIELD_LINEAR, 0

    def __init__(self, minimum, maximum, bits, width, periodic=False):
        minimum, maximum, bits, width = float(minimum), float(maximum), int(bits), int(width)
        if not (np.isfinite(minimum) and np.isfinite(maximum) and minimum < maximum):
            raise ValueError(f"ScalarField: finite minimum < maximum, got {minimum}, {maximum}")
        if not 1 <= width <= bits:
            raise ValueError(f"ScalarField: 1 <= width <= bits, got width {width}, bits {bits}")
        self.minimum, self.maximum, self.bits, self.width, self.periodic = minimum, maximum, bits, width, bool(periodic)
        self.buckets = bits if self.periodic else bits - width + 1
        self.scale = float(self.buckets) / (maximum - minimum)
        if not (np.isfinite(self.scale) and self.scale > 0.0):
            raise ValueError(f"ScalarField: buckets / (maximum - minimum) is not a positive finite double ({self.scale})")

    def bucket(self, v):
        """float64 [...] -> int32 [...]: the bucket of every value, -1 for a missing one."""
        v = np.asarray(v, dtype=np.float64)
        with np.errstate(invalid="ignore", over="ignore"):
            t = (v - self.minimum) * self.scale
            if self.periodic:
                ok = (t >= -2147483648.0) & (t < 2147483648.0)
                b = np.mod(np.floor(np.where(ok, t, 0.0)).astype(np.int64), self.buckets)
            else:
                ok = ~np.isnan(t)
                b = np.clip(np.floor(np.where(ok, t, 0.0)), 0.0, float(self.buckets - 1)).astype(np.int64)
        return np.where(ok, b, -1).astype(np.int32)

    def value_of(self, bucket):
        """int [...] -> float64 [...]: the middle of the bucket, NaN for -1."""
        b = np.asarray(bucket, dtype=np.int64)
        return np.where(b >= 0, self.minimum + (b + 0.5) / self.scale, np.nan)

    def window(self, bucket):
        """int64 [n] buckets (all >= 0) -> int64 [n, width]: the bits of the field, counted from its offset, each bucket sets."""
        return (bucket[:, None] + np.arange(self.width)) % self.bits

    def scores(self, votes):
        """int64 [..., bits], the field's votes -> int64 [..., buckets]: score[b] of the definition."""
        v = votes
        if self.periodic:
            v = np.concatenate([v, v[..., :self.width - 1]], axis=-1)
        p = np.concatenate([np.zeros(v.shape[:-1] + (1,), np.int64), np.cumsum(v, axis=-1)], axis=-1)
        return p[..., self.width:self.width + self.buckets] - p[..., :self.buckets]

    def decode_elements(self):
        """How many prefix sums less one the device's decode block forms for this field (at most DECODE_MAX_BITS)."""
        return self.bits

    def key(self):
        return (self.minimum, self.scale, self.bits, self.width, self.periodic)


class CategoryField(ScalarField):
    """One of `categories` ids (the values 0.0, 1.0, ...) over `bits` input bits: category c owns the `width` bits c * width ..
    c * width + width - 1, so no two categories share a bit.  `bits` defaults to categories * width; a larger value leaves the
    trailing bits unused.  An id outside [0, categories) -- NaN and +-inf too -- is missing, not clamped."""

    kind, kind_code = "category", FIELD_CATEGORY

    def __init__(self, categories, width, bits=None):
        categories, width = int(categories), int(width)
        if categories < 1 or width < 1:
            raise ValueError(f"CategoryField: categories >= 1 and width >= 1, got {categories}, {width}")
        bits = categories * width if bits is None else int(bits)
        if bits < categories * width:
            raise ValueError(f"CategoryField: {categories} categories of width {width} need {categories * width} bits, got {bits}")
        self.minimum, self.maximum, self.bits, self.width, self.periodic = 0.0, float(categories), bits, width, False
        self.categories = self.buckets = categories
        self.scale = 1.0

    def bucket(self, v):
        v = np.asarray(v, dtype=np.float64)
        with np.errstate(invalid="ignore", over="ignore"):
            t = (v - self.minimum) * self.scale
            c = np.floor(t)
            ok = (c >= 0.0) & (c < float(self.buckets))             # (NaN and +-inf fail the comparison)
        return np.where(ok, np.where(ok, c, 0.0).astype(np.int64), -1).astype(np.int32)

    def value_of(self, bucket):
        b = np.asarray(bucket, dtype=np.int64)
        return np.where(b >= 0, b.astype(np.float64), np.nan)

    def window(self, bucket):
        return bucket[:, None] * self.width + np.arange(self.width)

    def scores(self, votes):
        used = votes[..., :self.buckets * self.width]
        return used.reshape(used.shape[:-1] + (self.buckets, self.width)).sum(axis=-1)

    def key(self):
        return ScalarField.key(self) + (self.kind, self.buckets, 0)


class HashedField(ScalarField):
    """A random distributed scalar field: `buckets` buckets over [minimum, maximum] (or as many as `resolution` asks for) in
    `bits` input bits, whatever `bits` is.  Bucket b sets the bits pos(b), ..., pos(b + width - 1) of a keyed hash (stream 7 of
    htm_rng.h under `seed`), so neighbouring buckets share width - 1 of their positions and distant ones next to none.  Positions
    may collide, so decode(encode(b)) can be a bucket a little below b.  Never periodic."""

    kind, kind_code = "hashed", FIELD_HASHED

    def __init__(self, minimum, maximum, bits, width, buckets=None, resolution=None, seed=0):
        minimum, maximum, bits, width, seed = float(minimum), float(maximum), int(bits), int(width), int(seed)
        if not (np.isfinite(minimum) and np.isfinite(maximum) and minimum < maximum):
            raise ValueError(f"HashedField: finite minimum < maximum, got {minimum}, {maximum}")
        if bits < 1 or not 1 <= width <= HASHED_MAX_WIDTH:
            raise ValueError(f"HashedField: bits >= 1 and 1 <= width <= {HASHED_MAX_WIDTH}, got bits {bits}, width {width}")
        if not 0 <= seed < 1 << 29:
            raise ValueError(f"HashedField: 0 <= seed < 2**29, got {seed}")
        if (buckets is None) == (resolution is None):
            raise ValueError("HashedField: give exactly one of buckets and resolution")
        if buckets is None:
            resolution = float(resolution)
            if not (np.isfinite(resolution) and resolution > 0.0):
                raise ValueError(f"HashedField: resolution must be a positive finite number, got {resolution}")
            count = np.ceil((maximum - minimum) / resolution)
            if not count < 2.0 ** 31:
                raise ValueError(f"HashedField: resolution {resolution} asks for {count} buckets")
            buckets = int(count)
        buckets = int(buckets)
        if not 1 <= buckets < (1 << 31) - HASHED_MAX_WIDTH:
            raise ValueError(f"HashedField: buckets >= 1 (and below 2**31 - {HASHED_MAX_WIDTH}), got {buckets}")
        self.minimum, self.maximum, self.bits, self.width, self.periodic = minimum, maximum, bits, width, False
        self.buckets, self.seed = buckets, seed
        self.scale = float(buckets) / (maximum - minimum)
        if not (np.isfinite(self.scale) and self.scale > 0.0):
            raise ValueError(f"HashedField: buckets / (maximum - minimum) is not a positive finite double ({self.scale})")
        self._pos = None

    def positions(self):
        """int64 [buckets + width - 1]: pos(i) of the definition."""
        if self._pos is None:
            i = np.arange(self.buckets + self.width - 1, dtype=np.uint32)
            self._pos = ((draw32(self.seed, STREAM_FIELD_HASH, 0, i).astype(np.uint64) * np.uint64(self.bits)) >> np.uint64(32)).astype(np.int64)
        return self._pos

    def window(self, bucket):
        return self.positions()[bucket[:, None] + np.arange(self.width)]

    def scores(self, votes):
        g = votes[..., self.positions()]
        p = np.concatenate([np.zeros(g.shape[:-1] + (1,), np.int64), np.cumsum(g, axis=-1)], axis=-1)
        return p[..., self.width:self.width + self.buckets] - p[..., :self.buckets]

    def decode_elements(self):
        return self.buckets + self.width - 1

    def key(self):
        return ScalarField.key(self) + (self.kind, self.buckets, self.seed)


class CoordinateAxis(ScalarField):
    """The y column or the radius column of a CoordinateField: a table entry of its own (the C ABI counts value columns) that holds
    no bits -- bits, width and buckets 0, at its field's offset.  Made by the field; `field` is the CoordinateField it belongs to."""

    kind, kind_code = "coordinate-axis", FIELD_COORDINATE

    def __init__(self, field, minimum, scale):
        self.field, self.minimum, self.maximum, self.scale = field, float(minimum), float("nan"), float(scale)
        self.bits = self.width = self.buckets = 0
        self.periodic = False

    def value_of(self, bucket):
        return np.full(np.shape(bucket), np.nan)

    def key(self):
        return ScalarField.key(self) + (self.kind, 0, 0)


class CoordinateField(ScalarField):
    """A 2-D position and a radius over `bits` input bits, NuPIC's CoordinateEncoder: of the (2r + 1)**2 integer cells of the square
    of radius r round the position's cell, the `width` that a keyed hash (stream 8 of htm_rng.h under `seed`) ranks highest each set
    one bit.  Nearby positions share most of their bits; positions more than 2r apart share next to none.  The field reads three
    value columns -- x, y and the radius in cells (clamped to `max_radius`) -- and stands in a ScalarEncoder as three entries: itself
    at x, and `axes` (two CoordinateAxis objects) behind it.  A cell is `resolution` wide (a scalar, or an (x, y) pair) and cell 0
    begins at `origin`.  There is no decode: the three columns decode to (-1, 0) and their value is NaN."""

    kind, kind_code = "coordinate", FIELD_COORDINATE

    def __init__(self, bits, width, max_radius, resolution=1.0, origin=(0.0, 0.0), seed=0):
        bits, width, max_radius, seed = int(bits), int(width), int(max_radius), int(seed)
        if bits < 1 or not 1 <= width <= HASHED_MAX_WIDTH:
            raise ValueError(f"CoordinateField: bits >= 1 and 1 <= width <= {HASHED_MAX_WIDTH}, got bits {bits}, width {width}")
        if not 0 <= max_radius <= COORD_MAX_RADIUS:
            raise ValueError(f"CoordinateField: 0 <= max_radius <= {COORD_MAX_RADIUS}, got {max_radius}")
        if not 0 <= seed < 1 << 29:
            raise ValueError(f"CoordinateField: 0 <= seed < 2**29, got {seed}")
        res = np.broadcast_to(np.asarray(resolution, dtype=np.float64), (2,)) if np.ndim(resolution) <= 1 and np.size(resolution) in (1, 2) else None
        org = np.asarray(origin, dtype=np.float64)
        if res is None or not (np.isfinite(res).all() and (res > 0.0).all()):
            raise ValueError(f"CoordinateField: resolution must be a positive finite number or an (x, y) pair of them, got {resolution}")
        if org.shape != (2,) or not np.isfinite(org).all():
            raise ValueError(f"CoordinateField: origin must be a finite (x, y) pair, got {origin}")
        scales = [1.0 / float(r) for r in res]
        if not all(np.isfinite(x) and x > 0.0 for x in scales):
            raise ValueError(f"CoordinateField: 1 / resolution is not a positive finite double ({scales})")
        self.minimum, self.maximum, self.scale = float(org[0]), float("nan"), scales[0]
        self.bits, self.width, self.periodic, self.seed = bits, width, False, seed
        self.max_radius = self.buckets = max_radius         # (the table's `buckets` member carries max_radius)
        self.axes = (CoordinateAxis(self, float(org[1]), scales[1]), CoordinateAxis(self, 0.0, 1.0))

    def cells(self, values):
        """float64 [..., 3] (x, y, radius) -> (cx int64 [...], cy int64 [...], r int64 [...], ok bool [...]): the centre's cell, the
        clamped radius, and whether the row has all three (where it has not, the other three are 0)."""
        v = np.asarray(values, dtype=np.float64)
        ok, out = np.ones(v.shape[:-1], dtype=np.bool_), []
        with np.errstate(invalid="ignore", over="ignore"):
            for j, axis in enumerate((self, self.axes[0])):
                t = (v[..., j] - axis.minimum) * axis.scale
                good = (t >= -1073741824.0) & (t < 1073741824.0)
                out.append(np.floor(np.where(good, t, 0.0)).astype(np.int64))
                ok &= good
            t = (v[..., 2] - self.axes[1].minimum) * self.axes[1].scale
            good = ~np.isnan(t) & ~(t < 0.0)
            out.append(np.minimum(np.floor(np.where(good, t, 0.0)), float(self.max_radius)).astype(np.int64))
            ok &= good
        return tuple(np.where(ok, a, 0) for a in out) + (ok,)

    def order(self, x, y):
        """int [...] cells -> int64 [...]: order(x, y) of the definition, in [0, 2**24)."""
        return (draw32(self.seed, STREAM_COORDINATE, 0, np.asarray(x, np.int64), np.asarray(y, np.int64)) >> np.uint32(8)).astype(np.int64)

    def bit(self, x, y):
        """int [...] cells -> int64 [...]: bit(x, y) of the definition, in [0, bits)."""
        h = draw32(self.seed, STREAM_COORDINATE, 1, np.asarray(x, np.int64), np.asarray(y, np.int64))
        return ((h.astype(np.uint64) * np.uint64(self.bits)) >> np.uint64(32)).astype(np.int64)

    def candidates(self, cx, cy, r):
        """One row's candidates in index order: (x int64 [N], y int64 [N]), N = (2r + 1)**2, y-major."""
        side = 2 * int(r) + 1
        i = np.arange(side * side, dtype=np.int64)
        return int(cx) - int(r) + i % side, int(cy) - int(r) + i // side

    def selected(self, cx, cy, r):
        """One row's winners: int64 [min(width, N)] candidate indices, by falling order, equal orders by rising index."""
        x, y = self.candidates(cx, cy, r)
        if x.size <= self.width:
            return np.arange(x.size, dtype=np.int64)
        return np.argsort(-self.order(x, y), kind="stable")[:self.width]

    def positions(self, cx, cy, r):
        """One row's bits, counted from the field's offset: int64 [min(width, N)], possibly with repeats."""
        x, y = self.candidates(cx, cy, r)
        pick = self.selected(cx, cy, r)
        return self.bit(x[pick], y[pick])

    def value_of(self, bucket):
        return np.full(np.shape(bucket), np.nan)

    def key(self):
        return ScalarField.key(self) + (self.kind, self.max_radius, self.seed)


class ScalarEncoder:
    """1 to 16 value columns side by side: a ScalarField is one column and occupies the input bits [offset_j, offset_j + bits_j),
    offset_j the sum of the earlier fields' bits; a CoordinateField is three columns (x, y, radius) -- `fields` holds the field at x
    and its two axis objects, of 0 bits at the field's offset, behind it.  `input_dim` defaults to the sum of the bits; a larger
    one leaves the trailing bits 0."""

    def __init__(self, fields, input_dim=None):
        fields = tuple(fields)
        if not all(isinstance(f, ScalarField) and not isinstance(f, CoordinateAxis) for f in fields):
            raise ValueError("ScalarEncoder: every field must be a ScalarField (a CoordinateField brings its axes itself)")
        self.fields = tuple(c for f in fields for c in ((f,) + f.axes if f.kind_code == FIELD_COORDINATE else (f,)))
        if not 1 <= len(self.fields) <= MAX_FIELDS:
            raise ValueError(f"ScalarEncoder: 1 to {MAX_FIELDS} value columns (a CoordinateField is three), got {len(self.fields)}")
        offsets, total = [], 0
        for f in self.fields:
            offsets.append(offsets[-1] if isinstance(f, CoordinateAxis) else total)
            total += f.bits
        self.offsets = tuple(offsets)
        self.input_dim = total if input_dim is None else int(input_dim)
        if self.input_dim < total:
            raise ValueError(f"ScalarEncoder: the fields take {total} bits, input_dim is {self.input_dim}")

    def __len__(self):
        return len(self.fields)

    def _values(self, values):
        v = np.asarray(values, dtype=np.float64)
        if v.ndim < 1 or v.shape[-1] != len(self.fields):
            raise ValueError(f"values: float64 [..., {len(self.fields)}], got shape {v.shape}")
        return v

    def bucket(self, values):
        """float64 [..., F] -> int32 [..., F]."""
        v = self._values(values)
        cols = []
        for j, f in enumerate(self.fields):
            if f.kind_code != FIELD_COORDINATE:
                cols.append(f.bucket(v[..., j]))
            elif f.kind == "coordinate":            # (0 in its three columns where the field has a value, -1 where one is missing)
                cols += [np.where(f.cells(v[..., j:j + 3])[3], 0, -1).astype(np.int32)] * 3
        return np.stack(cols, axis=-1)

    def encode(self, values):
        """float64 [..., F] -> bool [..., input_dim]."""
        b = self.bucket(values)
        out = np.zeros(b.shape[:-1] + (self.input_dim,), dtype=np.bool_)
        flat, bflat = out.reshape(-1, self.input_dim), b.reshape(-1, len(self.fields)).astype(np.int64)
        vflat = self._values(values).reshape(-1, len(self.fields))
        for j, (f, off) in enumerate(zip(self.fields, self.offsets)):
            rows = np.flatnonzero(bflat[:, j] >= 0)
            if f.kind_code == FIELD_COORDINATE:
                if f.kind == "coordinate":
                    cx, cy, r, _ = f.cells(vflat[rows, j:j + 3])
                    for i, row in enumerate(rows):
                        flat[row, off + f.positions(cx[i], cy[i], r[i])] = True
                continue
            flat[rows[:, None], off + f.window(bflat[rows, j])] = True
        return out

    def decode(self, votes):
        """int [..., input_dim] -> (bucket int32 [..., F], score int32 [..., F])."""
        votes = np.asarray(votes)
        if votes.ndim < 1 or votes.shape[-1] != self.input_dim:
            raise ValueError(f"votes: int [..., {self.input_dim}], got shape {votes.shape}")
        buckets = np.empty(votes.shape[:-1] + (len(self.fields),), dtype=np.int32)
        scores = np.empty_like(buckets)
        for j, (f, off) in enumerate(zip(self.fields, self.offsets)):
            if f.kind_code == FIELD_COORDINATE:     # (no decode)
                buckets[..., j], scores[..., j] = -1, 0
                continue
            score = f.scores(votes[..., off:off + f.bits].astype(np.int64))
            best = np.argmax(score, axis=-1)                        # (the first of equal maxima: the lowest bucket)
            top = np.take_along_axis(score, best[..., None], -1)[..., 0]
            buckets[..., j] = np.where(top > 0, best, -1)
            scores[..., j] = np.where(top > 0, top, 0)
        return buckets, scores

    def value_of(self, bucket):
        """int [..., F] -> float64 [..., F]."""
        b = np.asarray(bucket)
        if b.ndim < 1 or b.shape[-1] != len(self.fields):
            raise ValueError(f"bucket: int [..., {len(self.fields)}], got shape {b.shape}")
        return np.stack([f.value_of(b[..., j]) for j, f in enumerate(self.fields)], axis=-1)

    def table(self):
        """The fields as the htm_scalar_field array the C ABI takes."""
        tab = (L.HtmScalarField * len(self.fields))()
        for t, f, off in zip(tab, self.fields, self.offsets):
            t.minimum, t.scale = f.minimum, f.scale
            t.offset, t.bits, t.width, t.buckets, t.periodic, t.reserved = off, f.bits, f.width, f.buckets, int(f.periodic), f.kind_code | f.seed << 2
        return tab

    def check_model(self, input_dim, column_dim=None):
        """ValueError unless this encoder fits a model of `input_dim` inputs (and, with `column_dim`, unless every decode score --
        at most column_dim votes per bit, width bits -- fits an int32, and every field the decode launch's LDS)."""
        if self.input_dim != int(input_dim):
            raise ValueError(f"encoder: its input_dim {self.input_dim} is not the model's {int(input_dim)}")
        if column_dim is not None:
            for f in self.fields:
                if f.kind_code == FIELD_COORDINATE:                 # (not decoded: no score, no prefix sums)
                    continue
                if int(column_dim) * f.width >= 1 << 31:
                    raise ValueError(f"encoder: column_dim * width = {int(column_dim) * f.width} does not fit an int32 score")
                if f.kind_code == FIELD_HASHED and f.decode_elements() > DECODE_MAX_BITS:
                    raise ValueError(f"encoder: a hashed field of buckets + width - 1 = {f.decode_elements()} positions is above the "
                                     f"{DECODE_MAX_BITS} the device decodes")
                if f.kind_code != FIELD_HASHED and f.bits > DECODE_MAX_BITS:
                    raise ValueError(f"encoder: a field of {f.bits} bits is above the {DECODE_MAX_BITS} the device decodes")

    def bank_values(self, values):
        """float64 [n >= 1, F], contiguous: the values of a bank of n rows."""
        v = np.ascontiguousarray(self._values(values))
        if v.ndim != 2 or v.shape[0] < 1:
            raise ValueError(f"values: float64 [n >= 1, {len(self.fields)}], got shape {v.shape}")
        return v

    def key(self):
        """What makes two encoders encode alike (a non-linear field adds its kind, buckets and seed)."""
        return (self.input_dim,) + tuple(f.key() for f in self.fields)


def date_fields(time_of_day=(96, 11), day_of_week=(56, 8), weekend=11):
    """The fields of a timestamp, for ScalarEncoder([...] + date_fields(...)): a periodic time-of-day field over [0, 24) hours, a
    periodic day-of-week field over [0, 7) days (Monday = 0) -- each given as (bits, width) -- and a CategoryField(2, weekend).
    A part passed as None is left out.  date_values gives the values, in this order."""
    fields = []
    if time_of_day is not None:
        fields.append(ScalarField(0.0, 24.0, time_of_day[0], time_of_day[1], periodic=True))
    if day_of_week is not None:
        fields.append(ScalarField(0.0, 7.0, day_of_week[0], day_of_week[1], periodic=True))
    if weekend is not None:
        fields.append(CategoryField(2, weekend))
    return fields


def date_values(times, time_of_day=True, day_of_week=True, weekend=True):
    """datetime64 [...] -> float64 [..., F]: per timestamp the hour of the day in [0, 24), the day of the week in [0, 7) (Monday
    0.0, Monday noon 0.5, ...) and 1.0 on Saturdays and Sundays, else 0.0 -- the parts whose flag is set (None or False leaves a
    part out, as in date_fields).  NaT gives NaN in every part."""
    t = np.asarray(times, dtype="datetime64[us]")
    nat = np.isnat(t)
    us = np.where(nat, 0, t.astype(np.int64))
    day_us = 86400 * 1000000
    days, in_day = np.divmod(us, day_us)
    fraction = in_day.astype(np.float64) / float(day_us)
    weekday = (days + 3) % 7                                        # (1970-01-01 was a Thursday)
    parts = []
    if time_of_day:
        parts.append(fraction * 24.0)
    if day_of_week:
        parts.append(weekday.astype(np.float64) + fraction)
    if weekend:
        parts.append((weekday >= 5).astype(np.float64))
    if not parts:
        raise ValueError("date_values: every part is left out")
    return np.where(nat[..., None], np.nan, np.stack(parts, axis=-1))


EARTH_RADIUS = 6378137.0                            # metres: the sphere of the spherical Mercator projection (EPSG:3857)


def geo_values(longitude, latitude, speed, scale, timestep=1.0, width=21):
    """Degrees and metres per second -> float64 [..., 3], the three value columns of CoordinateField(resolution=scale), as NuPIC's
    GeospatialCoordinateEncoder forms them: the spherical Mercator metres x = R * lon, y = R * ln tan(pi / 4 + lat / 2) (angles in
    radians, R = 6 378 137), and the radius in cells max(rint(speed * timestep / scale / 2 * 1.5), ceil((sqrt(width) - 1) / 2)) --
    `scale` metres per cell, `timestep` seconds between readings, `width` the field's.  NaN in, NaN out."""
    lon, lat, speed = np.broadcast_arrays(np.asarray(longitude, np.float64), np.asarray(latitude, np.float64), np.asarray(speed, np.float64))
    scale, timestep = float(scale), float(timestep)
    if not (np.isfinite(scale) and scale > 0.0 and np.isfinite(timestep) and timestep > 0.0 and int(width) >= 1):
        raise ValueError(f"geo_values: scale and timestep above 0 and width >= 1, got {scale}, {timestep}, {width}")
    with np.errstate(invalid="ignore", divide="ignore", over="ignore"):
        x = EARTH_RADIUS * np.deg2rad(lon)
        y = EARTH_RADIUS * np.log(np.tan(np.pi / 4.0 + np.deg2rad(lat) / 2.0))
        least = np.ceil((np.sqrt(float(int(width))) - 1.0) / 2.0)
        cells = speed * timestep / scale / 2.0 * 1.5
        radius = np.where(np.isnan(cells), np.nan, np.maximum(np.rint(cells), least))
    return np.stack([x, y, radius], axis=-1)
