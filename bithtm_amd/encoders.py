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

date_fields / date_values put a timestamp into such fields on the host (time of day, day of week, a weekend flag).
"""

import numpy as np

from . import _lib as L
from ._keyed import STREAM_FIELD_HASH, draw32

MAX_FIELDS = 16                                     # HTM_SCALAR_MAX_FIELDS
DECODE_MAX_BITS = 8192                              # HTM_DECODE_MAX_BITS: bits per field htm_decode_votes takes
HASHED_MAX_WIDTH = 256                              # HTM_HASHED_MAX_WIDTH: the positions of a hashed window live in the encode block's LDS
FIELD_LINEAR, FIELD_CATEGORY, FIELD_HASHED = 0, 1, 2        # htm_scalar_field.reserved & 3 (HTM_FIELD_CATEGORY, HTM_FIELD_HASHED)


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


class ScalarEncoder:
    """1 to 16 ScalarFields side by side: field j occupies the input bits [offset_j, offset_j + bits_j), offset_j the sum of the
    earlier fields' bits.  `input_dim` defaults to the sum of the bits; a larger one leaves the trailing bits 0."""

    def __init__(self, fields, input_dim=None):
        self.fields = tuple(fields)
        if not 1 <= len(self.fields) <= MAX_FIELDS or not all(isinstance(f, ScalarField) for f in self.fields):
            raise ValueError(f"ScalarEncoder: 1 to {MAX_FIELDS} ScalarFields, got {len(self.fields)}")
        self.offsets = tuple(int(x) for x in np.cumsum([0] + [f.bits for f in self.fields[:-1]]))
        total = self.offsets[-1] + self.fields[-1].bits
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
        return np.stack([f.bucket(v[..., j]) for j, f in enumerate(self.fields)], axis=-1)

    def encode(self, values):
        """float64 [..., F] -> bool [..., input_dim]."""
        b = self.bucket(values)
        out = np.zeros(b.shape[:-1] + (self.input_dim,), dtype=np.bool_)
        flat, bflat = out.reshape(-1, self.input_dim), b.reshape(-1, len(self.fields)).astype(np.int64)
        for j, (f, off) in enumerate(zip(self.fields, self.offsets)):
            rows = np.flatnonzero(bflat[:, j] >= 0)
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
