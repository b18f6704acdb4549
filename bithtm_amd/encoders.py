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
"""

import numpy as np

from . import _lib as L

MAX_FIELDS = 16                                     # HTM_SCALAR_MAX_FIELDS
DECODE_MAX_BITS = 8192                              # HTM_DECODE_MAX_BITS: bits per field htm_decode_votes takes


class ScalarField:
    """One scalar of a stream: values in [minimum, maximum] over `bits` input bits, `width` of them set per value.
    buckets = bits for a periodic field (the window wraps round the field's end), else bits - width + 1;
    scale = buckets / (maximum - minimum), formed once here in float64 and handed to the device as that double."""

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
            flat[rows[:, None], off + (bflat[rows, j][:, None] + np.arange(f.width)) % f.bits] = True
        return out

    def decode(self, votes):
        """int [..., input_dim] -> (bucket int32 [..., F], score int32 [..., F])."""
        votes = np.asarray(votes)
        if votes.ndim < 1 or votes.shape[-1] != self.input_dim:
            raise ValueError(f"votes: int [..., {self.input_dim}], got shape {votes.shape}")
        buckets = np.empty(votes.shape[:-1] + (len(self.fields),), dtype=np.int32)
        scores = np.empty_like(buckets)
        for j, (f, off) in enumerate(zip(self.fields, self.offsets)):
            v = votes[..., off:off + f.bits].astype(np.int64)
            if f.periodic:
                v = np.concatenate([v, v[..., :f.width - 1]], axis=-1)
            p = np.concatenate([np.zeros(v.shape[:-1] + (1,), np.int64), np.cumsum(v, axis=-1)], axis=-1)
            score = p[..., f.width:f.width + f.buckets] - p[..., :f.buckets]
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
            t.offset, t.bits, t.width, t.buckets, t.periodic, t.reserved = off, f.bits, f.width, f.buckets, int(f.periodic), 0
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
                if f.bits > DECODE_MAX_BITS:
                    raise ValueError(f"encoder: a field of {f.bits} bits is above the {DECODE_MAX_BITS} the device decodes")

    def bank_values(self, values):
        """float64 [n >= 1, F], contiguous: the values of a bank of n rows."""
        v = np.ascontiguousarray(self._values(values))
        if v.ndim != 2 or v.shape[0] < 1:
            raise ValueError(f"values: float64 [n >= 1, {len(self.fields)}], got shape {v.shape}")
        return v

    def key(self):
        """What makes two encoders encode alike."""
        return (self.input_dim,) + tuple((f.minimum, f.scale, f.bits, f.width, f.periodic) for f in self.fields)
