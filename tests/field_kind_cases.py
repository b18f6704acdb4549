"""Cases of the field-kind tests (CategoryField and HashedField beside linear ScalarFields; bithtm_amd/encoders.py is the
definition, bithtm_amd/csrc/htm_fields.h the device side).  Shared by tests/test_field_kinds_cpu.py, which
checks that every case reaches the path it names, and tests/test_hip_field_kinds.py, which holds the device to the definition
on them.

A field is written ("linear", minimum, maximum, bits, width[, periodic]), ("category", categories, width[, bits]) or
("hashed", minimum, maximum, bits, width, buckets, seed).

Row shapes -- the block of the encode launch has a thread per 16-byte store, in whole waves, at most 256:
  input_dim 300     12 words, 3 stores: one wave
  input_dim 8 200   260 words, 65 stores: a block of more than one wave (two; a block of four waves is 33 000's)
  input_dim 33 000  1 032 words, 258 stores for 256 threads: the store loop takes a second pass (encode only: its linear field is
                    above the decode cap)
"""
import numpy as np

CASES = {
    # linear, periodic, category and hashed fields at the unaligned offsets 0, 61, 158, 172, 222; bits 259 .. 299 unused.  The
    # category field has 14 bits for 3 x 4 (bits no multiple of width); the second hashed field is the parameter set (1, 37, 5, 60),
    # whose census shows windows with a collision inside
    "mixed-300": (300, [("linear", 0, 100, 61, 9), ("hashed", -1, 1, 97, 7, 128, 1), ("category", 3, 4, 14), ("linear", 0, 24, 50, 5, True),
                        ("hashed", 0, 1, 37, 5, 60, 1)],
                  "one wave; every kind in one row; category bits not a multiple of width; collisions inside hashed windows"),
    # 1 000 buckets in 400 bits; width 256 (the LDS rows of the encode block are full, and longer than a one-wave pass); a category
    # field of 7 x 33 in 250 bits; a hashed field of width 1; trailing bits unused
    "mixed-8200": (8200, [("linear", 0, 100, 3000, 37), ("hashed", 0, 1, 400, 21, 1000, 1), ("category", 7, 33, 250),
                          ("linear", 0, 24, 1001, 11, True), ("hashed", 0, 1, 3000, 256, 500, 4), ("hashed", -5, 5, 50, 1, 77, 6)],
                   "several waves; width 256; width 1; 1 000 buckets in 400 bits"),
    # buckets + width - 1 == 8 192 exactly (the decode's prefix array is full); one category; a hashed field of one bit (every
    # position is 0); a hashed field of one bucket
    "cap-8200": (8200, [("hashed", 0, 1, 5000, 64, 8129, 2), ("category", 1, 5, 7), ("hashed", 0, 1, 1, 3, 10, 3), ("hashed", 0, 1, 64, 9, 1, 7)],
                 "buckets + width - 1 == 8192; categories 1; bits 1; buckets 1"),
    # the second pass of the store loop: stores 256 and 257 hold the last field's bits 32 768 .. 32 871
    "mixed-33000": (33000, [("linear", 0, 1, 20000, 301), ("hashed", 0, 1, 12000, 64, 8129, 2), ("category", 1, 5, 7), ("hashed", 0, 1, 1, 3, 10, 3),
                            ("hashed", 0, 1, 64, 9, 1, 7), ("linear", 0, 24, 600, 11, True), ("hashed", -5, 5, 200, 1, 77, 6)],
                    "more 16-byte stores than threads: a hashed field in the second pass of the store loop"),
}
DECODED = ("mixed-300", "mixed-8200", "cap-8200")           # (the cases whose every field the device decodes)

# the parameter sets (seed, bits, width, buckets) of the collision census, and what the census gives for each: the worst
# |b - decode(encode(b))|, and how many buckets decode to another one.  DESIGN.md section 23 quotes these figures.
CENSUS = {(1, 400, 21, 1000): (2, 52), (3, 64, 5, 200): (3, 17), (1, 37, 5, 60): (1, 7), (5, 130, 21, 300): (2, 44), (1, 97, 7, 128): (1, 8),
          (9, 40, 3, 90): (2, 10)}


def field(spec):
    import bithtm_amd as B
    kind, args = spec[0], spec[1:]
    if kind == "linear":
        return B.ScalarField(*args)
    if kind == "category":
        return B.CategoryField(*args)
    minimum, maximum, bits, width, buckets, seed = args
    return B.HashedField(minimum, maximum, bits, width, buckets=buckets, seed=seed)


def encoder(name):
    import bithtm_amd as B
    input_dim, specs, _ = CASES[name]
    return B.ScalarEncoder([field(s) for s in specs], input_dim)


def linear_twin(name):
    """The case's linear fields alone, at the offsets they have in the case (what a table without the other kinds encodes)."""
    enc = encoder(name)
    return [(j, f, off) for j, (f, off) in enumerate(zip(enc.fields, enc.offsets)) if f.kind == "linear"]


def values(enc, extra, seed):
    """float64 [n, F]: per field its special values -- NaN, +-inf, the maximum exactly, values below the minimum; for a category
    the ids -1, `categories`, 2.7 and -0.0 -- then `extra` random rows over and beyond every range."""
    rng = np.random.RandomState(seed)
    cols = []
    for f in enc.fields:
        lo, hi = f.minimum, f.maximum
        if f.kind == "category":
            table = [0.0, -1.0, float(f.buckets), 2.7, -0.0, np.nan, np.inf, -np.inf, f.buckets - 1.0, np.nextafter(float(f.buckets), 0.0), -1e-300, 1e300]
            rest = rng.randint(-1, f.buckets + 1, extra).astype(np.float64) + rng.choice([0.0, 0.25], extra)
        else:
            table = [0.5 * (lo + hi), lo, hi, np.nextafter(lo, -np.inf), np.nan, np.inf, -np.inf, 1e300, lo - 1e-300 if lo else -1e-300,
                     hi + 3 * (hi - lo), lo - 0.5 * (hi - lo), np.nextafter(hi, lo)]
            rest = rng.uniform(lo - 0.2 * (hi - lo), hi + 0.2 * (hi - lo), extra)
        cols.append(np.concatenate([table, rest]))
    return np.ascontiguousarray(np.stack(cols, axis=1))


def double_hit(f):
    """(b, position) of a hashed field: the lowest bucket whose window holds one position twice, or None."""
    pos = f.positions()
    for b in range(f.buckets):
        w = pos[b:b + f.width].tolist()
        twice = [p for p in w if w.count(p) > 1]
        if twice:
            return b, twice[0]
    return None


def vote_rows(enc, column_dim, seed):
    """int64 [9, input_dim] and what each row is for:
      0  all zero: (-1, 0) everywhere                     1  all ones: every bucket of a field ties (or nearly): the lowest wins
      2  random counts below 50                           3  random counts up to column_dim
      4  column_dim in every bit (the largest score)      5  per field the windows of two buckets far apart, 5 votes a bit: a tie
      6  per hashed field with such a window, one hot bit that the window hits twice (score 2 from one vote)
      7  a lone vote in every field's last used bit       8  only the unused bits of the row and of the category fields"""
    rng = np.random.RandomState(seed)
    I = enc.input_dim
    votes = np.zeros((9, I), np.int64)
    votes[1] = 1
    votes[2] = rng.randint(0, 50, I)
    votes[3] = rng.randint(0, column_dim + 1, I)
    votes[4] = column_dim
    used = np.zeros(I, bool)
    for f, off in zip(enc.fields, enc.offsets):
        a, b = f.buckets // 5, f.buckets - 1 - f.buckets // 7
        for bucket in {a, b}:
            votes[5, off + f.window(np.array([bucket]))[0]] = 5
        if f.kind == "hashed" and double_hit(f):
            votes[6, off + double_hit(f)[1]] = 1
        last = f.buckets * f.width - 1 if f.kind == "category" else f.bits - 1
        votes[7, off + last] = 1
        used[off:off + (f.buckets * f.width if f.kind == "category" else f.bits)] = True
    votes[8, ~used] = 9
    return votes
