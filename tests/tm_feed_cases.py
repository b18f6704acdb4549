"""Lists for the feed launch of batched stand-alone Temporal Memory runs (k_tm_feed, bithtm_amd/csrc/htm_tm_feed.h; DESIGN.md
section 16): the contract of the launch in NumPy, a census of the size-dependent paths a row takes through it, and the smallest
table of cases that reaches every path.  Shared by tests/test_tm_feed_cases_cpu.py (the contract against independent NumPy, every
case against its path) and tests/test_hip_tm_feed_geometry.py (the device against the contract and against process()).

What the launch does with (column_dim C, list length n), restated here and not imported -- if a constant of the kernel moves, the
census and with it the table's assertions move away from the kernel and the device test says so:
  * words = ((C + 31) / 32 + 3) & ~3 bitmap words in LDS, 4 * words + 32 bytes, refused above 64 KiB (C above 524 032);
  * per = ((words + 255) / 256 + 3) & ~3 consecutive words per thread: thread t owns words [t * per, min(t * per + per, words));
  * the counts of the threads go through a block prefix sum of four waves of 64: a wave's total matters to the waves behind it;
  * the row is read by 256 threads, entry i by thread i % 256 in pass i / 256;
  * the clearing loop runs min((C + 255) / 256, 1024) blocks of 256 threads over C * WPC cell words, WPC = 2 for cell_dim above 32.

Pure NumPy; nothing here touches a device."""

from types import SimpleNamespace

import numpy as np

THREADS, WAVE, GRID_MAX, LDS_MAX = 256, 64, 1024, 64 * 1024
INT32_MAX = 2 ** 31 - 1


# ------------------------------------------------------------------------------------------ the contract

def feed_contract(row, C, n):
    """(sorted list int32[n], bad): what the steps behind the feed launch run on.  A good row -- n distinct ids in [0, C) -- sorted.
    A bad one (bad = True): the distinct ids in [0, C) it lists, and the lowest columns not among them until n are present."""
    row = np.asarray(row, dtype=np.int64).reshape(-1)
    assert len(row) == n and 1 <= n <= C
    listed = np.zeros(C, dtype=bool)
    listed[row[(row >= 0) & (row < C)]] = True
    have = int(listed.sum())
    if have == n:
        return np.flatnonzero(listed).astype(np.int32), False
    listed[np.flatnonzero(~listed)[:n - have]] = True
    return np.flatnonzero(listed).astype(np.int32), True


def repaired(rows, C):
    """The bank as the device steps on it: every row by feed_contract."""
    rows = np.asarray(rows)
    return np.stack([feed_contract(r, C, rows.shape[1])[0] for r in rows])


# ------------------------------------------------------------------------------------------ the census

def feed_words(C):
    return ((C + 31) // 32 + 3) & ~3


def feed_per(C):
    return ((feed_words(C) + THREADS - 1) // THREADS + 3) & ~3


def feed_lds_bytes(C):
    return 4 * feed_words(C) + 32


def clear_iterations(C, K):
    """Iterations of the clearing loop's busiest thread."""
    wpc = 2 if K > 32 else 1
    stride = min((C + 255) // 256, GRID_MAX) * THREADS
    return -(-(C * wpc) // stride)


def feed_census(row, C, n, K=4):
    """Which paths the row takes: see the module's docstring.  Bits are those the block counts and emits (feed_contract's)."""
    cols, bad = feed_contract(row, C, n)
    words, per = feed_words(C), feed_per(C)
    given = np.asarray(row, dtype=np.int64).reshape(-1)
    bit_word = cols.astype(np.int64) // 32
    threads = np.unique(bit_word // per)
    last = int(threads[-1])
    return SimpleNamespace(
        bad=bad, words=words, per=per, lds=feed_lds_bytes(C),
        bitmap_threads=-(-words // per),                        # threads whose run holds a word at all
        threads=threads, waves=sorted({int(t) // WAVE for t in threads}),
        wave_totals=[int(np.sum(bit_word // per // WAVE == w)) for w in range(THREADS // WAVE)],
        passes=-(-n // THREADS),
        cut_last=last * per + per > words,                      # the last owning thread's run ends at `words`, not after `per`
        full_words=int(np.sum(np.bincount(bit_word, minlength=words) == 32)),
        pad_ids=given[(given >= C) & (given < 32 * words)],     # ids the bitmap has room for and the model has no column for
        clear_iterations=clear_iterations(C, K))


def zero_wave_between(census):
    """A wave without a bit between two waves that own some: its total in the block scan is zero and must still be passed over."""
    w = census.waves
    return any(x not in w for x in range(w[0], w[-1]))


def entry_place(i):
    """(pass, thread, wave) that reads entry i of a row."""
    return i // THREADS, i % THREADS, (i % THREADS) // WAVE


# ------------------------------------------------------------------------------------------ rows

def _row(rng, C, n, must=(), lo=0, hi=None, avoid=()):
    """n distinct ids: `must`, and the rest drawn from [lo, hi) without `avoid`; in random order."""
    hi = C if hi is None else hi
    pool = np.setdiff1d(np.arange(lo, hi), np.r_[np.asarray(must, np.int64), np.asarray(avoid, np.int64)])
    row = np.r_[np.asarray(must, np.int64), rng.choice(pool, n - len(must), replace=False)]
    return row[rng.permutation(n)].astype(np.int32)


def _variants(rng, C, base, rows, keep=()):
    """`rows` rows: the base rows, then copies with a tenth of their ids exchanged (never those of `keep`), reshuffled."""
    out = [b.copy() for b in base[:rows]]
    for r in range(len(base), rows):
        row = base[r % len(base)].copy()
        free = np.flatnonzero(~np.isin(row, keep))
        m = max(1, min(len(free), len(row) // 10))
        row[rng.choice(free, m, replace=False)] = rng.choice(np.setdiff1d(np.arange(C), row), m, replace=False)
        out.append(row[rng.permutation(len(row))])
    return np.asarray(out, dtype=np.int32)


def _spread(rng, C, n, waves=(0, 1, 2, 3), must=()):
    """A row with its ids divided evenly among the id ranges of the given waves' threads."""
    per_wave = 32 * feed_per(C) * WAVE
    parts, left = [np.asarray(must, np.int64)], n - len(must)
    pools = [np.setdiff1d(np.arange(w * per_wave, min((w + 1) * per_wave, C)), must) for w in waves]
    takes = [min(left // len(waves), len(pool) // 2) for pool in pools]       # (a short last wave gives half of what it has)
    takes[0] += left - sum(takes)
    for pool, take in zip(pools, takes):
        parts.append(rng.choice(pool, take, replace=False))
    row = np.concatenate(parts)
    return row[rng.permutation(n)].astype(np.int32)


def _case(name, C, K, n, rows, calls, pool=False):
    rows = np.ascontiguousarray(rows, dtype=np.int32)
    assert rows.shape[1] == n and all(len(set(r.tolist())) == n and r.min() >= 0 and r.max() < C for r in rows), name
    steps = sum(calls)
    assert steps % len(rows) and calls[0] % 2 == 1, name       # no multiple of the rows; the second call starts at an odd step
    # (an explicit pool for the large shapes: room for 2 n new segments a step, the rate pool_look plans with)
    capacity = 2 * n * (steps + 16) if pool else None
    return SimpleNamespace(name=name, C=C, K=K, n=n, rows=rows, calls=calls, steps=steps, segment_capacity=capacity, segment_slots=128)


def _wave1_one_thread():
    C, n = 8219, 40
    rng = np.random.RandomState(101)
    base = [_row(rng, C, n, must=(0, C - 1)) for _ in range(3)]
    return _case("wave1-one-thread", C, 4, n, _variants(rng, C, base, 5, keep=(0, C - 1)), (7, 6))


def _all_four_waves():
    C, n = 24700, 300
    rng = np.random.RandomState(102)
    full = np.arange(7 * 32, 8 * 32)                            # word 7, and nothing below it
    rest = _row(rng, C, n - 32, must=(C - 1,), lo=8 * 32)
    rows = [_spread(rng, C, n, must=(0, C - 1)), _spread(rng, C, n), _spread(rng, C, n, waves=(0, 3)),
            np.r_[full, rest][rng.permutation(n)], _spread(rng, C, n, must=(C - 1,))]
    return _case("all-four-waves", C, 2, n, rows, (7, 6), pool=True)


def _per8_cut_run():
    C, n = 32865, 600
    rng = np.random.RandomState(103)
    rows = [_row(rng, C, n, must=np.r_[C - 1, 32768 + rng.choice(96, 8, replace=False)]) for _ in range(3)]
    return _case("per8-cut-run", C, 2, n, rows, (7, 7), pool=True)


def _wpc2():
    C, n = 8219, 48
    rng = np.random.RandomState(104)
    base = [_row(rng, C, n, must=(C - 1,)) for _ in range(3)]
    return _case("wpc2", C, 48, n, _variants(rng, C, base, 5, keep=(C - 1,)), (7, 6))


def _grid_capped():
    C, n = 300000, 64
    rng = np.random.RandomState(105)
    ids = 262145 + rng.permutation(C - 1 - 262145)[:4 * n]      # four disjoint rows, all behind the grid's first iteration
    ids[0], ids[n] = 262144, C - 1
    rows = ids.reshape(4, n)
    assert len(set(ids.tolist())) == 4 * n and ids.min() == 262144
    return _case("grid-capped", C, 2, n, rows, (7, 6), pool=True)


def _lds_cap():
    C, n = 524032, 257
    rng = np.random.RandomState(106)
    run0 = (feed_words(C) - 1) // feed_per(C) * feed_per(C) * 32          # first id of the last thread's run
    rows = [_row(rng, C, n, must=(0, C - 1, run0 + int(rng.randint(0, 64)))) for _ in range(3)]
    return _case("lds-cap", C, 2, n, rows, (7, 6), pool=True)


def _n_is_1():
    return _case("n-is-1", 8219, 4, 1, [[8218], [0], [4100]], (7, 6))


def n_below_active():
    """For the all-four-waves handle (active_columns = 300) after its run: lists of 260, still two passes and two record blocks."""
    C, n = 24700, 260
    rng = np.random.RandomState(107)
    rows = [_spread(rng, C, n, must=(0, C - 1)) for _ in range(5)]
    return _case("n-below-active", C, 2, n, rows, (7, 6))


CASES = [f() for f in (_wave1_one_thread, _all_four_waves, _per8_cut_run, _wpc2, _grid_capped, _lds_cap, _n_is_1)]
CASE_IDS = [c.name for c in CASES]
BY_NAME = {c.name: c for c in CASES}
LDS_CAP_C = 524032                                              # the largest column_dim htm_tm_run takes; one more is refused


# ------------------------------------------------------------------------------------------ bad rows

def _bad(name, C, n, seed, spoil, avoid=()):
    """Three rows, the middle one spoilt by `spoil(row)` (in place): (name, C, n, rows, index of the bad row)."""
    rng = np.random.RandomState(seed)
    rows = np.stack([_row(rng, C, n, must=(C - 1,), avoid=avoid) for _ in range(3)])       # (C - 1: a bit in the last owning thread)
    spoil(rows[1])
    assert not feed_contract(rows[0], C, n)[1] and feed_contract(rows[1], C, n)[1] and not feed_contract(rows[2], C, n)[1], name
    return SimpleNamespace(name=name, C=C, K=4 if C < 20000 else 2, n=n, rows=rows.astype(np.int32), bad_row=1, steps=7,
                           segment_capacity=2 * n * 24, segment_slots=128)


def _set(at, value):
    def spoil(row):
        row[at] = value
    return spoil


def _copy(src, dst):
    def spoil(row):
        row[dst] = row[src]
    return spoil


def _fill(values):
    def spoil(row):
        row[:] = np.resize(np.asarray(values, dtype=np.int64), len(row)).astype(np.int32)
    return spoil


def _twice(a, b, value):
    def spoil(row):
        row[a] = row[b] = value
    return spoil


BAD_C, BAD_N = 8219, 300
BAD_ROWS = [
    _bad("twice-two-passes", BAD_C, BAD_N, 201, _copy(17, 17 + 256)),            # thread 17 meets it in passes 0 and 1
    _bad("twice-two-waves", BAD_C, BAD_N, 202, _copy(5, 70)),                    # waves 0 and 1 of pass 0
    _bad("pad-range", BAD_C, BAD_N, 203, _set(9, 8230)),                         # C <= id < 32 * words = 8 320
    _bad("id-is-C", BAD_C, BAD_N, 204, _set(299, BAD_C)),
    _bad("negative", BAD_C, BAD_N, 205, _set(0, -1)),
    _bad("int32-max", BAD_C, BAD_N, 206, _set(128, INT32_MAX)),
    _bad("one-id-n-times", BAD_C, BAD_N, 207, _fill([4100])),
    _bad("all-outside", BAD_C, BAD_N, 208, _fill([BAD_C, -1, INT32_MAX, 8230, -INT32_MAX - 1, 8319, 8320])),
    _bad("twice-in-cut-run", 32865, BAD_N, 209, _twice(3, 259, 32800), avoid=(32800,)),
]
BAD_IDS = [b.name for b in BAD_ROWS]
