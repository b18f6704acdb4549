"""CPU: the lists of tests/tm_feed_cases.py.  feed_contract against independent NumPy; every case of the table against the path of
k_tm_feed it is there for, by feed_census -- a table that drifts away from its paths fails here, without a device; the bad rows
against the place they are bad at; and the host-side check of the same rows (check_lists)."""

import os

import numpy as np
import pytest

import tm_feed_cases as F

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _census(case, K=None):
    return [F.feed_census(row, case.C, case.n, case.K if K is None else K) for row in case.rows]


def test_contract_equals_independent_numpy():
    """A few hundred random rows, good and bad, column_dim 1 included: np.unique for what is kept, np.setdiff1d for what is added."""
    rng = np.random.RandomState(7)
    seen_good = seen_bad = 0
    for trial in range(400):
        C = 1 if trial < 3 else int(rng.choice([2, 31, 32, 33, 100, 257, 1000]))
        n = int(rng.randint(1, min(C, 80) + 1))
        if trial % 3 == 0:
            row = rng.choice(C, n, replace=False)
        else:                                                   # repeats, ids either side of the range, the extremes of int32
            row = rng.randint(-3, C + 40, n).astype(np.int64)
            if trial % 5 == 0:
                row[rng.randint(n)] = rng.choice([F.INT32_MAX, -F.INT32_MAX - 1, C, -1])
        got, bad = F.feed_contract(row, C, n)
        kept = np.unique(row[(row >= 0) & (row < C)])
        want_bad = len(kept) != n
        want = np.sort(np.r_[kept, np.setdiff1d(np.arange(C), kept)[:n - len(kept)]])
        assert bad == want_bad and got.dtype == np.int32 and np.array_equal(got, want), (trial, C, n)
        assert len(got) == n and (np.diff(got) > 0).all() and got[0] >= 0 and got[-1] < C
        if not want_bad:
            assert np.array_equal(got, np.sort(row))
        seen_good += not want_bad
        seen_bad += want_bad
    assert seen_good > 100 and seen_bad > 100
    assert np.array_equal(F.feed_contract([0], 1, 1)[0], [0]) and F.feed_contract([0], 1, 1)[1] is False
    assert np.array_equal(F.feed_contract([1], 1, 1)[0], [0]) and F.feed_contract([1], 1, 1)[1] is True
    assert np.array_equal(F.feed_contract([5, 5, 5], 9, 3)[0], [0, 1, 5])
    assert np.array_equal(F.feed_contract([9, -1, 40], 9, 3)[0], [0, 1, 2])


def test_formulas_at_the_sizes_the_kernel_documents():
    """words, per, LDS bytes and clearing iterations at the boundaries DESIGN.md section 16 and htm_tm_feed.h name."""
    assert [F.feed_words(C) for C in (1, 128, 129, 1024, 8219, 24700, 32865, 524032, 524033)] == [4, 4, 8, 32, 260, 772, 1028, 16376, 16380]
    assert [F.feed_per(C) for C in (1, 1024, 32768, 32769, 65536, 65537, 524032)] == [4, 4, 4, 8, 8, 12, 64]
    assert F.feed_lds_bytes(524032) == 65536 == F.LDS_MAX and F.feed_lds_bytes(524033) > F.LDS_MAX and F.feed_lds_bytes(1024) == 160
    assert F.LDS_CAP_C == max(C for C in range(523900, 524200) if F.feed_lds_bytes(C) <= F.LDS_MAX)
    assert [F.clear_iterations(C, 4) for C in (1, 256, 8219, 262144, 262145, 300000, 524032)] == [1, 1, 1, 1, 2, 2, 2]
    assert [F.clear_iterations(C, K) for C, K in ((8219, 32), (8219, 33), (8219, 48), (300000, 64))] == [1, 2, 2, 3]
    assert [F.entry_place(i) for i in (0, 63, 64, 255, 256, 273, 599)] == [(0, 0, 0), (0, 63, 0), (0, 64, 1), (0, 255, 3), (1, 0, 0), (1, 17, 0), (2, 87, 1)]
    one = F.feed_census([8218], 8219, 1)
    assert one.threads.tolist() == [64] and one.waves == [1] and one.wave_totals == [0, 1, 0, 0] and one.bitmap_threads == 65


def test_every_case_reaches_its_path():
    by = F.BY_NAME
    assert F.CASE_IDS == ["wave1-one-thread", "all-four-waves", "per8-cut-run", "wpc2", "grid-capped", "lds-cap", "n-is-1"]
    for case in F.CASES + [F.n_below_active()]:
        assert 12 <= case.steps <= 16 and case.steps % len(case.rows) and case.calls[0] % 2 == 1, case.name
        assert 2 <= case.K <= 4 or case.name == "wpc2", case.name
        assert (case.segment_capacity is not None) == (case.C >= 24700 and case.name != "n-below-active"), case.name
        for row in case.rows:
            got, bad = F.feed_contract(row, case.C, case.n)
            assert not bad and np.array_equal(got, np.sort(row)), case.name

    # owning threads in two waves: lane 0 of wave 1 owns id 8 218 alone; no second word in the last ballot of the record
    c = by["wave1-one-thread"]
    assert (c.C, c.n) == (8219, 40) and c.C % 32 == 27 and c.C % 64 <= 32
    for s, row in zip(_census(c), c.rows):
        assert 0 in row and 8218 in row
        assert s.words == 260 and s.per == 4 and s.passes == 1 and s.bitmap_threads == 65 and not s.cut_last
        assert s.waves == [0, 1] and s.threads[-1] == 64 and s.wave_totals[1] == 1 and 8218 // 32 // s.per == 64

    # all four waves, two passes; a zero wave between two that own bits; a full word
    c = by["all-four-waves"]
    cs = _census(c)
    assert (c.C, c.n) == (24700, 300) and all(s.words == 772 and s.per == 4 and s.bitmap_threads == 193 and s.passes == 2 for s in cs)
    assert [s.waves for s in cs] == [[0, 1, 2, 3], [0, 1, 2, 3], [0, 3], [0, 1, 2, 3], [0, 1, 2, 3]]
    assert F.zero_wave_between(cs[2]) and cs[2].wave_totals[1] == cs[2].wave_totals[2] == 0 and not any(F.zero_wave_between(s) for s in cs[:2])
    assert cs[3].full_words == 1 and np.array_equal(np.sort(c.rows[3])[:32], np.arange(224, 256)) and sum(s.full_words for s in cs) == 1
    assert all(min(s.wave_totals) > 0 for i, s in enumerate(cs) if i != 2)

    # per = 8, the last owning thread's run cut by `words`, three passes
    c = by["per8-cut-run"]
    for s, row in zip(_census(c), c.rows):
        assert (c.C, c.n) == (32865, 600) and s.words == 1028 and s.per == 8 and s.passes == 3 and s.bitmap_threads == 129
        assert s.cut_last and s.threads[-1] == 128 and s.waves == [0, 1, 2] and c.C - 1 in row
        assert np.sum((row >= 1024 * 32) & (row < 1028 * 32)) >= 9

    # clearing iterations beyond one: by WPC, by the grid cap
    c = by["wpc2"]
    assert (c.C, c.K, c.n) == (8219, 48, 48) and all(s.clear_iterations == 2 and s.waves == [0, 1] for s in _census(c))
    assert all(s.clear_iterations == 1 for s in _census(c, K=32))
    c = by["grid-capped"]
    assert c.C == 300000 > 262144 and c.n == 64 and all(s.clear_iterations == 2 for s in _census(c))
    assert c.rows.min() == 262144 and c.rows.max() == c.C - 1 and len(np.unique(c.rows)) == c.rows.size       # disjoint rows
    assert F.clear_iterations(262144, c.K) == 1

    # the cap: 64 words a thread, exactly 64 KiB, the last thread's run cut, two passes
    c = by["lds-cap"]
    for s, row in zip(_census(c), c.rows):
        assert (c.C, c.n) == (F.LDS_CAP_C, 257) and s.lds == 65536 and s.per == 64 and s.words == 16376 and s.passes == 2
        assert s.cut_last and s.threads[0] == 0 and s.threads[-1] == 255 and s.bitmap_threads == 256 and 0 in row and c.C - 1 in row
        assert np.sum(row // 32 // 64 == 255) >= 2 and s.clear_iterations == 2

    c = by["n-is-1"]
    assert c.rows.tolist() == [[8218], [0], [4100]] and [s.waves for s in _census(c)] == [[1], [0], [0]]

    c = F.n_below_active()
    assert (c.C, c.n) == (24700, 260) and c.n < by["all-four-waves"].n and all(s.passes == 2 and s.waves == [0, 1, 2, 3] for s in _census(c))
    assert -(-c.n // 256) == 2                                  # entries in two blocks of the record launch

    # over the table: per in {4, 8, 64}; one, two and three passes; a cut run; a full word; the cap; both kinds of second iteration
    every = [s for case in F.CASES for s in _census(case)]
    assert {s.per for s in every} >= {4, 8, 64} and {s.passes for s in every} == {1, 2, 3}
    assert any(s.cut_last for s in every) and any(not s.cut_last for s in every) and any(s.full_words for s in every)
    assert any(len(s.waves) >= 2 for s in every) and any(len(s.waves) == 4 for s in every) and any(F.zero_wave_between(s) for s in every)
    assert max(s.lds for s in every) == F.LDS_MAX


def test_every_bad_row_is_bad_where_it_says():
    by = {b.name: b for b in F.BAD_ROWS}
    assert F.BAD_IDS == ["twice-two-passes", "twice-two-waves", "pad-range", "id-is-C", "negative", "int32-max", "one-id-n-times",
                         "all-outside", "twice-in-cut-run"]
    for b in F.BAD_ROWS:
        assert b.rows.dtype == np.int32 and b.rows.shape == (3, 300) and b.C == (32865 if b.name == "twice-in-cut-run" else 8219)
        flags = [F.feed_contract(r, b.C, b.n)[1] for r in b.rows]
        assert flags == [False, True, False], b.name
        s = F.feed_census(b.rows[1], b.C, b.n)
        assert s.bad and s.passes == 2, b.name
        assert len(s.waves) >= 2 or b.name in ("one-id-n-times", "all-outside"), b.name        # (the counts cross a wave)
        fixed = F.repaired(b.rows, b.C)
        assert np.array_equal(fixed[0], np.sort(b.rows[0])) and np.array_equal(fixed[2], np.sort(b.rows[2]))
    row = by["twice-two-passes"].rows[1]
    assert row[17] == row[273] and F.entry_place(17)[1] == F.entry_place(273)[1] and F.entry_place(17)[0] != F.entry_place(273)[0]
    row = by["twice-two-waves"].rows[1]
    assert row[5] == row[70] and F.entry_place(5)[0] == F.entry_place(70)[0] == 0 and (F.entry_place(5)[2], F.entry_place(70)[2]) == (0, 1)
    s = F.feed_census(by["pad-range"].rows[1], 8219, 300)
    assert s.pad_ids.tolist() == [8230] and 8219 <= 8230 < 32 * s.words == 8320
    assert by["id-is-C"].rows[1].max() == 8219 and by["negative"].rows[1].min() == -1 and by["int32-max"].rows[1].max() == F.INT32_MAX
    for name in ("twice-two-passes", "twice-two-waves", "pad-range", "id-is-C", "negative", "int32-max", "twice-in-cut-run"):
        b = by[name]                                            # one entry lost: what was validly listed, and the lowest unlisted column
        row = b.rows[1].astype(np.int64)
        kept = np.unique(row[(row >= 0) & (row < b.C)])
        assert len(kept) == 299
        assert np.array_equal(F.repaired(b.rows, b.C)[1], np.sort(np.r_[kept, np.setdiff1d(np.arange(b.C), kept)[0]])), name
    assert np.array_equal(F.repaired(by["one-id-n-times"].rows, 8219)[1], np.r_[np.arange(299), 4100])
    assert np.array_equal(F.repaired(by["all-outside"].rows, 8219)[1], np.arange(300))
    assert len(F.feed_census(by["all-outside"].rows[1], 8219, 300).pad_ids) > 0
    b = by["twice-in-cut-run"]
    s = F.feed_census(b.rows[1], b.C, b.n)
    assert b.rows[1][3] == b.rows[1][259] == 32800 and s.per == 8 and 32800 // 32 // s.per == 128 and 128 * s.per + s.per > s.words
    assert F.entry_place(3)[0] != F.entry_place(259)[0]


@pytest.fixture(scope="module")
def built():
    import __graft_entry__ as ge
    ge.build()


def test_check_lists_refuses_the_bad_rows(built):
    """The host-side check of a bank refuses what the device repairs, with its documented messages."""
    from bithtm_amd.engine import check_lists
    by = {b.name: b for b in F.BAD_ROWS}
    for name, what in (("pad-range", r"row 1 has a column id outside \[0, 8219\)"), ("id-is-C", r"row 1 has a column id outside \[0, 8219\)"),
                       ("negative", r"row 1 has a column id outside \[0, 8219\)"), ("int32-max", r"row 1 has a column id outside"),
                       ("all-outside", r"row 1 has a column id outside"), ("twice-two-passes", "row 1 lists a column twice"),
                       ("twice-two-waves", "row 1 lists a column twice"), ("one-id-n-times", "row 1 lists a column twice"),
                       ("twice-in-cut-run", "row 1 lists a column twice")):
        b = by[name]
        with pytest.raises(ValueError, match=what):
            check_lists(b.rows, b.C)
        assert np.array_equal(check_lists(b.rows[[0, 2]], b.C), b.rows[[0, 2]])
    for case in F.CASES:
        assert np.array_equal(check_lists(case.rows, case.C), case.rows)
