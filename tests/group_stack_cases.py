"""Shared by tests/test_group_stack_cpu.py and tests/test_hip_group_stack.py: the cases of htm_group_pack_columns and
htm_group_pool_columns.  A group case is ONE call over several members: tests/pooling_cases.py's cases of equal geometry (C, k, the
link, windows, bank_rows -- a group call takes them once for all members), each member a pooling case named with the path it
reaches, and the contract of the call is pooling_cases' NumPy statement (and stack_fixture.pack_columns) member by member.  Not
collected by pytest."""

from types import SimpleNamespace

import numpy as np

import pooling_cases as pc
import stack_fixture as sf

TRIP = pc.TRIP


def full_row(c, r):
    """The first window's row holds union_bits bits, cut out of more positive columns than that."""
    rows = np.unpackbits(r.bank.view(np.uint8), axis=1, bitorder="little")
    return c.link.union_bits < (r.snapshots[0] > 0).sum() and rows[c.first_row].sum() == c.link.union_bits


def no_tie(c, r):
    """The cut of the last snapshot falls between two values: every column at the cut wins."""
    cut, want, ties = pc.cut_of(r.snapshots[-1], c.link.union_bits)
    return cut > 0 and want == ties >= 2


def clean(c, r):
    return not r.bad and r.bank.any()


def no_reset(c, r):
    return c.resets is None and c.persistence.any() and (r.snapshots[0] >= 8).any()      # (the preset state lives on: nothing cleared it)


def unrotated(c, r):
    return c.first_row == 0 and c.bank_rows > c.windows


def wrapped(c, r):
    return c.first_row + c.windows > c.bank_rows and c.first_row == c.bank_rows - 1


def three_batches(c, r):
    return c.batch_windows is not None and -(-c.windows // c.batch_windows) == 3 and r.snapshots[c.batch_windows - 1].any()


def _tie_free_case():
    """pooling_cases._tie_case's geometry and union_bits (6 above the cut + 3), with exactly three columns at the cut."""
    C, k = 2 * TRIP + 37, 8
    P = np.zeros(C, dtype=np.uint8)
    P[[1, 77, 300, 4097, 8200, C - 1]], P[[2 * TRIP - 3, 2 * TRIP, 2 * TRIP + 2]] = 12, 6
    lists = np.array([[2, 9, 500, 900, 4100, 4200, 8000, 8100]])
    return pc.case("no tie at the cut", C, k, 1, 1, no_tie, union_bits=9, lists=lists, colpred=np.zeros((1, C), bool), persistence=P)


def _clean_like(bad, name, seed, first_row):
    lists, colpred = pc.stream(bad.C, bad.k, bad.link.stride * bad.windows, seed)
    return pc.case(name, bad.C, bad.k, bad.link.stride, bad.windows, clean, lists=lists, colpred=colpred, bank_rows=bad.bank_rows, first_row=first_row)


def group(name, members, batch_windows=None):
    c0 = members[0]
    for c in members:
        assert (c.C, c.k, c.link, c.windows, c.bank_rows, c.calls) == (c0.C, c0.k, c0.link, c0.windows, c0.bank_rows, [c0.windows]), (name, c.name)
    return SimpleNamespace(name=name, members=members, batch_windows=batch_windows, C=c0.C, k=c0.k, link=c0.link, windows=c0.windows, bank_rows=c0.bank_rows)


def groups():
    by_name = {c.name: c for c in pc.cases()}
    short = dict(union_bits=290, decay=3, ceiling=9)
    tie = by_name["ties across a trip's boundary"]
    assert tie.link.union_bits == 9
    bad = by_name["an id outside the range"]
    held = dict(persistence=np.full(300, 9), prev=np.ones(300, bool))
    out = [
        group("a short row beside a full one", [
            by_name["a short row"],
            pc.case("a full row", 300, 20, 1, 4, full_row, persistence=np.full(300, 9), **short)]),
        group("a tie at the cut across a trip boundary beside none", [tie, _tie_free_case()]),
        group("a bad id in one member only", [_clean_like(bad, "a clean member in front", 11, 0), bad, _clean_like(bad, "a clean member behind", 12, 4)]),
        group("reset bits for one member and NULL for another", [
            by_name["a reset at window 0"],
            pc.case("no reset bits", 300, 20, 2, 4, no_reset, **held)]),
        group("different first_rows", [
            by_name["first_row != 0 with bank_rows > n_rows"],
            pc.case("first_row 0", 1000, 20, 1, 5, unrotated, bank_rows=7, first_row=0, seed=3),
            pc.case("the last first_row", 1000, 20, 1, 5, wrapped, bank_rows=7, first_row=6, seed=4)]),
        group("three batches", [pc.case(f"three batches, member {i}", 257, 16, 2, 9, three_batches, batch_windows=3, seed=20 + i, first_row=i) for i in range(3)],
              batch_windows=3),
    ]
    assert len({g.name for g in out}) == len(out)
    return out


def replay(g):
    """The contract of htm_group_pool_columns over a group case: pooling_cases.replay member by member."""
    return [pc.replay(c) for c in g.members]


def replay_pack(g):
    """The contract of htm_group_pack_columns over the group case's lists at the link's stride: per member
    SimpleNamespace(bank, before, bad) (stack_fixture.pack_columns)."""
    out = []
    for i, c in enumerate(g.members):
        W = pc.bank_words(c.C)
        before = np.random.RandomState(c.C + c.windows + i).randint(0, 2 ** 32, size=(c.bank_rows, W), dtype=np.uint64).astype(np.uint32)
        bank = before.copy()
        bad = bool(sf.pack_columns(c.lists.astype(np.int64), c.C, c.link.stride, bank, c.first_row))
        out.append(SimpleNamespace(bank=bank, before=before, bad=bad))
    return out
