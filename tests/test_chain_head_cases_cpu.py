"""CPU: the cases of tests/chain_head_cases.py reach the paths they are for (the oracle alone; the GPU tests compare with the same
records)."""

import numpy as np
import pytest

import chain_head_cases as ch


@pytest.mark.parametrize("name", list(ch.ROWS))
def test_row_cases_move_mask_bits_both_ways(name):
    """The winner rows' update is what the cases are about: over the steps connected bits are gained AND lost (an increment or a
    threshold read wrongly changes which), in columns that won, and the widths are the ones the row loop treats differently."""
    case, (tr, ora) = ch.build(name), ch.oracle_trace(name)
    thr = case.sp_params.permanence_threshold
    before, after = case.permanence >= thr, ora.spatial_pooler.permanence >= thr
    assert (after & ~before).sum() > 20 and (before & ~after).sum() > 20
    assert case.C == 512 and len(tr) == 30 and case.I in (100, 130, 1024)
    assert sum(len(r.tm.winner_cell[0]) for r in tr) > 0 and tr[-1].S > 0
    if name == "rows_i130_thr":
        p = case.sp_params
        assert p.permanence_threshold > 0 and p.permanence_increment != 2 * p.permanence_decrement
