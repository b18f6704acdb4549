"""GPU: the winner rows' update (role_sp_row: DenseProjection.update, projections.py:23-24, fused with the rebuild of the row's connected
mask) with its two increments and its threshold held in registers -- in the two-launch schedule's first launch (htm.run: the rows
that also count their column's coming overlap, and the plain rows of a call's last step) and in the host-fed step (process()).
Cases and comparison: tests/chain_head_cases.py (input widths 100, 130 and 1 024 on 512 columns; one case with a threshold above
zero and increments that are not 2 : 1); 30 learning steps each, compared with the oracle bit for bit.
  * an increment taken for the other (on for off), or the threshold for an increment: the permanences differ after the first step,
    the mask and the next step's overlaps and active columns with them;
  * constants read per element but the tail mishandled (elements at or past I changed, or the padded tail of 130 = 128 + 2 skipped):
    SP permanence of the last elements differs, or overlaps count padding bits;
  * a threshold compared as `>` for `>=`, or in float32: mask bits of permanences on the threshold differ -- overlaps, then columns."""

import pytest

import chain_head_cases as ch

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("name", list(ch.ROWS))
def test_winner_rows_through_process(name):
    ch.host_fed(name)


@pytest.mark.parametrize("name", list(ch.ROWS))
def test_winner_rows_through_a_two_launch_run(name):
    ch.batched(name)
