"""The hand-built pools of tests/pool_geometry_cases.py without a device and without the reference: every case's precondition --
the proof, on the oracle alone, that it reaches the path it is named for -- and, for every case but natural_2p20_*, the oracle's
store and States after every step against what the UNMODIFIED reference computed from the same crafted store
(tests/golden/pool_geometry.npz, recorded by tests/golden/generate_pool_geometry.py).

natural_2p20_* (2^20 + 3 000 rows) are not recorded: they rest on the oracle alone, whose allocation rule -- lowest recyclable ids
first, then append, bind in ascending cell order -- the small allocation cases pin here against the reference, id by id."""

import os
import sys

import numpy as np
import pytest

import pool_geometry_cases as pg

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden"))
import generate_pool_geometry as gen  # noqa: E402  (input_digest / trace_digests: pure NumPy; the reference is imported by main() only)

FIXTURE = np.load(gen.PATH)
RECORDED = [str(n) for n in FIXTURE["cases"]]

# the builders are deterministic: a digest of everything a replay starts from -- permanence, duty cycle, the exported state, the
# patterns, the step list, the shape and the parameters (generate_pool_geometry.input_digest); the fixture holds the small cases' too
INPUTS = {
    "alloc_block_edges_1": 17742667783118506434,
    "alloc_block_edges_1023": 17546756174130752786,
    "alloc_exact_cut_minus1": 14315509633904718430,
    "alloc_exact_cut_equal": 14395492933862402825,
    "alloc_exact_cut_plus1": 12734529345485301796,
    "alloc_many_blocks": 11467266902707057538,
    "alloc_stay_dead": 12344223554991007418,
    "alloc_after_death": 8998608850983979390,
    "classify_words": 17159195136227305264,
    "scan_rows_k32": 805343264049441843,
    "scan_rows_k48": 12237135966112356665,
    "natural_2p20_hi": 17436854379185125639,
    "natural_2p20_both": 15246624531344168224,
}


def test_every_small_case_is_in_the_fixture():
    assert RECORDED == pg.SMALL and len(RECORDED) == 11 and list(INPUTS) == pg.CASE_NAMES
    assert pg.CASE_NAMES == pg.SMALL + pg.LARGE


@pytest.mark.parametrize("name", RECORDED)
def test_the_case_is_the_one_that_was_recorded(name):
    case = pg.build(name)
    assert int(gen.input_digest(case)) == INPUTS[name] == int(FIXTURE[f"{name}/inputs"])
    assert np.array_equal(FIXTURE[f"{name}/steps"], case.steps)


@pytest.mark.parametrize("name", RECORDED)
def test_oracle_gives_every_recorded_value(name):
    """After every step: seg_cell, seg_nsyn, segcount, the canonical synapses (permanences by their bits) and every field of the
    Spatial Pooler's and the Temporal Memory's State -- exactly the reference's; the ids the allocation recycled and appended."""
    tr = pg.oracle_trace(name)
    names, dig = gen.trace_digests(tr)
    assert names == [str(n) for n in FIXTURE["field_names"]]
    want = FIXTURE[f"{name}/digests"]
    assert dig.shape == want.shape
    bad = np.argwhere(dig != want)
    assert len(bad) == 0, [(int(i) + 1, names[j]) for i, j in bad[:8]]
    assert tr[-1].S == int(FIXTURE[f"{name}/segments"])
    for r in tr:
        assert np.array_equal(r.last.recycled, FIXTURE[f"{name}/step{r.t}/recycled"]) and np.array_equal(r.last.fresh, FIXTURE[f"{name}/step{r.t}/fresh"])


@pytest.mark.parametrize("name", pg.SMALL)
def test_the_case_reaches_the_path_it_is_named_for(name):
    pg.check_preconditions(name)


@pytest.mark.parametrize("name", pg.LARGE)
def test_the_natural_size_case_reaches_its_paths_and_is_deterministic(name):
    try:
        pg.check_preconditions(name)
        assert int(gen.input_digest(pg.build(name))) == INPUTS[name]
    finally:
        pg.release(name)


def test_recount_counts_rows_below_the_matching_threshold_per_1024_and_per_2p20_ids():
    nsyn = np.full((1 << 20) + 5, 9)
    nsyn[[0, 1023, 1024, (1 << 20) - 1, 1 << 20]] = [0, 3, 2, 1, 0]
    c1, c2 = pg.recount(nsyn, 3)
    assert len(c1) == 1025 and len(c2) == 2 and c1[0] == 1 and c1[1] == 1 and c1[1023] == 1 and c1[1024] == 1 and c1.sum() == 4
    assert c2.tolist() == [3, 1]
