"""GPU: the fused step (htm_step / htm_run) on the hand-built pools of tests/pool_geometry_cases.py -- every size-dependent form of
the allocation, the classification, the sparse clear and the scan, under every launch schedule.

Every case loads its permanence, duty cycle and exported Temporal Memory state into a device model (hip_impl.make_htm,
Engine.import_tm_state) and takes the case's steps, once host-fed in lock step with the oracle and once as one htm.run over the
case's pattern bank (hipGraph replay), compared at the end.  tests/test_pool_geometry_cpu.py pins that oracle to the unmodified
reference and proves that each case reaches its path.  Compared EXACTLY after every lock-step step: every field of
hip_impl.compare_with_oracle, the whole segment_potential, max_jittered_potential by its bits, the store (owners, counts, segcount,
sorted synapses, permanence bits), htm_info's allocation counters against the oracle's last_update, the recyclable counts
(Engine.read_recyclable_counts) against a recount from the oracle's seg_nsyn -- read before the next step is enqueued, so that a
stale count is an assertion here and not something the next allocation acts on -- and check_capacity() clean.  No case, step or
schedule is skipped; nothing is repeated to catch a race; no mutated kernel is run."""

import numpy as np
import pytest

import pool_geometry_cases as pg
from pool_geometry_device import compare_step, device_model

pytestmark = pytest.mark.gpu

SCHEDULES = {"two-launch": {}, "three-launch": {"BITHTM_LEAN": "1"}, "four-launch": {"BITHTM_LEAN": "0"}, "scan-large": {"BITHTM_SCAN_LARGE": "1"}}
WORD_FORM = {"classify-words": {"BITHTM_CLASSIFY_WORDS_ABOVE": "0"},
             "classify-words-four-launch": {"BITHTM_CLASSIFY_WORDS_ABOVE": "0", "BITHTM_LEAN": "0"}}     # (n_cls = 384: the by_xcd mapping)
MODES = ("host-fed", "batched")


def run_case(name, env, mode, monkeypatch):
    case, tr = pg.build(name), pg.oracle_trace(name)
    for key, value in env.items():
        monkeypatch.setenv(key, value)
    htm, eng = device_model(case)
    if "BITHTM_SCAN_LARGE" in env:
        assert eng.run_plan(len(case.steps))["scan_large"]
    if mode == "host-fed":
        for r, j in zip(tr, case.steps):
            h_sp, h_tm = htm.process(case.patterns[j], learning=True)
            compare_step(case, eng, r, h_sp, h_tm, (name, mode, r.t))
    else:
        assert eng.run_plan(len(case.steps))["hip_graph"], "the batched run would launch eagerly"
        htm.run(case.bank(), len(case.steps), learning=True)
        assert eng.steps == 1 + len(case.steps)
        sp_state = type(htm.spatial_pooler).State(eng, eng.steps)
        compare_step(case, eng, tr[-1], sp_state, htm.temporal_memory.last_state, (name, mode, "end"))
    return htm, eng


def _params(names, schedules):
    return [pytest.param(n, env, mode, id=f"{n}-{sid}-{mode}") for n in names for sid, env in schedules.items() for mode in MODES]


ALLOC = [n for n in pg.SMALL if n.startswith("alloc_")]


@pytest.mark.parametrize("name,env,mode", _params(ALLOC, SCHEDULES))
def test_allocation_takes_the_lowest_recyclable_ids_and_keeps_its_counts(name, env, mode, monkeypatch):
    """role_mid, block 0 (projections.py:80-94, 275-281): recycle the lowest-id rows with fewer synapses than the matching
    threshold, append the rest, bind in ascending cell order.
      * a block's count read one entry off, or a block boundary handled as `>` for `>=` (dead rows at 0, 1023, 1024, 2047, S - 1;
        S = 1 and 1 023 mod 1 024): another id is bound -- seg_cell, segcount and the synapses of rows 0 / 1023 / 1024 differ at
        step 1, or info.recycled_segments != 3;
      * the cut `carry + ex < n_un` / `rank < n_r` off by one inside the block of 20 (alloc_exact_cut_*): one row too many or too
        few is recycled -- info.recycled / appended differ, S differs, the 20th dead row's owner differs;
      * needed blocks beyond slot NEED_LDS = 128 read from s_words instead of d.recyc_need (alloc_many_blocks, 151 needed
        blocks): the recycled rows of the later blocks keep their old owner and synapses, the work list holds unwritten entries;
      * a count left unchanged at binding, or fresh ids not added when grown < match_thr (alloc_stay_dead), or not changed
        when a punished row crosses the threshold (alloc_after_death): the recyclable counts differ from the recount after that
        very step; one step later n_r exceeds the rows that exist (S and the store differ) or a dead row is passed over
        (alloc_after_death: step 2 must recycle rows 10..15 first)."""
    run_case(name, env, mode, monkeypatch)


@pytest.mark.parametrize("name,env,mode", _params(["classify_words"], {**SCHEDULES, **WORD_FORM}))
def test_classification_by_rows_and_by_words_finds_every_matching_row_once(name, env, mode, monkeypatch):
    """role_mid, blocks 1..n_cls (projections.py:264-269), the one-row-per-thread form and the word form (forced at any size by
    BITHTM_CLASSIFY_WORDS_ABOVE=0; with 384 blocks through the by_xcd mapping w = ((x + 8 * (u >> 5)) << 5) + (u & 31)).  The matching
    rows are 40 fully set words, single rows at bit 0 and bit 31 of words in every residue class mod 8 of their line, and the last,
    partial word (S = 70 003); each is one of: learns as an active segment, learns as the best match of a bursting column,
    matches without being the best, is punished, none of these.
      * a word mapped to no block: its learning rows keep their permanences and grow nothing, its punished rows keep theirs --
        syn_perm_bits / syn_presyn of those rows differ after step 1;
      * a word mapped to two blocks: the row is updated twice (permanence bits), or listed twice (work_items, a capacity flag);
      * bit 31 or the partial last word dropped: rows 25247.., 70001, 70002 differ; a row at or above S classified: S or a
        capacity flag differs;
      * `best` taken with the wrong cell's maximum, or an unpredicted test on the wrong word: a `not_best` / `other` row learns."""
    run_case(name, env, mode, monkeypatch)


@pytest.mark.parametrize("name,env,mode", _params(["scan_rows_k32", "scan_rows_k48"], SCHEDULES))
def test_scan_of_rows_of_every_length_at_every_threshold(name, env, mode, monkeypatch):
    """k_tm_scan / k_tm_scan_wide / the streaming form (projections.py:245-255), and the SELF form of the learning role in the schedules
    where it shares a launch with the scan; segment_slots 64, cell_dim 32 and 48.  Step 1 scans the crafted rows as imported, none of
    them on the work list, against every cell of the source columns (the plain forms).  At steps 2 and 3 the same cells are active again
    while the rows learn or are punished: the wave that rewrites a row scans it (SELF), with potentials 64, M, M - 1, activations A,
    A - 1 and permanences the update puts exactly on f32(threshold) and one ulp below (the case's precondition asserts all of these
    among the listed rows).
      * the one-chunk path taken for a row of 33 synapses, or the loop for a lane's third and later hits ending early (64 synapses
        on active cells: eight hits per lane): segment_potential of that row is short, it may drop out of matching_segment;
      * a connected flag at `> threshold` for `>=` (permanence == f32(0.5)) or at `>=` one ulp below -- in the stored flag of the
        plain forms or in the permanence the SELF form has just computed: matching_segment_activation and matching_segment_active
        of those rows differ, then prediction bits and the next step's winners;
      * `>` for `>=` at the matching or the activation threshold: rows of potential 7 / activation 9 differ, rows one short must not
        (SELF: the punished row that drops from 7 to 6 must leave matching_segment and enter the recyclable counts);
      * the second cell word of a 48-cell column ignored: potentials of rows on cells 32..47 are short;
      * a row on a 16- or 64-row boundary handled by two waves or none, or a listed row scanned by the plain form as well (SEG_BUSY
        ignored): its potential is doubled or zero, max_jittered_potential of its cell differs."""
    run_case(name, env, mode, monkeypatch)


@pytest.mark.parametrize("name,env", [pytest.param(n, env, id=f"{n}-{sid}") for n in pg.LARGE
                                      for sid, env in (("two-launch", {}), ("four-launch", {"BITHTM_LEAN": "0"}))])
def test_pool_of_2p20_rows_above_every_threshold(name, env, monkeypatch):
    """S = 2^20 + 3 000 on 4 096 x 32 cells, four host-fed steps: the word forms of the classification and of the sparse clear (each
    with its own by_xcd mapping), the streaming scan, two second-level recyclable counts.
      * a stale per-cell maximum surviving a step (a word of match bits the sparse clear maps to no wave): max_jittered_potential
        differs at the cells the case's precondition counts (non-zero before, zero after), then `best` and the winners;
      * the first 2^20 range not skipped although its count is 0, or skipped although it holds dead rows (`both`): other ids are
        recycled -- info.recycled, seg_cell and the counts differ; recyc_cnt2 not kept with recyc_cnt: the counts' second part differs;
      * a matching word near or across 2^20 classified by no block or two: as in the classification test.
    Rests on the oracle alone (tests/pool_geometry_cases.py says why).  The full store (270 MB each way) is compared after the
    first and the last step, everything else after every step."""
    try:
        case, tr = pg.build(name), pg.oracle_trace(name)
        for key, value in env.items():
            monkeypatch.setenv(key, value)
        htm, eng = device_model(case)
        assert eng.run_plan(4)["scan_large"]
        for r, j in zip(tr, case.steps):
            h_sp, h_tm = htm.process(case.patterns[j], learning=True)
            compare_step(case, eng, r, h_sp, h_tm, (name, r.t))
        del htm, eng
    finally:
        if env:                                     # (the last schedule of the case: its gigabyte goes)
            pg.release(name)


def test_a_smaller_pool_imported_over_a_larger_one_starts_with_clean_counts(monkeypatch):
    """Regression (the segment pool): htm_import_commit recounted only the 1 024-blocks below the new segment count, so the
    count of a block the earlier, larger pool had dead rows in survived the import.  A handle first holds alloc_block_edges_1023's
    pool extended by 60 dead rows (ids 3 071..3 130: 59 of them in block 3), then imports the case's own state (S = 3 071, three
    blocks).  Step 2 appends ids 3 071..3 073 into block 3: with the stale count the recyclable counts read 59 for that block where
    the recount says 0, and the next allocation that looks at the block binds rows that do not exist (work-list entries never
    written).  Every compared value of the case must be the oracle's all the same."""
    name = "alloc_block_edges_1023"
    case = pg.build(name)
    st, extra = dict(case.state0), 60
    S = int(st["S"])
    st["S"] = np.int64(S + extra)
    st["seg_cell"] = np.r_[st["seg_cell"], np.full(extra, case.quiet[3], dtype=np.int32)]
    st["seg_nsyn"] = np.r_[st["seg_nsyn"], np.zeros(extra, dtype=np.int32)]
    st["presyn"] = np.concatenate([st["presyn"], np.full((extra, st["presyn"].shape[1]), -1, dtype=np.int32)])
    st["perm"] = np.concatenate([st["perm"], np.full((extra, st["perm"].shape[1]), -1.0, dtype=np.float32)])
    st["segcount"] = st["segcount"].copy()
    st["segcount"][case.quiet[3]] += extra
    st["segment_potential"] = np.r_[st["segment_potential"], np.zeros(extra, dtype=np.int64)]
    assert S + extra <= case.capacity
    tr = pg.oracle_trace(name)
    htm, eng = device_model(case, state=st)
    cnt1, _ = eng.read_recyclable_counts()
    assert cnt1[3] == 59 and cnt1[2] == 2
    eng.import_tm_state(case.state0)
    cnt1, _ = eng.read_recyclable_counts()
    assert len(cnt1) == 3
    for r, j in zip(tr, case.steps):
        h_sp, h_tm = htm.process(case.patterns[j], learning=True)
        compare_step(case, eng, r, h_sp, h_tm, (name, "re-import", r.t))


def test_the_recyclable_counts_are_read_only():
    """htm_write refuses HTM_F_RECYCLABLE_COUNTS (HTM_ERR_ARGUMENT, nothing written); a read with too small a buffer is refused, and
    so is a read on a column-sharded handle (HTM_ERR_STATE: it keeps a dead bit per id instead)."""
    from bithtm_amd import _lib as L
    from bithtm_amd.engine import HtmError
    case = pg.build("alloc_block_edges_1")
    htm, eng = device_model(case)
    before = eng.read_recyclable_counts()
    with pytest.raises(HtmError, match="not writable"):
        eng.write(L.F_RECYCLABLE_COUNTS, np.zeros(5, np.int32), np.int32)
    with pytest.raises(HtmError, match="too small"):
        eng.read(L.F_RECYCLABLE_COUNTS, np.int32, 2)
    after = eng.read_recyclable_counts()
    from bithtm_amd.distributed import LocalGroup
    group = LocalGroup(2, 64, 1024, 8, permanence=np.zeros((1024, 64)))
    with pytest.raises(HtmError, match="column-sharded"):
        group.engines[0].read(L.F_RECYCLABLE_COUNTS, np.int32, 8)
    want = pg.recount(case.state0["seg_nsyn"], case.params.segment_matching_threshold)
    assert all(np.array_equal(a, b) and np.array_equal(a, w) for a, b, w in zip(before, after, want)) and len(after[0]) == 4 and len(after[1]) == 1
