"""The hand-built top-down states of tests/topdown_cases.py without a device: every builder is deterministic (a pinned digest of
its arrays), every named wrong implementation differs from the definition (tests/forecast_fixture.py's votes_of and encode) on a
case of each family named for it -- the proof that the family reaches its path --, every tie-placement row puts its cut where
its name says, and the mask-under-learning scenario, on the oracle's Spatial Pooler step, moves entries across the threshold in
both directions and exactly onto it from both sides.  tests/test_hip_topdown_geometry.py runs the same cases on the device."""

import functools

import numpy as np
import pytest

import topdown_cases as td
from forecast_fixture import encode, votes_of

SHAPES = list(zip(td.SHAPE_IDS, td.SHAPES))

PREDICTIONS = {
    "1x64x1": 13753828951646748997,
    "33x257x33": 11038946559521403561,
    "1023x1023x8": 8093614290234354706,
    "1024x1024x32": 2977625761111740640,
    "1025x1025x64": 10841423474728658183,
    "2049x3000x48": 18209273474032567037,
    "4100x1024x8": 14822573699018334410,
    "40000x64x8": 1092461162856032920,
    "333x8192x4": 10533012919583499800,
}
PERMANENCES = {
    "1x64x1/seeded-0.0": 11806891870824556760,
    "1x64x1/seeded-0.02": 13731030051982330248,
    "1x64x1/boundary-0.0": 14951958449387054884,
    "1x64x1/boundary-0.02": 8957075250175318062,
    "1x64x1/staircase": 9983716268552525502,
    "33x257x33/seeded-0.0": 6435757783974743992,
    "33x257x33/seeded-0.02": 15984250092276910983,
    "33x257x33/boundary-0.0": 3470243640423443855,
    "33x257x33/boundary-0.02": 13511957404647753544,
    "33x257x33/staircase": 16436792817113437894,
    "1023x1023x8/seeded-0.0": 1808071145602276468,
    "1023x1023x8/seeded-0.02": 1479046005881846769,
    "1023x1023x8/boundary-0.0": 1007939834025218760,
    "1023x1023x8/boundary-0.02": 10144492600379365881,
    "1023x1023x8/staircase": 4214647899694691819,
    "1024x1024x32/seeded-0.0": 4702759458259937408,
    "1024x1024x32/seeded-0.02": 12409282054353336867,
    "1024x1024x32/boundary-0.0": 16061285771413107356,
    "1024x1024x32/boundary-0.02": 7509032949474047021,
    "1024x1024x32/staircase": 11989299003607056187,
    "1025x1025x64/seeded-0.0": 5475984376739638926,
    "1025x1025x64/seeded-0.02": 5583303183000378924,
    "1025x1025x64/boundary-0.0": 18105237796779515882,
    "1025x1025x64/boundary-0.02": 13998526857234924124,
    "1025x1025x64/staircase": 10683342115676294003,
    "2049x3000x48/seeded-0.0": 13472207192972744389,
    "2049x3000x48/seeded-0.02": 13349573230079061430,
    "2049x3000x48/boundary-0.0": 15836697861727157968,
    "2049x3000x48/boundary-0.02": 15240293704570447495,
    "2049x3000x48/staircase": 4070732008798001498,
    "4100x1024x8/seeded-0.0": 15435895302249401542,
    "4100x1024x8/seeded-0.02": 7971389338365487136,
    "4100x1024x8/boundary-0.0": 14425966808060694500,
    "4100x1024x8/boundary-0.02": 15324973054400023915,
    "4100x1024x8/staircase": 6354622633699629261,
    "40000x64x8/seeded-0.0": 7484455413657695989,
    "40000x64x8/seeded-0.02": 9340163193713997952,
    "40000x64x8/boundary-0.0": 13923040677240411087,
    "40000x64x8/boundary-0.02": 13174312581658962865,
    "40000x64x8/staircase": 14764914182777449791,
    "333x8192x4/seeded-0.0": 14226528164011670184,
    "333x8192x4/seeded-0.02": 1445922951329457507,
    "333x8192x4/boundary-0.0": 622102055346743993,
    "333x8192x4/boundary-0.02": 5748356999728202945,
    "333x8192x4/staircase": 5242701357443502461,
}
ENCODER_ROWS = {
    "1x64x1": 8526640640775647809,
    "33x257x33": 10618015893959696107,
    "1023x1023x8": 9591717310665322990,
    "1024x1024x32": 15186630581827974105,
    "1025x1025x64": 17341207913192378106,
    "2049x3000x48": 1471405522893375240,
    "4100x1024x8": 11731019573971643455,
    "40000x64x8": 5373325936978956359,
    "333x8192x4": 12192338526980186196,
}
SCENARIOS = {
    "defaults-0.0": 8856002968203385332,
    "dyadic-3/128": 14977755746353374004,
}
CHAIN = 18321073264790556117


@functools.lru_cache(maxsize=2)
def _permanence(shape, family):
    return td.permanence_case(shape, family)


def test_the_shapes_are_pinned_and_every_family_exists_where_it_can():
    assert td.SHAPES == [(1, 64, 1), (33, 257, 33), (1023, 1023, 8), (1024, 1024, 32), (1025, 1025, 64), (2049, 3000, 48), (4100, 1024, 8),
                         (40000, 64, 8), (333, 8192, 4)]
    names = {sid: [n for n, _, _ in td.prediction_cases(s)] for sid, s in SHAPES}
    assert names["1x64x1"] == ["none-cell0", "only0-cell0", "only63-cell0", "chunk0-1-cell0", "chunk0-7-cell0", "chunk0-8-cell0", "chunk0-9-cell0",
                               "every-cell0", "third-cell0"]
    big = names["2049x3000x48"]
    for cols in ("none", "only0", "only1023", "only1024", "only2999", "chunk0-1024", "chunk1-1023", "chunk2-9", "every", "third"):
        for cells in ("cell0", "cell47", "cell31", "cell32", "all"):
            assert f"{cols}-{cells}" in big
    assert "chunk2-1023-all" not in big and len(big) == 23 * 5          # (the last chunk has 952 columns)
    assert "chunk0-1-cell32" in names["33x257x33"] and "chunk1-1-cell63" in names["1025x1025x64"]
    for sid, s in SHAPES:
        for name, cols, pred in td.prediction_cases(s):
            assert np.array_equal(np.flatnonzero(pred.any(axis=1)), cols), (sid, name)
            if "-cell" in name:
                assert pred.sum() == len(cols) and (not len(cols) or pred[:, int(name.rsplit("cell", 1)[1])].sum() == len(cols)), (sid, name)


@pytest.mark.parametrize("sid,shape", SHAPES, ids=td.SHAPE_IDS)
def test_every_builder_is_deterministic(sid, shape):
    assert td.digest(*[p for _, _, p in td.prediction_cases(shape)]) == PREDICTIONS[sid]
    for family in td.PERMANENCE_FAMILIES:
        thr, perm = td.permanence_case(shape, family)
        assert perm.shape == (shape[1], shape[0]) and perm.dtype == np.float64
        assert td.digest(np.float64(thr), perm) == PERMANENCES[f"{sid}/{family}"], family
    rows = td.encoder_rows(shape)
    assert td.digest(*[w for _, w, _, _ in rows], np.array([p for _, _, pairs, _ in rows for p in pairs])) == ENCODER_ROWS[sid]


def test_the_scenario_and_the_chain_rows_are_deterministic():
    for name in td.SCENARIOS:
        sc = td.learning_scenario(name)
        assert td.digest(sc.permanence, sc.bank) == SCENARIOS[name]
    assert td.digest(*td.chain_rows(td.SHAPES[-1])) == CHAIN


def test_the_boundary_family_holds_what_it_says():
    for thr in td.THRESHOLDS:
        vals = td.boundary_values(thr)
        assert np.array_equal(vals >= thr, [False, True] * 4)
        wrong = (vals.astype(np.float32) >= np.float32(thr)) & ~(vals >= thr)      # (what a float32 mask connects and must not:
        assert wrong.sum() == (2 if thr == 0.0 else 4)                             # -5e-324 becomes -0.0; 0.02 -+ 2^-40 is float32(0.02))
        assert (vals > thr).sum() == 2                                             # (`>` drops the two that sit on the threshold)
        assert np.nextafter(thr, -np.inf) in vals and thr - 2.0 ** -40 in vals and thr + 2.0 ** -40 in vals
    z = td.boundary_values(0.0)
    assert np.signbit(z[1]) and z[1] == 0.0 and z[0] == -5e-324 and z[5] == 5e-324 and not np.signbit(z[3])
    perm = td.boundary_permanence((33, 257, 33), 0.02)
    con = perm >= 0.02
    assert (con[1:, :] | con[:-1, :]).all() and (con[:, 1:] ^ con[:, :-1]).all() and (con[1:, :] ^ con[:-1, :]).all()


def _caught(fn, shape, family, match):
    """The prediction cases of (shape, family) -- those whose name holds one of `match` -- on which fn differs from votes_of."""
    thr, perm = _permanence(shape, family)
    out = []
    for name, cols, pred in td.prediction_cases(shape):
        if match is None or any(m in name for m in match):
            if not np.array_equal(fn(perm, thr, pred), votes_of(perm, thr, pred)):
                out.append(name)
                if match is None:
                    break                           # (one is enough where every case is of the family)
    return out


@pytest.mark.parametrize("mutant", list(td.VOTE_MUTANTS))
def test_every_votes_mutant_is_caught(mutant):
    """On every (shape, permanence family) pair listed for it, and there for every prediction family named for it."""
    fn, match = td.VOTE_MUTANTS[mutant]
    where = td.VOTE_MUTANT_WHERE[mutant]
    assert where
    for shape, family in where:
        caught = _caught(fn, shape, family, match)
        assert caught, (mutant, shape, family)
        for m in match or ():
            has = [n for n, _, _ in td.prediction_cases(shape) if m in n]
            assert not has or any(m in n for n in caught), (mutant, shape, family, m)


def test_the_unroll_tail_is_what_the_chunk_families_reach():
    """A chunk's list of 1, 7, 9 or 1 023 columns loses votes without its tail; one of 8 or 1 024 does not: the tail is the path."""
    fn, _ = td.VOTE_MUTANTS["unroll_tail_dropped"]
    shape = (2049, 3000, 48)
    thr, perm = _permanence(shape, "seeded-0.02")
    for name, cols, pred in td.prediction_cases(shape):
        if name.startswith("chunk") and name.endswith("-cell0"):
            n = int(name.split("-")[1])
            assert np.array_equal(fn(perm, thr, pred), votes_of(perm, thr, pred)) == (n % 8 == 0), name


def test_the_staircase_gives_the_votes_it_is_built_for():
    for sid, shape in SHAPES:
        I, C, K = shape
        want = td.staircase_want(shape)
        assert np.array_equal(votes_of(td.staircase_permanence(C, want), 0.0, np.ones((C, K), bool)), want), sid
        assert want.max() == C and (I == 1 or want.min() == 0)


def _encode_cases():
    for sid, shape in SHAPES:
        for name, want, pairs, cut in td.encoder_rows(shape):
            yield sid, shape, name, want, pairs, cut


@pytest.mark.parametrize("mutant", list(td.ENCODE_MUTANTS))
def test_every_encode_mutant_is_caught(mutant):
    fn, families = td.ENCODE_MUTANTS[mutant]
    caught = set()
    for sid, shape, name, want, pairs, cut in _encode_cases():
        for mv, mb in pairs:
            if not np.array_equal(fn(want, mv, mb), encode(want, mv, mb)):
                caught.add(name)
    for fam in families:
        assert any(n.startswith(fam) for n in caught), (mutant, fam, sorted(caught))


@pytest.mark.parametrize("mutant", list(td.WORD_MUTANTS))
def test_every_row_mutant_is_caught(mutant):
    """The raw row: against all-ones sentinels, on every row of every shape whose layout has the words the mutant gets wrong."""
    fn, _ = td.WORD_MUTANTS[mutant]
    caught = set()
    for sid, shape, name, want, pairs, cut in _encode_cases():
        if any(not np.array_equal(fn(want, mv, mb, 0xFFFFFFFF), td.encode_words(want, mv, mb)) for mv, mb in pairs):
            caught.add(sid)
    lay = {sid: td.enc_layout(s[0]) for sid, s in SHAPES}
    should = {"pad_bits_set": [sid for sid, s in SHAPES if s[0] % 128],
              "floor_chunks_per_wave": [sid for sid, s in SHAPES if lay[sid].n_chunks % 4],
              "data_chunks_only": [sid for sid, s in SHAPES if (s[0] + 63) // 64 < lay[sid].n_chunks]}[mutant]
    assert len(should) >= 4 and caught == set(should), (mutant, sorted(caught), should)


def test_the_layout_is_the_headers():
    assert [td.enc_layout(I).per_wave for I, _, _ in td.SHAPES] == [1, 1, 4, 4, 5, 9, 17, 157, 2]
    lay = td.enc_layout(33)
    assert lay.W == 4 and lay.runs == [(0, 33), (33, 33), (33, 33), (33, 33)]                # (waves 1 to 3 own no input)
    lay = td.enc_layout(333)
    assert lay.W == 12 and lay.runs == [(0, 128), (128, 256), (256, 333), (333, 333)]
    w = td.encode_words(np.r_[np.zeros(32, int), 1], 1, 0)
    assert w.tolist() == [0, 1, 0, 0]


def test_every_tie_row_puts_its_cut_where_its_name_says():
    seen = set()
    for sid, shape, name, want, pairs, cut in _encode_cases():
        if cut is None:
            continue
        seen.add(name)
        I = shape[0]
        lay = td.enc_layout(I)
        mv, mb = pairs[0]
        x = encode(want, mv, mb)
        tie = int(want[cut])
        ties = np.flatnonzero(want == tie)
        admitted = ties[x[ties]]
        assert x.sum() == mb and (want >= mv).sum() > mb, (sid, name)
        assert x[want > tie].all() and not x[want < tie].any(), (sid, name)
        assert len(ties) > len(admitted) >= 1 and len(ties) > 1, (sid, name)                 # (more than one input ties; one stays out)
        assert admitted[-1] == cut and want[cut + 1] == tie and not x[cut + 1], (sid, name)
        where = {"tie_ends_lane63": cut % 64 == 63 and cut // 64 == 0, "tie_ends_next_chunk_lane0": cut == 64,
                 "tie_ends_wave0_last": cut == lay.runs[0][1] - 1 and lay.runs[1][0] == cut + 1 < lay.runs[1][1],
                 "tie_ends_wave1_first": cut == lay.runs[1][0] and cut > 0,
                 "tie_quota_used_by_wave0": cut < lay.runs[0][1] - 1 and (I <= 64 or (want[lay.runs[1][0]:] == tie).any() or lay.runs[1][0] == I),
                 "tie_ends_before_last_input": cut == I - 2}
        assert where.get(name, True), (sid, name, cut)
        if name.startswith("tie_at_"):
            assert tie == int(name[7:]) and lay.runs[1][0] < cut < lay.runs[1][1] and want.max() == tie + 1
    assert seen == {"tie_ends_lane63", "tie_ends_next_chunk_lane0", "tie_ends_wave0_last", "tie_ends_wave1_first", "tie_quota_used_by_wave0",
                    "tie_ends_before_last_input", "tie_at_4095", "tie_at_4096", "tie_at_4097"}


def test_candidates_exactly_max_bits_and_one_more_are_among_the_pairs():
    for sid, shape in SHAPES:
        exact = over = above = last = 0
        for name, want, pairs, cut in td.encoder_rows(shape):
            for mv, mb in pairs:
                cand = int((want >= mv).sum())
                exact += mb > 0 and cand == mb
                over += mb > 0 and cand == mb + 1
                above += mv > want.max()
                last += bool(encode(want, mv, mb)[-1]) and mb > 0 and cand > mb
        assert exact and above and (over or shape[0] == 1) and (last or shape[0] == 1), sid


@pytest.mark.parametrize("name", list(td.SCENARIOS))
def test_learning_moves_the_mask_every_way_on_the_oracle(name):
    """The oracle's SP step over the scenario: the designated columns win at every step, and over the steps entries cross the
    threshold upward and downward and land exactly on it from below and from above."""
    from oracle.htm_oracle import SpatialPoolerOracle
    sc = td.learning_scenario(name)
    thr = sc.thr
    sp = SpatialPoolerOracle(sc.I, sc.C, sc.k, params=sc.params, permanence=sc.permanence.copy())
    total, per_step = {}, []
    for t in range(sc.steps):
        before = sp.permanence.copy()
        out = sp.step(sc.bank[t % len(sc.bank)], learning=True)
        assert np.array_equal(np.sort(out.active_column), sc.winners[t % len(sc.bank)]), t
        assert (out.overlaps[sc.winners[t % len(sc.bank)]] >= 4).all() and (out.overlaps > 0).sum() == sc.k
        per_step.append(td.crossings(before, sp.permanence, thr))
        td.add_crossings(total, per_step[-1])
    assert all(total[key] >= sc.k for key in ("up", "down", "on_from_below", "on_from_above")), total
    end = td.crossings(sc.permanence, sp.permanence, thr)                          # (what a batched run can show: first rows against last)
    assert all(end[key] >= 1 for key in ("up", "down", "on_from_below", "on_from_above")), end
    assert all(s["up"] and s["down"] for s in per_step), per_step                  # (both directions at the first AND the second win)
    on = np.flatnonzero(((sp.permanence >= thr) != (sc.permanence >= thr)).any(axis=0))
    assert on.max() >= sc.I - 40 >= 1024                                            # (mask words of the votes' second pass move too)
