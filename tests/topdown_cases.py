"""Hand-built states for the top-down pass: the votes of role_pin (bithtm_amd/csrc/htm_decode.h), the feedback row of role_encode
(htm_forecast.h) and the decoded value of k_decode_votes (htm_scalar.h), each reached exactly at the smallest shape at which one of
its size- or layout-dependent paths exists.  Shared by tests/test_topdown_cases_cpu.py (every builder pinned, every mutant
caught, every precondition) and tests/test_hip_topdown_geometry.py (the device against the definition).

A state is set, never trained: a float64 permanence [C, I] (engine.set_permanence) and a bool cell prediction [C, K]
(engine.import_prev_state(prediction, activation, None, None)).  The definition is tests/forecast_fixture.py's votes_of and encode
-- the reference's own expressions -- and every comparison is exact integer equality.

Which case reaches which path, and the constant it comes from -- if a constant moves, the case moves with it:
  * role_pin's bit loop, 256 threads x PIN_BITS = 4 bits = 1 024 inputs per pass: input_dim 1 023 / 1 024 (one pass), 1 025 (a second
    pass for one bit), 2 049, 4 100 (five), 40 000 (40).
  * chunks of PIN_COLS = 1 024 columns per block: column_dim 1 023, 1 024, 1 025 (a chunk of one column), 3 000 (the last partial),
    8 192; a chunk without a predicted column (early return) beside one with some: every `only` and `chunk` family.
  * PIN_UNROLL = 8 mask loads in flight: a chunk's list of 1, 7, 8, 9, 1 023 and 1 024 columns.
  * WPC = 2 prediction words per column (cell_dim 33 .. 64): cells 31 and 32 alone.
  * the connected mask against `permanence >= threshold` in float64: the boundary family (every entry on the threshold, one ulp or
    2^-40 either side of it, -0.0 and the subnormals +-5e-324 for threshold 0.0), and learning_scenario (entries that learning moves
    across the threshold and exactly onto it).
  * role_encode's layout, 64-input chunks, one contiguous run of ceil((W / 2) / 4) chunks per wave (enc_layout): rows whose waves
    2 and 3 own nothing (input_dim 1, 33), runs of 157 chunks (40 000); quota ends placed on lane 63, on lane 0 of the next chunk,
    on the last input of wave 0's run and the first of wave 1's; every input on one vote (one histogram bin for all 64 lanes);
    candidates == max_bits and max_bits + 1; votes either side of 4 096 = 2^ENC_DIGIT (the second radix pass).

Shapes: htm_create takes every shape of SHAPES as it stands (input_dim 1 and cell_dim 1 included); none had to be substituted.

Pure NumPy; nothing here touches a device."""

import hashlib
from types import SimpleNamespace

import numpy as np

from forecast_fixture import encode, votes_of

PIN_COLS, PIN_BITS, PIN_UNROLL, ENC_WAVES, ENC_DIGIT = 1024, 4, 8, 4, 12

#         input_dim, column_dim, cell_dim
SHAPES = [(1, 64, 1), (33, 257, 33), (1023, 1023, 8), (1024, 1024, 32), (1025, 1025, 64), (2049, 3000, 48), (4100, 1024, 8),
          (40000, 64, 8), (333, 8192, 4)]
SHAPE_IDS = ["x".join(map(str, s)) for s in SHAPES]
THRESHOLDS = (0.0, 0.02)


def active_columns(C):
    """The winner-list length of every crafted model (the top-down pass does not read it; a step needs one)."""
    return max(1, min(8, C // 8))


def digest(*arrays):
    """Eight bytes for the shapes, dtypes and bytes of the arrays (floats by their bits: -0.0 is not 0.0 here)."""
    h = hashlib.blake2b(digest_size=8)
    for a in arrays:
        a = np.ascontiguousarray(a)
        h.update(repr((a.shape, a.dtype.str)).encode())
        h.update(a.tobytes())
    return int.from_bytes(h.digest(), "little")


# ------------------------------------------------------------------------------------------ predictions

def column_sets(C, seed=0):
    """[(name, sorted column ids)]: none; single columns at the chunk edges; exactly n columns of one chunk, the others empty;
    every column; a seeded third."""
    rng = np.random.RandomState(1000 + seed)
    out = [("none", np.zeros(0, np.int64))]
    for c in sorted({0, C - 1} | ({1023} if C > 1023 else set()) | ({1024} if C > 1024 else set())):
        out.append((f"only{c}", np.array([c], np.int64)))
    n_chunks = (C + PIN_COLS - 1) // PIN_COLS
    for ch in range(n_chunks):
        lo, hi = ch * PIN_COLS, min(C, (ch + 1) * PIN_COLS)
        for n in (1, 7, 8, 9, 1023, 1024):
            if n <= hi - lo:
                out.append((f"chunk{ch}-{n}", np.sort(lo + rng.permutation(hi - lo)[:n]).astype(np.int64)))
    out.append(("every", np.arange(C, dtype=np.int64)))
    third = rng.rand(C) < 1.0 / 3.0
    third[C - 1] = True                             # (the last chunk is never empty, however small it is)
    out.append(("third", np.flatnonzero(third).astype(np.int64)))
    return out


def cell_placements(K):
    """[(name, cells)]: where the predicted cells of a predicted column sit."""
    out = [("cell0", [0])]
    if K > 1:
        out.append((f"cell{K - 1}", [K - 1]))
    if K > 32:
        out += [("cell31", [31])] + ([("cell32", [32])] if K - 1 != 32 else [])
    if K > 1:
        out.append(("all", list(range(K))))
    return out


def prediction(C, K, columns, cells):
    p = np.zeros((C, K), dtype=np.bool_)
    p[np.asarray(columns, np.int64)[:, None], np.asarray(cells, np.int64)[None, :]] = True
    return p


def prediction_cases(shape):
    """[(name, columns, prediction bool[C, K])] of a shape: every column set crossed with every cell placement."""
    I, C, K = shape
    return [(f"{cn}-{pn}", cols, prediction(C, K, cols, cells)) for cn, cols in column_sets(C) for pn, cells in cell_placements(K)]


# ------------------------------------------------------------------------------------------ permanences

def boundary_values(thr):
    """Eight values, alternately NOT connected and connected under `permanence >= thr` in float64."""
    e = 2.0 ** -40
    below, above = np.nextafter(thr, -np.inf), np.nextafter(thr, np.inf)
    if thr == 0.0:
        vals = [below, -0.0, -e, 0.0, -5e-324, 5e-324, -e, e]                 # (below == -5e-324, above == 5e-324)
    else:
        vals = [below, thr, thr - e, above, below, thr + e, thr - e, thr]
    vals = np.array(vals, dtype=np.float64)
    assert np.array_equal(vals >= thr, np.arange(8) % 2 == 1)
    return vals


def seeded_permanence(shape, seed=0):
    """randn * 0.1 (the reference's own initialisation); used with thresholds 0.0 and 0.02."""
    I, C, K = shape
    return np.random.RandomState(2000 + seed).randn(C, I) * 0.1


def boundary_permanence(shape, thr):
    """Every entry a boundary value: entry (c, i) holds value (c + i) % 8, so that a not-connected entry has connected neighbours at
    column c + 1 and at input i + 1.  A mask made through float32 connects entries that are not connected (-5e-324 becomes -0.0;
    0.02 - 2^-40 becomes float32(0.02)); one made with `>` drops the quarter that sits on the threshold."""
    I, C, K = shape
    return boundary_values(thr)[(np.arange(C)[:, None] + np.arange(I)[None, :]) % 8]


def staircase_permanence(C, want):
    """Column c is connected to input i iff c < want[i] (threshold 0.0): with every column predicted the votes are `want`."""
    want = np.asarray(want)
    assert want.min() >= 0 and want.max() <= C
    return np.where(np.arange(C)[:, None] < want[None, :], 1.0, -1.0)


def staircase_want(shape, seed=0):
    """A seeded vote row for the staircase family of the votes tests: 0, C and values round the chunk edges among random ones."""
    I, C, K = shape
    rng = np.random.RandomState(3000 + seed)
    edges = np.array(sorted({0, 1, C - 1, C} | {v for v in (1023, 1024, 1025, 2048) if v <= C}))
    want = np.where(rng.rand(I) < 0.5, edges[rng.randint(len(edges), size=I)], rng.randint(0, C + 1, size=I)).astype(np.int32)
    want[0], want[-1] = 0, C                        # (input_dim 1: the one input is connected to every column)
    return want


PERMANENCE_FAMILIES = ["seeded-0.0", "seeded-0.02", "boundary-0.0", "boundary-0.02", "staircase"]


def permanence_case(shape, family):
    """(threshold, permanence float64[C, I]) of a shape and a family name of PERMANENCE_FAMILIES."""
    if family == "staircase":
        return 0.0, staircase_permanence(shape[1], staircase_want(shape))
    kind, thr = family.split("-", 1)
    thr = float(thr)
    return thr, (seeded_permanence(shape) if kind == "seeded" else boundary_permanence(shape, thr))


def vote_cases(shape, family):
    """The builder of the votes tests: (I, C, K, k, threshold, permanence, [(name, columns, prediction)])."""
    I, C, K = shape
    thr, perm = permanence_case(shape, family)
    return I, C, K, active_columns(C), thr, perm, prediction_cases(shape)


# ------------------------------------------------------------------------------------------ feedback rows

def enc_layout(I):
    """htm_forecast.h's header: W words (input_dim padded to 128 bits), W / 2 chunks of 64 inputs, one contiguous run of
    ceil(chunks / 4) chunks per wave.  runs[w] = (first input, end input) of wave w, clipped to [0, I]."""
    W = (I + 127) // 128 * 4
    n_chunks = W // 2
    per_wave = (n_chunks + ENC_WAVES - 1) // ENC_WAVES
    runs = [(min(w * per_wave * 64, I), min((w + 1) * per_wave * 64, I)) for w in range(ENC_WAVES)]
    return SimpleNamespace(W=W, n_chunks=n_chunks, per_wave=per_wave, runs=runs)


def encode_words(votes, min_votes, max_bits, W=None):
    """The definition's row as the device stores it: uint32[W], bit i of the row = bit (i & 31) of word (i >> 5), pad bits 0."""
    votes = np.asarray(votes)
    W = enc_layout(votes.size).W if W is None else W
    bits = np.zeros(W * 32, dtype=np.bool_)
    bits[:votes.size] = encode(votes, min_votes, max_bits)
    return np.packbits(bits, bitorder="little").view(np.uint32)


def tie_row(I, C, p, tie=None):
    """A row whose cut-off falls among ties: most inputs hold `tie`, every seventh (i % 7 == 3) tie + 1, every fifth (i % 5 == 1)
    tie - 1 (a candidate below the cut), inputs p and p + 1 `tie`, and (min_votes, max_bits) such that the LAST admitted tie is
    input p: the cut falls between two neighbouring ties.  Returns (want, min_votes, max_bits)."""
    tie = min(C - 1, 2) if tie is None else tie
    assert 1 <= tie < C and 0 <= p < I - 1
    i = np.arange(I)
    want = np.full(I, tie, dtype=np.int32)
    want[i % 7 == 3] = tie + 1
    want[i % 5 == 1] = tie - 1
    want[p:p + 2] = tie
    return want, 1, int((want > tie).sum() + (want[:p + 1] == tie).sum())


def encoder_rows(shape):
    """[(name, want int32[I], [(min_votes, max_bits)], cut)]: the vote rows of a shape.  `cut`: None, or the input index the case's
    name says the quota ends on, for the first (min_votes, max_bits) pair (tests/test_topdown_cases_cpu.py checks it)."""
    I, C, K = shape
    lay = enc_layout(I)
    i = np.arange(I)
    out = []
    v = min(C, 3)
    caps = sorted({1, I - 1, I, I + 1} | {n for n in (63, 64, 65, lay.per_wave * 64, lay.per_wave * 64 + 1) if n < I})
    out.append(("all_equal", np.full(I, v, np.int32), [(1, 0), (v, 0), (v + 1, 0), (v + 1, 3)] + [(1, n) for n in caps if n >= 1], None))
    a, b = min(C, 5), min(C, 5) - 1                 # (b >= 1 unless C == 1: every shape has C >= 64)
    n_a = int((i % 2 == 0).sum())
    out.append(("alternating", np.where(i % 2 == 0, a, b).astype(np.int32),
                [(1, 0), (a, 0), (1, n_a), (1, n_a + 1), (a, n_a), (a, n_a + 1), (a + 1, 5)] + ([(1, n_a - 1), (a, n_a - 1)] if n_a > 1 else []), None))
    places = [("tie_ends_lane63", 63), ("tie_ends_next_chunk_lane0", 64)]
    if lay.runs[1][1] > lay.runs[1][0]:
        places += [("tie_ends_wave0_last", lay.runs[0][1] - 1), ("tie_ends_wave1_first", lay.runs[1][0])]
    places.append(("tie_quota_used_by_wave0", min(5, I - 2)))
    if I >= 3:
        places.append(("tie_ends_before_last_input", I - 2))
    for name, p in places:
        if 0 <= p < I - 1:                          # (a tie must stay out: the row goes on after p)
            want, mv, mb = tie_row(I, C, p)
            out.append((name, want, [(mv, mb), (mv, mb + 1), (mv, max(mb - 1, 1)), (2, mb), (1, 0)], p))
    last = np.full(I, 1, np.int32)
    last[I - 1] = min(C, 2)
    out.append(("last_input_is_the_candidate", last, [(1, 1), (2, 0), (2, 1), (2, 5), (1, 0)], None))
    if C >= 8192:
        for name, tie in (("tie_at_4095", 4095), ("tie_at_4096", 4096), ("tie_at_4097", 4097)):
            p = lay.runs[1][0] + 3
            want, mv, mb = tie_row(I, C, p, tie)
            out.append((name, want, [(mv, mb), (mv, mb + 1), (4096, mb), (4096, 0), (4097, 20), (1, 0)], p))
    return out


def chain_rows(shape):
    """Two vote rows for the chain to a value (votes above 4 096, many ties): seeded picks from a short list of values."""
    I, C, K = shape
    assert C >= 8192
    rows = []
    for seed in (0, 1):
        rng = np.random.RandomState(4000 + seed)
        rows.append(rng.choice([0, 1, 4095, 4096, 4097, 6000, 8191, 8192], size=I).astype(np.int32))
    return rows


# ------------------------------------------------------------------------------------------ the mask under learning

def _landing(thr, delta, toward, wins=1):
    """The float64 v nearest thr - wins * delta that `wins` additions of delta put exactly on thr (toward = 0), or on the far side of
    thr by as little as float64 allows (toward = -1: just below)."""
    def after(v):
        for _ in range(wins):
            v = v + delta
        return v
    v = thr - wins * delta
    for _ in range(64):
        s = after(v)
        if (toward == 0 and s == thr) or (toward < 0 and s < thr):
            return v
        v = np.nextafter(v, -np.inf if toward or s > thr else np.inf)
    raise AssertionError("no such float64")


# (threshold, increment, decrement) of the two scenarios: the reference's defaults on threshold 0.0, and dyadic steps on a
# dyadic threshold away from zero (with the defaults no float64 lands exactly on 0.02 from above: 0.035 - 0.015 misses it by an ulp)
SCENARIOS = {"defaults-0.0": (0.0, 0.03, 0.015), "dyadic-3/128": (0.0234375, 0.03125, 0.015625)}


def learning_scenario(name):
    """A Spatial Pooler whose winners are designated and whose learning moves mask bits: P = 3 patterns over disjoint input groups,
    k = 8 columns per pattern (A_j = {c : c % 3 == j, c < 24}) connected to 4 anchor inputs of group j at 0.5 and holding, on the
    group's 20 other inputs (in pattern j: + delta_on at every win) and on the 40 last inputs (in no pattern: + delta_off), values
    that cross the threshold upward / downward at the first or the second win, land exactly on it from below / above at the first
    or at the second win, or miss it by an ulp.  Every other entry is -0.5, so a pattern's overlap is positive on its own columns
    alone and those win whatever the boost factors are.  input_dim 1 100: the last inputs lie in the votes' second pass.
    Returns a namespace: I, C, K, k, params (oracle SPParams), permanence, bank bool[3, I], steps, winners[j]."""
    from oracle import SPParams
    I, C, K, k, P, G, OFF = 1100, 64, 4, 8, 3, 24, 40
    thr, inc, dec = SCENARIOS[name]
    params = SPParams(permanence_threshold=thr, permanence_increment=inc, permanence_decrement=dec)
    both = params.permanence_increment + params.permanence_decrement
    d_on, d_off = 1.0 * both - params.permanence_decrement, 0.0 * both - params.permanence_decrement
    on_kinds = [_landing(thr, d_on, 0), thr - d_on / 2, thr - 1.5 * d_on, _landing(thr, d_on, -1), thr - 3 * d_on,
                _landing(thr, d_on, 0, wins=2)]
    off_kinds = [_landing(thr, d_off, 0), thr - d_off / 2, thr - 1.5 * d_off, _landing(thr, d_off, -1), thr - 3 * d_off,
                 _landing(thr, d_off, 0, wins=2), np.nextafter(thr, np.inf)]
    perm = np.full((C, I), -0.5, dtype=np.float64)
    bank = np.zeros((P, I), dtype=np.bool_)
    winners = [np.arange(k, dtype=np.int64) * P + j for j in range(P)]
    for j in range(P):
        g0 = j * G
        bank[j, g0:g0 + G] = True
        for r, c in enumerate(winners[j]):
            perm[c, g0:g0 + 4] = 0.5
            perm[c, g0 + 4:g0 + G] = [on_kinds[(r + u) % len(on_kinds)] for u in range(G - 4)]
            perm[c, I - OFF:] = [off_kinds[(r + j + u) % len(off_kinds)] for u in range(OFF)]
    return SimpleNamespace(I=I, C=C, K=K, k=k, thr=thr, params=params, permanence=perm, bank=bank, steps=2 * P, winners=winners)


def crossings(before, after, thr):
    """What one learning step did to the mask, from the float64 rows before and after it: entries that became connected, that
    stopped being connected, that moved from below exactly onto the threshold, and from above exactly onto it."""
    return dict(up=int(((before < thr) & (after >= thr)).sum()), down=int(((before >= thr) & (after < thr)).sum()),
                on_from_below=int(((before < thr) & (after == thr)).sum()), on_from_above=int(((before > thr) & (after == thr)).sum()))


def add_crossings(total, step):
    for key, n in step.items():
        total[key] = total.get(key, 0) + n
    return total


# ------------------------------------------------------------------------------------------ mutants: wrong implementations in NumPy

def _any(pred):
    return np.asarray(pred).any(axis=1)


def votes_ignoring_cells_from_32(perm, thr, pred):
    """The second prediction word never read."""
    return votes_of(perm, thr, np.asarray(pred)[:, :32])


def votes_dropping_inputs_from_1024(perm, thr, pred):
    """The bit loop ends after one pass."""
    v = votes_of(perm, thr, pred)
    v[256 * PIN_BITS:] = 0
    return v


def votes_dropping_the_unroll_tail(perm, thr, pred):
    """Of every chunk's list only the whole groups of PIN_UNROLL columns counted (the last n % 8 dropped)."""
    cols = np.flatnonzero(_any(pred))
    keep = np.zeros(len(pred), dtype=np.bool_)
    for ch in np.unique(cols // PIN_COLS):
        mine = cols[cols // PIN_COLS == ch]
        keep[mine[:len(mine) // PIN_UNROLL * PIN_UNROLL]] = True
    return votes_of(perm, thr, keep[:, None])


def votes_dropping_the_partial_chunk(perm, thr, pred):
    """Blocks over C / 1 024 rounded down."""
    keep = _any(pred).copy()
    keep[len(keep) // PIN_COLS * PIN_COLS:] = False
    return votes_of(perm, thr, keep[:, None])


def votes_ending_at_an_empty_chunk(perm, thr, pred):
    """The early return of a chunk without a predicted column taken for the end of the whole launch: later chunks are lost."""
    keep = _any(pred).copy()
    n_chunks = (len(keep) + PIN_COLS - 1) // PIN_COLS
    for ch in range(n_chunks):
        if not keep[ch * PIN_COLS:(ch + 1) * PIN_COLS].any():
            keep[ch * PIN_COLS:] = False
            break
    return votes_of(perm, thr, keep[:, None])


def votes_with_greater_than(perm, thr, pred):
    """`>` for `>=`."""
    return (perm[_any(pred)] > thr).sum(axis=0).astype(np.int32)


def votes_from_a_float32_mask(perm, thr, pred):
    """The mask made from the permanence rounded to float32."""
    return (perm[_any(pred)].astype(np.float32) >= np.float32(thr)).sum(axis=0).astype(np.int32)


def votes_from_a_sign_bit_mask(perm, thr, pred):
    """Connected = the sign bit of permanence - threshold is clear: -0.0 on threshold 0.0 is lost."""
    return (~np.signbit(perm[_any(pred)] - thr)).sum(axis=0).astype(np.int32)


def _encode_with(votes, min_votes, max_bits, order=None, quota_per=None):
    """encode() with the tie order and the quota's scope made pluggable.  order: +1 ties to the lower index (the definition), -1 to
    the higher.  quota_per: None (global), or a list of (begin, end) runs each of which admits the quota's worth of ties anew."""
    votes = np.asarray(votes).astype(np.int64)
    I = votes.size
    x = votes >= min_votes
    if not max_bits or x.sum() <= max_bits:
        return x
    ranked = np.sort(votes[x])[::-1]
    vstar = ranked[max_bits - 1]
    quota = max_bits - int((votes > vstar).sum())
    out = votes > vstar
    ties = np.flatnonzero(votes == vstar)
    if order == -1:
        ties = ties[::-1]
    if quota_per is None:
        out[ties[:quota]] = True
    else:
        for b, e in quota_per:
            out[ties[(ties >= b) & (ties < e)][:quota]] = True
    return out


def encode_ties_to_the_higher_index(votes, min_votes, max_bits):
    return _encode_with(votes, min_votes, max_bits, order=-1)


def encode_quota_per_wave(votes, min_votes, max_bits):
    """The ties of the waves before never added to a wave's offset."""
    return _encode_with(votes, min_votes, max_bits, quota_per=enc_layout(np.asarray(votes).size).runs)


def encode_quota_per_chunk(votes, min_votes, max_bits):
    """The offset not carried from one 64-input chunk to the next."""
    I = np.asarray(votes).size
    return _encode_with(votes, min_votes, max_bits, quota_per=[(b, b + 64) for b in range(0, I, 64)])


def encode_cap_before_threshold(votes, min_votes, max_bits):
    """The cap taken over every input that has a vote, the threshold only where that cap does not bite."""
    votes = np.asarray(votes)
    if max_bits and (votes > 0).sum() > max_bits:
        return encode(votes, 1, max_bits)
    return encode(votes, min_votes, max_bits)


def encode_cap_off_by_one(votes, min_votes, max_bits):
    """`candidates > max_bits + 1` for `candidates > max_bits`: one candidate too many passes uncapped."""
    votes = np.asarray(votes)
    x = votes >= min_votes
    return x if (max_bits and x.sum() == max_bits + 1) else encode(votes, min_votes, max_bits)


def encode_low_digit_only(votes, min_votes, max_bits):
    """The select ranks by the low ENC_DIGIT bits of a vote alone (one radix pass whatever the largest vote)."""
    votes = np.asarray(votes).astype(np.int64)
    x = votes >= min_votes
    if not max_bits or x.sum() <= max_bits:
        return x
    low = np.where(x, votes & ((1 << ENC_DIGIT) - 1), -1)
    keep = np.lexsort((np.arange(votes.size), -low))[:max_bits]
    out = np.zeros(votes.size, dtype=np.bool_)
    out[keep] = True
    return out


def encode_dropping_ties(votes, min_votes, max_bits):
    """No input AT the cut-off admitted (a quota of 0)."""
    votes = np.asarray(votes)
    x = votes >= min_votes
    if not max_bits or x.sum() <= max_bits:
        return x
    return votes > np.sort(votes[x])[::-1][max_bits - 1]


def words_with_pad_bits_set(votes, min_votes, max_bits, sentinel):
    """The pad bits of the row (inputs from input_dim up to the end of its last word) set."""
    w = encode_words(votes, min_votes, max_bits).copy()
    bits = np.unpackbits(w.view(np.uint8), bitorder="little")
    bits[np.asarray(votes).size:] = 1
    return np.packbits(bits, bitorder="little").view(np.uint32)


def words_with_floor_chunks_per_wave(votes, min_votes, max_bits, sentinel):
    """chunks / 4 rounded down: the chunks past 4 * floor(chunks / 4) are nobody's and keep what the row held."""
    w = encode_words(votes, min_votes, max_bits).copy()
    lay = enc_layout(np.asarray(votes).size)
    w[2 * (lay.n_chunks // ENC_WAVES * ENC_WAVES):] = sentinel
    return w


def words_of_the_data_chunks_only(votes, min_votes, max_bits, sentinel):
    """Only the chunks that hold an input written: the pad words of the row keep what they held."""
    w = encode_words(votes, min_votes, max_bits).copy()
    w[2 * ((np.asarray(votes).size + 63) // 64):] = sentinel
    return w


# name -> (the wrong implementation, the families named for it): votes mutants over (shape, permanence family, prediction name
# prefix or None = all), encode mutants over encoder row names (None = all), word mutants likewise
VOTE_MUTANTS = {
    "cells_from_32_ignored": (votes_ignoring_cells_from_32, ["cell32", "cell47", "cell63"]),
    "inputs_from_1024_dropped": (votes_dropping_inputs_from_1024, None),
    "unroll_tail_dropped": (votes_dropping_the_unroll_tail, ["chunk"]),
    "partial_chunk_dropped": (votes_dropping_the_partial_chunk, ["only", "every", "third", "chunk"]),
    "empty_chunk_ends_the_launch": (votes_ending_at_an_empty_chunk, ["only", "chunk"]),
    "greater_than": (votes_with_greater_than, None),
    "float32_mask": (votes_from_a_float32_mask, None),
    "sign_bit_mask": (votes_from_a_sign_bit_mask, None),
}
# the shapes and permanence families on which each votes mutant must be caught (at least one prediction case of each pair)
VOTE_MUTANT_WHERE = {
    "cells_from_32_ignored": [(s, "seeded-0.0") for s in SHAPES if s[2] > 32],
    "inputs_from_1024_dropped": [(s, "seeded-0.0") for s in SHAPES if s[0] > 1024],
    "unroll_tail_dropped": [(s, "seeded-0.02") for s in SHAPES],
    "partial_chunk_dropped": [(s, "seeded-0.0") for s in SHAPES if s[1] % PIN_COLS],
    "empty_chunk_ends_the_launch": [(s, "seeded-0.0") for s in SHAPES if s[1] > PIN_COLS],
    "greater_than": [(s, f) for s in SHAPES for f in ("boundary-0.0", "boundary-0.02")],
    "float32_mask": [(s, f) for s in SHAPES for f in ("boundary-0.0", "boundary-0.02")],
    "sign_bit_mask": [(s, "boundary-0.0") for s in SHAPES],
}
ENCODE_MUTANTS = {
    "ties_to_the_higher_index": (encode_ties_to_the_higher_index, ["tie_", "all_equal"]),
    "quota_per_wave": (encode_quota_per_wave, ["tie_quota_used_by_wave0", "tie_ends_wave0_last", "all_equal"]),
    "quota_per_chunk": (encode_quota_per_chunk, ["tie_ends_lane63", "tie_quota_used_by_wave0", "all_equal"]),
    "cap_before_threshold": (encode_cap_before_threshold, ["alternating"]),
    "cap_off_by_one": (encode_cap_off_by_one, ["all_equal", "alternating"]),
    "low_digit_only": (encode_low_digit_only, ["tie_at_4095", "tie_at_4096"]),
    "ties_dropped": (encode_dropping_ties, ["all_equal", "tie_"]),
}
WORD_MUTANTS = {
    "pad_bits_set": (words_with_pad_bits_set, None),
    "floor_chunks_per_wave": (words_with_floor_chunks_per_wave, None),
    "data_chunks_only": (words_of_the_data_chunks_only, None),
}
