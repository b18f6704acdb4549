"""GPU: the stand-alone Spatial Pooler methods -- GlobalInhibition.process, ExponentialBoosting.process / .update,
DenseProjection.process / .update, the plug-in slots of SpatialPooler and the C entry behind them (htm_sp_phase) -- handed
the values at which they can go wrong, not the values a running model produces.

Every expected value is plain NumPy float64 or the oracle (stable_topk, exp_f32 with sp_derived's coef32, the NumPy
HostDenseProjection of tests/test_hip_plugins.py); every comparison is exact.  The arrays come from tests/sp_method_cases.py:
wherever values are close, or become equal once low mantissa bits or exponents are lost, the larger one sits at the higher
index, so "a tie, the lower index wins" is the wrong answer."""

import numpy as np
import pytest

import sp_method_cases as cases
from oracle import SPParams
from oracle.fexp import exp_f32
from oracle.htm_oracle import sp_derived, stable_topk
from test_hip_plugins import HostDenseProjection

pytestmark = pytest.mark.gpu


# ---- GlobalInhibition.process against stable_topk ----------------------------------------------------------------------
@pytest.fixture(scope="module")
def pairs():
    p = cases.near_tie_products()
    assert len(p[0]) >= 50, len(p[0])
    return p


@pytest.fixture(scope="module")
def select():
    """check(name, C, k, x): GlobalInhibition(k).process(x) is stable_topk(x, k).  One GlobalInhibition (and so one engine) per
    shape for the whole module, all of them released when the module is done: a live handle with a stream of its own keeps
    every other handle of the process from the schedules in which blocks wait for each other."""
    import gc
    import bithtm_amd as B
    made = {}

    def check(name, C, k, x, or_refused=False):
        want = stable_topk(x, k)
        if (C, k) not in made:
            made[C, k] = B.GlobalInhibition(k)
        try:
            got = made[C, k].process(x.copy())
        except (ValueError, B.HtmError) as e:
            assert or_refused and ("span" in str(e) or "range" in str(e)), e
            return
        assert got.dtype == np.int64 and got.shape == (k,), name
        assert np.array_equal(got, want), (name, C, k, np.setdiff1d(got, want)[:8], np.setdiff1d(want, got)[:8])

    yield check
    made.clear()
    gc.collect()


@pytest.mark.parametrize("C,k", cases.CASES)
def test_select_full_mantissas(C, k, select):
    x = cases.full_mantissa(C, k)
    assert cases.loses_without_low_bits(x, k)
    select("full mantissa", C, k, x)


@pytest.mark.parametrize("ramp", [False, True], ids=["permuted", "ramp"])
@pytest.mark.parametrize("C,k", cases.CASES)
def test_select_adjacent_doubles(C, k, ramp, select):
    x = cases.adjacent_doubles(C, k, ramp=ramp)
    assert cases.loses_without_low_bits(x, k)
    if ramp:
        assert np.array_equal(stable_topk(x, k), np.arange(C - k, C))
    select("adjacent doubles", C, k, x)


@pytest.mark.parametrize("C,k", cases.CASES)
def test_select_reference_shaped_near_ties(C, k, pairs, select):
    """float32 factor x integer overlap on both sides of the cut, less than 2^-30 apart."""
    x = cases.reference_shaped(C, k, pairs)
    assert cases.loses_without_low_bits(x, k)
    select("reference-shaped", C, k, x)


@pytest.mark.parametrize("extra", [0, 3], ids=["cut-at-the-zeros", "cut-inside"])
@pytest.mark.parametrize("C,k", cases.CASES)
def test_select_tiny_values(C, k, extra, select):
    """5e-324 .. 2^-149 among ordinary values, exact zeros at lower indices: a tiny value is not a zero."""
    x = cases.tiny_values(C, k, extra=extra)
    if extra == 0:
        assert np.count_nonzero(x) == k and (x[stable_topk(x, k)] > 0).all()
    select("tiny", C, k, x)


@pytest.mark.parametrize("C,k", cases.CASES)
def test_select_huge_values(C, k, select):
    x = cases.huge_values(C, k)
    assert x.max() == np.finfo(np.float64).max
    select("huge", C, k, x)


@pytest.mark.parametrize("C,k", cases.CASES)
def test_select_signed_zeros(C, k, select):
    """-0.0 == +0.0: the cut inside the zeros goes by index alone."""
    x = cases.signed_zeros(C, k)
    assert np.signbit(x[0]) and np.count_nonzero(x) < k
    select("signed zeros", C, k, x)


@pytest.mark.parametrize("C,k", cases.CASES)
def test_select_ties(C, k, select):
    select("repeated", C, k, cases.repeated_value(C, k))
    select("all equal", C, k, np.full(C, 3.5))
    select("all zero", C, k, np.zeros(C))
    # and the engine is none the worse for it
    select("after ties", C, k, cases.full_mantissa(C, k, seed=5))


@pytest.mark.parametrize("C,k", cases.CASES)
def test_select_extreme_span_is_exact_or_refused(C, k, select):
    """5e-324 and 1e308 in one array: exactly stable_topk, or a loud error that names the accepted span -- never another list."""
    select("extreme span", C, k, cases.extreme_span(C, k), or_refused=True)


# ---- the C entry point refuses what it cannot order ---------------------------------------------------------------------
def test_sp_phase_refuses_bad_values_and_the_handle_goes_on():
    import bithtm_amd as B
    from bithtm_amd import _lib as L
    from bithtm_amd.engine import Engine
    from bithtm_amd.regularizations import _Placeholder
    C, k = 1000, 40
    boost = B.ExponentialBoosting(C, k)
    eng = Engine(32, C, 0, k, proximal=_Placeholder(32, C), boosting=boost)
    good = cases.full_mantissa(C, k, seed=9)
    overlaps = np.random.RandomState(3).randint(0, 33, size=C)

    def select_ok():
        eng.sp_phase(L.SP_SELECT, good, np.float64)
        assert np.array_equal(eng.read(L.F_ACTIVE_COLUMN, np.int32, k), stable_topk(good, k))

    select_ok()
    for bad in (np.nan, np.inf, -1.0):
        x = good.copy()
        x[C // 2] = bad
        with pytest.raises(B.HtmError, match=r"\(-1\).*SELECT") as e:
            eng.sp_phase(L.SP_SELECT, x, np.float64)
        assert not isinstance(e.value, B.CapacityError)
        select_ok()
    bad_overlaps = overlaps.copy()
    bad_overlaps[C - 1] = -1
    with pytest.raises(B.HtmError, match=r"\(-1\).*BOOST"):
        eng.sp_phase(L.SP_BOOST, bad_overlaps, np.int32)
    eng.sp_phase(L.SP_BOOST, overlaps, np.int32)
    assert np.array_equal(eng.read(L.F_BOOSTED, np.float64, C).view(np.int64), overlaps.astype(np.float64).view(np.int64))     # (duty cycle 0: factor 1)
    eng.sp_phase(L.SP_SELECT)
    assert np.array_equal(eng.read(L.F_ACTIVE_COLUMN, np.int32, k), stable_topk(overlaps, k))
    select_ok()


# ---- the plug-in route: a caller's own float64 boosting -------------------------------------------------------------------
class Float64Boosting:
    """A user's boosting in double precision throughout: its factors reach far below 2^-150 and carry full mantissas."""

    def __init__(self, output_dim, active_outputs, intensity, momentum, duty_cycle):
        self.rate = intensity * output_dim / active_outputs
        self.momentum = momentum
        self.duty_cycle = np.array(duty_cycle, dtype=np.float64)
        self.factors = []

    def process(self, input_activation):
        factor = np.exp(-self.rate * self.duty_cycle)
        self.factors.append(factor)
        return factor * input_activation

    def update(self, active_input):
        self.duty_cycle *= self.momentum
        self.duty_cycle[active_input] += 1.0 - self.momentum


def test_pooler_with_a_float64_boosting_equals_numpy_in_lock_step():
    import bithtm_amd as B
    I, C, k, steps = 300, 2048, 41, 40
    np.random.seed(11)
    perm = np.random.randn(C, I) * 0.1
    duty0 = np.random.RandomState(12).rand(C) * 0.6                 # rate 399.6: factors from 1 down to e^-240 = 2^-346
    prox = B.DenseProjection(I, C)
    prox.permanence = perm
    dev_boost = Float64Boosting(C, k, 8.0, 0.6, duty0)
    sp = B.SpatialPooler(I, C, k, proximal_projection=prox, boosting=dev_boost)
    host_prox, host_boost = HostDenseProjection(perm), Float64Boosting(C, k, 8.0, 0.6, duty0)
    rng = np.random.RandomState(13)
    bank = rng.rand(8, I) < 0.3
    saw_tiny = saw_low_bits = False
    for t in range(steps):
        x = bank[t % 8] ^ (rng.rand(I) < 0.02)
        learning = t % 7 != 3
        overlaps = host_prox.process(x)
        boosted = host_boost.process(overlaps)
        active = stable_topk(boosted, k)
        if learning:
            host_prox.update(x, active)
        host_boost.update(active)
        got = sp.process(x, learning=learning)
        assert np.array_equal(np.asarray(got.overlaps), overlaps), t
        assert np.array_equal(np.asarray(got.boosted_overlaps).view(np.int64), boosted.view(np.int64)), t     # (the caller's own values)
        assert np.array_equal(np.asarray(got.active_column), active), t
        saw_tiny |= bool(((host_boost.factors[-1] < 2.0 ** -150) & (overlaps > 0)).any())
        saw_low_bits |= bool((boosted.view(np.uint64) & np.uint64((1 << 20) - 1)).any())
    assert saw_tiny and saw_low_bits
    assert np.array_equal(prox.permanence.view(np.int64), host_prox.permanence.view(np.int64))
    assert np.array_equal(dev_boost.duty_cycle.view(np.int64), host_boost.duty_cycle.view(np.int64))


# ---- ExponentialBoosting.process / .update alone -------------------------------------------------------------------------
def test_exponential_boosting_alone_over_the_whole_range_of_its_exponential():
    """coef32 * duty from 0 through the last float32-normal result (about -87.3), the denormal results (-88 .. -103) and
    underflow to 0 (below -104), against overlaps 0, 1, 2^17 and 2^31 - 1."""
    import bithtm_amd as B
    from bithtm_amd import _lib as L
    C, k, intensity = 1000, 10, 8.0
    boost = B.ExponentialBoosting(C, k, intensity=intensity)
    d = sp_derived(SPParams(boost_intensity=intensity), C, k)
    assert d.coef32 == np.float32(-800.0)
    targets = np.r_[0.0, -1e-42, -1e-39, -1e-30, -0.5, -1.0, -87.0, -87.3, -87.33654, -87.33655, -87.4, np.linspace(-88, -103.5, 32),
                    -103.9, -103.97, -103.98, -104.0, -104.5, -110.0, -200.0, -700.0, -745.2, -800.0]
    rng = np.random.RandomState(21)
    duty = rng.rand(C).astype(np.float32)
    duty[:4 * len(targets)] = np.repeat((targets / np.float64(d.coef32)).astype(np.float32), 4)
    assert duty[4] > 0 and duty[4] < np.finfo(np.float32).tiny            # a float32 denormal duty cycle
    overlaps = np.tile(np.array([0, 1, 2 ** 17, 2 ** 31 - 1], dtype=np.int64), C // 4)
    eng = boost._ensure_engine()
    eng.write(L.F_DUTY_CYCLE, duty, np.float32)
    arg = d.coef32 * duty
    assert arg.dtype == np.float32
    factor = exp_f32(arg)
    tiny32 = np.finfo(np.float32).tiny
    assert (factor == 1).any() and ((factor > 0) & (factor < tiny32)).sum() >= 64 and (factor[arg < -104.5] == 0).all()
    assert (factor[(arg < -87.4) & (arg > -103.9)] < tiny32).all() and (factor[(arg < -87.4) & (arg > -103.9)] > 0).all()
    want = factor.astype(np.float64) * overlaps
    got = boost.process(overlaps)
    assert got.dtype == np.float64
    bad = np.flatnonzero(got.view(np.int64) != want.view(np.int64))
    assert bad.size == 0, [(int(i), float(arg[i]), int(overlaps[i]), float(got[i]), float(want[i])) for i in bad[:8]]
    # update: float32, `duty *= momentum` then a fancy-indexed += (once per distinct index), for any list
    m32, inc32 = d.momentum32, d.increment32
    for active in ([], [7, 3, 999, 0, 500], [5, 5, 5, 6, 998, 6], list(range(9, -1, -1))):
        duty = duty * m32
        duty[np.asarray(active, dtype=np.int64)] += inc32
        boost.update(active)
        assert np.array_equal(boost.duty_cycle.view(np.int32), duty.view(np.int32)), active
    got = boost.process(overlaps)
    want = exp_f32(d.coef32 * duty).astype(np.float64) * overlaps
    assert np.array_equal(got.view(np.int64), want.view(np.int64))


# ---- DenseProjection.process / .update alone ------------------------------------------------------------------------------
THR, INC, DEC = 0.5, 0.25, 0.125           # dyadic: every permanence below is exact in float64
LEVELS = np.array([0.5, 0.375, 0.625, 0.25, 0.75, np.nextafter(0.5, 1.0), np.nextafter(0.5, 0.0)])


def _projection(I, C, seed):
    import bithtm_amd as B
    rng = np.random.RandomState(seed)
    perm = LEVELS[rng.randint(len(LEVELS), size=(C, I))]
    prox = B.DenseProjection(I, C, permanence_threshold=THR, permanence_increment=INC, permanence_decrement=DEC)
    prox.permanence = perm
    return prox, HostDenseProjection(perm, THR, INC, DEC), rng


def _same_projection(prox, host, I, rng, what):
    from bithtm_amd import _lib as L
    assert np.array_equal(prox.permanence.view(np.int64), host.permanence.view(np.int64)), what
    for x in (np.zeros(I, dtype=np.bool_), np.ones(I, dtype=np.bool_), rng.rand(I) < 0.5):
        got = prox.process(x)
        assert got.dtype == np.int64 and np.array_equal(got, host.process(x)), what
    # pad bits never count: an input word with every bit set beyond input_dim
    eng = prox._engine
    eng.sp_phase(L.SP_OVERLAP, np.full(eng.words, 0xFFFFFFFF, dtype=np.uint32))
    got = eng.read(L.F_OVERLAPS, np.int32, prox.output_dim)
    assert np.array_equal(got, (host.permanence >= THR).sum(axis=1)) and got.max() <= I, what


@pytest.mark.parametrize("I", [1, 31, 33, 64, 65, 127, 129, 300])
def test_dense_projection_alone_on_and_around_the_threshold(I):
    C = 257
    prox, host, rng = _projection(I, C, 100 + I)
    _same_projection(prox, host, I, rng, "initial")
    crossed_up = crossed_down = False
    updates = [(np.ones(I, dtype=np.bool_), np.arange(C)),                      # 0.25 -> 0.5: onto the threshold from below
               (np.zeros(I, dtype=np.bool_), np.arange(0, C, 2)),               # 0.625 -> 0.5: onto it from above; 0.5 -> 0.375: off it
               (rng.rand(I) < 0.5, np.zeros(0, dtype=np.int64)),                # nobody learns
               (rng.rand(I) < 0.5, np.array([256, 3, 3, 0, 256, 3, 128])),      # duplicates: once per distinct row
               (rng.rand(I) < 0.3, rng.permutation(C)[:100]),
               (np.zeros(I, dtype=np.bool_), rng.permutation(C)[:200])]
    for n, (x, rows) in enumerate(updates):
        before = host.permanence.copy()
        host.update(x, rows)
        prox.update(x, rows)
        crossed_up |= bool(((before < THR) & (host.permanence == THR)).any())
        crossed_down |= bool(((before > THR) & (host.permanence == THR)).any())
        _same_projection(prox, host, I, rng, n)
    assert crossed_up and crossed_down


def test_dense_projection_update_of_more_rows_than_one_winner_list_holds():
    """DenseProjection.update splits a list longer than the engine's active_columns (2048) into several device calls."""
    I, C = 33, 2100
    prox, host, rng = _projection(I, C, 7)
    x = rng.rand(I) < 0.5
    rows = np.r_[rng.permutation(C), rng.randint(C, size=50)]
    prox.update(x, rows)
    assert prox._engine.active_columns < len(np.unique(rows))
    host.update(x, rows)
    _same_projection(prox, host, I, rng, "chunked")
