"""Host side of the stand-alone Spatial Pooler methods (no device): the domain checks in front of the select and the boosting,
and the NumPy twin of the key the device gives a boosted overlap that came from the host."""

import numpy as np
import pytest

import sp_method_cases as cases
from oracle.htm_oracle import stable_topk


class _NoEngine:
    """Stands where an engine would: touching it means a check came too late."""

    def __getattr__(self, name):
        raise AssertionError(f"the engine was used ({name}) before the values were checked")


@pytest.mark.parametrize("bad", [np.nan, np.inf, -np.inf, -1.0, -5e-324], ids=["nan", "inf", "-inf", "negative", "negative-denormal"])
def test_global_inhibition_refuses_what_a_topk_cannot_order_before_any_engine_exists(bad):
    from bithtm_amd.regularizations import GlobalInhibition
    inh = GlobalInhibition(3)
    x = np.arange(10, dtype=np.float64)
    x[6] = bad
    with pytest.raises(ValueError, match="finite and >= 0"):
        inh.process(x)
    assert inh._engine is None


def test_checked_boosted_accepts_the_whole_domain_and_hands_the_values_back():
    from bithtm_amd.regularizations import checked_boosted
    x = np.array([0.0, -0.0, 5e-324, 2.0 ** -150, 1.0, 2.0 ** 362, np.finfo(np.float64).max])
    y = checked_boosted(x, "test")
    assert y.dtype == np.float64 and np.array_equal(y.view(np.int64), x.view(np.int64))
    assert checked_boosted(x[:5].astype(np.float32), "test").dtype == np.float64
    assert checked_boosted(np.zeros(0), "test").size == 0


class _Proximal:
    def __init__(self, out):
        self.out = out

    def process(self, x):
        return self.out

    def update(self, x, cols):
        raise AssertionError("update after a refused step")


class _Boosting:
    def __init__(self, out):
        self.out = out

    def process(self, overlaps):
        return self.out

    def update(self, cols):
        raise AssertionError("update after a refused step")


def _pooler(C, **kw):
    from bithtm_amd.networks import SpatialPooler
    sp = SpatialPooler(8, C, 2, **kw)
    sp._engine = _NoEngine()
    return sp


@pytest.mark.parametrize("bad", [np.nan, np.inf, -0.5])
def test_process_phases_checks_a_foreign_boostings_output(bad):
    C = 6
    boosted = np.array([1.0, 2.0, bad, 0.0, -0.0, 5e-324])
    sp = _pooler(C, proximal_projection=_Proximal(np.arange(C)), boosting=_Boosting(boosted))
    with pytest.raises(ValueError, match="_Boosting.process.*finite and >= 0"):
        sp._process_phases(np.zeros(8, dtype=np.bool_), True, True)


@pytest.mark.parametrize("overlaps", [np.array([1.0, 2.5, 3.0, 0.0, 0.0, 1.0]), np.array([1.0, np.nan, 3.0, 0.0, 0.0, 1.0]),
                                      np.array([1, -1, 3, 0, 0, 1]), np.array([1, 2 ** 31, 3, 0, 0, 1]),
                                      np.array([1.0, 2.0 ** 40, 3.0, 0.0, 0.0, 1.0])],
                         ids=["fraction", "nan", "negative", "int-too-large", "float-too-large"])
def test_process_phases_refuses_overlaps_that_are_not_counts(overlaps):
    """... instead of truncating them to int32 on their way to the device's boosting."""
    sp = _pooler(6, proximal_projection=_Proximal(overlaps))
    with pytest.raises(ValueError, match="_Proximal.process: overlaps must"):
        sp._process_phases(np.zeros(8, dtype=np.bool_), True, True)


def test_checked_overlaps_keeps_whole_numbers_of_any_dtype():
    from bithtm_amd.regularizations import checked_overlaps
    want = np.array([0, 1, 131072, 2 ** 31 - 1], dtype=np.int32)
    for dtype in (np.int64, np.uint32, np.float64, np.int32):
        got = checked_overlaps(want.astype(dtype), "test")
        assert got.dtype == np.int32 and np.array_equal(got, want)
    assert np.array_equal(checked_overlaps(np.array([True, False]), "test"), [1, 0])


# ---- the key of a host-supplied boosted overlap (k_sp_keys, SP_KEYS_HOST) and the test data themselves -------------------
@pytest.fixture(scope="module")
def pairs():
    p = cases.near_tie_products()
    assert len(p[0]) >= 50, len(p[0])
    return p


def test_near_tie_products_are_reference_shaped(pairs):
    p1, p2 = pairs
    assert (p1 != p2).all() and (np.abs(p1 - p2) < p1 * 2.0 ** -30).all()
    assert (cases.mask_low(p1) == cases.mask_low(p2)).all()
    assert (p1 >= 1).all() and (p1 < 2 ** 17).all() and (p2 >= 1).all() and (p2 < 2 ** 17).all()


@pytest.mark.parametrize("C,k", cases.CASES)
def test_host_select_key_preserves_the_order_of_every_family(C, k, pairs):
    """A full-width select on the twin's keys (descending key, ascending index) is stable_topk on the values, and the families
    that are about low mantissa bits do lose when those bits are ignored."""
    from bithtm_amd.regularizations import host_select_key
    for name, x in cases.select_cases(C, k, pairs).items():
        assert x.shape == (C,) and np.isfinite(x).all() and not (x < 0).any(), name
        key = host_select_key(x)
        assert key.dtype == np.uint64
        by_key = np.sort(np.lexsort((np.arange(C), ~key))[:k])          # (~key ascending = key descending)
        assert np.array_equal(by_key, stable_topk(x, k)), name
        # strictly monotone, and equal exactly where the values are equal
        order = np.argsort(x, kind="stable")
        xs, ks = x[order], key[order]
        assert (ks[1:] >= ks[:-1]).all() and np.array_equal(ks[1:] == ks[:-1], xs[1:] == xs[:-1]), name
        if name in cases.LOW_BIT_FAMILIES:
            assert cases.loses_without_low_bits(x, k), name


def test_families_cut_where_they_claim(pairs):
    """The layout of the families: zeros below tiny values, the cut inside the zeros / the repeated group, -0.0 first."""
    for C, k in cases.CASES:
        x = cases.tiny_values(C, k)
        want = stable_topk(x, k)
        assert (x[want] > 0).all() and np.count_nonzero(x) == k and (x[:C - k] == 0).all()
        assert (x[want] <= 2.0 ** -149).any() and x[want].min() == 5e-324
        x = cases.signed_zeros(C, k)
        want = stable_topk(x, k)
        assert (x[want] == 0).any() and np.count_nonzero(x) < k and np.signbit(x[0]) and want[0] == 0
        x = cases.repeated_value(C, k)
        want = stable_topk(x, k)
        chosen = np.count_nonzero(x[want] == 7.25)
        assert 0 < chosen < np.count_nonzero(x == 7.25)
        x = cases.extreme_span(C, k)
        assert x.max() == 1e308 or x.max() == np.finfo(np.float64).max
        assert x[x > 0].min() == 5e-324
