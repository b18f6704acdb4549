"""htm_classifier_* and htm_classifiers_* act on one state, on the device (tests/classifier_doors.py): one object
fed alternately through both update calls -- learning and frozen, with an htm_classifiers_reset in the middle -- equals the definition
fed the same stream bit for bit, whichever door reads it."""
import numpy as np
import pytest

import classifier_doors as D
import group_classifier_cases as G


@pytest.mark.gpu
def test_one_object_fed_through_both_doors_equals_the_definition():
    want_best, want_dist, d = D.definition()
    home, engine = D.home_engine()
    got = D.alternate(engine)
    assert np.array_equal(got["best"], want_best), np.argwhere(got["best"] != want_best)[:5]
    assert np.array_equal(got["dist"], want_dist), np.argwhere(got["dist"] != want_dist)[:5]
    weights = d.dense_weights()
    assert weights.any()
    assert np.array_equal(got["weights_one"], weights) and np.array_equal(got["weights_bank"], weights)
    blob = np.concatenate([np.array([d.total, d.count], np.int64).view(np.uint8), d.ring_arrays(G.MIXED["max_pairs"]).view(np.uint8).ravel()])
    assert d.total == D.STEPS and 0 < d.count < D.STEPS
    assert np.array_equal(got["blob_one"], got["blob_bank"]) and np.array_equal(got["blob_one"], blob)
