"""One KNN store through both doors: a KNNClassifier (htm_knn_*) and a KNNClassifierBank of one stream (htm_knns_*) are the same host
code at n = 1 over different kernels (DESIGN.md sections 26 and 27).  Fed the same stream they give the same rows and votes -- the
definition's, bithtm_amd/knn.py -- and the same state blob, byte for byte, which each loads from the other.  Every comparison is
exact.  The stream is CHUNK + 3 labelled steps in two calls cut at step 2: the second call appends behind a store that is not empty
and runs over a chunk boundary (CHUNK + 1 steps); five more steps are asked frozen."""
import ctypes as C
import functools

import numpy as np
import pytest

import knn_cases as cases
from knn_cases import CHUNK, GLOBAL_SHAPE, SHAPE

FORMS = {"tables-in-lds": SHAPE, "global-table": GLOBAL_SHAPE}
PARAMS = dict(labels=6, k=3, capacity=96)
T, CUT, ASKED = CHUNK + 3, 2, 5


@functools.lru_cache(maxsize=None)
def _stream(form):
    """-> (shape, index, words, labels of T + ASKED steps, the definition's (best, votes) of the two learning calls and of the frozen
    one); computed once and shared, never written."""
    from bithtm_amd.knn import KNNDefinition
    shape = FORMS[form]
    index, words, labels = cases.clustered(shape, T + ASKED, 21, labelled=0.8, columns=np.arange(50))
    d = KNNDefinition(PARAMS["labels"], PARAMS["k"], 1, PARAMS["capacity"], *shape)
    want = [d.update(index[a:b], words[a:b], labels[a:b]) for a, b in ((0, CUT), (CUT, T))]
    want.append(d.update(index[T:], words[T:], labels[T:], learning=False))
    assert 0 < d.count < T                          # (some steps carry no label: the stores hold fewer slots than steps)
    return shape, index, words, labels, want


def _same(got, want, what):
    assert np.array_equal(got[0], want[0]) and np.array_equal(got[1], want[1]), (what, np.argwhere(got[0] != want[0])[:5])


@pytest.mark.parametrize("form", list(FORMS))
def test_the_bank_definition_of_one_stream_equals_the_definition(form):
    from bithtm_amd.knn import KNNBankDefinition
    shape, index, words, labels, want = _stream(form)
    bank = KNNBankDefinition(1, PARAMS["labels"], PARAMS["k"], 1, PARAMS["capacity"], *shape)
    for n, (a, b) in enumerate(((0, CUT), (CUT, T))):
        best, votes = bank.update(index[None, a:b], words[None, a:b], labels[None, a:b])
        _same((best[0], votes[0]), want[n], n)
    best, votes = bank.update(index[None, T:], words[None, T:], labels[None, T:], learning=False)
    _same((best[0], votes[0]), want[2], "frozen")


def _blob(obj):
    size = obj.info()["state_bytes"]
    blob = np.zeros(size, dtype=np.uint8)
    obj._call(obj._engine(), "export", blob.ctypes.data_as(C.c_void_p), size)
    return blob


@pytest.mark.gpu
@pytest.mark.parametrize("form", list(FORMS))
def test_one_stream_and_a_bank_of_one_give_the_same_rows_and_the_same_blob_and_load_each_others_state(form):
    import bithtm_amd as B
    shape, index, words, labels, want = _stream(form)
    knn, bank = B.KNNClassifier(shape=shape, **PARAMS), B.KNNClassifierBank(1, shape=shape, **PARAMS)
    for n, (a, b) in enumerate(((0, CUT), (CUT, T))):
        solo = knn.update_patterns(index[a:b], words[a:b], labels[a:b], votes=True, device=0)
        best, votes = bank.update_patterns(index[None, a:b], words[None, a:b], labels[None, a:b], votes=True, device=0)
        assert best.shape == (1, b - a, 5) and votes.shape == (1, b - a, PARAMS["labels"])
        _same(solo, want[n], ("one stream", n))
        _same((best[0], votes[0]), solo, ("bank", n))
    assert knn.count == int(bank.count[0]) > 0 and knn.total == bank.total == T
    mine, theirs = _blob(knn), _blob(bank)
    assert len(mine) == len(theirs) == knn.info()["state_bytes"] == bank.info()["state_bytes"] == 16 + knn.count * (8 * shape[2] + 12)
    assert np.array_equal(mine, theirs)
    state, stream0 = knn.state_dict(), bank.stream_state(0)
    asked = knn.update_patterns(index[T:], words[T:], labels[T:], learning=False, votes=True)
    _same(asked, want[2], "frozen")
    fresh_bank = B.KNNClassifierBank(1, shape=shape, **PARAMS)
    fresh_bank.load_state_dict(dict(state, streams=1, count=[int(state["count"])]))
    best, votes = fresh_bank.update_patterns(index[None, T:], words[None, T:], None, learning=False, votes=True, device=0)
    _same((best[0], votes[0]), asked, "a bank with the one-stream state")
    fresh = B.KNNClassifier(shape=shape, **PARAMS)
    fresh.load_state_dict(stream0)
    _same(fresh.update_patterns(index[T:], words[T:], labels[T:], learning=False, votes=True, device=0), asked, "one stream with the bank's state")
