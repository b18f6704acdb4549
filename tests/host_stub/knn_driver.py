"""Driver of the launch traces of the KNN classifier (tests/test_knn_cpu.py; used as classifier_driver.py is: the engine's host code
host-only, no sanitizer, nothing preloaded, over tests/host_stub's runtime with BITHTM_STUB_TRACE).

Prints one JSON object:
  "frozen"   {"T=<steps>": the trace lines of update_patterns(learning=False) over T steps on a store of 300 slots}
  "learning" {"T=<steps>": ... of update_patterns over T labelled steps}
  "global"   {"T=<steps>": ... of frozen calls on an object whose tables lie in the global scratch table}
  "run"      the lines of runs of 6 steps on twin models with the same history (every kind of call made once before), launched eagerly:
               "recorded"       run(record=True)
               "knn"            run(knn=) on the twin whose last run had one
               "both"           run(knn=, classifier=) on that twin
               "classified"     run(classifier=) on it
               "plain"          run()
               "recorded after", "plain after"   the same two calls on the twin that has just made the knn runs
  "graphs"   the same runs replayed from graphs
  "refused"  the messages of the Python refusals that need a bound model, "refused_lines" what they enqueued (nothing)

Kernels do nothing in the stub: the trace says which launches and copies the host code makes, not what they compute."""
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
TRACE = os.environ["BITHTM_STUB_TRACE"]
os.environ["BITHTM_EAGER_BELOW"] = "0"              # use_graph alone decides between graphs and eager launches
import bithtm_amd as B  # noqa: E402
import knn_cases as cases  # noqa: E402
from knn_cases import CHUNK, GLOBAL_SHAPE, SHAPE  # noqa: E402

I, Cn, K, k = 64, 256, 8, 8


def lines():
    with open(TRACE) as f:
        return f.read().splitlines()


def traced(call):
    n = len(lines())
    call()
    return lines()[n:]


def model(seed=3):
    np.random.seed(seed)
    tm = B.TemporalMemory(Cn, K, distal_projection=B.PredictiveProjection(Cn * K, segment_capacity=8192), seed=seed)
    return B.HierarchicalTemporalMemory(I, Cn, K, active_columns=k, temporal_memory=tm)


def main():
    out = {"frozen": {}, "learning": {}, "global": {}, "run": {}, "graphs": {}}
    knn = B.KNNClassifier(6, k=3, capacity=1000, shape=SHAPE)
    index, words, labels = cases.clustered(SHAPE, 300, 1)
    knn.update_patterns(index, words, labels, device=0)                                 # (untraced: 300 slots, two blocks of the distance launch)
    for T in (1, 13, CHUNK, CHUNK + 1, 2 * CHUNK + 3):
        index, words, labels = cases.clustered(SHAPE, T, T)
        out["frozen"][f"T={T}"] = traced(lambda: knn.update_patterns(index, words, labels, learning=False))
    for T in (1, 13, CHUNK + 1):
        index, words, labels = cases.clustered(SHAPE, T, T)
        out["learning"][f"T={T}"] = traced(lambda: knn.update_patterns(index, words, labels))
    out["learning"]["unlabelled"] = traced(lambda: knn.update_patterns(index, words, np.full(len(index), -1)))
    wide = B.KNNClassifier(6, k=3, capacity=64, shape=GLOBAL_SHAPE)
    index, words, labels = cases.clustered(GLOBAL_SHAPE, 9, 2, columns=np.arange(50))
    wide.update_patterns(index, words, labels, device=0)
    for T in (5, CHUNK + 1):
        index, words, labels = cases.clustered(GLOBAL_SHAPE, T, T, columns=np.arange(50))
        out["global"][f"T={T}"] = traced(lambda: wide.update_patterns(index, words, labels, learning=False))

    inputs, _, names = cases.model_inputs()             # (every row labelled with its pattern's number)
    for key, use_graph in (("run", False), ("graphs", True)):
        plain, near = model(), model()
        kn, clf = B.KNNClassifier(6, k=3, capacity=1000), B.SDRClassifier(buckets=6, steps=(1, 3))
        targets = np.maximum(names, 0)
        for htm, kws in ((plain, [{}]), (near, [dict(classifier=clf, targets=targets), dict(classifier=clf, targets=targets, classifier_learning=False),
                                                dict(knn=kn, labels=names, classifier=clf, targets=targets), dict(knn=kn, labels=names)])):
            # (untraced: every kind of call once, so that its graphs and its buffers exist)
            htm.run(inputs, 6, record=True, use_graph=use_graph)
            htm.run(inputs, 6, use_graph=use_graph)
            for kw in kws:
                htm.run(inputs, 6, record=True, use_graph=use_graph, **kw)
        out[key]["recorded"] = traced(lambda: plain.run(inputs, 6, record=True, use_graph=use_graph))
        out[key]["knn"] = traced(lambda: near.run(inputs, 6, knn=kn, labels=names, use_graph=use_graph))
        out[key]["both"] = traced(lambda: near.run(inputs, 6, knn=kn, labels=names, classifier=clf, targets=targets, classifier_learning=False, use_graph=use_graph))
        out[key]["classified"] = traced(lambda: near.run(inputs, 6, classifier=clf, targets=targets, classifier_learning=False, use_graph=use_graph))
        out[key]["plain"] = traced(lambda: plain.run(inputs, 6, use_graph=use_graph))
        out[key]["recorded after"] = traced(lambda: near.run(inputs, 6, record=True, use_graph=use_graph))
        out[key]["plain after"] = traced(lambda: near.run(inputs, 6, use_graph=use_graph))

    # the refusals that need a bound model: nothing is enqueued
    htm = model()
    refused = {}

    def refuse(name, call, kind=ValueError):
        try:
            call()
            refused[name] = None
        except kind as e:
            refused[name] = str(e)
    small = B.KNNClassifier(6, k=3, capacity=4)
    htm.run(inputs, 3, knn=small, labels=names)
    n = len(lines())
    refuse("past capacity", lambda: htm.run(inputs, 2, knn=small, labels=names))
    refuse("labels shape", lambda: htm.run(inputs, 4, knn=small, labels=np.zeros(3, int)))
    refuse("labels dtype", lambda: htm.run(inputs, 4, knn=small, labels=np.zeros(len(inputs))))
    refuse("labels alone", lambda: htm.run(inputs, 4, labels=names))
    refuse("learning alone", lambda: htm.run(inputs, 4, knn_learning=True))
    refuse("another shape", lambda: htm.run(inputs, 4, knn=B.KNNClassifier(6, shape=(Cn, K, 3)), labels=names))
    refuse("patterns past capacity", lambda: small.update_patterns(np.arange(16).reshape(2, 8), np.ones((2, 8), np.uint32), [1, 2]))
    out["refused"], out["refused_lines"] = refused, lines()[n:]
    print(json.dumps(out))


if __name__ == "__main__":
    main()
