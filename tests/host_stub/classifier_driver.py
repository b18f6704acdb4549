"""Driver of the launch traces of the SDR classifier (tests/test_classifier_cpu.py; used as likelihood_driver.py is: the engine's host
code host-only, no sanitizer, nothing preloaded, over tests/host_stub's runtime with BITHTM_STUB_TRACE).

Prints one JSON object:
  "frozen"   {"T=<steps>": the trace lines of update_patterns(learning=False) over T steps}
  "learning" {"T=<steps>": ... of update_patterns over T steps}
  "run"      the lines of runs of 6 steps on twin models with the same history (every kind of call made once before), launched eagerly:
               "recorded"       run(record=True)
               "classified"     run(classifier=) on the twin whose last run was classified
               "plain"          run()
               "recorded after", "plain after"   the same two calls on the twin that has just made the classified runs
  "graphs"   the same recorded and classified second runs replayed from graphs
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
import classifier_cases as cases  # noqa: E402
from classifier_cases import CHUNK  # noqa: E402

I, Cn, K, k = 64, 128, 64, 8


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
    out = {"frozen": {}, "learning": {}, "run": {}, "graphs": {}}
    p = cases.params(5, (0, 1, 5), 655, 48, 32, 40)
    clf = B.SDRClassifier(buckets=5, steps=p["steps"], alpha=0.01, shape=(48, 32, 40))
    for T in (1, CHUNK, CHUNK + 1, 2 * CHUNK + 3):
        index, words, targets, resets = cases.stream(p, T, 17, seed=T)
        if T == 1:
            clf.update_patterns(index, words, targets, learning=False, device=0)        # (untraced: the first frozen call allocates)
        out["frozen"][f"T={T}"] = traced(lambda: clf.update_patterns(index, words, targets, learning=False, resets=resets, device=0))
    for T in (1, 7):
        index, words, targets, resets = cases.stream(p, T, 40, seed=T)
        out["learning"][f"T={T}"] = traced(lambda: clf.update_patterns(index, words, targets, resets=resets))

    enc = cases.model_encoder()
    values, flags = cases.model_values()
    for key, use_graph in (("run", False), ("graphs", True)):
        plain, classified = model(), model()
        c = B.SDRClassifier(field=enc.fields[0], steps=(1, 3))
        for htm, kw in ((plain, {}), (classified, dict(classifier=c))):         # (untraced: every kind of call once, so that its graphs exist)
            htm.run(values, 6, encoder=enc, record=True, use_graph=use_graph)
            htm.run(values, 6, encoder=enc, use_graph=use_graph)
            htm.run(values, 6, encoder=enc, record=True, use_graph=use_graph, **kw)
        out[key]["recorded"] = traced(lambda: plain.run(values, 6, encoder=enc, record=True, use_graph=use_graph))
        out[key]["classified"] = traced(lambda: classified.run(values, 6, encoder=enc, classifier=c, use_graph=use_graph))
        out[key]["plain"] = traced(lambda: plain.run(values, 6, encoder=enc, use_graph=use_graph))
        out[key]["recorded after"] = traced(lambda: classified.run(values, 6, encoder=enc, record=True, use_graph=use_graph))
        out[key]["plain after"] = traced(lambda: classified.run(values, 6, encoder=enc, use_graph=use_graph))

    # the refusals that need a bound model: nothing is enqueued
    htm = model()
    refused = {}

    def refuse(name, call, kind=ValueError):
        try:
            call()
            refused[name] = None
        except kind as e:
            refused[name] = str(e)
    c = B.SDRClassifier(field=enc.fields[0])
    n = len(lines())
    refuse("targets above", lambda: htm.run(values, 4, encoder=enc, classifier=B.SDRClassifier(buckets=3), targets=np.arange(10)))
    refuse("targets shape", lambda: htm.run(values, 4, encoder=enc, classifier=c, targets=np.zeros(3, int)))
    refuse("no targets", lambda: htm.run(values, 4, encoder=enc, classifier=B.SDRClassifier(buckets=3)))
    refuse("foreign field", lambda: htm.run(values, 4, encoder=enc, classifier=B.SDRClassifier(field=B.ScalarField(0, 1, 64, 9))))
    refuse("targets alone", lambda: htm.run(values, 4, encoder=enc, targets=np.zeros(10, int)))
    other = B.SDRClassifier(buckets=3, shape=(Cn, K, 3))
    refuse("another shape", lambda: htm.run(values, 4, encoder=enc, classifier=other, targets=np.zeros(10, int)))
    out["refused"], out["refused_lines"] = refused, lines()[n:]
    print(json.dumps(out))


if __name__ == "__main__":
    main()
