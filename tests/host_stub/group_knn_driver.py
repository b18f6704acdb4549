"""Driver of the launch traces of the KNN classifier banks (tests/test_group_knn_cpu.py; used as knn_driver.py is: the engine's host code
host-only, no sanitizer, nothing preloaded, over tests/host_stub's runtime with BITHTM_STUB_TRACE).

Prints one JSON object.  Section "before" holds the calls that existed before the banks -- run with the argument `before` it prints that
section alone, which is how tests/golden/group_knn_traces_before.json was recorded from the commit before the banks:
  "before"   "knn frozen", "knn learning"   update_patterns of a one-stream KNNClassifier over 5 steps on a store of 300 slots
             "run knn"                      htm.run(knn=) of 6 steps, eager
             per mode ("run": eager, "graphs"), a group of three members with the same history:
               "<mode> plain", "<mode> recorded", "<mode> classified"   group.run of 6 steps
             "tick plain", "tick classified"                            group.tick, eager
The other sections need the banks:
  "update"   {"S=<streams> learning T=1" / "frozen T=1" / "learning T=<chunk + 3>": bank.update_patterns on stores of up to 300 slots}
  "unlabelled"  a learning call in which no stream has a label
  "global"   a frozen call of 5 steps on a bank of 2 streams whose tables lie in the global scratch table
  "shared"   {"S=<streams> T=<steps>": a shared bank over a one-stream store of 300 slots}
  per mode   "<mode> knn", "<mode> both": group.run(knn=bank) and group.run(knn=bank, classifier=) on the same group
  "tick"     {"B=<members> plain" / "learning" / "unlabelled" / "frozen" / "both": group.tick without knn=, with a learning bank (every
             member labelled; no member labelled), with a frozen one, and with classifier= and knn= together; "views B=9": a shared bank}
  "tick_waits"  per key of "tick": the hipStreamSynchronize calls of that tick (the stub's trace has no line for a wait; the library is
             linked with tests/host_stub/wait_counter.cpp, which counts them in the file BITHTM_STUB_WAITS names)
  "refused"  the messages of the refusals that need a bound group, "refused_lines" what they enqueued (nothing)

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
MEMBERS = 3


def lines():
    with open(TRACE) as f:
        return f.read().splitlines()


def traced(call):
    n = len(lines())
    call()
    return lines()[n:]


def waits():
    path = os.environ.get("BITHTM_STUB_WAITS")
    if not path or not os.path.exists(path):
        return 0
    with open(path) as f:
        return len(f.read().splitlines())


def traced_waits(call):
    """-> (the trace lines of the call, its waits)."""
    n = waits()
    got = traced(call)
    return got, waits() - n


def model(seed=3):
    np.random.seed(seed)
    tm = B.TemporalMemory(Cn, K, distal_projection=B.PredictiveProjection(Cn * K, segment_capacity=8192), seed=seed)
    return B.HierarchicalTemporalMemory(I, Cn, K, active_columns=k, temporal_memory=tm)


def group():
    return B.ModelGroup([model() for _ in range(MEMBERS)])


def before(with_banks):
    """The section "before" -- and, with the banks, the group sections "<mode> knn" and "<mode> both" taken on the same groups."""
    out, more = {}, {}
    knn = B.KNNClassifier(6, k=3, capacity=1000, shape=SHAPE)
    index, words, labels = cases.clustered(SHAPE, 300, 1)
    knn.update_patterns(index, words, labels, device=0)                                 # (untraced: 300 slots)
    index, words, labels = cases.clustered(SHAPE, 5, 5)
    out["knn frozen"] = traced(lambda: knn.update_patterns(index, words, labels, learning=False))
    out["knn learning"] = traced(lambda: knn.update_patterns(index, words, labels))
    inputs, _, names = cases.model_inputs()
    htm, kn = model(), B.KNNClassifier(6, k=3, capacity=1000)
    htm.run(inputs, 6, knn=kn, labels=names, use_graph=False)
    out["run knn"] = traced(lambda: htm.run(inputs, 6, knn=kn, labels=names, use_graph=False))
    every, targets = np.stack([inputs] * MEMBERS), np.stack([np.maximum(names, 0)] * MEMBERS)
    every_names = np.stack([names] * MEMBERS)
    for mode, use_graph in (("run", False), ("graphs", True)):
        g, clf = group(), B.SDRClassifierBank(MEMBERS, buckets=6, steps=(1, 3))
        kws = [{}, dict(record=True), dict(classifier=clf, targets=targets, classifier_learning=False)]
        if with_banks:
            bank = B.KNNClassifierBank(MEMBERS, 6, k=3, capacity=1000)
            kws += [dict(knn=bank, labels=every_names), dict(knn=bank, labels=every_names, classifier=clf, targets=targets, classifier_learning=False)]
        for kw in kws:                              # (untraced: every kind of call once, so that its graphs and its buffers exist)
            g.run(every, 6, use_graph=use_graph, **kw)
        if with_banks:
            more[f"{mode} knn"] = traced(lambda: g.run(every, 6, use_graph=use_graph, **kws[3]))
            more[f"{mode} both"] = traced(lambda: g.run(every, 6, use_graph=use_graph, **kws[4]))
        for name, kw in zip(("plain", "recorded", "classified"), kws):
            out[f"{mode} {name}"] = traced(lambda: g.run(every, 6, use_graph=use_graph, **kw))
    g, clf = group(), B.SDRClassifierBank(MEMBERS, buckets=6, steps=(1, 3))
    for _ in range(2):                              # (both parities once, untraced)
        g.tick(every[:, 0], use_graph=False)
        g.tick(every[:, 0], classifier=clf, targets=targets[:, 0], use_graph=False)
    out["tick plain"] = traced(lambda: g.tick(every[:, 0], use_graph=False))
    out["tick classified"] = traced(lambda: g.tick(every[:, 1], classifier=clf, targets=targets[:, 1], use_graph=False))
    return out, more


def streams(shape, S, T, seed, **kw):
    parts = [cases.clustered(shape, T, seed + s, **kw) for s in range(S)]
    return tuple(np.stack([p[j] for p in parts]) for j in range(3))


def main():
    if sys.argv[1:] == ["before"]:
        print(json.dumps({"before": before(False)[0]}))
        return
    out = {"update": {}, "shared": {}}
    out["before"], more = before(True)
    out.update(more)
    for S in (1, 7):
        bank = B.KNNClassifierBank(S, 6, k=3, capacity=1000, shape=SHAPE)
        index, words, labels = streams(SHAPE, S, 300, 1)
        labels[-1, 40:] = -1                        # (the last stream holds 40 slots, the others 300: the grid is the largest's)
        bank.update_patterns(index, words, labels, device=0)
        for T, learning in ((1, True), (1, False), (CHUNK + 3, True)):
            index, words, labels = streams(SHAPE, S, T, 5)
            out["update"][f"S={S} {'learning' if learning else 'frozen'} T={T}"] = traced(lambda: bank.update_patterns(index, words, labels, learning=learning))
        if S == 7:
            out["unlabelled"] = traced(lambda: bank.update_patterns(index, words, None))
    wide = B.KNNClassifierBank(2, 6, k=3, capacity=64, shape=GLOBAL_SHAPE)
    index, words, labels = streams(GLOBAL_SHAPE, 2, 9, 2, columns=np.arange(50))
    wide.update_patterns(index, words, labels, device=0)
    index, words, labels = streams(GLOBAL_SHAPE, 2, 5, 3, columns=np.arange(50))
    out["global"] = traced(lambda: wide.update_patterns(index, words, None, learning=False))
    src = B.KNNClassifier(6, k=3, capacity=1000, shape=SHAPE)
    index, words, labels = cases.clustered(SHAPE, 300, 1)
    src.update_patterns(index, words, labels, device=0)
    for S, T in ((9, 1), (64, 1), (9, CHUNK // 8 + 1)):
        shared = B.KNNClassifierBank.shared(src, S)
        index, words, _ = streams(SHAPE, S, T, 7)
        shared.update_patterns(index, words, None, learning=False)                      # (untraced: the first call allocates)
        out["shared"][f"S={S} T={T}"] = traced(lambda: shared.update_patterns(index, words, None, learning=False))

    inputs, _, names = cases.model_inputs()
    out["tick"], out["tick_waits"] = {}, {}
    for n in (1, 7):
        g = B.ModelGroup.create(n, I, Cn, K, active_columns=k)      # (on one shared stream, as live groups are made: the group joins no member streams)
        bank, clf = B.KNNClassifierBank(n, 6, k=3, capacity=1000), B.SDRClassifierBank(n, buckets=6, steps=(1, 3))
        X, lab, none = np.stack([inputs[0]] * n), np.full(n, 2), np.full(n, -1)
        kinds = {"plain": {}, "learning": dict(knn=bank, labels=lab), "unlabelled": dict(knn=bank, labels=none), "frozen": dict(knn=bank, knn_learning=False),
                 "both": dict(knn=bank, labels=lab, classifier=clf, targets=lab), "classified": dict(classifier=clf, targets=lab)}
        for _ in range(2):                          # (both parities once, untraced)
            for kw in kinds.values():
                g.tick(X, use_graph=False, **kw)
        for name, kw in kinds.items():
            out["tick"][f"B={n} {name}"], out["tick_waits"][f"B={n} {name}"] = traced_waits(lambda: g.tick(X, use_graph=False, **kw))
    parent, own = model(), B.KNNClassifier(6, k=3, capacity=1000)
    parent.run(inputs, 30, knn=own, labels=names)
    views, shared = B.ModelGroup.views(parent, 9), B.KNNClassifierBank.shared(own, 9)
    X = np.stack([inputs[0]] * 9)
    for _ in range(2):
        views.tick(X, knn=shared, use_graph=False)
        views.tick(X, use_graph=False)
    out["tick"]["views B=9"], out["tick_waits"]["views B=9"] = traced_waits(lambda: views.tick(X, knn=shared, use_graph=False))
    out["tick"]["views B=9 plain"], out["tick_waits"]["views B=9 plain"] = traced_waits(lambda: views.tick(X, use_graph=False))

    # the refusals that need a bound group: nothing is enqueued
    every, every_names = np.stack([inputs] * MEMBERS), np.stack([names] * MEMBERS)
    g, small = group(), B.KNNClassifierBank(MEMBERS, 6, k=3, capacity=4)
    refused = {}

    def refuse(name, call, kind=ValueError):
        try:
            call()
            refused[name] = None
        except kind as e:
            refused[name] = str(e)
    g.run(every, 3, knn=small, labels=every_names)
    g.tick(every[:, 0], knn=small, labels=np.array([-1, 2, -1]))       # (stream 1 is full now)
    n = len(lines())
    only_one = np.where(np.arange(MEMBERS)[:, None] == 1, every_names, -1)
    refuse("one stream past capacity", lambda: g.run(every, 2, knn=small, labels=only_one))
    refuse("labels shape", lambda: g.run(every, 4, knn=small, labels=names))
    refuse("labels alone", lambda: g.run(every, 4, labels=every_names))
    refuse("learning alone", lambda: g.run(every, 4, knn_learning=True))
    refuse("another stream count", lambda: g.run(every, 4, knn=B.KNNClassifierBank(2, 6)))
    refuse("one stream on a group", lambda: g.run(every, 4, knn=B.KNNClassifier(6)))
    refuse("a tick past capacity", lambda: g.tick(every[:, 0], knn=small, labels=np.array([-1, 2, -1])))
    refuse("tick labels alone", lambda: g.tick(every[:, 0], labels=np.array([-1, 2, -1])))
    refuse("one stream on a tick", lambda: g.tick(every[:, 0], knn=B.KNNClassifier(6)))
    refuse("a bank on one model", lambda: g.models[0].run(inputs, 4, knn=small))
    refuse("another shape", lambda: g.run(every, 4, knn=B.KNNClassifierBank(MEMBERS, 6, shape=(Cn, K, 3))))
    out["refused"], out["refused_lines"] = refused, lines()[n:]
    print(json.dumps(out))


if __name__ == "__main__":
    main()
