"""Driver of the launch traces of the classifier bank (tests/test_group_classifier_cpu.py; used as classifier_driver.py and
live_tick_driver.py are: the engine's host code host-only, no sanitizer, nothing preloaded, over tests/host_stub's runtime with
BITHTM_STUB_TRACE).

Prints one JSON object:
  "before"  the calls that existed before the bank, eagerly, per "B=<n>": {"tick", "scored tick": one tick behind a warm-up tick;
            "run", "recorded run": group.run of 6 steps}, and "graphs": the recorded run of B = 3 replayed from graphs.
            tests/golden/group_classifier_traces_before.json holds these lines as the commit before the bank gave them (this driver run
            with --before against that commit's host code): the test asserts that they are unchanged.
  "tick"    per "B=<n>": {"learning", "frozen", "scored learning", "packed frozen": one classified tick of that kind behind warm-ups}
  "run"     per "B=<n>": {"learning", "frozen": a classified group.run of 6 steps; "long frozen": of 2 * chunk + 3 steps}
  "graphs"  the classified run of B = 3 replayed from graphs
  "update"  per "n=<streams>": {"learning", "frozen": bank.update_patterns of 3 / of chunk + 1 steps}
  "refused" the messages of the refusals that need a bound group, "refused_lines" what they enqueued (nothing)

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

I, Cn, K, k = 64, 128, 64, 8
STEPS = (1, 3)
KW = dict(learning_period=4, estimation_samples=4, history=16, averaging_window=3, reestimation_period=2)


def lines():
    with open(TRACE) as f:
        return f.read().splitlines()


def traced(call):
    n = len(lines())
    call()
    return lines()[n:]


def group_of(n):
    return B.ModelGroup.create(n, I, Cn, K, active_columns=k, seeds=range(3, 3 + n))


def values(n, rows, seed):
    return np.random.RandomState(seed).rand(n, rows, 1) * 100.0


def before(out):
    enc = cases.model_encoder()
    for n in (1, 7):
        leg = out.setdefault(f"B={n}", {})
        group, scored = group_of(n), group_of(n)
        lk = B.AnomalyLikelihood(n, **KW)
        group.tick(values(n, 1, 1)[:, 0], encoder=enc, use_graph=False)
        scored.tick(values(n, 1, 1)[:, 0], encoder=enc, use_graph=False, likelihood=lk)
        leg["tick"] = traced(lambda: group.tick(values(n, 1, 2)[:, 0], encoder=enc, use_graph=False))
        leg["scored tick"] = traced(lambda: scored.tick(values(n, 1, 2)[:, 0], encoder=enc, use_graph=False, likelihood=lk))
        v = values(n, 10, 3)
        for g in (group, scored):                   # (untraced: every kind of call once)
            g.run(v, 6, encoder=enc, use_graph=False)
            g.run(v, 6, encoder=enc, use_graph=False, record=True)
        leg["run"] = traced(lambda: group.run(v, 6, encoder=enc, use_graph=False))
        leg["recorded run"] = traced(lambda: group.run(v, 6, encoder=enc, use_graph=False, record=True))
    group = group_of(3)
    v = values(3, 10, 4)
    group.run(v, 6, encoder=enc, record=True)
    out["graphs"] = traced(lambda: group.run(v, 6, encoder=enc, record=True))


def main():
    out = {"before": {}}
    before(out["before"])
    if "--before" in sys.argv:
        print(json.dumps(out["before"]))
        return
    from group_classifier_cases import chunk_steps
    enc = cases.model_encoder()
    out.update(tick={}, run={}, update={})
    for n in (1, 7):
        leg = out["tick"].setdefault(f"B={n}", {})
        group, scored, packed = group_of(n), group_of(n), group_of(n)
        lk = B.AnomalyLikelihood(n, **KW)
        banks = [B.SDRClassifierBank(n, field=enc.fields[0], steps=STEPS) for _ in range(3)]
        X = np.random.RandomState(5).rand(n, I) < 0.1
        tg = np.arange(n) % 5
        for learn in (True, False):                 # (untraced: the first tick of a kind allocates)
            group.tick(values(n, 1, 1)[:, 0], encoder=enc, use_graph=False, classifier=banks[0], classifier_learning=learn)
            scored.tick(values(n, 1, 1)[:, 0], encoder=enc, use_graph=False, likelihood=lk, classifier=banks[1], classifier_learning=learn)
            packed.tick(X, use_graph=False, classifier=banks[2], targets=tg, classifier_learning=learn)
        v = values(n, 1, 2)[:, 0]
        leg["learning"] = traced(lambda: group.tick(v, encoder=enc, use_graph=False, classifier=banks[0], classifier_learning=True))
        leg["frozen"] = traced(lambda: group.tick(v, encoder=enc, use_graph=False, classifier=banks[0], classifier_learning=False))
        leg["scored learning"] = traced(lambda: scored.tick(v, encoder=enc, use_graph=False, likelihood=lk, classifier=banks[1], classifier_learning=True))
        leg["packed frozen"] = traced(lambda: packed.tick(X, use_graph=False, classifier=banks[2], targets=tg, classifier_learning=False))
        leg["plain after"] = traced(lambda: group.tick(v, encoder=enc, use_graph=False))

        leg = out["run"].setdefault(f"B={n}", {})
        group = group_of(n)
        bank = B.SDRClassifierBank(n, field=enc.fields[0], steps=STEPS)
        v = values(n, 10, 3)
        long = 2 * chunk_steps(n, len(STEPS)) + 3
        for learn in (True, False):
            group.run(v, 6, encoder=enc, use_graph=False, classifier=bank, classifier_learning=learn)
        group.run(v, long, encoder=enc, use_graph=False, classifier=bank, classifier_learning=False)
        group.run(v, 6, encoder=enc, use_graph=False, record=True)
        leg["learning"] = traced(lambda: group.run(v, 6, encoder=enc, use_graph=False, classifier=bank, classifier_learning=True))
        leg["frozen"] = traced(lambda: group.run(v, 6, encoder=enc, use_graph=False, classifier=bank, classifier_learning=False))
        leg["long frozen"] = traced(lambda: group.run(v, long, encoder=enc, use_graph=False, classifier=bank, classifier_learning=False))
        leg["recorded after"] = traced(lambda: group.run(v, 6, encoder=enc, use_graph=False, record=True))
    group = group_of(3)
    bank = B.SDRClassifierBank(3, field=enc.fields[0], steps=STEPS)
    v = values(3, 10, 4)
    group.run(v, 6, encoder=enc, classifier=bank)
    group.run(v, 6, encoder=enc, record=True)
    out["graphs"] = {"classified": traced(lambda: group.run(v, 6, encoder=enc, classifier=bank)),
                     "recorded": traced(lambda: group.run(v, 6, encoder=enc, record=True))}

    p = cases.params(5, (0, 1, 5), 655, 48, 32, 40)
    for n in (1, 4):
        bank = B.SDRClassifierBank(n, buckets=5, steps=p["steps"], alpha=0.01, shape=(48, 32, 40))
        chunk = chunk_steps(n, 3)
        streams = lambda T, pairs: [np.stack([cases.stream(p, T, pairs, seed=T + i)[j] for i in range(n)]) for j in range(4)]
        index, words, targets, resets = streams(1, 17)
        bank.update_patterns(index, words, targets, learning=False, device=0)
        index, words, targets, resets = streams(chunk + 1, 17)
        frozen = traced(lambda: bank.update_patterns(index, words, targets, learning=False, resets=resets))
        index, words, targets, resets = streams(3, 40)
        out["update"][f"n={n}"] = {"frozen": frozen, "learning": traced(lambda: bank.update_patterns(index, words, targets, resets=resets))}

    # the refusals that need a bound group: nothing is enqueued
    group = group_of(2)
    refused = {}

    def refuse(name, call, kind=ValueError):
        try:
            call()
            refused[name] = None
        except kind as e:
            refused[name] = str(e)
    v = values(2, 10, 6)
    bank = B.SDRClassifierBank(2, field=enc.fields[0], steps=STEPS)
    n0 = len(lines())
    refuse("run: streams", lambda: group.run(v, 4, encoder=enc, classifier=B.SDRClassifierBank(3, field=enc.fields[0])))
    refuse("run: plain classifier", lambda: group.run(v, 4, encoder=enc, classifier=B.SDRClassifier(field=enc.fields[0])))
    refuse("run: no targets", lambda: group.run(v, 4, encoder=enc, classifier=B.SDRClassifierBank(2, buckets=3)))
    refuse("run: targets shape", lambda: group.run(v, 4, encoder=enc, classifier=bank, targets=np.zeros((2, 3), int)))
    refuse("run: targets above", lambda: group.run(v, 4, encoder=enc, classifier=B.SDRClassifierBank(2, buckets=3), targets=np.full((2, 10), 3)))
    refuse("run: targets alone", lambda: group.run(v, 4, encoder=enc, targets=np.zeros((2, 10), int)))
    refuse("run: resets", lambda: group.run(v, 4, encoder=enc, classifier=bank, resets=np.zeros(10, bool)), NotImplementedError)
    refuse("tick: streams", lambda: group.tick(v[:, 0], encoder=enc, classifier=B.SDRClassifierBank(3, field=enc.fields[0])))
    refuse("tick: plain classifier", lambda: group.tick(v[:, 0], encoder=enc, classifier=B.SDRClassifier(field=enc.fields[0])))
    refuse("tick: targets shape", lambda: group.tick(v[:, 0], encoder=enc, classifier=bank, targets=np.zeros(3, int)))
    refuse("tick: another shape", lambda: group.tick(v[:, 0], encoder=enc, classifier=B.SDRClassifierBank(2, buckets=3, shape=(Cn, K, 3)), targets=np.zeros(2, int)))
    refuse("tick: distribution alone", lambda: group.tick(v[:, 0], encoder=enc, class_distribution=True))
    refuse("solo run: a bank", lambda: group.models[0].run(v[0], 4, encoder=enc, classifier=bank))
    out["refused"], out["refused_lines"] = refused, lines()[n0:]
    print(json.dumps(out))


if __name__ == "__main__":
    main()
