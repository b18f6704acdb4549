"""What the SDR classifier costs on the device, as one JSON line (and, with --out, a file:
profiles/r18_classifier_rate.json).  Two shapes: "2048x32" (1 000 inputs -> 2 048 columns x 32 cells, 41 active) and "bench"
(bench.py's workload: 1 024 inputs -> 65 536 columns x 32 cells, 1 311 active); a bank of --patterns random patterns, the target of a
step the index of its pattern, horizons (1,), one bucket per pattern.  Per shape, behind --train untimed learning steps and two untimed
runs of each kind, --repeats rounds of --steps steps, the legs in alternating order, the median with the lowest and the highest:

  run_recorded           run(record=True): the recorded run without a classifier (the launches of the commit before the classifier:
                         tests/test_classifier_cpu.py holds the trace to that)
  run_classified         run(classifier=clf): pattern capture, the learning update (two launches per step) behind the batch
  run_classified_frozen  run(classifier=clf, classifier_learning=False): one update launch per 512 steps
  then_numpy             per step, the definition (bithtm_amd/classifier.py) looped on the host over --loop_steps of the patterns the
                         classified run captured, read back: what the same run followed by the NumPy definition would add
  kernels                device time per launch of kcls_capture, kcls_sum, kcls_apply and kcls_frozen (htm_profile, one launch per
                         kernel boundary)

    python tools/classifier_rate.py [--shapes 2048x32,bench] [--steps 1000] [--repeats 3] [--out profiles/r18_classifier_rate.json]
"""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np  # noqa: E402

import bithtm_amd as B  # noqa: E402
from bithtm_amd.classifier import ClassifierDefinition  # noqa: E402

SHAPES = {"2048x32": dict(input_dim=1000, column_dim=2048, cell_dim=32), "bench": dict(input_dim=1024, column_dim=65536, cell_dim=32)}


def log(*a):
    print(*a, file=sys.stderr, flush=True)


def median(times, per=1):
    ms = sorted(1e3 * t / per for t in times)
    return dict(ms=round(ms[len(ms) // 2], 4), lowest=round(ms[0], 4), highest=round(ms[-1], 4))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--shapes", default="2048x32,bench")
    ap.add_argument("--patterns", type=int, default=50)
    ap.add_argument("--steps", type=int, default=1000)
    ap.add_argument("--train", type=int, default=500)
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--loop_steps", type=int, default=20)
    ap.add_argument("--out")
    args = ap.parse_args()
    out = dict(tool="classifier_rate", steps=args.steps, patterns=args.patterns, horizons=[1], shapes={})
    for name in args.shapes.split(","):
        shape = SHAPES[name]
        np.random.seed(3)
        htm = B.HierarchicalTemporalMemory(seed=3, **shape)
        bank = np.random.RandomState(5).rand(args.patterns, shape["input_dim"]) < 0.02
        targets = np.arange(args.patterns)
        clf = B.SDRClassifier(buckets=args.patterns, steps=(1,), alpha=0.1)
        htm.run(bank, args.train)
        legs = dict(run_recorded=lambda: htm.run(bank, args.steps, record=True),
                    run_classified=lambda: htm.run(bank, args.steps, classifier=clf, targets=targets),
                    run_classified_frozen=lambda: htm.run(bank, args.steps, classifier=clf, targets=targets, classifier_learning=False))
        for _ in range(2):
            for fn in legs.values():
                fn()
        times = {leg: [] for leg in legs}
        for r in range(args.repeats):
            for leg in (list(legs) if r % 2 == 0 else list(legs)[::-1]):
                htm.engine.sync()
                t0 = time.perf_counter()
                rec = legs[leg]()
                times[leg].append(time.perf_counter() - t0)
        res = {leg: median(times[leg]) for leg in legs}
        res["steps_per_s"] = {leg: round(args.steps / (res[leg]["ms"] / 1e3)) for leg in legs}
        hits = rec.classified_bucket[:, 0] == (htm.engine.steps - args.steps + np.arange(args.steps) + 1) % args.patterns if rec.classified_bucket is not None else None
        res["hit_rate_of_the_last_classified_run"] = None if hits is None else round(float(hits.mean()), 4)
        res["weights_mib"] = round(shape["column_dim"] * shape["cell_dim"] * ((args.patterns + 3) & ~3) * 4 / 2 ** 20, 1)
        # the definition on the host over patterns the run captured
        eng = htm.engine
        per = clf.shape[2]
        n = min(args.loop_steps, args.steps)
        pairs = eng.read_words(clf._bufs["pairs"][0], 2 * n * per, np.int32).reshape(n, per, 2)
        d = ClassifierDefinition(args.patterns, (1,), 0.1, units=shape["column_dim"] * shape["cell_dim"], cell_dim=shape["cell_dim"])
        t0 = time.perf_counter()
        d.update(pairs[:, :, 0], pairs[:, :, 1].view(np.uint32), np.arange(n) % args.patterns)
        res["then_numpy"] = dict(ms_per_step=round(1e3 * (time.perf_counter() - t0) / n, 3), steps=n, pairs_per_step=per)
        # device time of the kernels
        eng.profile(True)
        htm.run(bank, 64, classifier=clf, targets=targets, use_graph=False)
        htm.run(bank, 64, classifier=clf, targets=targets, classifier_learning=False, use_graph=False)
        prof = eng.profile_read()
        eng.profile(False)
        res["kernels_us_per_launch"] = {k: dict(us=round(1e3 * ms / max(c, 1), 2), launches=c) for k, (ms, c) in prof.items()
                                        if k.startswith("classifier:") or k == "active_cells"}
        out["shapes"][name] = res
        log(name, res)
        del htm, clf
    print(json.dumps(out))
    if args.out:
        with open(args.out, "w") as fh:
            json.dump(out, fh, indent=1)


if __name__ == "__main__":
    main()
