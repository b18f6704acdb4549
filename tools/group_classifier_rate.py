"""What a bank of SDR classifiers costs on a group's live ticks and runs, at tools/tick_rate.py's shape (1 000
inputs -> 2 048 columns x 32 cells, two scalar fields, learned members), 50 buckets, horizon 1, as one JSON line (and, with --out, a
file: profiles/r19_group_classifier_rate.json).

  ticks    per group size B (default 1, 8, 64, 256), the legs taking turns in one process (every 20 ticks inside a round, the leg that
           comes first alternating), --repeats rounds, the median with the lowest and the highest: host wall time per group.tick(values,
           encoder=enc) unclassified, with a frozen bank and with a learning bank; the launches per tick of each (htm_profile) --
           expected: + 2 frozen, + 3 learning, whatever B is -- and the device time of each new launch
  host     the alternative without the bank, per tick: a one-step recorded group.run, every member's active cells read back, and the
           definition (bithtm_amd/classifier.py) looped per member -- over --host-ticks ticks (it costs milliseconds per member)
  twins    kcls_sum / kcls_apply of a one-stream SDRClassifier against kgcls_sum / kgcls_apply of a bank of one stream on IDENTICAL
           patterns (40 pairs a step: every cell of the word set -- bursting columns -- or one cell), device time per launch under
           htm_profile, the two objects taking turns, --repeats rounds
  run      at --run-size members: group.run(values, --steps steps, encoder=enc, classifier=bank, targets=) against the same run with
           record=True, behind two untimed runs, the leg that comes first alternating

    python tools/group_classifier_rate.py [--sizes 1,8,64,256] [--ticks 200] [--steps 1000] [--repeats 3] [--out profiles/r19_group_classifier_rate.json]
"""
import argparse
import json
import os
import sys
import time

os.environ["BITHTM_EAGER_BELOW"] = "0"
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))
import numpy as np  # noqa: E402

import bithtm_amd as B  # noqa: E402
from bithtm_amd.classifier import ClassifierDefinition  # noqa: E402
from tick_rate import SHAPE, encoder, log, spread, stream  # noqa: E402

SLICE = 20                                  # ticks a leg takes before the next leg's turn
BUCKETS, STEPS, ALPHA = 50, (1,), 0.01
NEW_LAUNCHES = ("group:active_cells", "classifiers:sum", "classifiers:apply", "classifiers:frozen")


def median(times):
    ms = sorted(1e3 * t for t in times)
    return dict(ms=round(ms[len(ms) // 2], 3), lowest=round(ms[0], 3), highest=round(ms[-1], 3))


def targets_of(values):
    """The bucket of the first field's value among 50 buckets over [0, 100]."""
    return np.clip(np.floor(values[..., 0] / 2.0), 0, BUCKETS - 1).astype(np.int32)


def pairs_of(activation, columns):
    """bool [C, 32] and the step's active columns -> the pattern the device captures (cell_dim 32: one word a column)."""
    words = np.packbits(activation[columns].astype(np.uint8), axis=1, bitorder="little").view(np.uint32).reshape(-1)
    return zip(np.asarray(columns, dtype=np.int64), words)


def twins(model, repeats, steps=100):
    """Device us per launch of the solo kernels and of their member-major twins over the same patterns -> {pattern kind: {launch: median}}."""
    eng = model.engine
    rng = np.random.RandomState(3)
    C, K, pairs = SHAPE["column_dim"], SHAPE["cell_dim"], 40
    index = np.stack([rng.choice(C, pairs, replace=False) for _ in range(steps)]).astype(np.int32)
    targets = rng.randint(0, BUCKETS, steps).astype(np.int32)
    out = {}
    for label, word in (("bursting", 0xFFFFFFFF), ("predicted", 1)):
        words = np.full((steps, pairs), word, dtype=np.uint32)
        solo = B.SDRClassifier(buckets=BUCKETS, steps=STEPS, alpha=ALPHA, shape=(C, K, pairs)).bind(model)
        bank = B.SDRClassifierBank(1, buckets=BUCKETS, steps=STEPS, alpha=ALPHA, shape=(C, K, pairs)).bind(model)
        calls = dict(solo=lambda: solo.update_patterns(index, words, targets), bank=lambda: bank.update_patterns(index[None], words[None], targets[None]))
        for fn in calls.values():
            fn()
        seen = {}
        for r in range(repeats):
            for name in (("solo", "bank") if r % 2 == 0 else ("bank", "solo")):
                eng.sync()
                eng.profile(True)
                calls[name]()
                prof = eng.profile_read()
                eng.profile(False)
                for launch, (ms, count) in prof.items():
                    if launch.startswith("classifier") and count > 0:
                        seen.setdefault(launch, []).append(1e3 * ms / count)
        out[label] = {launch: round(sorted(us)[len(us) // 2], 2) for launch, us in sorted(seen.items())}
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sizes", default="1,8,64,256")
    ap.add_argument("--ticks", type=int, default=200)
    ap.add_argument("--host-ticks", type=int, default=4)
    ap.add_argument("--steps", type=int, default=1000)
    ap.add_argument("--run-size", type=int, default=64)
    ap.add_argument("--train", type=int, default=200)
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--out")
    args = ap.parse_args()
    enc = encoder()
    units = SHAPE["column_dim"] * SHAPE["cell_dim"]
    out = dict(tool="group_classifier_rate", shape="1000 inputs -> 2048 columns x 32 cells, 2 fields, 50 buckets, horizon 1", ticks=args.ticks, steps=args.steps,
               sizes={})
    for n in [int(x) for x in args.sizes.split(",")]:
        group = B.ModelGroup.create(n, seeds=range(n), **SHAPE)
        rows = args.train + max(args.ticks, args.steps if n == args.run_size else 0)
        values = stream(n, rows, 7 + n)
        banked = np.ascontiguousarray(values.transpose(1, 0, 2))
        group.run(banked[:, :args.train], args.train, encoder=enc)
        live = values[args.train:]
        sync = group.models[0].engine.sync
        frozen, learning = B.SDRClassifierBank(n, buckets=BUCKETS, steps=STEPS, alpha=ALPHA), B.SDRClassifierBank(n, buckets=BUCKETS, steps=STEPS, alpha=ALPHA)
        legs = dict(tick=lambda v: group.tick(v, encoder=enc),
                    tick_frozen=lambda v: group.tick(v, encoder=enc, classifier=frozen, targets=targets_of(v), classifier_learning=False),
                    tick_learning=lambda v: group.tick(v, encoder=enc, classifier=learning, targets=targets_of(v), classifier_learning=True))
        times = {name: [] for name in legs}
        for fn in legs.values():                    # (untraced: the first tick of a kind allocates)
            fn(live[0])
        names = list(legs)
        for r in range(args.repeats):
            spent, at = {name: 0.0 for name in legs}, 0
            for piece in range(-(-args.ticks // SLICE)):
                count = min(SLICE, args.ticks - piece * SLICE)
                order = names[(piece + r) % 3:] + names[:(piece + r) % 3]
                for name in order:
                    sync()
                    t0 = time.perf_counter()
                    for t in range(at, at + count):
                        legs[name](live[t % len(live)])
                    sync()
                    spent[name] += time.perf_counter() - t0
                at += count
            for name in legs:
                times[name].append(spent[name])
        res = {name: spread(times[name], args.ticks) for name in legs}
        eng = group.models[0].engine
        for name, fn in legs.items():
            fn(live[0])
            eng.profile(True)
            for t in range(20):
                fn(live[t % len(live)])
            prof = eng.profile_read()
            eng.profile(False)
            res[name]["launches_per_tick"] = sum(c for _, c in prof.values()) / 20
            res[name]["device_us"] = round(1e3 * sum(ms for ms, _ in prof.values()) / 20, 1)
            for launch in NEW_LAUNCHES:
                if launch in prof and prof[launch][1] > 0:
                    res[name][launch + "_us"] = round(1e3 * prof[launch][0] / prof[launch][1], 2)
        # the host alternative: a recorded one-step run, the active cells read back, the definition looped per member
        defs = [ClassifierDefinition(BUCKETS, STEPS, ALPHA, units=units, cell_dim=SHAPE["cell_dim"]) for _ in range(n)]

        def host_tick(v):
            recs = group.run(v[:, None], 1, encoder=enc, record=("counters", "active_column"))
            tg = targets_of(v)
            for i, (m, rec, d) in enumerate(zip(group.models, recs, defs)):
                act = np.asarray(m.temporal_memory.last_state.cell_activation)
                d.step(pairs_of(act, np.sort(rec.active_column[0])), tg[i], False, True, False)
        host_tick(live[0])
        ts = []
        for r in range(args.repeats):
            sync()
            t0 = time.perf_counter()
            for t in range(args.host_ticks):
                host_tick(live[t % len(live)])
            ts.append(time.perf_counter() - t0)
        res["host_alternative"] = spread(ts, args.host_ticks)
        if n == args.run_size:
            rows_run = banked[:, args.train:args.train + args.steps]
            tg = targets_of(rows_run)
            bank = B.SDRClassifierBank(n, buckets=BUCKETS, steps=STEPS, alpha=ALPHA)
            classified, recorded = [], []

            def timed(store, **kw):
                sync()
                t0 = time.perf_counter()
                group.run(rows_run, args.steps, encoder=enc, **kw)
                store.append(time.perf_counter() - t0)
            for _ in range(2):                      # untimed: the banks' upload, the object's buffers, the pools' growth to this stream
                group.run(rows_run, args.steps, encoder=enc, classifier=bank, targets=tg)
            for r in range(args.repeats):
                for leg in ((0, 1) if r % 2 == 0 else (1, 0)):
                    if leg == 0:
                        timed(classified, classifier=bank, targets=tg)
                    else:
                        timed(recorded, record=True)
            res["run_classified"], res["run_recorded"] = median(classified), median(recorded)
        if "twins_us_per_launch" not in out:
            out["twins_us_per_launch"] = twins(group.models[0], args.repeats)
            log("twins", out["twins_us_per_launch"])
        out["sizes"][str(n)] = res
        log(n, res)
        del group, frozen, learning
    print(json.dumps(out))
    if args.out:
        with open(args.out, "w") as fh:
            json.dump(out, fh, indent=1)


if __name__ == "__main__":
    main()
