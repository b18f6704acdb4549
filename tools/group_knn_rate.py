"""What a bank of KNN classifiers costs on a group's live ticks and runs, at tools/tick_rate.py's shape (1 000
inputs -> 2 048 columns x 32 cells, two scalar fields, learned members), k = 5, stores of --slots slots (default 1 024 and 16 384)
filled with random patterns of 40 pairs, as one JSON line (and, with --out, a file: profiles/r21_group_knn_rate.json).

  ticks    per group size B (default 1, 8, 64, 256) and store size, the legs taking turns in one process (every 20 ticks inside a round,
           the leg that comes first alternating), --repeats rounds, the median with the lowest and the highest: host wall time per
           group.tick(values, encoder=enc) without knn=, with a frozen bank and with a learning bank (every member labelled); the launches
           per tick of each (htm_profile) and the device time of each new launch.  Own stores of 16 384 slots are measured up to
           --big-limit members (B x 5.3 MiB of store are built on the host first)
  views    the same over ModelGroup.views(parent, B) with KNNClassifierBank.shared(knn, B), against what there was before the banks: B
           one-stream view.run(values, 1, knn=knn) calls per tick
  host     the other alternative, per tick: a one-step recorded group.run, every member's active cells read back, and the definition
           (bithtm_amd/knn.py) looped per member over a store of the same size -- over --host-ticks ticks
  twins    kknn_distance_lds of a one-stream KNNClassifier against kgknn_distance_lds of a bank of one stream on IDENTICAL patterns and
           stores, device time per launch under htm_profile, the two objects taking turns
  run      at --run-size members: group.run(values, --steps steps, encoder=enc, knn=bank) frozen against the same run with record=True

    python tools/group_knn_rate.py [--sizes 1,8,64,256] [--slots 1024,16384] [--ticks 200] [--steps 1000] [--repeats 3] [--out profiles/r21_group_knn_rate.json]
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
from bithtm_amd.knn import KNNDefinition  # noqa: E402
from bithtm_amd.sdr_classifier import model_shape  # noqa: E402
from tick_rate import SHAPE, encoder, log, spread, stream  # noqa: E402

SLICE = 20                                  # ticks a leg takes before the next leg's turn
LABELS, K_NEAR = 12, 5
NEW_LAUNCHES = ("group:active_cells", "knns:append", "knns:distance", "knns:select")


def median(times):
    ms = sorted(1e3 * t for t in times)
    return dict(ms=round(ms[len(ms) // 2], 3), lowest=round(ms[0], 3), highest=round(ms[-1], 3))


def store(slots, seed, n_pairs):
    """A store of `slots` random patterns: n_pairs columns of 2 048 with three cells each -> (pairs int32 [slots, n_pairs, 2], labels, stamps)."""
    rng = np.random.default_rng(seed)
    cols = np.argsort(rng.random((slots, SHAPE["column_dim"])), axis=1)[:, :n_pairs].astype(np.int32)
    words = (1 << rng.integers(0, 32, (slots, n_pairs))) | (1 << rng.integers(0, 32, (slots, n_pairs))) | (1 << rng.integers(0, 32, (slots, n_pairs)))
    pairs = np.stack([cols, words.astype(np.uint32).view(np.int32)], axis=2)
    return np.ascontiguousarray(pairs), rng.integers(0, LABELS, slots).astype(np.int32), np.arange(slots, dtype=np.int64)


def params(capacity, n_pairs):
    return np.array([LABELS, K_NEAR, 1, capacity, SHAPE["column_dim"], SHAPE["cell_dim"], n_pairs], dtype=np.int64)


def solo_of(slots, capacity, n_pairs, seed=1):
    pairs, labels, stamps = store(slots, seed, n_pairs)
    knn = B.KNNClassifier(LABELS, k=K_NEAR, capacity=capacity)
    knn.load_state_dict(dict(params=params(capacity, n_pairs), total=np.int64(slots), count=np.int64(slots), pairs=pairs, labels=labels, stamps=stamps))
    return knn


def bank_of(n, slots, capacity, n_pairs, seed=1):
    pairs, labels, stamps = store(slots, seed, n_pairs)     # (every stream holds the same slots: the cost does not depend on what they hold)
    bank = B.KNNClassifierBank(n, LABELS, k=K_NEAR, capacity=capacity)
    bank.load_state_dict(dict(params=params(capacity, n_pairs), streams=np.int64(n), total=np.int64(slots), count=np.full(n, slots, dtype=np.int64),
                              pairs=np.tile(pairs, (n, 1, 1)), labels=np.tile(labels, n), stamps=np.tile(stamps, n)))
    return bank


def pairs_of(activation, columns):
    words = np.packbits(activation[columns].astype(np.uint8), axis=1, bitorder="little").view(np.uint32).reshape(-1)
    return zip(np.asarray(columns, dtype=np.int64), words)


def timed_legs(legs, ticks, repeats, sync, rows):
    times = {name: [] for name in legs}
    for fn in legs.values():                        # (untimed: the first tick of a kind allocates)
        fn(rows[0])
    names = list(legs)
    for r in range(repeats):
        spent, at = {name: 0.0 for name in legs}, 0
        for piece in range(-(-ticks // SLICE)):
            count = min(SLICE, ticks - piece * SLICE)
            shift = (piece + r) % len(names)
            for name in names[shift:] + names[:shift]:
                sync()
                t0 = time.perf_counter()
                for t in range(at, at + count):
                    legs[name](rows[t % len(rows)])
                sync()
                spent[name] += time.perf_counter() - t0
            at += count
        for name in legs:
            times[name].append(spent[name])
    return {name: spread(times[name], ticks) for name in legs}


def profiled(res, legs, eng, rows):
    for name, fn in legs.items():
        fn(rows[0])
        eng.profile(True)
        for t in range(20):
            fn(rows[t % len(rows)])
        prof = eng.profile_read()
        eng.profile(False)
        res[name]["launches_per_tick"] = sum(c for _, c in prof.values()) / 20
        res[name]["device_us"] = round(1e3 * sum(ms for ms, _ in prof.values()) / 20, 1)
        for launch in NEW_LAUNCHES + ("knn:distance", "knn:select"):
            if launch in prof and prof[launch][1] > 0:
                res[name][launch + "_us"] = round(1e3 * prof[launch][0] / prof[launch][1], 2)


def twins(model, slots, repeats, n_pairs, steps=64):
    """Device us per launch of the one-stream distance kernel and of the bank's over the same store and queries."""
    eng = model.engine
    solo, bank = solo_of(slots, slots + steps, n_pairs).bind(model), bank_of(1, slots, slots + steps, n_pairs).bind(model)
    pairs, _, _ = store(steps, 5, n_pairs)
    index, words, none = pairs[:, :, 0], pairs[:, :, 1].view(np.uint32), np.full(steps, -1)
    calls = dict(solo=lambda: solo.update_patterns(index, words, none, learning=False), bank=lambda: bank.update_patterns(index[None], words[None], None, learning=False))
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
                if launch.startswith("knn") and count > 0:
                    seen.setdefault(launch, []).append(1e3 * ms / count)
    return {launch: round(sorted(us)[len(us) // 2], 2) for launch, us in sorted(seen.items())}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sizes", default="1,8,64,256")
    ap.add_argument("--slots", default="1024,16384")
    ap.add_argument("--big-limit", type=int, default=64)
    ap.add_argument("--ticks", type=int, default=200)
    ap.add_argument("--host-ticks", type=int, default=2)
    ap.add_argument("--steps", type=int, default=1000)
    ap.add_argument("--run-size", type=int, default=64)
    ap.add_argument("--train", type=int, default=200)
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--out")
    args = ap.parse_args()
    enc = encoder()
    slot_sizes = [int(x) for x in args.slots.split(",")]
    out = dict(tool="group_knn_rate", shape="1000 inputs -> 2048 columns x 32 cells, 2 fields, k = 5, 40 pairs a pattern", ticks=args.ticks, steps=args.steps, sizes={})
    for n in [int(x) for x in args.sizes.split(",")]:
        group = B.ModelGroup.create(n, seeds=range(n), **SHAPE)
        n_pairs = model_shape(group.models[0].engine)[2]    # (the pairs a captured step has: active columns x words per column)
        rows = args.train + max(args.ticks, args.steps if n == args.run_size else 0)
        values = stream(n, rows, 7 + n)
        banked = np.ascontiguousarray(values.transpose(1, 0, 2))
        group.run(banked[:, :args.train], args.train, encoder=enc)
        live = values[args.train:]
        sync = group.models[0].engine.sync
        names = np.arange(n) % LABELS
        res = {}
        for slots in slot_sizes:
            if slots > 4096 and n > args.big_limit:
                res[f"own {slots}"] = "not measured: above --big-limit members"
            else:
                frozen, learning = bank_of(n, slots, slots + 64, n_pairs), bank_of(n, slots, slots + 8 * args.ticks * (args.repeats + 2), n_pairs)
                legs = dict(tick=lambda v: group.tick(v, encoder=enc), tick_frozen=lambda v: group.tick(v, encoder=enc, knn=frozen, knn_learning=False),
                            tick_learning=lambda v: group.tick(v, encoder=enc, knn=learning, labels=names))
                part = timed_legs(legs, args.ticks, args.repeats, sync, live)
                profiled(part, legs, group.models[0].engine, live)
                part["chunk"], part["device_mib"] = frozen.info()["chunk"], round(frozen.info()["device_bytes"] / 2 ** 20, 1)
                res[f"own {slots}"] = part
                if n == args.run_size and slots == slot_sizes[0]:
                    rows_run = banked[:, args.train:args.train + args.steps]
                    with_knn, recorded = [], []

                    def timed(store_in, **kw):
                        sync()
                        t0 = time.perf_counter()
                        group.run(rows_run, args.steps, encoder=enc, **kw)
                        store_in.append(time.perf_counter() - t0)
                    for _ in range(2):
                        group.run(rows_run, args.steps, encoder=enc, knn=frozen, knn_learning=False)
                    for r in range(args.repeats):
                        for leg in ((0, 1) if r % 2 == 0 else (1, 0)):
                            if leg == 0:
                                timed(with_knn, knn=frozen, knn_learning=False)
                            else:
                                timed(recorded, record=True)
                    res["run_knn"], res["run_recorded"] = median(with_knn), median(recorded)
                del frozen, learning
            # views of member 0 with a shared bank, against B one-stream view.run(knn=) calls per tick
            parent = group.models[0]
            knn = solo_of(slots, slots + 64, n_pairs).bind(parent)
            views, shared = B.ModelGroup.views(parent, n), B.KNNClassifierBank.shared(knn, n)
            lone = [parent.inference_view() for _ in range(n)]

            def per_view(v):
                for i, view in enumerate(lone):
                    view.run(v[i:i + 1], 1, encoder=enc, knn=knn)
            legs = dict(tick=lambda v: views.tick(v, encoder=enc), tick_shared=lambda v: views.tick(v, encoder=enc, knn=shared), per_view_runs=per_view)
            part = timed_legs(legs, args.ticks if n <= 64 else max(args.ticks // 5, SLICE), args.repeats, sync, live)
            profiled(part, {k: v for k, v in legs.items() if k != "per_view_runs"}, views.models[0].engine, live)
            res[f"views {slots}"] = part
            del views, shared, lone
            # the host alternative: a recorded one-step run, the active cells read back, the definition looped per member
            if n <= (8 if slots <= 4096 else 1):
                pairs, labels, stamps = store(slots, 1, n_pairs)
                d = KNNDefinition(LABELS, K_NEAR, 1, slots + 64, SHAPE["column_dim"], SHAPE["cell_dim"], n_pairs)
                d.load_store(pairs, labels, stamps, slots)      # (the store the device objects were loaded with)

                def host_tick(v):
                    recs = group.run(v[:, None], 1, encoder=enc, record=("counters", "active_column"))
                    for m, rec in zip(group.models, recs):
                        act = np.asarray(m.temporal_memory.last_state.cell_activation)
                        d.step(pairs_of(act, np.sort(rec.active_column[0])), -1, False)
                host_tick(live[0])
                ts = []
                for r in range(args.repeats):
                    sync()
                    t0 = time.perf_counter()
                    for t in range(args.host_ticks):
                        host_tick(live[t % len(live)])
                    ts.append(time.perf_counter() - t0)
                res[f"host_alternative {slots}"] = spread(ts, args.host_ticks)
        if "twins_us_per_launch" not in out:
            out["twins_us_per_launch"] = {str(s): twins(group.models[0], s, args.repeats, n_pairs) for s in slot_sizes}
            log("twins", out["twins_us_per_launch"])
        out["sizes"][str(n)] = res
        log(n, res)
        del group
    print(json.dumps(out))
    if args.out:
        with open(args.out, "w") as fh:
            json.dump(out, fh, indent=1)


if __name__ == "__main__":
    main()
