"""What the KNN classifier costs on the device, as one JSON line (and, with --out, a file:
profiles/r20_knn_rate.json).  Two shapes: "2048x32" (1 000 inputs -> 2 048 columns x 32 cells, 41 active) and "bench" (bench.py's
workload: 1 024 inputs -> 65 536 columns x 32 cells, 1 311 active); stores of --stores slots (1 k, 16 k, 64 k) of random patterns
of the model's shape (one cell per active column), loaded as a state.  Per shape and store, behind --train untimed learning steps
and two untimed runs of each kind, --repeats rounds of --steps steps, the legs in alternating order, the median with the lowest and
the highest:

  run_recorded     run(record=True): the recorded run without knn= (the launches of the commit before the KNN classifier)
  run_knn          run(knn=, knn_learning=False): pattern capture, and the frozen update (two launches per 64 steps, four in the
                   global-table form) behind the batch
  distance         device time per launch of the distance kernel and per query step (htm_profile, one launch per kernel
                   boundary), the store's bytes, the passes over them per launch (one per group of staged queries), the read rate
                   that makes, and its share of the bare stream of the same bytes (tools/hbm_read, the contiguous shape, best of
                   its grids; built by --build_stream, skipped when the binary is not there)
  select           device time per launch of the select kernel
  then_numpy       per step, a NumPy form of the definition over --loop_steps of the patterns the run captured, read back: what the
                   same run followed by the host's own search would add

    python tools/knn_rate.py [--shapes 2048x32,bench] [--stores 1024,16384,65536] [--steps 1000] [--repeats 3] [--out profiles/r20_knn_rate.json]
"""
import argparse
import json
import os
import re
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np  # noqa: E402

import bithtm_amd as B  # noqa: E402
from bithtm_amd import _lib as L  # noqa: E402

SHAPES = {"2048x32": dict(input_dim=1000, column_dim=2048, cell_dim=32), "bench": dict(input_dim=1024, column_dim=65536, cell_dim=32)}
STREAM = os.path.join(ROOT, "tools", "hbm_read")
POPCOUNT = np.array([bin(i).count("1") for i in range(256)], dtype=np.uint8)


def log(*a):
    print(*a, file=sys.stderr, flush=True)


def median(times, per=1):
    ms = sorted(1e3 * t / per for t in times)
    return dict(ms=round(ms[len(ms) // 2], 4), lowest=round(ms[0], 4), highest=round(ms[-1], 4))


def random_store(count, column_dim, cell_dim, pairs, labels, seed):
    """A state of `count` slots: per slot `pairs` distinct columns (an odd stride from a random start) with one cell each."""
    rng = np.random.default_rng(seed)
    start, step = rng.integers(0, column_dim, (count, 1)), rng.integers(0, column_dim // 2, (count, 1)) * 2 + 1
    cols = (start + np.arange(pairs)[None, :] * step) % column_dim
    state = np.empty((count, pairs, 2), dtype=np.int32)
    state[:, :, 0] = cols
    state[:, :, 1] = (1 << rng.integers(0, min(cell_dim, 31), (count, pairs))).astype(np.int32)
    return dict(total=np.int64(count), count=np.int64(count), pairs=state, labels=rng.integers(0, labels, count).astype(np.int32),
                stamps=np.arange(count, dtype=np.int64))


def numpy_search(store, labels_of, query, words, k, n_labels):
    """One step of the definition over a store in NumPy: dense query table, gathered words, byte-table popcount, a stable sort."""
    table = np.zeros(words, dtype=np.uint32)
    live = query[:, 0] >= 0
    table[query[live, 0]] = query[live, 1].view(np.uint32)
    both = store[:, :, 1].view(np.uint32) & table[np.maximum(store[:, :, 0], 0)]
    ov = POPCOUNT[both.view(np.uint8)].reshape(len(store), -1).sum(axis=1, dtype=np.int64)
    cand = np.flatnonzero(ov >= 1)
    near = cand[np.argsort(-ov[cand], kind="stable")][:k]
    votes = np.bincount(labels_of[near], minlength=n_labels)
    return int(np.argmax(votes)) if len(near) else -1


def bare_stream(mib):
    """GB/s of the contiguous read of `mib` MiB by tools/hbm_read (the best of its grids), or None without the binary."""
    if not os.path.exists(STREAM):
        return None
    r = subprocess.run([STREAM, str(mib)], capture_output=True, text=True, timeout=600)
    rates = [float(x) for x in re.findall(r"stride 128 used 128 .*?:\s+[\d.]+ us\s+([\d.]+) GB/s", r.stdout)]
    return max(rates) if rates else None


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--shapes", default="2048x32,bench")
    ap.add_argument("--stores", default="1024,16384,65536")
    ap.add_argument("--patterns", type=int, default=50)
    ap.add_argument("--steps", type=int, default=1000)
    ap.add_argument("--train", type=int, default=500)
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--loop_steps", type=int, default=8)
    ap.add_argument("--k", type=int, default=5)
    ap.add_argument("--build_stream", action="store_true", help="build tools/hbm_read with hipcc first")
    ap.add_argument("--out")
    args = ap.parse_args()
    if args.build_stream:
        subprocess.run([os.environ.get("HIPCC", "/opt/rocm/bin/hipcc"), "--offload-arch=gfx950", "-O3", STREAM + ".hip", "-o", STREAM], check=True)
    out = dict(tool="knn_rate", steps=args.steps, patterns=args.patterns, k=args.k, chunk=L.KNN_CHUNK, shapes={})
    for name in args.shapes.split(","):
        shape = SHAPES[name]
        np.random.seed(3)
        htm = B.HierarchicalTemporalMemory(seed=3, **shape)
        eng = htm.engine
        bank = np.random.RandomState(5).rand(args.patterns, shape["input_dim"]) < 0.02
        htm.run(bank, args.train)
        per = eng.active_columns * ((shape["cell_dim"] + 31) // 32)
        words = shape["column_dim"] * ((shape["cell_dim"] + 31) // 32)
        res = {}
        for count in (int(x) for x in args.stores.split(",")):
            knn = B.KNNClassifier(args.patterns, k=args.k, capacity=count).bind(htm)
            state = random_store(count, shape["column_dim"], shape["cell_dim"], per, args.patterns, count)
            knn.load_state_dict(dict(state, params=np.asarray(knn._params(), dtype=np.int64)))
            info = knn.info()
            legs = dict(run_recorded=lambda: htm.run(bank, args.steps, record=True), run_knn=lambda: htm.run(bank, args.steps, knn=knn, knn_learning=False))
            for _ in range(2):
                for fn in legs.values():
                    fn()
            times = {leg: [] for leg in legs}
            for r in range(args.repeats):
                for leg in (list(legs) if r % 2 == 0 else list(legs)[::-1]):
                    eng.sync()
                    t0 = time.perf_counter()
                    rec = legs[leg]()
                    times[leg].append(time.perf_counter() - t0)
            one = {leg: median(times[leg]) for leg in legs}
            one["steps_per_s"] = {leg: round(args.steps / (one[leg]["ms"] / 1e3)) for leg in legs}
            one["form"] = "lds" if info["table_in_lds"] else "global table"
            one["queries_per_block"], one["device_mib"] = info["queries_per_block"], round(info["device_bytes"] / 2 ** 20, 1)
            # the host alternative over patterns the run captured
            n = min(args.loop_steps, args.steps)
            pairs = eng.read_words(knn._bufs["pairs"][0], 2 * n * per, np.int32).reshape(n, per, 2)
            t0 = time.perf_counter()
            for q in pairs:
                numpy_search(state["pairs"], state["labels"], q, words, args.k, args.patterns)
            one["then_numpy"] = dict(ms_per_step=round(1e3 * (time.perf_counter() - t0) / n, 3), steps=n, pairs_per_step=per)
            # device time of the kernels: whole chunks of 64 steps, launched eagerly
            eng.profile(True)
            htm.run(bank, 4 * L.KNN_CHUNK, knn=knn, knn_learning=False, use_graph=False)
            prof = eng.profile_read()
            eng.profile(False)
            us = {k: (1e3 * ms / max(c, 1), c) for k, (ms, c) in prof.items() if k.startswith("knn:")}
            store_bytes = count * per * 8
            passes = -(-L.KNN_CHUNK // info["queries_per_block"])
            d_us = us["knn:distance"][0]
            one["distance"] = dict(us_per_launch=round(d_us, 2), us_per_query_step=round(d_us / L.KNN_CHUNK, 3), launches=us["knn:distance"][1],
                                   store_bytes=store_bytes, bytes_per_query_step=store_bytes // info["queries_per_block"], passes_per_launch=passes,
                                   read_GBps=round(store_bytes * passes / (d_us * 1e-6) / 1e9, 1))
            stream = bare_stream(max(1, -(-store_bytes // 2 ** 20)))
            if stream:
                one["distance"].update(bare_stream_GBps=stream, share_of_bare_stream=round(one["distance"]["read_GBps"] / stream, 3))
            one["select"] = dict(us_per_launch=round(us["knn:select"][0], 2), launches=us["knn:select"][1])
            one["other_kernels_us_per_launch"] = {k: round(v[0], 2) for k, v in us.items() if k not in ("knn:distance", "knn:select")}
            one["labels_of_the_last_run"] = int((rec.knn_label >= 0).sum()) if rec.knn_label is not None else None
            res[str(count)] = one
            log(name, count, one)
            del knn
        out["shapes"][name] = res
        del htm
    print(json.dumps(out))
    if args.out:
        with open(args.out, "w") as fh:
            json.dump(out, fh, indent=1)


if __name__ == "__main__":
    main()
