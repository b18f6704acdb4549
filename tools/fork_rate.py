"""Stream-fork and look-ahead rates at the bench shape (65 536 columns x 32 cells, bench.py's headline workload, learned), as one
JSON line (and, with --out, a file: profiles/r12_fork_rate.json).

  sync        one InferenceView.sync() (htm_view_sync): the kernel's own time by HIP events over --syncs syncs (htm_profile stamps
              each launch), the wall time per sync of the same loop, and bytes per second from the bytes DESIGN.md section 19
              counts (fork_bytes below: the same formula)
  state_dict  twin.load_state_dict(parent.state_dict()): what the parent commit offers for the same hand-over, through the host
  replay      view.reset(); view.run(context, c) for c = 10 and c = 100: the parent commit's other way to bring a view to "now"
  lookahead   model steps per second of htm.lookahead(inputs, steps, horizon, every=) at (every, horizon) = (1, 5) and (10, 50),
              against the host loop of its definition (run(every); fork().forecast(horizon)) and against a plain run()

The back-to-back syncs copy the same 23 MB between the same two handles: 46 MB of traffic that stay in the 256 MB Infinity
Cache, so their time is a cache-resident one; "behind a source step" is the sync as a look-ahead makes it.  The look-ahead legs
run one after the other on the same learning parent (lookahead, plain run, host loop; then the second shape): each starts from
a state that has learned more than the one before it, so their ratios are not taken from one state.

Each timed leg runs after an untimed call (graphs captured), between synchronisations; rates are the median of --repeats with
the lowest and highest.  Legs that were not run are written as "not measured".

    python tools/fork_rate.py [--syncs 100] [--repeats 3] [--legs sync,state_dict,replay,lookahead] [--out profiles/r12_fork_rate.json]
"""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np  # noqa: E402

from bench import WORKLOAD, build_htm, make_inputs  # noqa: E402

LEGS = ("sync", "state_dict", "replay", "lookahead")


def log(*a):
    print(*a, file=sys.stderr, flush=True)


def fork_bytes(C, k, cell_dim, segments, capacity):
    """(bytes copied, bytes zeroed) by one htm_view_sync: DESIGN.md section 19's formula."""
    KP = 64 if cell_dim > 32 else 32
    WPC = KP // 32
    P = (C + 255) // 256 * 8                        # padded column-bitmap words
    per_parity = C * (8 + 8 + 4) + 3 * C * WPC * 4 + k * KP * 4 + (k + 8) * 4 + P * 4 + P * 2
    fixed = (2 * C * KP * 4 + 2 * per_parity + C * 4 + 2 * 6 * 4096 * 4 + 2 * (4 * 4096 + 16 * 1024) * 4 + (C + 255) // 256 * 33 * 4
             + 2 * 16 * 32 * 4 + k + 3 * (k * WPC + 8) * 4 + (k * WPC + 8) + (k * WPC + 16) * 4 + k * KP * 4 + 640)
    bit_words, cap_words = (segments + 31) // 32, (capacity + 255) // 256 * 8
    return fixed + 8 * segments + 2 * 4 * bit_words, 2 * 4 * (cap_words - bit_words)


def timed(fn, sync, repeats):
    fn()
    out = []
    for _ in range(repeats):
        sync()
        t0 = time.perf_counter()
        fn()
        sync()
        out.append(time.perf_counter() - t0)
    out.sort()
    return out[len(out) // 2], out[0], out[-1]


def rate(steps, times):
    med, lo, hi = times
    return dict(steps_per_s=round(steps / med, 1), lowest=round(steps / hi, 1), highest=round(steps / lo, 1))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--syncs", type=int, default=100)
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--train", type=int, default=1000)
    ap.add_argument("--legs", default=",".join(LEGS))
    ap.add_argument("--out")
    args = ap.parse_args()
    legs = args.legs.split(",")
    w = dict(WORKLOAD)
    noisy, perm = make_inputs(w)
    parent = build_htm(w, perm, 0)
    parent.run(noisy, args.train)
    eng = parent.engine
    segments = int(eng.check_capacity().segments)
    copied, zeroed = fork_bytes(eng.column_dim, eng.active_columns, eng.cell_dim, segments, eng.segment_capacity)
    log(f"parent: {args.train} learning steps, {segments} segments of {eng.segment_capacity}; a sync copies {copied} bytes, zeroes {zeroed}")
    out = dict(tool="fork_rate", shape="65536 columns x 32 cells, 1024 inputs", segments=segments, segment_capacity=int(eng.segment_capacity),
               sync_bytes_copied=copied, sync_bytes_zeroed=zeroed, **{leg: "not measured" for leg in LEGS})
    context = noisy[:w["patterns"]]

    if "sync" in legs:
        f = parent.fork()
        f.run(context, 4)
        fe = f.engine
        fe.profile(True)
        for _ in range(args.syncs):
            fe.view_sync(eng)
        prof = fe.profile_read()
        fe.profile(False)
        ms, n = prof["stream_fork"]
        wall = timed(lambda: [fe.view_sync(eng) for _ in range(args.syncs)], fe.sync, args.repeats)
        us = 1e3 * ms / n
        # ... and as a look-ahead makes them: each behind a learning step of the source, which has rewritten part of what the
        # sync reads and has had the caches to itself (back to back, the 46 MB of a sync's traffic stay in the 256 MB Infinity Cache)
        fe.profile(True)
        for _ in range(args.syncs):
            parent.run(noisy, 1)
            fe.view_sync(eng)
        ms2, n2 = fe.profile_read()["stream_fork"]
        fe.profile(False)
        us2 = 1e3 * ms2 / n2
        out["sync"] = dict(syncs=int(n), kernel_us=round(us, 2), wall_us_per_sync=round(1e6 * wall[0] / args.syncs, 2),
                           copied_GB_per_s=round(copied / us / 1e3, 1), traffic_GB_per_s=round((2 * copied + zeroed) / us / 1e3, 1),
                           kernel_us_behind_a_source_step=round(us2, 2), traffic_GB_per_s_behind_a_source_step=round((2 * copied + zeroed) / us2 / 1e3, 1))
        log("sync", out["sync"])
        del f, fe
    if "state_dict" in legs:
        twin = build_htm(w, perm, 0)
        t = timed(lambda: twin.load_state_dict(parent.state_dict()), twin.engine.sync, 1)
        out["state_dict"] = dict(seconds=round(t[0], 3))
        log("state_dict", out["state_dict"])
        del twin
    if "replay" in legs:
        v = parent.inference_view()
        out["replay"] = {}
        for c in (10, 100):
            t = timed(lambda: (v.reset(), v.run(context, c)), v.engine.sync, args.repeats)
            out["replay"][str(c)] = dict(us=round(1e6 * t[0], 1), lowest_us=round(1e6 * t[1], 1), highest_us=round(1e6 * t[2], 1))
        log("replay", out["replay"])
        del v
    if "lookahead" in legs:
        out["lookahead"] = {}
        for every, horizon, windows, host_windows in ((1, 5, 256, 32), (10, 50, 64, 16)):
            steps = every * windows

            def definition(n):
                for _ in range(n):
                    parent.run(noisy, every)
                    parent.fork().forecast(horizon, 1, 20)
            leg = dict(every=every, horizon=horizon, windows=windows)
            leg["lookahead"] = rate(steps, timed(lambda: parent.lookahead(noisy, steps, horizon, 1, 20, every=every), eng.sync, args.repeats))
            leg["plain_run"] = rate(steps, timed(lambda: parent.run(noisy, steps), eng.sync, args.repeats))
            leg["host_loop"] = dict(rate(every * host_windows, timed(lambda: definition(host_windows), eng.sync, 1)), windows=host_windows)
            out["lookahead"][f"every{every}_horizon{horizon}"] = leg
            log("lookahead", leg)
    print(json.dumps(out))
    if args.out:
        with open(args.out, "w") as fh:
            json.dump(out, fh, indent=1)


if __name__ == "__main__":
    main()
