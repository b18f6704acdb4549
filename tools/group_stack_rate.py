"""What a stack of model groups buys, as one JSON object: B streams through 1 000 -> 2 048 x 32 -> 512 x 32 (stride --stride), with
a plain link and with a PoolingLink (the defaults), at B = 1 / 8 / 64.  Per link and B, on one device, one stream, one process:

  group, solo     seconds per round of --steps steps of every stream, the median of --repeats rounds wrapped in synchronisations
                  with the lowest and the highest: ONE GroupStack.run call against B RegionStack.run calls one after another (the
                  B stacks made on one stream, RegionStack.of), the two legs taking turns and the one that comes first alternating
  launches        kernel launches of one chunk run eagerly (htm_profile counts them): the group's whatever B is, and one solo
                  stack's, which a round makes B times
  link            device time and launch count of the link's launches over one call of --steps steps (the kernels' own begin and
                  end stamps): group:pack_columns, or group:pool_pack, group:pool_scan and group:pool_select

    python tools/group_stack_rate.py [--steps 2000] [--repeats 5] [--members 1,8,64] [--out profiles/r24_group_stack_rate.json]
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
from bithtm_amd.group import SharedStream  # noqa: E402

INPUT, LEVELS = 1000, [(2048, 32), (512, 32)]


def log(*a):
    print(*a, file=sys.stderr, flush=True)


def spread(ts):
    return dict(median=round(float(np.median(ts)), 5), low=round(float(min(ts)), 5), high=round(float(max(ts)), 5))


def once(sync, fn):
    sync()
    t0 = time.perf_counter()
    fn()
    sync()
    return time.perf_counter() - t0


def solo_stacks(n, link):
    """n RegionStacks of the shape on ONE stream, member b with the seeds GroupStack gives it."""
    stream = SharedStream(0)
    out = []
    for b in range(n):
        models, below = [], INPUT
        for l, (c, k) in enumerate(LEVELS):
            models.append(B.HierarchicalTemporalMemory(below, c, k, seed=b + l, stream=stream))
            below = c
        out.append(B.RegionStack.of(models, links=[link]))
    return out


def profiled(engines, fn):
    """{launch name: (device ms, launches)} summed over `engines` for what fn() enqueues."""
    for e in engines:
        e.profile(True)
    fn()
    total = {}
    for e in engines:
        e.sync()
        for name, (ms, n) in e.profile_read(256).items():
            a = total.setdefault(name, [0.0, 0])
            a[0] += ms
            a[1] += int(n)
        e.profile(False)
    return total


def measure(kind, n, stride, steps, repeats, patterns=50):
    link = stride if kind == "plain" else B.PoolingLink(stride)
    inputs = np.random.RandomState(0).rand(n, patterns, INPUT) < 0.1
    group = B.GroupStack(n, INPUT, LEVELS, links=[link])
    solos = solo_stacks(n, link)
    sync = group.groups[0].models[0].engine.sync
    sync_solos = solos[0].levels[0].engine.sync     # (one stream: the first engine's wait is every stack's)
    run_group = lambda: group.run(inputs, steps)
    run_solos = lambda: [s.run(x, steps) for s, x in zip(solos, inputs)]
    for _ in range(2):                              # untimed: graphs captured, the default-sized pools grown
        run_group()
        run_solos()
    times = {"group": [], "solo": []}
    for r in range(repeats):
        for name in (("group", "solo") if r % 2 == 0 else ("solo", "group")):
            times[name].append(once(sync, run_group) if name == "group" else once(sync_solos, run_solos))
    row = dict(link=kind, members=n, stride=stride, steps=steps, chunk_steps=group.last_run_chunks[0], group_seconds=spread(times["group"]),
               solo_seconds=spread(times["solo"]), solo_over_group=round(float(np.median(times["solo"]) / np.median(times["group"])), 3),
               stream_steps_per_s=dict(group=round(n * steps / float(np.median(times["group"])), 1), solo=round(n * steps / float(np.median(times["solo"])), 1)))
    # the launches of one chunk, run eagerly so that every launch is counted
    chunk = group.last_run_chunks[0]
    heads = [g.models[0].engine for g in group.groups]
    eager = profiled(heads, lambda: group.run(inputs, chunk, use_graph=False))
    one = profiled([m.engine for m in solos[0].levels], lambda: solos[0].run(inputs[0], chunk, use_graph=False))
    row["launches"] = dict(chunk_steps=chunk, group=sum(c for _, c in eager.values()), one_solo_stack=sum(c for _, c in one.values()),
                           solo_round=n * sum(c for _, c in one.values()))
    over = profiled(heads, run_group)
    row["link"] = {name: dict(ms=round(ms, 4), launches=c) for name, (ms, c) in over.items() if name.startswith(("group:pack_columns", "group:pool_"))}
    log(row)
    return row


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=2000)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--stride", type=int, default=4)
    ap.add_argument("--members", default="1,8,64")
    ap.add_argument("--out")
    args = ap.parse_args()
    out = dict(tool="group_stack_rate", shape="1000 -> 2048 x 32 -> 512 x 32",
               runs=[measure(kind, int(n), args.stride, args.steps, args.repeats) for kind in ("plain", "pooled") for n in args.members.split(",") if n])
    print(json.dumps(out))
    if args.out:
        with open(args.out, "w") as f:
            json.dump(out, f, indent=1)


if __name__ == "__main__":
    main()
