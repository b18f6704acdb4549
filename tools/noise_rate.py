"""What a fresh noise draw per timestep costs at the bench shape (65 536 columns x 32 cells, bench.py's WORKLOAD, learned), as one
JSON line.  The stream is the example's: pattern (t mod P) XOR flip noise, a new draw every step.

  fixed                  today's noise-free run over the resident, pre-noised bank (bench.py's): one call of --steps steps
  host_noise             per epoch of P steps: the noise drawn with NumPy, the noisy bank uploaded, run() over it -- what
                         `python -m bithtm_amd.example --batched` does
  device_noise           per epoch of P steps: run(bank, P, noise=p) -- the bank uploaded once, the noise drawn on the device
                         (`--batched --device_noise`); the same calls as host_noise
  device_noise_one_call  run(bank, steps, noise=p) in one call: the same call as `fixed`, plus one fill per noise_chunk steps

Each leg is timed --repeats times between synchronisations after an untimed call (graphs captured); the line holds the median
rate and the lowest and highest (the run-to-run spread) in timesteps per second.  `fixed` and `host_noise` use nothing this
tool's commit added, so the same file runs beside an older checkout with --legs fixed,host_noise.

    python tools/noise_rate.py [--steps 2000] [--repeats 5] [--train 1000] [--legs fixed,host_noise,device_noise,device_noise_one_call]
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


def log(*a):
    print(*a, file=sys.stderr, flush=True)


def rates(fn, sync, steps, repeats):
    """fn() timed `repeats` times after one untimed call: (median, lowest, highest) steps per second."""
    fn()
    out = []
    for _ in range(repeats):
        sync()
        t0 = time.perf_counter()
        fn()
        sync()
        out.append(steps / (time.perf_counter() - t0))
    out.sort()
    return dict(steps_per_s=round(out[len(out) // 2], 1), lowest=round(out[0], 1), highest=round(out[-1], 1))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=2000)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--train", type=int, default=1000)
    ap.add_argument("--legs", default="fixed,host_noise,device_noise,device_noise_one_call")
    ap.add_argument("--out")
    args = ap.parse_args()
    legs = args.legs.split(",")
    w = dict(WORKLOAD)
    noisy, perm = make_inputs(w)
    np.random.seed(0)
    bank = np.random.rand(w["patterns"], w["input_dim"]) < w["density"]          # (make_inputs' first draw: the clean patterns)
    P, p = w["patterns"], w["noise"]
    epochs = max(1, args.steps // P)
    steps = epochs * P
    htm = build_htm(w, perm, 0)
    htm.run(noisy, args.train)
    segments = htm.engine.check_capacity().segments
    log(f"{args.train} learning steps, {segments} segments")
    out = dict(tool="noise_rate", shape="65536 columns x 32 cells, 1024 inputs", patterns=P, flip_noise=p, segments=int(segments),
               steps=steps, epoch_steps=P, repeats=args.repeats)
    sync = lambda: htm.engine.sync()                # noqa: E731  (the engine may be re-created by pool growth)
    rng = np.random.RandomState(1)

    def host_noise():
        for _ in range(epochs):
            htm.run(bank ^ (rng.rand(*bank.shape) < p), P)

    def device_noise():
        for _ in range(epochs):
            htm.run(bank, P, noise=p)

    fns = dict(fixed=lambda: htm.run(noisy, steps), host_noise=host_noise, device_noise=device_noise,
               device_noise_one_call=lambda: htm.run(bank, steps, noise=p))
    for leg in legs:
        out[leg] = rates(fns[leg], sync, steps, args.repeats)
        log(leg, out[leg])
    out["segments_after"] = int(htm.engine.check_capacity().segments)

    def gap(a, b):
        """How far leg a's median is above leg b's, and the combined spread of the two (their highest minus lowest, added)."""
        if a not in out or b not in out:
            return None
        spread = (out[a]["highest"] - out[a]["lowest"]) + (out[b]["highest"] - out[b]["lowest"])
        return dict(steps_per_s=round(out[a]["steps_per_s"] - out[b]["steps_per_s"], 1), combined_spread=round(spread, 1))

    out["device_noise_over_host_noise"] = gap("device_noise", "host_noise")
    out["fixed_over_device_noise_one_call"] = gap("fixed", "device_noise_one_call")
    print(json.dumps(out))
    if args.out:
        with open(args.out, "w") as f:
            json.dump(out, f, indent=1)


if __name__ == "__main__":
    main()
