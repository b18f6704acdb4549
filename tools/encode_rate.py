"""Scalar-stream rates at the bench shape (65 536 columns x 32 cells; input_dim 1 000, two fields), as one JSON line (and, with
--out, a file: profiles/r13_encode_rate.json).  Both baselines are paths the parent commit has.

  encode   a bank of --rows rows from values: the host's encoder.encode(values) + Engine.upload_bank (rows x input_dim bools built
           and packed on the host, rows x words_per_row words uploaded) against Engine.upload_values + a new bank + Engine.bank_encode
           (8 F bytes per row uploaded, one launch: what Engine.encoded_bank does for new values); both allocate their bank inside
           the timed call; wall time from the values to a bank a run can read, the engine's stream waited for.  The host side's
           two parts -- the NumPy encode, upload_bank of rows that exist -- are timed on their own too
  decode   a recorded run of --steps steps with learning off: record=("predicted_input",) read back (input_dim int32 per step)
           and decoded with encoder.decode in NumPy, against record=("predicted_value",) (the votes stay on the device, one decode
           launch behind the run, 2 F ints per step read back); the run itself is the same decoding run in both

Each timed leg runs after an untimed call (graphs captured, buffers made), between synchronisations; times are the median of
--repeats with the lowest and highest.

    python tools/encode_rate.py [--rows 1000] [--steps 1000] [--train 1000] [--repeats 5] [--out profiles/r13_encode_rate.json]
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
    return dict(us=round(1e6 * out[len(out) // 2], 1), lowest_us=round(1e6 * out[0], 1), highest_us=round(1e6 * out[-1], 1))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", type=int, default=1000)
    ap.add_argument("--steps", type=int, default=1000)
    ap.add_argument("--train", type=int, default=1000)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--out")
    args = ap.parse_args()
    import bithtm_amd as B
    w = dict(WORKLOAD, input_dim=1000)
    _, perm = make_inputs(w)
    htm = build_htm(w, perm, 0)
    eng = htm.engine
    enc = B.ScalarEncoder([B.ScalarField(0.0, 100.0, 600, 21), B.ScalarField(0.0, 24.0, 400, 21, periodic=True)], 1000)
    t = np.arange(args.rows, dtype=np.float64)
    period = 50                                      # (the bench's 50 patterns: a stream the model can learn)
    values = np.stack([50.0 + 45.0 * np.sin(2 * np.pi * t / period), (24.0 * t / period) % 24.0], axis=1)
    out = dict(tool="encode_rate", shape="65536 columns x 32 cells, 1000 inputs, 2 fields", rows=args.rows, steps=args.steps)

    # Both sides pay for the same things: a new bank allocated inside the timed call (upload_bank makes one per call; the device
    # leg is what Engine.encoded_bank does for new values: values buffer, bank, one launch).  The parts of the host side are timed
    # on their own as well: the NumPy encode, and upload_bank of rows that exist.
    rows = enc.encode(values)
    kept = []

    def on_host():
        eng.upload_bank(enc.encode(values))

    def on_device():
        d_values, d_bank = eng.upload_values(values), eng.device_buffer(args.rows * eng.words * 4)
        eng.bank_encode(enc, d_values, args.rows, d_bank, args.rows)
        kept.append((d_values, d_bank))
    out["encode"] = dict(host_encode_and_upload_bank=timed(on_host, eng.sync, args.repeats),
                         host_encode_alone=timed(lambda: enc.encode(values), eng.sync, args.repeats),
                         upload_bank_alone=timed(lambda: eng.upload_bank(rows), eng.sync, args.repeats),
                         upload_values_allocate_bank_and_bank_encode=timed(on_device, eng.sync, args.repeats),
                         bytes_uploaded_host=args.rows * eng.words * 4, bytes_uploaded_device=int(values.nbytes))
    assert np.array_equal(eng.read_bank(kept[-1][1], args.rows), rows)
    for pair in kept:
        for ptr in pair:
            eng.lib.hipFree(ptr)
    log("encode", out["encode"])

    htm.run(values, args.train, encoder=enc)
    log(f"trained {args.train} steps; {int(eng.check_capacity().segments)} segments")
    got = {}

    def votes_to_host():
        rec = htm.run(values, args.steps, learning=False, record=("predicted_input",), encoder=enc)
        got["host"] = enc.decode(rec.predicted_input)

    def decoded_on_device():
        rec = htm.run(values, args.steps, learning=False, record=("predicted_value",), encoder=enc)
        got["device"] = (rec.predicted_bucket, rec.predicted_score)
    out["decode"] = dict(record_predicted_input_and_numpy_decode=timed(votes_to_host, eng.sync, args.repeats),
                         record_predicted_value=timed(decoded_on_device, eng.sync, args.repeats),
                         bytes_read_back_host=args.steps * 1000 * 4, bytes_read_back_device=args.steps * len(enc) * 8,
                         steps_with_a_prediction=int((got["device"][1].max(axis=1) > 0).sum()))
    log("decode", out["decode"])
    print(json.dumps(out))
    if args.out:
        with open(args.out, "w") as fh:
            json.dump(out, fh, indent=1)
            fh.write("\n")


if __name__ == "__main__":
    main()
