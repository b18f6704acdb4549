"""Driver of the launch trace for scalar streams (tests/test_scalar_encoder_cpu.py; built and run as tests/test_launch_trace_cpu.py
runs trace_driver.py: the engine's host code host-only, no sanitizer, nothing preloaded, over tests/host_stub's runtime with
BITHTM_STUB_TRACE).  Prints one JSON object of trace lines:
    bank_encode      one Engine.bank_encode of 5 rows            decode_votes   one Engine.decode_votes of 5 rows
    predicted_value  one htm.predicted_value(encoder)            refused        every refused call of the list below (and their codes)
    first_run        run(values, 6, encoder=) on new values      second_run     the same call again (the bank is cached)
    recorded         run(values, 6, encoder=, record=("predicted_value",))
    with_votes       ... record=("predicted_input", "predicted_value")
    plain            run(encoder.encode(values), 6, record=("predicted_input",)), on a twin
    stack_refusal    the ValueError of RegionStack.run(record=("counters", "predicted_value"))
Kernels do nothing in the stub: the trace says which launches and copies the host code makes, not what they compute."""
import ctypes as C
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
TRACE = os.environ["BITHTM_STUB_TRACE"]
os.environ["BITHTM_EAGER_BELOW"] = "0"
import bithtm_amd as B  # noqa: E402
from bithtm_amd import _lib  # noqa: E402

I, Cn, K = 300, 512, 8


def lines():
    with open(TRACE) as f:
        return f.read().splitlines()


def traced(call):
    n = len(lines())
    call()
    return lines()[n:]


def table(rows):
    tab = (_lib.HtmScalarField * len(rows))()
    for t, (minimum, scale, offset, bits, width, buckets, periodic) in zip(tab, rows):
        t.minimum, t.scale, t.offset, t.bits, t.width, t.buckets, t.periodic = minimum, scale, offset, bits, width, buckets, periodic
    return tab


def model():
    np.random.seed(K)
    tm = B.TemporalMemory(Cn, K, distal_projection=B.PredictiveProjection(Cn * K, segment_capacity=8192), seed=K)
    return B.HierarchicalTemporalMemory(I, Cn, K, temporal_memory=tm)


def main():
    enc = B.ScalarEncoder([B.ScalarField(0, 100, 130, 21), B.ScalarField(0, 24, 96, 11, periodic=True), B.ScalarField(-5, 5, 70, 1)], I)
    values = np.random.RandomState(2).uniform(0, 5, (5, 3))
    htm, twin = model(), model()
    eng = htm.engine
    d_values, d_bank = eng.upload_values(values), eng.zero_bank(5)
    d_votes, d_out = eng.device_buffer(5 * I * 4, np.zeros((5, I), np.int32)), eng.device_buffer(5 * 3 * 2 * 4)
    out = {"bank_encode": traced(lambda: eng.bank_encode(enc, d_values, 5, d_bank, 5)),
           "decode_votes": traced(lambda: eng.decode_votes(enc, d_votes, 5, d_out)),
           "predicted_value": traced(lambda: htm.predicted_value(enc))}
    good = [(0.0, 1.1, 0, 130, 21, 110, 0), (0.0, 4.0, 130, 96, 11, 96, 1), (-5.0, 7.0, 226, 70, 1, 70, 0)]
    names = ("minimum", "scale", "offset", "bits", "width", "buckets", "periodic")

    def swapped(j, **kw):
        rows = [list(r) for r in good]
        for key, v in kw.items():
            rows[j][names.index(key)] = v
        return table(rows)
    ok, void, lib, h = table(good), C.c_void_p, eng.lib, eng.h
    bad = [swapped(0, bits=0, width=0, buckets=0), swapped(0, width=0), swapped(0, width=131), swapped(0, buckets=111), swapped(1, buckets=86),
           swapped(0, offset=-1), swapped(2, offset=231), swapped(1, offset=129), swapped(0, minimum=float("nan")), swapped(0, minimum=float("inf")),
           swapped(0, scale=float("inf")), swapped(0, scale=0.0), swapped(0, scale=-1.0), swapped(2, scale=float("nan")),
           table([(0.0, 1.0, 0, 8193, 3, 8191, 0)])]
    host = np.zeros((3, 2), np.int32)
    calls = [lambda t=t: lib.htm_bank_encode(h, t, len(t), void(d_values), 5, void(d_bank), 5, 0) for t in bad[:-1]]
    calls += [lambda t=t: lib.htm_decode_votes(h, t, len(t), void(d_votes), 5, void(d_out)) for t in bad[:-1]]
    calls += [lambda t=t: lib.htm_predicted_value(h, t, len(t), host.ctypes.data_as(void)) for t in bad[:-1]]
    calls += [lambda: lib.htm_bank_encode(h, None, 3, void(d_values), 5, void(d_bank), 5, 0),
              lambda: lib.htm_bank_encode(h, ok, 3, None, 5, void(d_bank), 5, 0),
              lambda: lib.htm_bank_encode(h, ok, 3, void(d_values), 5, None, 5, 0),
              lambda: lib.htm_bank_encode(h, ok, 0, void(d_values), 5, void(d_bank), 5, 0),
              lambda: lib.htm_bank_encode(h, ok, 17, void(d_values), 5, void(d_bank), 5, 0),
              lambda: lib.htm_bank_encode(h, ok, 3, void(d_values), -1, void(d_bank), 5, 0),
              lambda: lib.htm_bank_encode(h, ok, 3, void(d_values), 5, void(d_bank), 5, -1),
              lambda: lib.htm_bank_encode(h, ok, 3, void(d_values), 5, void(d_bank), 5, 1),
              lambda: lib.htm_bank_encode(h, ok, 3, void(d_values), 1, void(d_bank + 4), 5, 0),
              lambda: lib.htm_decode_votes(h, None, 3, void(d_votes), 5, void(d_out)),
              lambda: lib.htm_decode_votes(h, ok, 3, None, 5, void(d_out)),
              lambda: lib.htm_decode_votes(h, ok, 3, void(d_votes), 5, None),
              lambda: lib.htm_decode_votes(h, ok, 3, void(d_votes), -1, void(d_out)),
              lambda: lib.htm_predicted_value(h, ok, 3, None),
              lambda: lib.htm_predicted_value(h, ok, 17, host.ctypes.data_as(void))]
    codes = []
    out["refused"] = traced(lambda: codes.extend(call() for call in calls))
    out["codes"] = codes
    # (the cap is the decoding calls' alone -- on an engine wide enough for such a field)
    wide = B.SpatialPooler(8200, 64, 4)._ensure_engine()
    big = bad[-1]
    w_bank = wide.zero_bank(1)
    out["cap_codes"] = [lib.htm_bank_encode(wide.h, big, 1, void(d_values), 1, void(w_bank), 1, 0),
                        lib.htm_decode_votes(wide.h, big, 1, void(d_votes), 1, void(d_out)),
                        lib.htm_bank_encode(wide.h, ok, 3, void(d_values), 0, void(w_bank), 1, 0),
                        lib.htm_predicted_value(wide.h, ok, 3, host.ctypes.data_as(void))]
    out["first_run"] = traced(lambda: htm.run(values, 6, encoder=enc))
    out["second_run"] = traced(lambda: htm.run(values, 6, encoder=enc))
    twin.run(enc.encode(values), 12)
    htm.run(values, 6, encoder=enc, record=("predicted_input", "predicted_value"))      # (the record buffers are made here)
    twin.run(enc.encode(values), 6, record=("predicted_input",))
    rec = []
    out["recorded"] = traced(lambda: rec.append(htm.run(values, 6, encoder=enc, record=("predicted_value",))))
    out["with_votes"] = traced(lambda: rec.append(htm.run(values, 6, encoder=enc, record=("predicted_input", "predicted_value"))))
    out["plain"] = traced(lambda: twin.run(enc.encode(values), 6, record=("predicted_input",)))
    assert rec[0].fields == ("predicted_value",) and rec[0].predicted_bucket.shape == (6, 3) and rec[0].predicted_input is None
    assert rec[1].fields == ("predicted_input", "predicted_value") and rec[1].predicted_input.shape == (6, I)
    assert rec[1].predicted_value.shape == (6, 3) and rec[1].predicted_value.dtype == np.float64
    value, score = htm.forecast_values(3, enc)
    assert value.shape == (3, 3) and score.shape == (3, 3) and htm.engine.steps == 33 and twin.engine.steps == 24
    # a group's predicted_value is its members'; a stack takes no encoder, so it refuses the record as run() does without one
    group = B.ModelGroup([htm, twin])
    value, score = group.predicted_value(enc)
    assert value.shape == (2, 3) and value.dtype == np.float64 and score.shape == (2, 3) and score.dtype == np.int32
    stack = B.RegionStack(I, [(128, 4), (64, 4)])
    try:
        stack.run(np.zeros((2, I), bool), 2, record=("counters", "predicted_value"))
        out["stack_refusal"] = "not refused"
    except ValueError as e:
        out["stack_refusal"] = str(e)
    assert stack.run(np.zeros((2, I), bool), 2, record=("counters",))[0].fields == ("counters",)
    print(json.dumps(out))


if __name__ == "__main__":
    main()
