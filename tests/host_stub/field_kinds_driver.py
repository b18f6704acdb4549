"""Driver of the launch traces of the field kinds (tests/test_field_kinds_cpu.py; used as scalar_driver.py is: the engine's host code
host-only, no sanitizer, nothing preloaded, over tests/host_stub's runtime with BITHTM_STUB_TRACE).  Two encoders of two fields over
the same 300-bit row: "linear" (tests/live_tick_cases.py's) and "mixed" (a hashed and a category field of the same bits).

Prints one JSON object:
  "trace"    {"<linear|mixed> <call>": trace lines}, the calls being
               bank_encode, decode_votes      one Engine.bank_encode / decode_votes of 5 rows
               predicted_value                htm.predicted_value(encoder)
               recorded                       run(values, 6, encoder=, record=("predicted_value",)) behind a first such call
               tick B=1, tick B=3, scored B=3 one eager tick behind a warm-up tick of the same kind
  "refused"  the trace lines of every refused call below (none), "codes" their return codes
  "cap"      the codes of htm_bank_encode and htm_decode_votes for a hashed field one position above the decode cap, and of both
             for the field exactly at it
  "after"    a tick with the linear encoder right behind one with the mixed encoder on the same group: its trace

Kernels do nothing in the stub: the trace says which launches and copies the host code makes, not what they compute."""
import ctypes as C
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
TRACE = os.environ["BITHTM_STUB_TRACE"]
os.environ["BITHTM_EAGER_BELOW"] = "0"
import bithtm_amd as B  # noqa: E402
from bithtm_amd import _lib  # noqa: E402
from likelihood_cases import P_SMALL, as_kwargs  # noqa: E402
from live_tick_cases import MID, encoder_for  # noqa: E402

I, Cn, K, k = MID
CATEGORY, HASHED = 1, 2


def lines():
    with open(TRACE) as f:
        return f.read().splitlines()


def traced(call):
    n = len(lines())
    call()
    return lines()[n:]


def encoders():
    mixed = B.ScalarEncoder([B.HashedField(0.0, 24.0, 260, 21, buckets=500, seed=5), B.CategoryField(3, 5, bits=37)], input_dim=I)
    return {"linear": encoder_for(MID), "mixed": mixed}


def table(rows):
    tab = (_lib.HtmScalarField * len(rows))()
    for t, (minimum, scale, offset, bits, width, buckets, periodic, reserved) in zip(tab, rows):
        t.minimum, t.scale, t.offset, t.bits, t.width, t.buckets, t.periodic, t.reserved = minimum, scale, offset, bits, width, buckets, periodic, reserved
    return tab


def model(seed):
    np.random.seed(seed)
    tm = B.TemporalMemory(Cn, K, distal_projection=B.PredictiveProjection(Cn * K, segment_capacity=8192), seed=seed)
    return B.HierarchicalTemporalMemory(I, Cn, K, active_columns=k, temporal_memory=tm)


def main():
    out = {"trace": {}}
    values = np.random.RandomState(2).uniform(0, 3, (5, 2))
    htm = model(3)                                  # (one model for both tables: its schedule is the same in either leg)
    eng = htm.engine
    for enc in encoders().values():                 # (untimed first uses: the handle's buffers, the banks, the graphs of either parity)
        htm.predicted_value(enc)
        htm.run(values, 6, encoder=enc, record=("predicted_value",))
    for name, enc in encoders().items():
        d_values, d_bank = eng.upload_values(values), eng.zero_bank(5)
        d_votes, d_out = eng.device_buffer(5 * I * 4, np.zeros((5, I), np.int32)), eng.device_buffer(5 * 2 * 2 * 4)
        out["trace"][f"{name} bank_encode"] = traced(lambda: eng.bank_encode(enc, d_values, 5, d_bank, 5))
        out["trace"][f"{name} decode_votes"] = traced(lambda: eng.decode_votes(enc, d_votes, 5, d_out))
        out["trace"][f"{name} predicted_value"] = traced(lambda: htm.predicted_value(enc))
        htm.run(values, 6, encoder=enc, record=("predicted_value",))
        out["trace"][f"{name} recorded"] = traced(lambda: htm.run(values, 6, encoder=enc, record=("predicted_value",)))
        for n, scored in ((1, 0), (3, 0), (3, 1)):
            group = B.ModelGroup.create(n, I, Cn, K, active_columns=k, seeds=range(3, 3 + n))
            lk = B.AnomalyLikelihood(n, **as_kwargs(P_SMALL)) if scored else None
            x = np.random.RandomState(n).uniform(0, 3, (2, n, 2))
            group.tick(x[0], encoder=enc, use_graph=False, likelihood=lk)
            out["trace"][f"{name} {'scored' if scored else 'tick'} B={n}"] = traced(lambda: group.tick(x[1], encoder=enc, use_graph=False, likelihood=lk))
    # a linear tick right behind a mixed one, on one group
    both = encoders()
    group = B.ModelGroup.create(3, I, Cn, K, active_columns=k, seeds=range(3, 6))
    x = np.random.RandomState(9).uniform(0, 3, (4, 3, 2))
    group.tick(x[0], encoder=both["linear"], use_graph=False)
    group.tick(x[1], encoder=both["mixed"], use_graph=False)
    group.tick(x[2], encoder=both["mixed"], use_graph=False)
    out["after"] = traced(lambda: group.tick(x[3], encoder=both["linear"], use_graph=False))

    # ---- refusals: (minimum, scale, offset, bits, width, buckets, periodic, reserved); the second field is a good linear one
    good = (-1.0, 16.5, 260, 37, 5, 33, 0, 0)
    bad = {"reserved < 0": (0.0, 1.0, 0, 260, 21, 240, 0, -1),
           "reserved < 0, kind bits 2": (0.0, 1.0, 0, 260, 21, 240, 0, -2),
           "kind 3": (0.0, 1.0, 0, 260, 21, 240, 0, 3),
           "kind 3 with a seed": (0.0, 1.0, 0, 260, 21, 240, 0, 3 | 7 << 2),
           "a seed on a linear field": (0.0, 1.0, 0, 260, 21, 240, 0, 1 << 2),
           "a seed on a category": (0.0, 1.0, 0, 260, 21, 12, 0, CATEGORY | 1 << 2),
           "a periodic category": (0.0, 1.0, 0, 260, 21, 12, 1, CATEGORY),
           "a periodic hashed field": (0.0, 1.0, 0, 260, 21, 500, 1, HASHED | 5 << 2),
           "a category without buckets": (0.0, 1.0, 0, 260, 21, 0, 0, CATEGORY),
           "a category of negative buckets": (0.0, 1.0, 0, 260, 21, -3, 0, CATEGORY),
           "a category wider than its bits": (0.0, 1.0, 0, 260, 21, 13, 0, CATEGORY),
           "a hashed field without buckets": (0.0, 1.0, 0, 260, 21, 0, 0, HASHED),
           "a hashed field of width 257": (0.0, 1.0, 0, 260, 257, 500, 0, HASHED),
           "a hashed field of width 0": (0.0, 1.0, 0, 260, 0, 500, 0, HASHED),
           # the refusals every kind shares
           "a hashed field past the row": (0.0, 1.0, 50, 260, 21, 500, 0, HASHED),
           "a category over the next field": (0.0, 1.0, 10, 260, 21, 12, 0, CATEGORY),
           "a hashed field with an infinite scale": (0.0, float("inf"), 0, 260, 21, 500, 0, HASHED),
           "a category with a NaN minimum": (float("nan"), 1.0, 0, 260, 21, 12, 0, CATEGORY)}
    htm = model(4)
    eng = htm.engine
    lib, h, void = eng.lib, eng.h, C.c_void_p
    d_values, d_bank = eng.upload_values(values), eng.zero_bank(5)
    d_votes, d_out = eng.device_buffer(5 * I * 4, np.zeros((5, I), np.int32)), eng.device_buffer(5 * 2 * 2 * 4)
    group = B.ModelGroup.create(2, I, Cn, K, active_columns=k, seeds=range(3, 5))
    lk = B.AnomalyLikelihood(2, **as_kwargs(P_SMALL))
    warm = np.random.RandomState(1).uniform(0, 3, (2, 2))
    group.tick(warm, encoder=both["mixed"], use_graph=False, likelihood=lk)         # (binds the likelihood, makes the tick's buffers)
    group._current()
    host = np.zeros((2, 2), np.int32)
    rows, pairs, scores = np.zeros(2, dtype=_lib.HtmLiveRow), np.zeros((2, 2, 2), np.int32), np.zeros(2)
    ptr = lambda a: a.ctypes.data_as(void)
    calls = []
    for name, row in bad.items():
        t = table([row, good])
        calls += [(name, "htm_bank_encode", lambda t=t: lib.htm_bank_encode(h, t, 2, void(d_values), 5, void(d_bank), 5, 0)),
                  (name, "htm_decode_votes", lambda t=t: lib.htm_decode_votes(h, t, 2, void(d_votes), 5, void(d_out))),
                  (name, "htm_predicted_value", lambda t=t: lib.htm_predicted_value(h, t, 2, ptr(host))),
                  (name, "htm_live_tick", lambda t=t: lib.htm_live_tick(group._g, ptr(warm), t, 2, None, None, 1, 0, ptr(rows), ptr(pairs), None)),
                  (name, "htm_likelihood_tick", lambda t=t: lib.htm_likelihood_tick(group._g, ptr(warm), t, 2, None, None, 1, 0, ptr(rows), ptr(pairs), None,
                                                                                      lk._lk, ptr(scores)))]
    codes = {}
    out["refused"] = traced(lambda: codes.update({f"{name}: {fn}": call() for name, fn, call in calls}))
    out["codes"] = codes
    # the decode cap of a hashed field is on buckets + width - 1, and the decoding calls' alone (an engine wide enough for it)
    wide = B.SpatialPooler(8200, 64, 4)._ensure_engine()
    w_bank, w_votes = wide.zero_bank(1), wide.device_buffer(8200 * 4, np.zeros(8200, np.int32))
    over, exact = table([(0.0, 1.0, 0, 5000, 64, 8130, 0, HASHED | 2 << 2)]), table([(0.0, 1.0, 0, 5000, 64, 8129, 0, HASHED | 2 << 2)])
    out["cap"] = [lib.htm_bank_encode(wide.h, over, 1, void(d_values), 1, void(w_bank), 1, 0),
                  lib.htm_decode_votes(wide.h, over, 1, void(w_votes), 1, void(d_out)),
                  lib.htm_bank_encode(wide.h, exact, 1, void(d_values), 1, void(w_bank), 1, 0),
                  lib.htm_decode_votes(wide.h, exact, 1, void(w_votes), 1, void(d_out))]
    # ... and every handle goes on
    eng.bank_encode(both["mixed"], d_values, 5, d_bank, 5)
    group.tick(warm, encoder=both["mixed"], use_graph=False, likelihood=lk)
    print(json.dumps(out))


if __name__ == "__main__":
    main()
