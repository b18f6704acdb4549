"""Driver of the launch traces of the coordinate fields (tests/test_coordinate_cpu.py; used as field_kinds_driver.py is: the engine's
host code host-only, no sanitizer, nothing preloaded, over tests/host_stub's runtime with BITHTM_STUB_TRACE).  Three encoders of
three value columns over the same 300-bit row: "linear" (three linear fields), "mixed" (a hashed, a category and a linear field)
and "coordinate" (one coordinate field: a group of three table entries).

Prints one JSON object:
  "trace"    {"<linear|mixed|coordinate> <call>": trace lines}, the calls being
               bank_encode, decode_votes      one Engine.bank_encode / decode_votes of 5 rows
               predicted_value                htm.predicted_value(encoder)
               recorded                       run(values, 6, encoder=, record=("predicted_value",)) behind a first such call
               tick B=1, tick B=3, scored B=3 one eager tick behind a warm-up tick of the same kind
  "refused"  the trace lines of every refused call below (none), "codes" their return codes
  "accepted" the codes of good tables from every entry point (all 0): a group at the table's end, two groups, sixteen entries
  "after"    {"linear", "mixed"}: a tick with that encoder right behind one with the coordinate encoder on the same group

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
from live_tick_cases import MID  # noqa: E402

I, Cn, K, k = MID
COORD = 3
ENTRIES = ("htm_bank_encode", "htm_decode_votes", "htm_predicted_value", "htm_live_tick", "htm_likelihood_tick")


def lines():
    with open(TRACE) as f:
        return f.read().splitlines()


def traced(call):
    n = len(lines())
    call()
    return lines()[n:]


def encoders():
    linear = B.ScalarEncoder([B.ScalarField(0.0, 3.0, 200, 21, periodic=True), B.ScalarField(0.0, 3.0, 60, 5), B.ScalarField(0.0, 3.0, 37, 5)], input_dim=I)
    mixed = B.ScalarEncoder([B.HashedField(0.0, 3.0, 200, 21, buckets=500, seed=5), B.CategoryField(3, 5, bits=60), B.ScalarField(0.0, 3.0, 37, 5)], input_dim=I)
    coordinate = B.ScalarEncoder([B.CoordinateField(297, 21, 9, seed=5)], input_dim=I)
    return {"linear": linear, "mixed": mixed, "coordinate": coordinate}


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
    values = np.random.RandomState(2).uniform(0, 3, (5, 3))
    htm = model(3)                                  # (one model for the three tables: its schedule is the same in every leg)
    eng = htm.engine
    for enc in encoders().values():                 # (untimed first uses: the handle's buffers, the banks, the graphs of either parity)
        htm.predicted_value(enc)
        htm.run(values, 6, encoder=enc, record=("predicted_value",))
    for name, enc in encoders().items():
        d_values, d_bank = eng.upload_values(values), eng.zero_bank(5)
        d_votes, d_out = eng.device_buffer(5 * I * 4, np.zeros((5, I), np.int32)), eng.device_buffer(5 * 3 * 2 * 4)
        out["trace"][f"{name} bank_encode"] = traced(lambda: eng.bank_encode(enc, d_values, 5, d_bank, 5))
        out["trace"][f"{name} decode_votes"] = traced(lambda: eng.decode_votes(enc, d_votes, 5, d_out))
        out["trace"][f"{name} predicted_value"] = traced(lambda: htm.predicted_value(enc))
        htm.run(values, 6, encoder=enc, record=("predicted_value",))
        out["trace"][f"{name} recorded"] = traced(lambda: htm.run(values, 6, encoder=enc, record=("predicted_value",)))
        for n, scored in ((1, 0), (3, 0), (3, 1)):
            group = B.ModelGroup.create(n, I, Cn, K, active_columns=k, seeds=range(3, 3 + n))
            lk = B.AnomalyLikelihood(n, **as_kwargs(P_SMALL)) if scored else None
            x = np.random.RandomState(n).uniform(0, 3, (2, n, 3))
            group.tick(x[0], encoder=enc, use_graph=False, likelihood=lk)
            out["trace"][f"{name} {'scored' if scored else 'tick'} B={n}"] = traced(lambda: group.tick(x[1], encoder=enc, use_graph=False, likelihood=lk))
    # a linear and a mixed tick right behind a coordinate one, on one group
    three = encoders()
    group = B.ModelGroup.create(3, I, Cn, K, active_columns=k, seeds=range(3, 6))
    x = np.random.RandomState(9).uniform(0, 3, (6, 3, 3))
    out["after"] = {}
    for n, name in enumerate(("linear", "mixed")):
        group.tick(x[3 * n], encoder=three[name], use_graph=False)
        group.tick(x[3 * n + 1], encoder=three["coordinate"], use_graph=False)
        out["after"][name] = traced(lambda: group.tick(x[3 * n + 2], encoder=three[name], use_graph=False))

    # ---- tables: (minimum, scale, offset, bits, width, buckets, periodic, reserved)
    head = (0.0, 1.0, 0, 200, 21, 9, 0, COORD | 5 << 2)
    tail = (0.0, 1.0, 0, 0, 0, 0, 0, COORD)
    lin = lambda offset: (-1.0, 16.5, offset, 37, 5, 33, 0, 0)
    alter = lambda row, **kw: tuple(kw.get(name, v) for name, v in zip(("minimum", "scale", "offset", "bits", "width", "buckets", "periodic", "reserved"), row))
    bad = {"a head at the end of the table": [lin(200), head],
           "a head with one continuation at the end": [lin(200), head, tail],
           "a head followed by a linear field": [head, lin(200), lin(240)],
           "a head with one continuation, then a linear field": [head, tail, lin(200)],
           "a head with one continuation, then a head": [head, tail, alter(head, offset=200, bits=50), tail, tail],
           "a continuation first in the table": [tail, lin(200), lin(240)],
           "a continuation behind a linear field": [lin(200), tail, tail],
           "two continuations without a head": [tail, tail, lin(200)],
           "a third continuation": [head, tail, tail, tail],
           "a third continuation in front of a linear field": [head, tail, tail, tail, lin(200)],
           "max_radius 128": [alter(head, buckets=128), tail, tail],
           "max_radius -1": [alter(head, buckets=-1), tail, tail],
           "width 0": [alter(head, width=0), tail, tail],
           "width 257": [alter(head, width=257), tail, tail],
           "a periodic head": [alter(head, periodic=1), tail, tail],
           "a periodic continuation": [head, tail, alter(tail, periodic=1)],
           "a seed on a continuation": [head, alter(tail, reserved=COORD | 5 << 2), tail],
           "a width on a continuation": [head, tail, alter(tail, width=21)],
           "buckets on a continuation": [head, alter(tail, buckets=9), tail],
           "a continuation at another offset": [head, tail, alter(tail, offset=1)],
           "negative bits on a continuation": [head, alter(tail, bits=-1), tail],
           "a head past the row": [alter(head, offset=150), alter(tail, offset=150), alter(tail, offset=150)],
           "a head at a negative offset": [alter(head, offset=-1), alter(tail, offset=-1), alter(tail, offset=-1)],
           "a head over the field in front of it": [lin(0), alter(head, offset=30), alter(tail, offset=30), alter(tail, offset=30)],
           "a linear field over the head behind it": [head, tail, tail, lin(199)],
           "a head with an infinite scale": [alter(head, scale=float("inf")), tail, tail],
           "a head with a NaN minimum": [alter(head, minimum=float("nan")), tail, tail],
           "a y column with scale 0": [head, alter(tail, scale=0.0), tail],
           "a radius column with a NaN minimum": [head, tail, alter(tail, minimum=float("nan"))],
           "a negative reserved": [alter(head, reserved=-1), tail, tail]}
    good = {"a group alone": [head, tail, tail],
            "a group at the table's end": [lin(200), head, tail, tail],
            "two groups": [head, tail, tail, alter(head, offset=200, bits=100, reserved=COORD), alter(tail, offset=200), alter(tail, offset=200)],
            "max_radius 0 and 127, width 1 and 256": [alter(head, buckets=0, width=1), tail, tail, alter(head, offset=200, bits=1, buckets=127, width=256),
                                                       alter(tail, offset=200), alter(tail, minimum=-3.0, scale=0.5, offset=200)],
            "sixteen entries ending in a group": [(0.0, 1.0, 200 + 2 * j, 2, 1, 2, 0, 0) for j in range(13)] + [head, tail, tail]}
    htm = model(4)
    eng = htm.engine
    lib, h, void = eng.lib, eng.h, C.c_void_p
    wide = np.random.RandomState(2).uniform(0, 3, (5, 16))
    d_values, d_bank = eng.upload_values(wide), eng.zero_bank(5)
    d_votes, d_out = eng.device_buffer(5 * I * 4, np.zeros((5, I), np.int32)), eng.device_buffer(5 * 16 * 2 * 4)
    group = B.ModelGroup.create(2, I, Cn, K, active_columns=k, seeds=range(3, 5))
    lk = B.AnomalyLikelihood(2, **as_kwargs(P_SMALL))
    warm = np.random.RandomState(1).uniform(0, 3, (2, 16))
    group.tick(warm[:, :3], encoder=three["coordinate"], use_graph=False, likelihood=lk)        # (binds the likelihood, makes the tick's buffers)
    group._current()
    host = np.zeros((16, 2), np.int32)
    rows, pairs, scores = np.zeros(2, dtype=_lib.HtmLiveRow), np.zeros((2, 16, 2), np.int32), np.zeros(2)
    ptr = lambda a: a.ctypes.data_as(void)

    def calls(name, entries):
        t, n = table(entries), len(entries)
        return [(name, "htm_bank_encode", lambda: lib.htm_bank_encode(h, t, n, void(d_values), 5, void(d_bank), 5, 0)),
                (name, "htm_decode_votes", lambda: lib.htm_decode_votes(h, t, n, void(d_votes), 5, void(d_out))),
                (name, "htm_predicted_value", lambda: lib.htm_predicted_value(h, t, n, ptr(host))),
                (name, "htm_live_tick", lambda: lib.htm_live_tick(group._g, ptr(warm), t, n, None, None, 1, 0, ptr(rows), ptr(pairs), None)),
                (name, "htm_likelihood_tick", lambda: lib.htm_likelihood_tick(group._g, ptr(warm), t, n, None, None, 1, 0, ptr(rows), ptr(pairs), None,
                                                                              lk._lk, ptr(scores)))]
    codes = {}
    refused = [c for name, entries in bad.items() for c in calls(name, entries)]
    out["refused"] = traced(lambda: codes.update({f"{name}: {fn}": call() for name, fn, call in refused}))
    out["codes"] = codes
    out["accepted"] = {f"{name}: {fn}": call() for name, entries in good.items() for name, fn, call in calls(name, entries)}
    # ... and every handle goes on
    eng.bank_encode(three["coordinate"], d_values, 5, d_bank, 5)
    group.tick(warm[:, :3], encoder=three["coordinate"], use_graph=False, likelihood=lk)
    print(json.dumps(out))


if __name__ == "__main__":
    main()
