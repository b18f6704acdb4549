"""One classifier object through both sets of C calls (tests/test_classifier_doors_cpu.py, tests/test_hip_classifier_doors.py; DESIGN.md
section 24): htm_classifier_* and htm_classifiers_* are two doors to one implementation and act on one state.  An object made by
htm_classifier_create with the parameters of group_classifier_cases.MIXED is fed stream 0 of mixed_stream(), twice over, in the short
calls of PLAN -- alternately through htm_classifier_update and htm_classifiers_update, learning and frozen, with one
htm_classifiers_reset with a flag in the middle -- and read back through both doors.  Not collected by pytest; run as a program (over
the host stub library, with BITHTM_STUB_TRACE) it prints the launches of the alternation as one JSON object."""
import ctypes as C
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if __name__ == "__main__":
    sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]

import group_classifier_cases as G  # noqa: E402

# (door, steps, learn) per update call; "reset": htm_classifiers_reset(clf, h, [1]) there, the definition's reset()
PLAN = [("one", 2, 1), ("bank", 1, 1), ("bank", 3, 1), ("one", 2, 0), ("bank", 1, 0), ("one", 3, 1), "reset", ("bank", 2, 1), ("one", 4, 1), ("bank", 3, 0),
        ("one", 3, 1)]
STEPS = sum(c[1] for c in PLAN if c != "reset")


def stream():
    """Stream 0 of mixed_stream(), twice over: (index int32 [24, 7], words uint32 [24, 7], targets int32 [24], resets bool [24])."""
    return tuple(np.concatenate([a[0], a[0]]) for a in G.mixed_stream())


def expected_kernels():
    out = []
    for c in PLAN:
        if c != "reset":
            k = "kcls_" if c[0] == "one" else "kgcls_"
            out += [k + "sum", k + "apply"] * c[1] if c[2] else [k + "frozen"]
    return out


def definition():
    """ClassifierDefinition over the same calls -> (best [24, H, 2], dist [24, H, B], the definition)."""
    index, words, targets, resets = stream()
    d = G.definition(G.MIXED)
    best, dist, at = [], [], 0
    for c in PLAN:
        if c == "reset":
            d.reset()
            continue
        n = c[1]
        b, q = d.update(index[at:at + n], words[at:at + n], targets[at:at + n], resets[at:at + n], bool(c[2]))
        best.append(b)
        dist.append(q)
        at += n
    return np.concatenate(best), np.concatenate(dist), d


def alternate(engine):
    """The calls of PLAN on a new object through `engine`'s handle -> dict(best, dist, weights_one, weights_bank, blob_one, blob_bank)."""
    from bithtm_amd import _lib as L
    from bithtm_amd.classifier import EXP_TABLE
    p, lib = G.MIXED, engine.lib
    H, Bk, units, P = len(p["steps"]), p["buckets"], p["column_dim"] * p["cell_dim"], p["max_pairs"]
    index, words, targets, resets = stream()
    assert len(index) == STEPS
    cfg = L.HtmClassifierConfig(C.sizeof(L.HtmClassifierConfig), Bk, H, p["alpha_q"], units, p["cell_dim"], P, (C.c_int32 * 8)(*p["steps"]))
    clf = C.c_void_p()
    ptr = lambda a: a.ctypes.data_as(C.c_void_p)
    table = lambda address: (C.c_void_p * 1)(address)

    def ok(rc, what):
        assert rc == 0, (what, rc, lib.htm_last_error(engine.h).decode())
    ok(lib.htm_classifier_create(engine.h, C.byref(cfg), ptr(EXP_TABLE), C.byref(clf)), "htm_classifier_create")
    bufs = []

    def device(a):
        bufs.append(engine.device_buffer(a.nbytes, a))
        return bufs[-1]
    try:
        pairs = np.empty(index.shape + (2,), np.int32)
        pairs[..., 0], pairs[..., 1] = index, words.view(np.int32)
        best, dist, at = device(np.zeros((STEPS, H, 2), np.int32)), device(np.zeros((STEPS, H, Bk), np.int32)), 0
        for c in PLAN:
            if c == "reset":
                ok(lib.htm_classifiers_reset(clf, engine.h, ptr(np.ones(1, np.uint8))), "htm_classifiers_reset")
                continue
            door, n, learn = c
            bits = np.zeros(4, np.uint8)                # (a call of at most 32 steps: one word of reset bits)
            bits[:1] = np.packbits(resets[at:at + n], bitorder="little")
            dp, dt, dr = device(np.ascontiguousarray(pairs[at:at + n])), device(np.ascontiguousarray(targets[at:at + n])), device(bits)
            out = (C.c_void_p(best + at * H * 2 * 4), C.c_void_p(dist + at * H * Bk * 4))
            if door == "one":
                ok(lib.htm_classifier_update(clf, engine.h, C.c_void_p(dp), index.shape[1], n, C.c_void_p(dt), n, 0, C.c_void_p(dr), learn, *out), "htm_classifier_update")
            else:
                ok(lib.htm_classifiers_update(clf, engine.h, table(dp), index.shape[1], n, table(dt), n, 0, table(dr), learn, *out), "htm_classifiers_update")
            at += n
        engine.sync()
        got = dict(best=engine.read_words(best, STEPS * H * 2, np.int32).reshape(STEPS, H, 2),
                   dist=engine.read_words(dist, STEPS * H * Bk, np.int32).reshape(STEPS, H, Bk))
        size = 16 + (p["steps"][-1] + 1) * P * 8
        assert lib.htm_classifier_state_bytes(clf) == lib.htm_classifiers_state_bytes(clf) == size
        got["blob_one"], got["blob_bank"] = np.zeros(size, np.uint8), np.full(size, 255, np.uint8)
        ok(lib.htm_classifier_export(clf, engine.h, ptr(got["blob_one"]), size), "htm_classifier_export")
        ok(lib.htm_classifiers_export(clf, engine.h, ptr(got["blob_bank"]), size), "htm_classifiers_export")
        got["weights_one"], got["weights_bank"] = np.zeros((H, units, Bk), np.int32), np.full((H, units, Bk), -1, np.int32)
        for h in range(H):
            ok(lib.htm_classifier_read_weights(clf, engine.h, h, 0, units, ptr(got["weights_one"][h])), "htm_classifier_read_weights")
            ok(lib.htm_classifiers_read_weights(clf, engine.h, 0, h, 0, units, ptr(got["weights_bank"][h])), "htm_classifiers_read_weights")
        return got
    finally:
        engine.sync()
        lib.htm_classifier_destroy(clf)
        for b in bufs:
            lib.hipFree(b)


def home_engine():
    """A small model's engine on device 0: the handle the calls go through."""
    import bithtm_amd as B
    home = B.HierarchicalTemporalMemory(32, 64, 4, active_columns=4, device=0)
    return home, home.engine


def main():
    trace = os.environ["BITHTM_STUB_TRACE"]
    home, engine = home_engine()
    with open(trace) as f:
        n = len(f.read().splitlines())
    got = alternate(engine)
    with open(trace) as f:
        lines = f.read().splitlines()[n:]
    print(json.dumps(dict(lines=lines, total_one=int(got["blob_one"][:8].view(np.int64)[0]), total_bank=int(got["blob_bank"][:8].view(np.int64)[0]),
                          blobs_equal=bool(np.array_equal(got["blob_one"], got["blob_bank"])))))


if __name__ == "__main__":
    main()
