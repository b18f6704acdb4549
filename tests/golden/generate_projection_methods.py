#!/usr/bin/env python3
"""Records tests/golden/projection_methods.npz from the UNMODIFIED reference, for tests/test_projection_methods_cpu.py.

Needs a checkout of the reference (cokwa/bitHTM):   BITHTM_REFERENCE=<checkout> python tests/golden/generate_projection_methods.py

Every case of tests/projection_method_cases.py is replayed on the reference's own PredictiveProjection (projections.py:194-293):
its store is loaded with the case's rows in the reference's layout (bithtm_amd.projections.SegmentProjectionView builds
it), and `process` / `update` / `get_jittered_potential_info` are called with the case's arguments while `np.random.rand`
is the keyed generator (oracle.ref_hooks.keyed_rand).  The step that keys the draws follows the oracle's convention:
`update` uses the current index, `process` uses it and then advances it; the jitter of a State asked for without it
(return_jittered_potential_info=False) is drawn with the index of the process call that made the State.

Kept per case: a digest of its inputs (the exported store and first State, every argument of every call; the arguments
themselves where they are small), and after every call a digest of every field of the store in canonical form and, for a
process, of every field of the State.  Asserted while recording: no growth of any call has a priority tie across its cut
(KeyedRand.growth_ties == 0) -- such ties are implementation-defined in the reference.  An empty
`winner_input` goes to the reference as None (its add_edge raises IndexError on an empty list)."""

import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

import projection_method_cases as pc  # noqa: E402
from refdiff import digest, reference_store  # noqa: E402
from oracle.ref_hooks import import_reference, keyed_rand  # noqa: E402
from bithtm_amd.projections import SegmentProjectionView  # noqa: E402

PATH = os.path.join(HERE, "projection_methods.npz")
SMALL = 20000                   # arguments of at most this many elements are kept as they are


def load_reference_projection(ref, case):
    """The reference's PredictiveProjection holding the case's exported store."""
    st, N = case.state0, case.N
    p = case.params
    proj = ref.projections.PredictiveProjection(N, **{f: getattr(p, f) for f in p.__dataclass_fields__})
    S = int(st["S"])
    view = SegmentProjectionView(st["presyn"], st["perm"], N)
    D = ref.projections.DynamicArray2D
    sp = proj.segment_projection

    def filled(dtype, values, growth, on_grow=None):
        a = D(dtype, size=values.shape, growth_exponential=growth, on_grow=on_grow)
        a[:] = values
        return a
    sp.output_dim = S
    sp.output_edges = filled(np.int32, view.output_edges, (True, False))
    sp.output_edge = filled(np.int32, view.output_edge.astype(np.int32), (True, True), sp.on_output_edge_grow)
    sp.output_permanence = filled(np.float32, view.output_permanence, (True, True), sp.on_output_permanence_grow)
    sp.input_edge = filled(np.int32, view.input_edge, (False, True), sp.on_input_edge_grow)
    proj.segment_bundle = filled(np.int32, np.asarray(st["seg_cell"], dtype=np.int32)[:, None], (True, False))
    proj.bundle_segments = np.asarray(st["segcount"], dtype=np.int32).copy()
    return proj


class ReferenceTarget:
    """The reference behind the interface projection_method_cases.replay drives."""

    def __init__(self, ref, case, patch):
        self.proj, self.patch, self.case = load_reference_projection(ref, case), patch, case
        self.step = int(case.state0["step_index"]) - 1
        self.first_state = self.process(case.first_active)
        for f in pc.STATE_FIELDS:
            assert digest(getattr(self.first_state, f)) == digest(case.state0[f]), f"{case.name}: first State, {f}"

    def process(self, active, return_jittered_potential_info=True):
        self.patch.step = self.step
        st = self.proj.process(active, return_jittered_potential_info=return_jittered_potential_info)
        st.made_at = self.step
        self.step += 1
        return st

    def get_jittered_potential_info(self, st):
        self.patch.step = st.made_at
        return self.proj.get_jittered_potential_info(st)

    def update(self, prev, activation, learning, punish, winner, output_learning, eps, raises):
        self.patch.step = self.step
        if winner is not None and len(winner) == 0:
            winner = None               # (the reference's add_edge raises IndexError on an empty list; the contract: empty means None)
        self.proj.update(prev, activation, learning, punish, winner_input=winner, output_learning=output_learning, epsilon=eps)

    def snapshot(self):
        holder = type("T", (), {"distal_projection": self.proj})()
        seg_cell, presyn, perm, nsyn, segcount = reference_store(holder)
        return pc.store_snapshot(seg_cell, presyn, perm, nsyn, segcount)


def input_digests(case):
    """One digest for the exported store and first State, one per call."""
    first = digest(np.array([digest(case.state0[k]) for k in sorted(case.state0)], dtype=np.uint64).view(np.int64))
    calls = []
    for call in case.calls:
        parts = [digest(np.frombuffer(call["op"].encode(), dtype=np.uint8))]
        for k in sorted(call):
            v = call[k]
            if isinstance(v, np.ndarray):
                parts.append(digest(v))
            elif isinstance(v, (bool, float)):
                parts.append(digest(np.float64(v)))
            else:
                parts.append(digest(np.frombuffer(repr(v).encode(), dtype=np.uint8)))
        calls.append(digest(np.array(parts, dtype=np.uint64).view(np.int64)))
    return np.array([first] + calls, dtype=np.uint64)


def trace_digests(case, tr):
    """uint64 [calls, store fields + State fields]; 0 where a call has no such field."""
    names = list(tr[0].store) + list(pc.STATE_FIELDS)
    out = np.zeros((len(tr), len(names)), dtype=np.uint64)
    for i, r in enumerate(tr):
        for j, n in enumerate(names):
            src = r.store if n in r.store else (r.state or {})
            if n in src:
                out[i, j] = digest(src[n])
    return names, out


def record_case(ref, name):
    case = pc.build(name)
    with keyed_rand(case.seed, case.cell_dim) as patch:
        tr = pc.replay(case, target=ReferenceTarget(ref, case, patch))
        assert patch.growth_ties == 0, f"{name}: {patch.growth_ties} growth ties across the cut -- choose another seed"
    names, dig = trace_digests(case, tr)
    ora_names, ora_dig = trace_digests(case, pc.oracle_trace(name)[0])
    assert names == ora_names
    bad = np.argwhere(dig != ora_dig)
    assert len(bad) == 0, f"{name}: the oracle differs from the reference at (call, field) {[(int(i), names[j]) for i, j in bad[:6]]}"
    out = {f"{name}/inputs": input_digests(case), f"{name}/digests": dig, f"{name}/segments": np.int64(len(tr[-1].store["seg_cell"]))}
    for i, call in enumerate(case.calls):               # the arguments themselves, where small
        for k in ("active", "learning", "winner"):
            v = call.get(k)
            if isinstance(v, np.ndarray) and v.size <= SMALL:
                out[f"{name}/call{i}/{k}"] = v.astype(np.int32)
        for k in ("activation", "punish", "output_learning"):
            v = call.get(k)
            if isinstance(v, np.ndarray) and v.size <= SMALL:
                out[f"{name}/call{i}/{k}"] = np.packbits(v)
    return names, out


def main():
    ref = import_reference()
    names, out = None, {}
    for name in pc.CASE_NAMES:
        if not pc.build(name).record:
            continue
        names, rec = record_case(ref, name)
        out.update(rec)
        print(f"{name}: {len(pc.build(name).calls)} calls, {int(rec[name + '/segments'])} segments")
    out["field_names"] = np.array(names)
    out["cases"] = np.array([n for n in pc.CASE_NAMES if pc.build(n).record])
    np.savez_compressed(PATH, **out)
    print(f"wrote {PATH}: {os.path.getsize(PATH)} bytes")


if __name__ == "__main__":
    main()
