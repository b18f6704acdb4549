#!/usr/bin/env python3
"""Records tests/golden/pool_geometry.npz from the UNMODIFIED reference, for tests/test_pool_geometry_cpu.py.

Needs a checkout of the reference (cokwa/bitHTM):   BITHTM_REFERENCE=<checkout> python tests/golden/generate_pool_geometry.py

Every recordable case of tests/pool_geometry_cases.py (all but natural_2p20_*) is run on the reference's own
HierarchicalTemporalMemory (networks.py:131-149): its DenseProjection holds the case's block-structured permanence, its
PredictiveProjection the case's crafted store in the reference's layout (generate_projection_methods.load_reference_projection),
the inhibition and the boosting are the documented stand-ins (oracle.ref_hooks.StableTopK / DocumentedExpBoosting) and
`np.random.rand` is the keyed generator (oracle.ref_hooks.keyed_rand).  It takes the case's first step with learning=False from its
empty state, as the case's builder did on the oracle, then the case's learning steps.

Kept per case: a digest of its inputs (permanence, duty cycle, the exported state, the patterns and the step list; the small index
arrays themselves) and after every step one digest per field of the store in canonical form (pool_geometry_cases.store_snapshot)
and of the step's States (refdiff.step_fields).  Asserted while recording: the oracle gives the same digests; no top-k call was
ambiguous; no growth had a priority tie across its cut (KeyedRand.growth_ties == 0)."""

import os
import sys
from types import SimpleNamespace

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
for p in (ROOT, os.path.join(ROOT, "tests"), HERE):
    if p not in sys.path:
        sys.path.insert(0, p)

import pool_geometry_cases as pg  # noqa: E402
from refdiff import digest, reference_store, step_fields  # noqa: E402

PATH = os.path.join(HERE, "pool_geometry.npz")


def _digest_of(parts):
    return digest(np.array(parts, dtype=np.uint64).view(np.int64))


def input_digest(case):
    """One digest for everything a replay of the case starts from."""
    st = case.state0
    parts = [digest(st[k]) for k in sorted(st)]
    parts += [digest(case.permanence), digest(case.duty0.view(np.int32)), digest(case.patterns), digest(np.array([case.first] + case.steps)),
              digest(np.array([case.I, case.C, case.K, case.k, case.slots, case.seed, case.capacity]))]
    p = case.params
    parts += [digest(np.float64(getattr(p, f))) for f in sorted(p.__dataclass_fields__)]
    return np.uint64(_digest_of(parts))


def trace_digests(tr):
    """(field names, uint64 [steps, fields]) of a trace: records with .store (store_snapshot), .sp and .tm (States)."""
    names, out = None, []
    for r in tr:
        fields = dict(r.store)
        fields.update(step_fields(r.sp, r.tm))
        names = names or list(fields)
        assert list(fields) == names
        out.append([digest(a) for a in fields.values()])
    return names, np.array(out, dtype=np.uint64)


def reference_trace(ref, case):
    from generate_projection_methods import load_reference_projection
    from oracle.ref_hooks import DocumentedExpBoosting, StableTopK, keyed_rand
    np.random.seed(case.seed)
    proximal = ref.projections.DenseProjection(case.I, case.C)
    proximal.permanence = case.permanence.copy()
    sp = ref.networks.SpatialPooler(case.I, case.C, case.k, proximal_projection=proximal, boosting=DocumentedExpBoosting(case.C, case.k),
                                    inhibition=StableTopK(case.k))
    distal = load_reference_projection(ref, SimpleNamespace(state0=case.store0, N=case.N, params=case.params))
    tm = ref.networks.TemporalMemory(case.C, case.K, distal_projection=distal)
    htm = ref.networks.HierarchicalTemporalMemory(case.I, case.C, case.K, active_columns=case.k, spatial_pooler=sp, temporal_memory=tm)
    out = []
    with keyed_rand(case.seed, case.K) as patch:
        patch.step = 0
        htm.process(case.patterns[case.first], learning=False)
        for t, j in enumerate(case.steps, 1):
            patch.step = t
            r_sp, r_tm = htm.process(case.patterns[j], learning=True)
            out.append(SimpleNamespace(t=t, sp=r_sp, tm=r_tm, store=pg.store_snapshot(*reference_store(htm.temporal_memory))))
        assert patch.growth_ties == 0, f"{case.name}: {patch.growth_ties} growth ties across the cut -- choose another seed"
    assert sp.inhibition.ambiguous_calls == 0, f"{case.name}: an ambiguous top-k"
    return out


def record_case(ref, name):
    case = pg.build(name)
    names, dig = trace_digests(reference_trace(ref, case))
    ora_names, ora_dig = trace_digests(pg.oracle_trace(name))
    assert names == ora_names
    bad = np.argwhere(dig != ora_dig)
    assert len(bad) == 0, f"{name}: the oracle differs from the reference at (step, field) {[(int(i) + 1, names[j]) for i, j in bad[:6]]}"
    tr = pg.oracle_trace(name)
    out = {f"{name}/inputs": input_digest(case), f"{name}/digests": dig, f"{name}/segments": np.int64(tr[-1].S),
           f"{name}/steps": np.array(case.steps, dtype=np.int32)}
    for t, r in enumerate(tr, 1):                       # what the allocation decided, as the ids themselves
        out[f"{name}/step{t}/recycled"] = r.last.recycled.astype(np.int32)
        out[f"{name}/step{t}/fresh"] = r.last.fresh.astype(np.int32)
    return names, out


def main():
    from oracle.ref_hooks import import_reference
    ref = import_reference()
    names, out = None, {}
    recorded = list(pg.SMALL)                        # (natural_2p20_* rest on the oracle alone)
    for name in recorded:
        names, rec = record_case(ref, name)
        out.update(rec)
        print(f"{name}: {len(pg.build(name).steps)} steps, {int(rec[name + '/segments'])} segments")
    out["field_names"] = np.array(names)
    out["cases"] = np.array(recorded)
    np.savez_compressed(PATH, **out)
    print(f"wrote {PATH}: {os.path.getsize(PATH)} bytes")


if __name__ == "__main__":
    main()
