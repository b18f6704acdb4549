"""htm_classifier_* and htm_classifiers_* act on one state (tests/classifier_doors.py) -- what holds without a GPU:
the alternation of tests/classifier_doors.py over the host code built host-only against tests/host_stub/hip_stub_runtime.cpp launches
the one-stream kernels through the one-stream door and the bank's kernels through the bank's, in the order of the calls, and both
exports give one blob.  (Kernels do nothing in the stub; tests/test_hip_classifier_doors.py holds the values to the definition.)"""
import json
import os
import subprocess
import sys

import classifier_doors as D
import group_classifier_cases as G
from test_likelihood_cpu import CLANG_DIR, ROOT, _host_objects, _kernel, _launch, needs_hipcc


def test_the_plan_alternates_the_doors_over_learning_and_frozen_calls_and_a_reset():
    calls = [c for c in D.PLAN if c != "reset"]
    assert D.STEPS == 24 == 2 * G.MIXED_T and all(1 <= c[1] <= 4 for c in calls)
    assert {(c[0], c[2]) for c in calls} == {("one", 1), ("one", 0), ("bank", 1), ("bank", 0)}
    assert [c[0] for c in calls] == ["one", "bank", "bank", "one", "bank", "one", "bank", "one", "bank", "one"] and D.PLAN.index("reset") == 6
    p = G.MIXED
    assert (p["buckets"], p["steps"], -(-p["max_pairs"] // 16)) == (3, (0, 2), 3)
    # the definition learns on both sides of the reset, and the reset shows: without it the weights end elsewhere
    best, dist, d = D.definition()
    assert d.total == 24 and d.dense_weights().any() and d.count < 24
    index, words, targets, resets = D.stream()
    whole = G.definition(p)
    at = 0
    for c in calls:
        whole.update(index[at:at + c[1]], words[at:at + c[1]], targets[at:at + c[1]], resets[at:at + c[1]], bool(c[2]))
        at += c[1]
    assert whole.count != d.count or not (whole.dense_weights() == d.dense_weights()).all()


@needs_hipcc
def test_the_alternation_launches_each_doors_kernels_in_the_order_of_the_calls(tmp_path):
    tmp = str(tmp_path)
    obj, stub, defsym = _host_objects(tmp)
    lib = os.path.join(tmp, "libbithtm_host_trace.so")
    subprocess.run([os.path.join(CLANG_DIR, "bin", "clang++"), "-shared", obj, stub, "-ldl", "-o", lib] + defsym, check=True, capture_output=True)
    env = dict(os.environ, BITHTM_LIBRARY=lib, BITHTM_STUB_TRACE=os.path.join(tmp, "trace.txt"))
    for name in ("LD_PRELOAD", "BITHTM_LEAN", "BITHTM_SCAN_LARGE"):
        env.pop(name, None)
    r = subprocess.run([sys.executable, os.path.join(ROOT, "tests", "classifier_doors.py")], env=env, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, (r.stdout + r.stderr)[-4000:]
    out = json.loads(r.stdout.splitlines()[-1])
    launches = [x for x in out["lines"] if x.startswith("launch ")]
    assert [_kernel(x) for x in launches] == D.expected_kernels(), launches
    H = len(G.MIXED["steps"])
    for x in launches:                                  # (one stream through either door: 40 pairs in three blocks, 7 a call in one)
        name, gx, gy, block, lds = _launch(x)
        assert (gx, block, lds) == (1 if name.endswith("frozen") else 3, 256, 0) and gy % H == 0 and (gy == H or name.endswith("frozen")), x
    frozen = [c[1] for c in D.PLAN if c != "reset" and not c[2]]
    assert [_launch(x)[2] for x in launches if _kernel(x).endswith("frozen")] == [H * n for n in frozen]
    # one stream: no pointer table is copied, whichever door; both exports give the one state, all 24 steps counted once
    assert not [x for x in out["lines"] if x == "memcpy 24"]
    assert out["blobs_equal"] and out["total_one"] == out["total_bank"] == D.STEPS
