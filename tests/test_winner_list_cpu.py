"""No GPU: the last launch of the batched run's two-launch step (k_last_handover, csrc/htm_handover_last.h) -- its compiler report,
a report of its own beside the reports whose sets of kernels earlier tests hold (bithtm_amd.build.LAST_REPORTS), and the launches
the host code makes (tests/host_stub/winner_list_driver.py): a step that begins with k_first_handover ends with k_last_handover,
always; every other caller keeps k_learn_scan_emit."""
import collections
import json
import os
import re
import subprocess
import sys

import pytest

from test_launch_trace_cpu import ROOT, _build, needs_hipcc


def test_the_last_launch_reports_alone_with_the_figures_of_the_kernel_it_stands_in_for():
    """Every instantiation: no scratch, at most 80 VGPRs, the LDS and the occupancy of k_learn_scan_emit with the same template
    arguments.  One instantiation is held to its twin's own figure instead of 80: k_learn_scan_emit<8, 4, false> (the large-pool form
    of 8 entries per lane, 5 waves per SIMD by its launch bounds' leave) has 86 VGPRs in tests/golden/kernel_resources_before_knn.json,
    and the kernel that stands in for it has the same 86."""
    from bithtm_amd.build import (BANK_REPORTS, LAST_REPORTS, LATER_REPORTS, OWN_REPORTS, all_kernel_resources, every_kernel_resources,
                                  kernel_resources, library_kernel_resources, whole_library_kernel_resources)
    new, old, whole = kernel_resources("htm_handover_last.h"), kernel_resources(), whole_library_kernel_resources()
    if new is None or old is None:
        pytest.skip("the library in the tree was not built here")
    assert list(LAST_REPORTS) == ["htm_handover_last.h"]
    assert (list(OWN_REPORTS), list(LATER_REPORTS), list(BANK_REPORTS)) == (["htm_knn.h"], ["htm_handover.h"], ["htm_knn_bank.h"])
    assert {re.match(r"_Z\d+([a-z_]+?)I", k).group(1) for k in new} == {"k_last_handover"}, sorted(new)
    assert len(new) == 12                           # EPL 1, 2, 4, 8 x (small pool with the LDS tables, without, large pool)
    # the four earlier functions return what they returned: none holds the new kernel, and the fifth is all of them and the new report
    knn, first, bank = kernel_resources("htm_knn.h"), kernel_resources("htm_handover.h"), kernel_resources("htm_knn_bank.h")
    assert all_kernel_resources() == {**old, **knn} and every_kernel_resources() == {**old, **knn, **first}
    library = library_kernel_resources()
    assert library == {**old, **knn, **first, **bank} and not set(new) & set(library)
    assert whole == {**library, **new} and len(whole) == len(library) + len(new)
    with open(os.path.join(ROOT, "tests", "golden", "kernel_resources_before_knn.json")) as f:
        assert old == json.load(f)
    # (the budget tests find kernels with re.search: no name inside another)
    names = {re.match(r"_Z\d+(k[a-z]*_[a-z_]+)", k).group(1).rstrip("I") for k in library if re.match(r"_Z\d+k[a-z]*_", k)}
    assert not [s for s in names if s in "k_last_handover" or "k_last_handover" in s]
    for name, r in sorted(new.items()):
        twin = old[re.sub(r"^_Z\d+k_last_handover", "_Z17k_learn_scan_emit", name)]
        print(name, r, "\n   k_learn_scan_emit:", twin)
        assert r["scratch_bytes_per_lane"] == 0 and r["agprs"] == 0, (name, r)
        assert r["vgprs"] <= max(80, twin["vgprs"]) and (twin["vgprs"] <= 80 or r["vgprs"] == twin["vgprs"]), (name, r, twin)
        assert r["lds_bytes"] == twin["lds_bytes"] and r["occupancy"] == twin["occupancy"], (name, r, twin)


@pytest.fixture(scope="module")
def launched(tmp_path_factory):
    tmp = str(tmp_path_factory.mktemp("winner_list_trace"))
    env = dict(os.environ, BITHTM_LIBRARY=_build(tmp), BITHTM_STUB_TRACE=os.path.join(tmp, "trace.txt"))
    for name in ("LD_PRELOAD", "BITHTM_LEAN", "BITHTM_SCAN_LARGE"):
        env.pop(name, None)
    open(env["BITHTM_STUB_TRACE"], "w").close()
    r = subprocess.run([sys.executable, os.path.join(ROOT, "tests", "host_stub", "winner_list_driver.py")], env=env, capture_output=True,
                       text=True, timeout=600)
    assert r.returncode == 0, (r.stdout + r.stderr)[-4000:]
    return json.loads(r.stdout.splitlines()[-1])


CALLS = ("", " more", " resume", " capture", " learning off")


@needs_hipcc
@pytest.mark.parametrize("K", [8, 40])
@pytest.mark.parametrize("form", ["run", "run large"])
def test_a_step_that_begins_with_the_hand_over_ends_with_the_list_kernel(launched, form, K):
    """The batched run's two-launch schedule, small-pool and large-pool scan: streamed calls, a call's last step, the resume fallback,
    graph capture, learning off.  Each k_first_handover is followed by exactly one k_last_handover before the next one, and the
    schedule launches no k_learn_scan_emit: the flag words are always reset and the list always has a writer."""
    for call in CALLS:
        kernels = launched[f"{form} K={K}{call}"]
        count = collections.Counter(kernels)
        assert count["k_first_handover"] >= 3 and count["k_first_handover"] == count["k_last_handover"], (call, count)
        assert not count["k_learn_scan_emit"] and not count["k_act_mid_rows"], (call, count)
        chain = [k for k in kernels if k in ("k_first_handover", "k_last_handover")]
        assert chain == ["k_first_handover", "k_last_handover"] * (len(chain) // 2), (call, chain)
    # one of each per steady step: the 12 steps of the streamed call
    count = collections.Counter(launched[f"{form} K={K}"])
    assert count["k_first_handover"] == 12 and count["k_last_handover"] == 12, count


@needs_hipcc
@pytest.mark.parametrize("K", [8, 40])
def test_the_other_callers_keep_their_kernels(launched, K):
    """process(), a model group's step and run, and the three- and four-launch schedules launch neither of the two kernels"""
    for name in [f"{form} K={K}{call}" for form in ("run lean1", "run lean0") for call in CALLS + (" process",)] + \
                [f"run K={K} process", f"run large K={K} process", "group step", "group run"]:
        count = collections.Counter(launched[name])
        assert sum(count.values()) > 0, name
        assert not count["k_first_handover"] and not count["k_last_handover"], (name, count)
    for call in CALLS:
        lean1, lean0 = collections.Counter(launched[f"run lean1 K={K}{call}"]), collections.Counter(launched[f"run lean0 K={K}{call}"])
        assert lean1["k_learn_scan_emit"] >= 3 and lean1["k_act_rows"] == lean1["k_mid_overlap"] == lean1["k_learn_scan_emit"], (call, lean1)
        assert not lean0["k_learn_scan_emit"], (call, lean0)
    assert collections.Counter(launched[f"run K={K} process"])["k_act_mid_rows"] == 1
