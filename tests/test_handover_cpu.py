"""No GPU: the compiler's report of the batched run's first launch (k_first_handover, csrc/htm_handover.h) -- a report of its own,
beside the reports whose sets of kernels earlier tests hold (bithtm_amd.build.LATER_REPORTS)."""

import re

import pytest

LDS_PER_CU = 160 * 1024          # gfx950
DYNAMIC_LDS = 4096 * 4           # what the launch asks for on every step: the overlap role's histogram, SEL_BINS words


def test_the_first_launch_reports_alone_and_leaves_eight_blocks_per_cu():
    from bithtm_amd.build import LATER_REPORTS, OWN_REPORTS, all_kernel_resources, every_kernel_resources, kernel_resources
    new, old, knn, pinned, every = (kernel_resources("htm_handover.h"), kernel_resources(), kernel_resources("htm_knn.h"),
                                    all_kernel_resources(), every_kernel_resources())
    if new is None or old is None or knn is None:
        pytest.skip("the library in the tree was not built here")
    assert list(LATER_REPORTS) == ["htm_handover.h"] and "htm_handover.h" not in OWN_REPORTS
    assert [re.match(r"_Z\d+([a-z_]+?)\d", k).group(1) for k in new] == ["k_first_handover"], sorted(new)
    # the three reports are disjoint, the pinned set does not hold the new kernel, and together they are every kernel of the library
    assert not set(new) & set(pinned) and set(pinned) == set(old) | set(knn)
    assert every == {**old, **knn, **new} and len(every) == len(old) + len(knn) + len(new)
    # (the budget tests find kernels with re.search: no name inside another)
    names = {re.match(r"_Z\d+(k[a-z]*_[a-z_]+)", k).group(1) for k in pinned if re.match(r"_Z\d+k[a-z]*_", k)}
    assert "k_act_mid_rows" in names
    assert not [s for s in names if s in "k_first_handover" or "k_first_handover" in s]
    (name, r), = new.items()
    print(name, r)
    # 64 registers are 8 waves per SIMD, 8 blocks of 4 waves per CU: the whole grid of the bench shape is resident at once
    assert r["occupancy"] >= 8 and r["vgprs"] <= 64 and r["agprs"] == 0, r
    assert r["scratch_bytes_per_lane"] <= 24, r
    # 8 blocks per CU beside the dynamic LDS: 8 x (static + 16 384) <= 163 840, that is static <= 4 096 bytes -- and no more than
    # k_act_mid_rows' own, the launch this one stands in for, which the library's occupancy query finds at 8 blocks per CU
    assert 8 * (r["lds_bytes"] + DYNAMIC_LDS) <= LDS_PER_CU, r
    first, = [v for k, v in old.items() if "k_act_mid_rows" in k]
    assert r["lds_bytes"] <= first["lds_bytes"], (r, first)
