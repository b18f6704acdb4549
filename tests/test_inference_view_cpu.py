"""CPU: inference views (include/bithtm_hip.h htm_create_view, htm_device_bytes) -- declared and bound, refusing NULL without a
GPU, the shared scan's compiler report, and the host code of views (reference counting, aliasing, refusals) under
AddressSanitizer + UndefinedBehaviorSanitizer over the host-memory HIP runtime of tests/host_stub."""

import ctypes as C
import glob
import os
import re
import subprocess
import sys

import pytest

from test_host_sanitizers import CLANG_DIR, _build

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
VIEW_ABI = {"htm_create_view": 2, "htm_device_bytes": 1}


def test_the_header_declares_the_view_abi_and_the_binding_matches_it():
    from bithtm_amd import _lib as L
    header = open(os.path.join(ROOT, "include", "bithtm_hip.h")).read()
    for name, n_args in VIEW_ABI.items():
        m = re.search(rf"^(int|int64_t) {name}\(([^)]*)\);", header, flags=re.M)
        assert m, name
        assert len([p for p in m.group(2).split(",") if p.strip()]) == n_args, name
        restype, argtypes = L.EXPORTS[name]
        assert len(argtypes) == n_args, name
    assert L.EXPORTS["htm_device_bytes"][0] is C.c_int64 and L.EXPORTS["htm_create_view"][0] is C.c_int
    assert L.ABI_VERSION == 4


def test_view_calls_refuse_null_without_touching_a_gpu():
    from bithtm_amd import _lib as L
    lib = L.load()
    out = C.c_void_p(1234)
    assert lib.htm_create_view(None, C.byref(out)) == -1 and out.value is None
    assert b"null parent" in lib.htm_last_error(None)
    assert lib.htm_create_view(None, None) == -1
    assert lib.htm_device_bytes(None) == -1


def test_inference_view_is_exported():
    import bithtm_amd as B
    assert issubclass(B.InferenceView, B.HierarchicalTemporalMemory)
    assert callable(B.ModelGroup.views) and callable(B.HierarchicalTemporalMemory.inference_view)


def test_the_shared_scan_has_no_scratch_and_keeps_its_occupancy():
    """kgrp_scan_shared as built: no scratch, 112 VGPRs and 4 waves per SIMD when it was written (its LDS -- up to 64 KiB of
    member bitmaps -- is what bounds it at the large shapes: two blocks per CU).  Its name matches no group twin pattern."""
    from bithtm_amd.build import kernel_resources
    res = kernel_resources()
    if res is None:
        pytest.skip("the library in the tree was not built here")
    k = [v for n, v in res.items() if "kgrp_scan_shared" in n]
    assert len(k) == 1, k
    assert k[0]["scratch_bytes_per_lane"] == 0 and k[0]["occupancy"] >= 4 and k[0]["vgprs"] <= 128, k[0]
    assert not [n for n in res if re.search(r"kgrp_scanILb", n) and "shared" in n]


@pytest.mark.skipif(not os.path.exists("/opt/rocm/bin/hipcc"), reason="needs hipcc")
def test_view_host_code_under_address_and_ub_sanitizers(tmp_path):
    lib = _build(str(tmp_path))
    runtime = glob.glob(os.path.join(CLANG_DIR, "lib", "clang", "*", "lib", "linux", "libclang_rt.asan-x86_64.so"))
    assert runtime, "AddressSanitizer runtime not found"
    env = dict(os.environ, BITHTM_LIBRARY=lib, LD_PRELOAD=runtime[0], ASAN_OPTIONS="detect_leaks=0:abort_on_error=0:halt_on_error=1",
               UBSAN_OPTIONS="print_stacktrace=1:halt_on_error=1", BITHTM_EAGER_BELOW="0")
    r = subprocess.run([sys.executable, os.path.join(ROOT, "tests", "host_stub", "view_driver.py")], env=env, capture_output=True, text=True,
                       timeout=600)
    tail = (r.stdout + r.stderr)[-4000:]
    assert r.returncode == 0 and "view sanitizer driver: ok" in r.stdout, tail
    assert "ERROR: AddressSanitizer" not in r.stderr and "runtime error:" not in r.stderr, tail
