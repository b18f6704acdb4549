"""The launches the engine's host code makes, without a GPU (tests/host_stub/trace_driver.py).

htm_engine.hip is compiled host-only (`hipcc --offload-host-only`, as tests/test_host_sanitizers.py does, but without a
sanitizer and with nothing preloaded) and linked against tests/host_stub/hip_stub_runtime.cpp, which with BITHTM_STUB_TRACE
writes one line per kernel launch.  Two properties of a batched call's modes (recorded, with reset bits, decoding) that hold
whatever the host code looks like inside: they end with their call, and the one step a call runs in the resume fallback --
the Spatial Pooler ahead, the pipelined schedule refused -- carries them like every other step of that call."""
import collections
import json
import os
import re
import subprocess
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CLANG_DIR = "/opt/rocm/lib/llvm"


def _build(tmp):
    hipcc = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
    clang = os.path.join(CLANG_DIR, "bin", "clang++")
    flags = ["-std=c++17", "-O1", "-g", "-fPIC", "-fno-omit-frame-pointer"]
    obj, stub, lib = (os.path.join(tmp, n) for n in ("engine_host.o", "hip_stub.o", "libbithtm_host_trace.so"))
    subprocess.run([hipcc, "--offload-host-only", "-ffp-contract=off", "-w"] + flags + ["-c", os.path.join(ROOT, "bithtm_amd", "csrc", "htm_engine.hip"), "-o", obj],
                   check=True, capture_output=True)
    subprocess.run([clang, "-D__HIP_PLATFORM_AMD__", "-I/opt/rocm/include", "-w"] + flags + ["-c", os.path.join(ROOT, "tests", "host_stub", "hip_stub_runtime.cpp"), "-o", stub],
                   check=True, capture_output=True)
    undefined = subprocess.run(["nm", "-u", obj], check=True, capture_output=True, text=True).stdout
    fatbin = re.search(r"__hip_fatbin_\w+", undefined)       # (the device image the host object expects beside it: there is none)
    subprocess.run([clang, "-shared", obj, stub, "-ldl", "-o", lib] + ([f"-Wl,--defsym={fatbin.group(0)}=0"] if fatbin else []),
                   check=True, capture_output=True)
    return lib


@pytest.fixture(scope="module")
def traces(tmp_path_factory):
    tmp = str(tmp_path_factory.mktemp("launch_trace"))
    env = dict(os.environ, BITHTM_LIBRARY=_build(tmp), BITHTM_STUB_TRACE=os.path.join(tmp, "trace.txt"))
    for name in ("LD_PRELOAD", "BITHTM_LEAN", "BITHTM_SCAN_LARGE"):
        env.pop(name, None)
    r = subprocess.run([sys.executable, os.path.join(ROOT, "tests", "host_stub", "trace_driver.py"), "invariants"], env=env, capture_output=True,
                       text=True, timeout=600)
    assert r.returncode == 0, (r.stdout + r.stderr)[-4000:]
    return json.loads(r.stdout.splitlines()[-1])


needs_hipcc = pytest.mark.skipif(not os.path.exists("/opt/rocm/bin/hipcc"), reason="needs hipcc")


@needs_hipcc
def test_modes_do_not_outlive_their_call(traces):
    """A plain 6-step run and a host-fed step behind an eager call with record + resets + predicted input make the launches they
    make behind a plain call of the same length: nothing of the call's modes is left on the handle."""
    tail = traces["tail_after_modes"]
    assert tail == traces["tail_after_plain"]
    assert sum(line.startswith("launch ") for line in tail) >= 6 * 2
    assert not [line for line in tail if re.search(r"k_(rec|pin|reset)_|k_tm_reset", line)], tail


@needs_hipcc
@pytest.mark.parametrize("n", [7, 1])
def test_the_fallback_step_carries_the_modes(traces, n):
    """An ahead call (continuing=True), then an eager pipeline=False call of n steps with record + resets + predicted input: the
    step it finishes for the call before and its other n - 1 steps are each reset, recorded and decoded, and each descriptor
    is filled once."""
    call = traces[f"fallback_{n}"]
    assert call["ahead"], "the first call did not leave the Spatial Pooler ahead: the second one took no fallback"
    count = collections.Counter(call["kernels"])
    assert [count[k] for k in ("k_rec_step", "k_pin_step", "k_tm_reset")] == [n, n, n], count
    assert [count[k] for k in ("k_rec_begin", "k_pin_begin", "k_reset_begin")] == [1, 1, 1], count
