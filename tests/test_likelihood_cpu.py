"""Anomaly likelihood (bithtm_amd/likelihood.py, AnomalyLikelihood, htm_likelihood_*) -- what holds without a
GPU: the C ABI's declarations and binding, the refusals, the tail table's error bound, hand-computed values of the definition,
the definition over split calls, the path every case of tests/likelihood_cases.py names, the compiler's report for the new
kernels, the launches and copies of a scored tick and of an update (the host code built host-only against
tests/host_stub/hip_stub_runtime.cpp), and the host code under ASan + UBSan as a stand-alone program
(tests/host_stub/likelihood_host.cpp), which also evaluates the kernel header's arithmetic on the host against the definition."""
import ctypes as C
import json
import math
import os
import re
import subprocess
import sys

import numpy as np
import pytest

import likelihood_cases as cases
from likelihood_cases import CHUNK, P_EVERY, P_SMALL, P_WIDE, SPLITS, SPLIT_IDS, as_kwargs

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CLANG_DIR = "/opt/rocm/lib/llvm"
HEADER = os.path.join(ROOT, "include", "bithtm_hip.h")
KERNELS = os.path.join(ROOT, "bithtm_amd", "csrc", "htm_likelihood.h")
needs_hipcc = pytest.mark.skipif(not os.path.exists("/opt/rocm/bin/hipcc"), reason="needs hipcc")

ABI = {"htm_likelihood_create": "htm_handle *h", "htm_likelihood_destroy": "htm_likelihood *lk", "htm_likelihood_update": "htm_likelihood *lk",
       "htm_likelihood_reset": "htm_likelihood *lk", "htm_likelihood_state_bytes": "const htm_likelihood *lk", "htm_likelihood_export": "htm_likelihood *lk",
       "htm_likelihood_import": "htm_likelihood *lk", "htm_likelihood_tick": "htm_group *g"}


# ---- the C ABI
def test_the_header_declares_the_likelihood_abi_and_the_binding_matches_it():
    from bithtm_amd import _lib as L
    header = open(HEADER).read()
    decl = {m.group(1): m.group(2) for m in re.finditer(r"\b(htm_likelihood_[a-z_]+)\s*\(([^)]*)\)\s*;", header)}
    assert set(decl) == set(ABI)
    for name, params in decl.items():
        assert params.split(",")[0].strip() == ABI[name], (name, params)
        assert len(L.EXPORTS[name][1]) == len(params.split(",")), name
    assert L.EXPORTS["htm_likelihood_destroy"][0] is None and L.EXPORTS["htm_likelihood_state_bytes"][0] is C.c_int64
    assert all(L.EXPORTS[n][0] is C.c_int for n in ABI if n not in ("htm_likelihood_destroy", "htm_likelihood_state_bytes"))
    # the scored tick is htm_live_tick's arguments and two more
    live = re.search(r"\bhtm_live_tick\s*\(([^)]*)\)\s*;", header).group(1)
    tick = [re.sub(r"\s+", " ", x.strip()) for x in decl["htm_likelihood_tick"].split(",")]
    assert tick[:-2] == [re.sub(r"\s+", " ", x.strip()) for x in live.split(",")] and tick[-2:] == ["htm_likelihood *lk", "double *likelihood"]
    assert L.EXPORTS["htm_likelihood_tick"][1][:-2] == L.EXPORTS["htm_live_tick"][1]
    assert L.ABI_VERSION == 4 and re.search(r"#define BITHTM_ABI_VERSION 4\b", header)
    body = re.search(r"typedef struct htm_likelihood_config \{(.*?)\} htm_likelihood_config;", header, re.S).group(1)
    assert [re.sub(r"\s+", " ", x.strip()) for x in body.split(";") if x.strip()] == [
        "uint32_t struct_bytes", "int32_t learning_period, estimation_samples, history, averaging_window, reestimation_period"]
    assert C.sizeof(L.HtmLikelihoodConfig) == 24
    assert [n for n, _ in L.HtmLikelihoodConfig._fields_[1:]] == list(cases.PARAMETERS)
    kernels = open(KERNELS).read()
    assert int(re.search(r"#define HTM_LIKELIHOOD_CHUNK (\d+)", kernels).group(1)) == L.LIKELIHOOD_CHUNK == CHUNK
    assert 2 * int(re.search(r"#define HTM_LIKELIHOOD_THREADS (\d+)", kernels).group(1)) == CHUNK      # (two steps per thread)


def test_the_c_calls_refuse_null_arguments_without_a_gpu():
    from bithtm_amd import _lib as L
    from bithtm_amd.likelihood import TAIL
    lib = L.load()
    cfg = L.HtmLikelihoodConfig(C.sizeof(L.HtmLikelihoodConfig), *P_SMALL)
    out = C.c_void_p(1)
    assert lib.htm_likelihood_create(None, C.byref(cfg), TAIL.ctypes.data_as(C.c_void_p), 1, C.byref(out)) == -1 and not out.value
    assert b"null" in lib.htm_last_error(None)
    assert lib.htm_likelihood_update(None, None, None, 1, None) == -1
    assert lib.htm_likelihood_reset(None, None, None) == -1
    assert lib.htm_likelihood_export(None, None, None, 0) == -1 and lib.htm_likelihood_import(None, None, None, 0) == -1
    assert lib.htm_likelihood_state_bytes(None) == -1
    rows = (L.HtmLiveRow * 2)()
    x = (C.c_uint32 * 8)()
    assert lib.htm_likelihood_tick(None, None, None, 0, x, None, 1, 1, rows, None, None, None, None) == -1
    lib.htm_likelihood_destroy(None)


def test_the_python_layer_refuses_before_any_library_call():
    import bithtm_amd as B
    from bithtm_amd.likelihood import check_counts, check_params
    assert check_params() == (288, 100, 8640, 10, 100)
    for bad in (dict(learning_period=-1), dict(estimation_samples=0), dict(history=0), dict(history=16385), dict(averaging_window=0),
                dict(averaging_window=65), dict(reestimation_period=0)):
        with pytest.raises(ValueError, match=list(bad)[0]):
            check_params(**bad)
        with pytest.raises(ValueError, match=list(bad)[0]):
            B.AnomalyLikelihood(2, **bad)
    with pytest.raises(ValueError, match="streams"):
        B.AnomalyLikelihood(0)
    for active, bursting in (([1, 2], [2, 2]), ([1, 2], [-1, 0]), ([1 << 24], [0]), ([1, 2], [0]), ([1.5], [1.0])):
        with pytest.raises(ValueError):
            check_counts(np.array(active), np.array(bursting))
    lk = B.AnomalyLikelihood(3, **as_kwargs(P_SMALL))
    with pytest.raises(ValueError, match=r"int \[3, T\]"):
        lk.update_counts(np.zeros((2, 5), int), np.zeros((2, 5), int))
    with pytest.raises(ValueError, match=r"bool \[3\]"):
        lk.reset([1, 0])
    with pytest.raises(RuntimeError, match="not bound"):
        lk.update_counts(np.zeros((3, 5), int), np.zeros((3, 5), int))
    # an unbound object holds a loaded state until it is bound
    state = lk.state_dict()
    assert state["t"].tolist() == [0, 0, 0] and state["a_ring"].shape == (3, 16) and state["q_ring"].shape == (3, 4)
    state["t"][:] = [4, 5, 6]
    state["a_ring"][1] = np.arange(16)
    lk.load_state_dict(state)
    again = lk.state_dict()
    assert all(np.array_equal(again[k], state[k]) for k in state)
    lk.reset([0, 1, 0])
    assert lk.state_dict()["t"].tolist() == [4, 0, 6] and not lk.state_dict()["a_ring"][1].any()
    with pytest.raises(ValueError, match="parameters"):
        B.AnomalyLikelihood(3).load_state_dict(state)
    state["t"][0] = -1
    with pytest.raises(ValueError, match="negative"):
        lk.load_state_dict(state)


def test_run_record_carries_the_likelihood_and_its_log_scale():
    import bithtm_amd as B
    from bithtm_amd.likelihood import log_likelihood
    rec = B.RunRecord(np.arange(3))
    assert rec.anomaly_likelihood is None and rec.log_likelihood is None
    L = np.array([0.5, 0.999995, 1.0 - 1e-15])
    rec = B.RunRecord(np.arange(3), anomaly_likelihood=L)
    assert rec.anomaly_likelihood is L and np.array_equal(rec.log_likelihood, log_likelihood(L))
    assert np.allclose(rec.log_likelihood, [math.log(0.5000000001) / math.log(1e-10), math.log(5.0001e-6) / math.log(1e-10), 1.0], atol=1e-6)
    rows = np.zeros(2, dtype=__import__("bithtm_amd")._lib.HtmLiveRow)
    assert B.GroupTick(rows).anomaly_likelihood is None
    assert B.GroupTick(rows, anomaly_likelihood=L[:2]).log_likelihood.shape == (2,)


# ---- the definition
def test_the_tail_table_interpolates_the_gaussian_tail_within_its_derived_bound():
    """Linear interpolation with step h = 1/64: |error| <= h^2 / 8 * max |Q''| = (1/64)^2 / 8 * phi(1) = 7.385e-6 (Q'' = z phi(z) peaks at
    z = 1).  Measured over z in [0, 8.5] on a grid 16 times finer than the table (beyond 8 the table stays at Q(8) = 6e-16)."""
    from bithtm_amd.likelihood import TAIL
    assert TAIL.shape == (513,) and TAIL.dtype == np.float64 and TAIL[0] == 0.5
    assert all(TAIL[i] == 0.5 * math.erfc((i / 64.0) / math.sqrt(2.0)) for i in range(513))
    bound = (1 / 64) ** 2 / 8 * math.exp(-0.5) / math.sqrt(2 * math.pi)
    assert 7.38e-6 < bound < 7.4e-6
    worst = 0.0
    for n in range(int(8.5 * 1024) + 1):
        z = n / 1024.0
        x = min(z, 8.0) * 64.0
        i = min(int(x), 511)
        f = x - i
        worst = max(worst, abs(TAIL[i] + f * (TAIL[i + 1] - TAIL[i]) - 0.5 * math.erfc(z / math.sqrt(2.0))))
    print("measured interpolation error", worst, "derived bound", bound)
    assert worst <= 7.4e-6


def _interp(z):
    from bithtm_amd.likelihood import TAIL
    x = min(abs(z), 8.0) * 64.0
    i = min(int(x), 511)
    return TAIL[i] + (x - i) * (TAIL[i + 1] - TAIL[i])


def test_hand_computed_values_of_a_12_step_stream():
    """P_small = (5, 3, 16, 4, 7): probation 8.  active = 32, so q = bursting * 2048; the averages over 4 steps and the estimate at
    t = 7 over a[5..7] = (4096, 12288, 24576) are worked out by hand: N = 3, S1 = 40960, S2 = 771751936, mean = 13653.33,
    var = (3 * 771751936 - 40960^2) / 9 = 70837134.2, std = 8416.48."""
    from bithtm_amd.likelihood import LikelihoodStream
    bursting = [0, 0, 0, 0, 0, 8, 16, 24, 32, 0, 0, 0]
    s = LikelihoodStream(**as_kwargs(P_SMALL))
    L = s.update(np.full(12, 32), np.array(bursting))
    assert s.t == 12 and s.estimates == 1 and s.has_estimate == 1
    a = [0, 0, 0, 0, 0, 4096, 12288, 24576, 40960, 36864, 28672, 16384]
    assert [s.a_ring[t % 16] for t in range(12)] == a
    assert s.q_ring == [65536, 0, 0, 0]                         # steps 8, 9, 10, 11
    assert 4096 ** 2 + 12288 ** 2 + 24576 ** 2 == 771751936
    mean, std = 40960.0 / 3.0, math.sqrt((3 * 771751936 - 40960 ** 2) / 9.0)
    assert (s.mean, s.std) == (mean, std) and abs(mean - 13653.33) < 0.01 and abs(std - 8416.48) < 0.01
    assert L[:7].tolist() == [0.5] * 7                          # no estimate before t + 1 = probation
    assert L[7:].tolist() == [1.0 - _interp((x - mean) / std) for x in a[7:]]
    # ... and against the normal distribution itself: z = 1.2978, 3.2444, 2.7578, 1.7844, 0.3245
    assert np.allclose(L[7:], [0.90282, 0.99941, 0.99709, 0.96282, 0.62720], atol=2e-5)
    # a value below the mean takes the tail itself
    low = LikelihoodStream(**as_kwargs(P_SMALL))
    low.update(np.full(8, 32), np.array([0, 0, 0, 0, 0, 32, 32, 0]))
    m7, s7 = low.mean, low.std                                  # over a[5..7] = (16384, 32768, 32768)
    assert low.a_ring[5:8] == [16384, 32768, 32768] and m7 == 81920.0 / 3.0
    L = low.update(np.array([32, 32]), np.array([0, 0]))        # a = 32768, then (65536 + 0 + 0 + 0) // 4 = 16384 < mean
    assert low.estimates == 1 and L[0] == 1.0 - _interp((32768 - m7) / s7) > 0.5 and L[1] == _interp((16384 - m7) / s7) < 0.5


@pytest.mark.parametrize("name,pname,splits", SPLITS, ids=SPLIT_IDS)
def test_the_definition_over_split_calls_equals_one_call(name, pname, splits):
    params = cases.PARAMS[pname]
    T = sum(splits)
    for stream in (("binomial", "alternating") if pname == "P_wide" else cases.STREAMS):
        active, bursting = cases.stream(stream, T, seed=3)
        whole, end = cases.reference(params, active[None], bursting[None])
        cut, end_cut = cases.reference(params, active[None], bursting[None], splits)
        assert np.array_equal(whole.view(np.uint64), cut.view(np.uint64)), (name, stream)
        a, b = cases.stacked_state(end), cases.stacked_state(end_cut)
        assert all(np.array_equal(a[k], b[k]) for k in a), (name, stream)
        assert ((0.0 <= whole) & (whole <= 1.0)).all()


def test_every_case_reaches_the_path_it_names():
    from bithtm_amd.likelihood import MEAN_FLOOR, VARIANCE_FLOOR, LikelihoodStream, estimate, q_of
    # the streams
    assert q_of(40, 40) == q_of(32, 32) == q_of(47, 47) == 65536 and q_of(0, 0) == 0 and q_of(37, 37) == 65536 and q_of(48, 3) == 4096 and q_of(3, 1) == 21845
    active, bursting = cases.member_streams(130, 64)
    keys = [(a.tobytes(), b.tobytes()) for a, b in zip(active, bursting)]
    assert len(set(keys[:10])) == 9 and all(x != y for x, y in zip(keys, keys[1:]))       # (only the idle stream repeats)
    assert (active[1] == 0).all() and (bursting[0] == active[0]).all() and set(bursting[3]) == {0, 37}
    # P_small: probation, a re-estimate and both rings wrapped within 60 steps
    s = LikelihoodStream(**as_kwargs(P_SMALL))
    L = s.update(*cases.stream("binomial", 60))
    assert (L[:7] == 0.5).all() and L[7] != 0.5 and s.estimates == 8 and s.t > 3 * P_SMALL[2] and s.t > P_SMALL[3]
    # ... and the splits that begin and end on its points (t + 1 = 8, 15, 22, 29, 36, ...)
    ends = np.cumsum(dict((n, sp) for n, _, sp in SPLITS)["on-points"])
    assert {15, 22, 36} <= set(ends.tolist()) and {7, 14} <= set(ends.tolist())       # (a call beginning at t = 7 / 14 ends the one before at 7 / 14)
    # constant streams: var = 0 -> the variance floor; q = 0 -> the mean floor too
    s = LikelihoodStream(**as_kwargs(P_SMALL))
    s.update(*cases.stream("constant", 30, seed=0))
    assert (s.mean, s.std) == (MEAN_FLOOR, math.sqrt(VARIANCE_FLOOR))
    s = LikelihoodStream(**as_kwargs(P_SMALL))
    s.update(*cases.stream("constant", 30, seed=1))
    assert (s.mean, s.std) == (4096.0, math.sqrt(VARIANCE_FLOOR))
    s = LikelihoodStream(**as_kwargs(P_SMALL))
    s.update(*cases.stream("idle", 30))
    assert (s.mean, s.std) == (MEAN_FLOOR, math.sqrt(VARIANCE_FLOOR)) and s.q_ring == [0] * 4
    # P_every: an estimate per step, a window that grows through the whole case, the averaging window filling at t = 63
    s = LikelihoodStream(**as_kwargs(P_EVERY))
    L = s.update(*cases.stream("alternating", CHUNK + 1))
    assert s.estimates == CHUNK + 1 == s.t < P_EVERY[2] and (L != 0.5).any()
    # P_wide: its points (t + 1 = 15 + 4096 k), more than `history` steps in one call, and the largest sums -- N * S2 = 2^60 at N = 16384
    s = LikelihoodStream(**as_kwargs(P_WIDE))
    s.update(*cases.stream("bursting", 16385 + 20000))
    assert s.estimates == 1 + (16385 + 20000 - 15) // 4096 == 9 and s.t > 2 * P_WIDE[2]
    assert set(s.a_ring) == {65536} and len(s.a_ring) == 16384
    n, s1, s2 = 16384, 16384 * 65536, 16384 * 65536 ** 2
    assert n * s2 == 2 ** 60 == s1 * s1 and (s.mean, s.std) == estimate(n, s1, s2) == (65536.0, math.sqrt(VARIANCE_FLOOR))
    wide = dict((n, sp) for n, _, sp in SPLITS)
    assert wide["wide"][0] > P_WIDE[2] and np.cumsum(wide["wide-on-points"]).tolist() == [14, 15, 4111, 8206, 8207]
    assert [sp for n, _, sp in SPLITS if n in ("chunk", "chunk+1", "2chunk+3")] == [[CHUNK], [CHUNK + 1], [2 * CHUNK + 3]]


# ---- the compiler's report
def test_the_new_kernels_have_no_scratch_and_the_existing_ones_keep_their_figures():
    from bithtm_amd.build import kernel_resources
    res = kernel_resources()
    if res is None:
        pytest.skip("the library in the tree was not built here")
    new = {k: v for k, v in res.items() if re.match(r"_Z\d+klik_", k)}
    assert sorted(re.match(r"_Z\d+(klik_[a-z]+)", k).group(1) for k in new) == ["klik_reset", "klik_tick", "klik_update"], sorted(new)
    for name, r in new.items():
        print(name, r)
        assert r["scratch_bytes_per_lane"] == 0, (name, r)
        assert r["lds_bytes"] <= 64 * 1024 and r["occupancy"] >= 1, (name, r)
    old_names = {re.match(r"_Z\d+(k[a-z]*_[a-z_]+)", k).group(1) for k in res if k not in new and re.match(r"_Z\d+k[a-z]*_", k)}
    for k in new:                                   # (the budget tests find kernels with re.search: no name inside another)
        assert not [s for s in old_names if s in k], k
    # every kernel that existed before the likelihood was added: the figures the compiler gave it then.  The fixture is
    # bithtm_amd/libbithtm_hip.resources.json (what bithtm_amd.build writes beside the library) of a build of the commit before
    # htm_likelihood.h, copied as it is.  Kernels added later are none of this test's business; a change that moves an older
    # kernel's figures on purpose regenerates the fixture from its own parent commit in the same way and says so.
    with open(os.path.join(ROOT, "tests", "golden", "kernel_resources_before_likelihood.json")) as f:
        before = json.load(f)
    changed = {k: (before[k], res.get(k)) for k in before if before[k] != res.get(k)}
    assert not changed, changed


# ---- the launch traces
def _host_objects(tmp, extra=()):
    """htm_engine.hip host-only and the stub runtime, as tests/test_live_tick_cpu.py builds them (`extra`: further flags for both)
    -> (engine object, stub object, the --defsym the link needs for the device image the host object expects)."""
    hipcc = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
    clang = os.path.join(CLANG_DIR, "bin", "clang++")
    flags = ["-std=c++17", "-O1", "-g", "-fPIC", "-fno-omit-frame-pointer"] + list(extra)
    obj, stub = (os.path.join(tmp, n) for n in ("engine_host.o", "hip_stub.o"))
    subprocess.run([hipcc, "--offload-host-only", "-ffp-contract=off", "-w"] + flags + ["-c", os.path.join(ROOT, "bithtm_amd", "csrc", "htm_engine.hip"), "-o", obj],
                   check=True, capture_output=True)
    subprocess.run([clang, "-D__HIP_PLATFORM_AMD__", "-I/opt/rocm/include", "-w"] + flags + ["-c", os.path.join(ROOT, "tests", "host_stub", "hip_stub_runtime.cpp"), "-o", stub],
                   check=True, capture_output=True)
    undefined = subprocess.run(["nm", "-u", obj], check=True, capture_output=True, text=True).stdout
    fatbin = re.search(r"__hip_fatbin_\w+", undefined)       # (the device image the host object expects beside it: there is none)
    return obj, stub, ([f"-Wl,--defsym={fatbin.group(0)}=0"] if fatbin else [])


@pytest.fixture(scope="module")
def traces(tmp_path_factory):
    tmp = str(tmp_path_factory.mktemp("likelihood_trace"))
    obj, stub, defsym = _host_objects(tmp)
    lib = os.path.join(tmp, "libbithtm_host_trace.so")
    subprocess.run([os.path.join(CLANG_DIR, "bin", "clang++"), "-shared", obj, stub, "-ldl", "-o", lib] + defsym, check=True, capture_output=True)
    env = dict(os.environ, BITHTM_LIBRARY=lib, BITHTM_STUB_TRACE=os.path.join(tmp, "trace.txt"))
    for name in ("LD_PRELOAD", "BITHTM_LEAN", "BITHTM_SCAN_LARGE"):
        env.pop(name, None)
    r = subprocess.run([sys.executable, os.path.join(ROOT, "tests", "host_stub", "likelihood_driver.py")], env=env, capture_output=True, text=True,
                       timeout=600)
    assert r.returncode == 0, (r.stdout + r.stderr)[-4000:]
    return json.loads(r.stdout.splitlines()[-1])


def _kernel(line):
    m = re.match(r"launch _Z(\d+)", line)
    return line[m.end():m.end() + int(m.group(1))] if m else None


def _launch(line):
    """(kernel, grid x, grid y, block, lds) of a launch line."""
    m = re.match(r"launch (\S+) grid (\d+) (\d+) block (\d+) lds (\d+)", line)
    return (_kernel(line),) + tuple(int(x) for x in m.groups()[1:])


@needs_hipcc
@pytest.mark.parametrize("enc", [0, 1])
def test_a_scored_tick_is_one_launch_more_with_the_same_two_copies(traces, enc):
    for n in (1, 7):
        plain, scored = (traces["tick"][f"B={n} enc={enc} scored={s}"] for s in (0, 1))
        assert [x.split()[0] for x in plain if not x.startswith("launch ")] == ["memcpy", "memcpy"], plain
        assert [x.split()[0] for x in scored if not x.startswith("launch ")] == ["memcpy", "memcpy"], scored
        # the scored tick is the plain one with klik_tick between the finish launch and the copy out
        assert scored[:-2] == plain[:-1] and _kernel(scored[-3]) == "klive_finish", (plain, scored)
        assert _launch(scored[-2]) == ("klik_tick", 1, n, 256, 0), scored[-2]
        assert plain[0] == scored[0]                                       # (the copy in)
        out_plain, out_scored = int(plain[-1].split()[1]), int(scored[-1].split()[1])
        assert out_plain == n * 48 + (n * 2 * 8 if enc else 0) and out_scored == out_plain + 8 * n
    # ... whatever B is
    strip = lambda lines: [(_kernel(x), x.split()[0]) for x in lines]
    assert strip(traces["tick"][f"B=1 enc={enc} scored=1"]) == strip(traces["tick"][f"B=7 enc={enc} scored=1"])


@needs_hipcc
def test_an_update_is_one_launch_per_chunk_and_one_copy_of_the_table_whatever_b_is(traces):
    for T in (1, CHUNK, CHUNK + 1, 2 * CHUNK + 3):
        launches = -(-T // CHUNK)
        for n in (1, 3, 130):
            lines = traces["update"][f"B={n} T={T}"]
            assert [_launch(x) for x in lines if x.startswith("launch ")] == [("klik_update", 1, n, 256, 0)] * launches, lines
            assert [x for x in lines if not x.startswith("launch ")] == ([] if n == 1 else [f"memcpy {8 * n}"]), lines
            if n > 1:
                assert lines[0].startswith("memcpy ")
    for n in (1, 3, 130):
        assert [_launch(x) for x in traces["reset"][f"B={n} mask=0"]] == [("klik_reset", 1, n, 256, 0)]
        masked = traces["reset"][f"B={n} mask=1"]
        assert masked[0] == f"memcpy {4 * n}" and [_launch(x) for x in masked[1:]] == [("klik_reset", 1, n, 256, 0)]


# ---- the host code under ASan + UBSan, as a stand-alone program, and the kernel header's arithmetic on the host
def _arithmetic_cases():
    """The lines of the case file and, per line, what the definition gives (strings as the program prints them)."""
    from bithtm_amd.likelihood import TAIL, estimate, likelihood_of, q_of
    bits = lambda x: "%016x" % np.float64(x).view(np.uint64)
    rng = np.random.default_rng(5)
    lines, expect = ["T " + " ".join(bits(x) for x in TAIL)], []
    for active, bursting in [(0, 0), (1, 0), (1, 1), (3, 1), (40, 40), (48, 3), ((1 << 24) - 1, (1 << 24) - 1), ((1 << 24) - 1, 1)] + \
            [(int(a), int(rng.integers(0, a + 1))) for a in rng.integers(1, 1 << 24, 40)]:
        lines.append(f"q {active} {bursting}")
        expect.append(str(q_of(active, bursting)))
    windows = [[0], [65536], [0] * 16384, [65536] * 16384, [0, 65536] * 8192, [4096] * 7, [1966, 1967], [65535, 65536, 65534]]
    windows += [rng.integers(0, 65537, int(n)).tolist() for n in rng.integers(1, 16385, 24)]
    windows += [rng.binomial(40, 0.1, int(n)).astype(np.int64).__mul__(65536 // 40).tolist() for n in (3, 100, 8640)]
    pairs = []
    for h in windows:
        n, s1, s2 = len(h), sum(h), sum(x * x for x in h)
        lines.append(f"e {n} {s1} {s2}")
        pairs.append(estimate(n, s1, s2))
        expect.append(bits(pairs[-1][0]) + " " + bits(pairs[-1][1]))
    for mean, std in pairs:
        for a in [0, 65536, int(mean), int(mean) + 1, min(65536, int(mean + 8 * std)), min(65536, int(mean + 8 * std) + 1),
                  max(0, int(mean - 3 * std))] + rng.integers(0, 65537, 6).tolist():
            lines.append(f"l {a} {bits(mean)} {bits(std)}")
            expect.append(bits(likelihood_of(a, mean, std)))
    return lines, expect


@needs_hipcc
def test_the_host_code_runs_clean_under_asan_and_ubsan_and_the_header_arithmetic_equals_the_definition(tmp_path):
    """tests/host_stub/likelihood_host.cpp and htm_engine.hip (host-only), both with -fsanitize=address,undefined, linked against the
    stub runtime into ONE program that is run directly: nothing is preloaded."""
    tmp = str(tmp_path)
    san = ["-fsanitize=address,undefined", "-fno-sanitize-recover=undefined"]
    obj, stub, defsym = _host_objects(tmp, san)
    clang = os.path.join(CLANG_DIR, "bin", "clang++")
    exe = os.path.join(tmp, "likelihood_host")
    subprocess.run([clang, "-std=c++17", "-O1", "-g", "-fno-omit-frame-pointer", "-ffp-contract=off"] + san +
                   [os.path.join(ROOT, "tests", "host_stub", "likelihood_host.cpp"), obj, stub, "-ldl", "-o", exe] + defsym, check=True, capture_output=True)
    lines, expect = _arithmetic_cases()
    path = os.path.join(tmp, "cases.txt")
    with open(path, "w") as f:
        f.write("\n".join(lines) + "\n")
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=0", UBSAN_OPTIONS="print_stacktrace=1")
    for name in ("LD_PRELOAD", "BITHTM_STUB_TRACE", "BITHTM_LIBRARY"):
        env.pop(name, None)
    r = subprocess.run([exe, path], env=env, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0 and r.stdout.strip().endswith("ok"), (r.stdout + r.stderr)[-6000:]
    assert "runtime error" not in r.stderr and "AddressSanitizer" not in r.stderr, r.stderr[-6000:]
    got = r.stdout.split("\n")[:-2]
    assert len(got) == len(expect) > 400
    wrong = [(line, g, e) for line, g, e in zip(lines[1:], got, expect) if g != e]
    assert not wrong, wrong[:5]
