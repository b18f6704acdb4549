"""Coordinate fields on the CPU (CoordinateField, geo_values; bithtm_amd/encoders.py is the definition): a row
worked by hand from mix32, every case of tests/coordinate_cases.py on the path it names (the ties at the cut among them), the
overlap property, geo_values against hand-computed numbers, the table and the key, the header's text, every refusal of the C ABI and
the launch traces of linear, mixed and coordinate tables (the host code built host-only against tests/host_stub/
hip_stub_runtime.cpp), the compiler's report for the three new kernels, and the host code under ASan + UBSan as a stand-alone
program (tests/host_stub/coordinate_host.cpp), which also evaluates the kernel header's arithmetic on the host against the
definition."""
import json
import math
import os
import re
import subprocess
import sys

import numpy as np
import pytest

import coordinate_cases as cases

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CLANG_DIR = "/opt/rocm/lib/llvm"
HEADER = os.path.join(ROOT, "include", "bithtm_hip.h")
needs_hipcc = pytest.mark.skipif(not os.path.exists("/opt/rocm/bin/hipcc"), reason="needs hipcc")


def _mix(x):
    """lowbias32 as htm_rng.h has it, in Python integers."""
    x ^= x >> 16
    x = x * 0x7FEB352D & 0xFFFFFFFF
    x ^= x >> 15
    x = x * 0x846CA68B & 0xFFFFFFFF
    return x ^ x >> 16


def _draw32(seed, step, x, y):
    """htm_draw32(htm_stream_base(seed, 8, step), (uint32)x, (uint32)y), not through bithtm_amd._keyed."""
    base = _mix(_mix((seed + 8 * 0x9E3779B9) & 0xFFFFFFFF) ^ step)
    return _mix(_mix(base ^ (x & 0xFFFFFFFF)) ^ (y & 0xFFFFFFFF))


def _by_hand(seed, bits, width, cx, cy, r):
    """The bits of one row from the definition's text: candidates y-major, by falling order and rising index, the first `width`."""
    cand = [(x, y) for y in range(cy - r, cy + r + 1) for x in range(cx - r, cx + r + 1)]
    ranked = sorted(range(len(cand)), key=lambda i: (-(_draw32(seed, 0, *cand[i]) >> 8), i))[:width]
    return sorted({_draw32(seed, 1, *cand[i]) * bits >> 32 for i in ranked}), sorted(ranked)


# ---- the definition
def test_one_row_by_hand():
    from bithtm_amd import CoordinateField, ScalarEncoder, ScalarField
    f = CoordinateField(37, 5, 3, resolution=(0.5, 2.0), origin=(10.0, -4.0), seed=6)
    assert (f.kind, f.bits, f.width, f.max_radius, f.buckets, f.seed, f.periodic) == ("coordinate", 37, 5, 3, 3, 6, False) and isinstance(f, ScalarField)
    assert (f.minimum, f.scale) == (10.0, 2.0) and [(a.minimum, a.scale, a.bits, a.width, a.buckets) for a in f.axes] == [(-4.0, 0.5, 0, 0, 0), (0.0, 1.0, 0, 0, 0)]
    enc = ScalarEncoder([ScalarField(0, 1, 11, 2), f], 50)
    assert len(enc) == 4 and enc.fields[1] is f and enc.fields[2:] == f.axes and enc.offsets == (0, 11, 11, 11)
    # x = 8.9 -> t = -2.2 -> cell -3; y = 3.9 -> t = 3.95 -> cell 3; radius 2.7 -> 2: 25 candidates, 5 winners
    cx, cy, r, ok = f.cells([8.9, 3.9, 2.7])
    assert (int(cx), int(cy), int(r), bool(ok)) == (-3, 3, 2, True)
    bits, winners = _by_hand(6, 37, 5, -3, 3, 2)
    assert sorted(f.selected(-3, 3, 2).tolist()) == winners and len(winners) == 5
    x = enc.encode([[np.nan, 8.9, 3.9, 2.7], [np.nan, 8.9, 3.9, 0.0], [np.nan, 8.9, 3.9, 9.0], [0.5, 8.9, np.nan, 1.0]])
    assert np.flatnonzero(x[0]).tolist() == [11 + b for b in bits]
    assert np.flatnonzero(x[1]).tolist() == [11 + (_draw32(6, 1, -3, 3) * 37 >> 32)]               # r = 0: the centre's bit alone
    assert np.flatnonzero(x[2]).tolist() == [11 + b for b in _by_hand(6, 37, 5, -3, 3, 3)[0]]     # 9 is clamped to max_radius 3
    assert np.flatnonzero(x[3]).tolist() == [5, 6]                                                 # a missing y: the linear field alone
    assert enc.bucket([[0.5, 8.9, 3.9, 2.7], [np.nan, 8.9, 3.9, -1.0]]).tolist() == [[5, 0, 0, 0], [-1, -1, -1, -1]]
    assert int(f.order(-3, 3)) == _draw32(6, 0, -3, 3) >> 8 and int(f.bit(-3, 3)) == _draw32(6, 1, -3, 3) * 37 >> 32
    # no decode: (-1, 0) and NaN in the three columns, whatever the votes
    bucket, score = enc.decode(np.full((2, 50), 7))
    assert bucket[:, 1:].tolist() == [[-1] * 3] * 2 and not score[:, 1:].any() and (bucket[:, 0] >= 0).all()
    assert np.isnan(enc.value_of(bucket)[:, 1:]).all() and np.isnan(enc.value_of([[0, 0, 0, 0]])[0, 1:]).all()
    for kw in (dict(bits=0), dict(width=0), dict(width=257), dict(max_radius=-1), dict(max_radius=128), dict(seed=-1), dict(seed=1 << 29), dict(resolution=0.0),
               dict(resolution=(1.0, np.inf)), dict(resolution=(1.0, 2.0, 3.0)), dict(origin=(0.0, np.nan)), dict(origin=0.0)):
        with pytest.raises(ValueError):
            CoordinateField(**dict(dict(bits=8, width=3, max_radius=2), **kw))
    assert CoordinateField(8, 256, 127, seed=(1 << 29) - 1).positions(0, 0, 127).shape == (256,)
    with pytest.raises(ValueError):
        ScalarEncoder([f.axes[0]])
    with pytest.raises(ValueError):                 # (sixteen value columns: five fields are fifteen, a sixth is eighteen)
        ScalarEncoder([CoordinateField(8, 3, 2) for _ in range(6)])
    assert len(ScalarEncoder([CoordinateField(8, 3, 2) for _ in range(5)] + [ScalarField(0, 1, 8, 2)])) == 16


def test_classifiers_refuse_a_coordinate_field_and_its_axes():
    from bithtm_amd import SDRClassifier, SDRClassifierBank
    enc = cases.track_encoder()
    assert SDRClassifier(field=enc.fields[0]).buckets == enc.fields[0].buckets
    for f in enc.fields[1:]:
        with pytest.raises(ValueError, match="coordinate"):
            SDRClassifier(field=f)
        with pytest.raises(ValueError, match="coordinate"):
            SDRClassifierBank(3, field=f)


def test_every_case_reaches_the_path_it_names():
    from bithtm_amd.engine import pack_bits  # noqa: F401  (the package imports)
    T = cases.THREADS
    reach = {}
    for name, (input_dim, _, _) in cases.CASES.items():
        enc, v = cases.encoder(name), cases.values(name)
        assert enc.input_dim == input_dim and v.shape[1] == len(enc) and 3 <= len(v) <= 64, name
        heads = [j for j, f in enumerate(enc.fields) if f.kind == "coordinate"]
        assert heads and all(enc.fields[j + 1:j + 3] == enc.fields[j].axes for j in heads), name
        rows = enc.encode(v)
        counts = []
        for j in heads:
            f = enc.fields[j]
            cx, cy, r, ok = f.cells(v[:, j:j + 3])
            assert np.array_equal(rows[:, enc.offsets[j]:enc.offsets[j] + f.bits].any(axis=1), ok), name
            counts.append((f, cx, cy, r, ok))
        reach[name] = counts
    N = lambda name, k=0: sorted({(2 * int(r) + 1) ** 2 for r, ok in zip(reach[name][k][3], reach[name][k][4]) if ok})
    assert N("r = 0 and N < width and N = width (no select)") == [1, 9, 25] and reach["r = 0 and N < width and N = width (no select)"][0][0].width == 25
    assert 25 in N("N = width + 1 (width 24, r = 2: the smallest select)") and reach["N = width + 1 (width 24, r = 2: the smallest select)"][0][0].width == 24
    around = N("N below and above the thread count (r = 3 .. 7: 49 .. 225; r = 8, 9, 11, 16: 289, 361, 529, 1089)")
    assert 225 in around and 289 in around and max(n for n in around if n < T) == 225 and min(n for n in around if n > T) == 289
    assert all(n % T for n in around) and {n // T for n in around} >= {0, 1, 2, 4, 6}             # (whole rounds of the block and a part of one)
    assert N("r = 127 (65 025 candidates, 255 rounds of the block)") == [253 ** 2, 255 ** 2] and 255 ** 2 == 65025 and -(-65025 // T) == 255
    f, cx, cy, r, ok = reach["a radius above max_radius is clamped (to 20; +inf too)"][0]
    assert r.tolist() == [20, 20, 20, 20, 20, 20, 19] and ok.all()
    assert N("max_radius 0 (every radius is 0: one candidate)") == [1]
    assert N("width 1 and width 256 (the cut is the maximum; 256 winners of 289)", 1) == [9, 225, 289, 361, 625]
    # ties: two candidates of the cut's order, 20 above it, and the lower index wins
    f, cx, cy, r, ok = reach["ties at the cut (two candidates of the cut's order, one slot: the lower index)"][0]
    assert (f.seed, f.width) == (cases.TIE_SEED, cases.TIE_WIDTH) and len(cases.TIES) == 4
    for (tx, ty, tr, (low, high), order), x, y, rad in zip(cases.TIES, cx, cy, r):
        assert (tx, ty, tr) == (x, y, rad) and low < high
        cut, above, at = cases.tie_rank(f, tx, ty, tr)
        assert (cut, above, at) == (order, 20, [low, high])
        won = f.selected(tx, ty, tr).tolist()
        assert low in won and high not in won and len(won) == 21
        assert sorted(won) == _by_hand(f.seed, f.bits, f.width, tx, ty, tr)[1]
    assert {tr for _, _, tr, _, _ in cases.TIES} == {8, 20} and any(high >= T > low for _, _, _, (low, high), _ in cases.TIES)   # (across two rounds of the block)
    # collisions
    f, cx, cy, r, ok = reach["bits 16 with width 21 (winners collide)"][0]
    rows = cases.encoder("bits 16 with width 21 (winners collide)").encode(cases.values("bits 16 with width 21 (winners collide)"))
    assert (f.bits, f.width) == (16, 21) and rows.sum(axis=1).max() <= 16 and len(set(f.positions(0, 0, 8).tolist())) < 21
    # values
    f, cx, cy, r, ok = reach["a missing x, y, radius and a negative radius, each alone"][0]
    assert ok.tolist() == [False] * 8 + [True, True, False] and r[8] == 0 and r[9] == 3
    f, cx, cy, r, ok = reach["coordinates negative, at 0, and at both ends of +-2**30"][0]
    v = cases.values("coordinates negative, at 0, and at both ends of +-2**30")
    for col, cell in ((0, cx), (1, cy)):
        for value, want in ((-cases.TWO30, -(1 << 30)), (cases.TWO30 - 1.0, (1 << 30) - 1), (cases.TWO30 - 0.5, (1 << 30) - 1), (-0.5, -1), (-0.0, 0), (0.0, 0)):
            hit = np.flatnonzero((v[:, col] == value) & (np.signbit(v[:, col]) == np.signbit(value)) & ok)
            assert len(hit) and (cell[hit] == want).all(), (col, value)
        for value in (cases.TWO30, -cases.TWO30 - 1.0, np.nextafter(-cases.TWO30, -np.inf), 1e300, -1e300):
            hit = np.flatnonzero(v[:, col] == value)
            assert len(hit) and not ok[hit].any(), (col, value)
    assert ok[-2:].all() and (cx[-2], cy[-2], cx[-1], cy[-1]) == (-(1 << 30), (1 << 30) - 1, (1 << 30) - 1, -(1 << 30))     # (candidates past +-2**30 wrap like uint32)
    f, cx, cy, r, ok = reach["a resolution and an origin per axis"][0]
    assert cx[:4].tolist() == [0, -1, 0, 1] and cy[:4].tolist() == [0, -1, 0, 1] and (f.scale, f.axes[0].scale) == (4.0, 1.0 / 3.0)
    # layout
    enc = cases.encoder("an offset that is no multiple of 32, the field across several 128-bit stores")
    assert enc.offsets[1] % 32 and enc.offsets[1] // 128 + 3 <= (enc.offsets[1] + enc.fields[1].bits - 1) // 128
    far = cases.encoder("a row wider than one pass of the storing loop (33 000 bits: 258 stores, 256 threads)")
    words = (far.input_dim + 31) // 32 + 3 & ~3
    assert words // 4 > T and far.offsets[1] < T * 128 < far.offsets[1] + far.fields[1].bits
    x = far.encode(cases.values("a row wider than one pass of the storing loop (33 000 bits: 258 stores, 256 threads)"))
    assert x[:, T * 128:].any() and x[:, far.offsets[1]:T * 128].any()          # (bits of the field in either pass of the store loop)
    assert sorted({f.kind for f in cases.encoder("linear + hashed + category + coordinate").fields}) == ["category", "coordinate", "coordinate-axis", "hashed", "linear"]
    two = cases.encoder("two coordinate fields with different seeds")
    x = two.encode(np.array([[5.0, 6.0, 4.0, 5.0, 6.0, 4.0]]))[0]
    assert two.fields[0].seed != two.fields[3].seed and not np.array_equal(x[:300], x[300:]) and x[:300].any() and x[300:].any()
    last = cases.encoder("sixteen entries ending in a coordinate group")
    assert len(last) == 16 and last.fields[13].kind == "coordinate" and last.fields[15].kind == "coordinate-axis"


def test_the_overlap_property():
    """The inputs of the table of DESIGN.md section 28: the mean overlap of a row with the row d cells away falls strictly over
    d = 1, r, 2r, 2r + 1, and at d = 2r + 1 it is below 2 (chance: width**2 / bits = 1.1)."""
    from bithtm_amd import CoordinateField, ScalarEncoder
    p = cases.OVERLAP
    enc = ScalarEncoder([CoordinateField(p["bits"], p["width"], 8, seed=p["seed"])])
    centres = p["centres"].astype(np.float64)
    design = open(os.path.join(ROOT, "DESIGN.md")).read()
    for r in (2, 4, 8):
        row = lambda d: enc.encode(np.concatenate([centres + [d, 0], np.full((len(centres), 1), float(r))], axis=1))
        base = row(0)
        mean = {d: float((base & row(d)).sum(axis=1).mean()) for d in (0, 1, 2, r, 2 * r, 2 * r + 1)}
        print(r, {d: round(m, 1) for d, m in mean.items()})
        assert mean[0] > mean[1] > mean[r] > mean[2 * r] > mean[2 * r + 1] and mean[2 * r + 1] < 2.0 and mean[0] > 20.0
        line = f"| {r} | " + " | ".join(f"{mean[d]:.1f}" for d in (0, 1, 2, r, 2 * r, 2 * r + 1)) + " |"
        assert line in design, line


def test_geo_values_against_hand_computed_numbers():
    from bithtm_amd import CoordinateField, ScalarEncoder, geo_values
    R = 6378137.0
    v = geo_values([0.0, 180.0, -122.229194, 10.0], [0.0, 0.0, 37.486782, -45.0], [0.0, 100.0, 5.0, 33.0], 30.0)
    assert v.shape == (4, 3) and v.dtype == np.float64
    assert v[0].tolist() == [0.0, R * math.log(math.tan(math.pi / 4)), 2.0] and abs(v[0, 1]) < 1e-9       # (the least radius of width 21: ceil((sqrt(21) - 1) / 2) = 2)
    assert abs(v[1, 0] - math.pi * R) < 1e-6 and abs(v[1, 0] - 20037508.342789244) < 1e-6 and v[1, 2] == 2.0      # (rint(100 / 30 / 2 * 1.5) = rint(2.5) = 2: to even)
    assert abs(v[2, 0] - R * math.radians(-122.229194)) < 1e-6 and abs(v[2, 1] - R * math.log(math.tan(math.pi / 4 + math.radians(37.486782) / 2))) < 1e-6
    assert abs(v[2, 0] + 13606491.63) < 0.01 and abs(v[2, 1] - 4507176.87) < 0.01
    assert abs(v[3, 1] + R * math.asinh(1.0)) < 1e-6 and v[3, 2] == 2.0                                   # (33 / 30 / 2 * 1.5 = 0.825 -> 1, below the least)
    assert geo_values(0.0, 0.0, 400.0, 30.0)[2] == 10.0 and geo_values(0.0, 0.0, 400.0, 30.0, timestep=2.0)[2] == 20.0
    assert geo_values(0.0, 0.0, 0.0, 30.0, width=1)[2] == 0.0 and geo_values(0.0, 0.0, 0.0, 30.0, width=50)[2] == 4.0
    n = geo_values([np.nan, 1.0, 1.0], [1.0, np.nan, 1.0], [1.0, 1.0, np.nan], 30.0)
    assert np.isnan(n[0, 0]) and np.isnan(n[1, 1]) and np.isnan(n[2, 2]) and np.isnan(n).sum() == 3
    assert geo_values(np.zeros((2, 5)), np.zeros((2, 5)), 1.0, 30.0).shape == (2, 5, 3)
    enc = ScalarEncoder([CoordinateField(400, 21, 20, resolution=30.0)])
    assert enc.bucket(n).tolist() == [[-1] * 3] * 3 and enc.encode(v).sum(axis=1).min() >= 15
    for kw in (dict(scale=0.0), dict(scale=30.0, timestep=0.0), dict(scale=30.0, width=0)):
        with pytest.raises(ValueError):
            geo_values(0.0, 0.0, 1.0, **kw)


def test_table_and_key():
    from bithtm_amd import CoordinateField, HashedField, ScalarEncoder, ScalarField
    mixed = lambda seed, radius=9: ScalarEncoder([ScalarField(0, 100, 130, 21), CoordinateField(96, 11, radius, resolution=(0.5, 4.0), origin=(3.0, -2.0), seed=seed),
                                                  HashedField(0, 24, 60, 5, buckets=300, seed=2)], 300)
    enc = mixed(5)
    assert len(enc) == 5 and enc.offsets == (0, 130, 130, 130, 226) and enc.bank_values(np.zeros((2, 5))).shape == (2, 5)
    with pytest.raises(ValueError):
        enc.bank_values(np.zeros((2, 3)))
    assert [(t.minimum, t.scale, t.offset, t.bits, t.width, t.buckets, t.periodic, t.reserved) for t in enc.table()] == \
        [(0.0, 1.1, 0, 130, 21, 110, 0, 0), (3.0, 2.0, 130, 96, 11, 9, 0, 3 | 5 << 2), (-2.0, 0.25, 130, 0, 0, 0, 0, 3), (0.0, 1.0, 130, 0, 0, 0, 0, 3),
         (0.0, 12.5, 226, 60, 5, 300, 0, 2 | 2 << 2)]
    assert mixed((1 << 29) - 1).table()[1].reserved == 0x7FFFFFFF
    assert enc.key() == mixed(5).key() and enc.key() != mixed(6).key() and enc.key() != mixed(5, 8).key() and len({mixed(s).key() for s in range(8)}) == 8
    assert enc.key()[2] == (3.0, 2.0, 96, 11, False, "coordinate", 9, 5) and enc.key()[3] == (-2.0, 0.25, 0, 0, False, "coordinate-axis", 0, 0)
    # check_model: no decode cap on a coordinate field (it is not decoded)
    ScalarEncoder([CoordinateField(9000, 64, 5)]).check_model(9000, column_dim=2048)
    with pytest.raises(ValueError, match="8192"):
        ScalarEncoder([ScalarField(0, 1, 9000, 64)]).check_model(9000, column_dim=2048)


def test_header_text():
    from bithtm_amd import _keyed, encoders
    header = open(HEADER).read()
    for line in ("#define HTM_FIELD_COORDINATE 3", "#define HTM_COORD_MAX_RADIUS 127", "#define HTM_HASHED_MAX_WIDTH 256", "#define HTM_SCALAR_MAX_FIELDS 16"):
        assert line in header, line
    assert re.search(r"#define BITHTM_ABI_VERSION\s+4\b", header)
    comment = header[header.index("Coordinate fields (DESIGN.md section 28)"):header.index("#define HTM_SCALAR_MAX_FIELDS")]
    for text in ("htm_stream_base(seed, 8, 0)", "htm_stream_base(seed, 8, 1)", "htm_draw24", "-2^30 <= t < 2^30", "to the lower index", "exactly two continuations",
                 "(-1, 0)", "3 | seed << 2", "max_radius"):
        assert text in comment, text
    rng = open(os.path.join(ROOT, "bithtm_amd", "csrc", "htm_rng.h")).read()
    assert "#define HTM_STREAM_COORDINATE 8u" in rng and _keyed.STREAM_COORDINATE == 8
    assert (encoders.FIELD_COORDINATE, encoders.COORD_MAX_RADIUS) == (3, 127)
    assert _keyed.draw32(6, 8, 1, np.array([-3, 5]), np.array([3, -7])).tolist() == [_draw32(6, 1, -3, 3), _draw32(6, 1, 5, -7)]


# ---- the compiler's report
def test_the_three_new_kernels_have_no_scratch_and_the_older_ones_keep_their_figures():
    from bithtm_amd.build import COORD_REPORTS, kernel_resources, whole_library_kernel_resources
    new, old, whole = kernel_resources("htm_coord.h"), kernel_resources(), whole_library_kernel_resources()
    if new is None or old is None:
        pytest.skip("the library in the tree was not built here")
    assert list(COORD_REPORTS) == ["htm_coord.h"]
    names = {re.match(r"_Z\d+(kcoord_[a-z]+)", k).group(1): v for k, v in new.items()}
    assert sorted(names) == ["kcoord_bank", "kcoord_finish", "kcoord_votes"] and len(new) == 3, sorted(new)
    for name, r in names.items():
        print(name, r)
        assert r["scratch_bytes_per_lane"] == 0 and r["lds_bytes"] <= 64 * 1024 and r["occupancy"] >= 1, (name, r)
    assert names["kcoord_finish"]["lds_bytes"] == names["kcoord_votes"]["lds_bytes"]
    assert names["kcoord_bank"]["lds_bytes"] >= 16 * 256 * 4 + 256 * 4
    assert not set(new) & set(whole)                # (the five older functions return what they returned)
    older = {re.match(r"_Z\d+(k[a-z]*_[a-z_0-9]+)", k).group(1) for k in whole if re.match(r"_Z\d+k[a-z]*_", k)}
    for name in names:                              # (the budget tests find kernels with re.search: no name inside another)
        assert not [s for s in older if s in name or name in s], name
    with open(os.path.join(ROOT, "tests", "golden", "kernel_resources_before_likelihood.json")) as f:
        before = json.load(f)
    changed = {k: (before[k], old.get(k)) for k in before if before[k] != old.get(k)}
    assert not changed, changed
    kenc = {k: v for k, v in old.items() if re.match(r"_Z\d+kenc_", k)}
    assert len(kenc) == 3


# ---- the launch traces and the refusals
@pytest.fixture(scope="module")
def traces(tmp_path_factory):
    from test_launch_trace_cpu import _build
    tmp = str(tmp_path_factory.mktemp("coordinate_trace"))
    env = dict(os.environ, BITHTM_LIBRARY=_build(tmp), BITHTM_STUB_TRACE=os.path.join(tmp, "trace.txt"))
    for name in ("LD_PRELOAD", "BITHTM_LEAN", "BITHTM_SCAN_LARGE"):
        env.pop(name, None)
    r = subprocess.run([sys.executable, os.path.join(ROOT, "tests", "host_stub", "coordinate_driver.py")], env=env, capture_output=True, text=True,
                       timeout=600)
    assert r.returncode == 0, (r.stdout + r.stderr)[-4000:]
    return json.loads(r.stdout.splitlines()[-1])


def _kernel(line):
    m = re.match(r"launch _Z(\d+)", line)
    return line[m.end():m.end() + int(m.group(1))] if m else None


def _shape(line):
    """A trace line without its kernel's name: grid, block and LDS of a launch, a copy or memset as it is.  The encode launch's block
    is left out: kcoord_bank's is 256 threads whatever the row's width (its select wants them), the others' follow the row."""
    m = re.match(r"launch \S+ (grid .*)$", line)
    if not m:
        return line
    return re.sub(r" block \d+", "", m.group(1)) if _kernel(line) in ("k_bank_encode", "kenc_bank", "kcoord_bank") else m.group(1)


OURS = {"k_bank_encode": "kcoord_bank", "k_decode_votes": "kcoord_votes", "klive_finish": "kcoord_finish"}
TWIN = {"k_bank_encode": "kenc_bank", "k_decode_votes": "kenc_votes", "klive_finish": "kenc_finish"}
CALLS = ("bank_encode", "decode_votes", "predicted_value", "recorded", "tick B=1", "tick B=3", "scored B=3")


@needs_hipcc
@pytest.mark.parametrize("call", CALLS)
def test_a_coordinate_table_launches_its_kernels_at_the_same_places(traces, call):
    linear, mixed, coord = (traces["trace"][f"{name} {call}"] for name in ("linear", "mixed", "coordinate"))
    if call == "recorded":
        # (how a step of the run selects its winners follows the model's history, not the table: the run's own launches are compared
        # by their graph replays, the table's launches and the copies line by line)
        assert [x for x in linear if x == "graph_launch"] == [x for x in coord if x == "graph_launch"] == ["graph_launch"] * 6
        ours = list(OURS) + list(OURS.values()) + list(TWIN.values())
        linear, mixed, coord = ([x for x in lines if not x.startswith("launch ") or _kernel(x) in ours] for lines in (linear, mixed, coord))
        assert len(linear) == 8
    assert [_shape(x) for x in linear] == [_shape(x) for x in coord] == [_shape(x) for x in mixed], (linear, coord)         # the same grids, copies and counts
    names = [_kernel(x) for x in linear]
    assert [_kernel(x) for x in coord] == [OURS.get(k, k) for k in names] and [_kernel(x) for x in mixed] == [TWIN.get(k, k) for k in names]
    assert not [k for k in names if k and k.startswith(("kenc_", "kcoord_"))]
    want = {"bank_encode": ["k_bank_encode"], "decode_votes": ["k_decode_votes"], "predicted_value": ["k_decode_votes"], "recorded": ["k_decode_votes"],
            "tick B=1": ["k_bank_encode", "klive_finish"], "tick B=3": ["k_bank_encode", "klive_finish"],
            "scored B=3": ["k_bank_encode", "klive_finish"]}[call]
    assert [k for k in names if k in OURS] == want, names
    encode = [x for x in coord if _kernel(x) == "kcoord_bank"]
    assert all(re.search(r" block 256 ", x) for x in encode) and len(encode) == (0 if "k_bank_encode" not in want else 1)
    if call.startswith("scored"):
        assert _kernel(linear[-2]) == _kernel(coord[-2]) == "klik_tick" and _kernel(coord[-3]) == "kcoord_finish"


@needs_hipcc
@pytest.mark.parametrize("name", ["linear", "mixed"])
def test_a_tick_behind_a_coordinate_one_launches_what_it_launched(traces, name):
    assert traces["after"][name] == traces["trace"][f"{name} tick B=3"]


@needs_hipcc
def test_every_refusal_of_the_group_layout_is_an_argument_error_and_enqueues_nothing(traces):
    codes = traces["codes"]
    assert len(codes) == 30 * 5 and set(codes.values()) == {-1}, {k: v for k, v in codes.items() if v != -1}
    for entry in ("htm_bank_encode", "htm_decode_votes", "htm_predicted_value", "htm_live_tick", "htm_likelihood_tick"):
        for what in ("a head at the end of the table", "a head with one continuation at the end", "a head with one continuation, then a linear field",
                     "a continuation first in the table", "a continuation behind a linear field", "a third continuation", "max_radius 128", "max_radius -1",
                     "width 0", "width 257", "a periodic head", "a seed on a continuation", "a width on a continuation", "buckets on a continuation",
                     "a continuation at another offset", "a head past the row", "a head over the field in front of it", "a linear field over the head behind it",
                     "a head with an infinite scale", "a head with a NaN minimum"):
            assert codes[f"{what}: {entry}"] == -1
    assert traces["refused"] == []
    assert len(traces["accepted"]) == 5 * 5 and set(traces["accepted"].values()) == {0}, {k: v for k, v in traces["accepted"].items() if v}


# ---- the host code under ASan + UBSan, as a stand-alone program, and the kernel header's arithmetic on the host
def _arithmetic_cases():
    from bithtm_amd import CoordinateField
    bits = lambda x: "%016x" % np.float64(x).view(np.uint64)
    rng = np.random.RandomState(5)
    lines, expect = [], []
    f = CoordinateField(300, 21, 20, resolution=(0.25, 3.0), origin=(100.5, -7.25), seed=8)
    plain = CoordinateField(300, 21, 127)
    special = [0.0, -0.0, -0.5, -1.0, 0.999999, -cases.TWO30, -cases.TWO30 - 1.0, np.nextafter(-cases.TWO30, -np.inf), cases.TWO30 - 1.0, cases.TWO30 - 0.5,
               np.nextafter(cases.TWO30, 0.0), cases.TWO30, np.nan, np.inf, -np.inf, 1e300, -1e300, 100.5, 100.49, -7.25, 0.1 + 0.2, 2.0 ** 31, -2.0 ** 31]
    for axis in (plain, plain.axes[0], f, f.axes[0]):
        for v in special + rng.uniform(-3e9, 3e9, 20).tolist() + rng.uniform(-50, 50, 20).tolist():
            field = axis if axis.kind == "coordinate" else axis.field
            column = 0 if axis.kind == "coordinate" else 1
            row = np.array([0.0, 0.0, 1.0])
            row[column] = v
            cx, cy, _, ok = field.cells(row)
            lines.append(f"c {bits(axis.minimum)} {bits(axis.scale)} {bits(v)}")
            expect.append(str(int((cx, cy)[column])) if ok else "missing")
    for max_radius in (0, 20, 127):
        g = CoordinateField(8, 3, max_radius)
        for v in [0.0, -0.0, -0.25, -1.0, 0.5, 1.0, 19.999, 20.0, 20.5, 127.0, 128.0, 1e300, np.inf, -np.inf, np.nan, -1e-300] + rng.uniform(-5, 150, 10).tolist():
            _, _, r, ok = g.cells(np.array([0.0, 0.0, v]))
            lines.append(f"r {bits(0.0)} {bits(1.0)} {max_radius} {bits(v)}")
            expect.append(str(int(r)) if ok else "-1")
    for seed, nbits in ((0, 1), (1, 400), (6, 37), ((1 << 29) - 1, 1 << 30)):
        g = CoordinateField(nbits, 1, 0, seed=seed)
        xs = [0, -1, 1, (1 << 30) - 1, -(1 << 30), (1 << 30) + 126, -(1 << 30) - 127] + rng.randint(-10 ** 6, 10 ** 6, 12).tolist()
        ys = [0, 5, -1, -(1 << 30), (1 << 30) - 1, -(1 << 30) - 127, (1 << 30) + 126] + rng.randint(-10 ** 6, 10 ** 6, 12).tolist()
        for x, y in zip(xs, ys):
            lines += [f"o {seed} {x} {y}", f"b {seed} {nbits} {x} {y}"]
            expect += [str(int(g.order(x, y))), str(int(g.bit(x, y)))]
    for cx, cy, r, (low, high), order in cases.TIES:
        lines.append(f"o {cases.TIE_SEED} {cx - r + low % (2 * r + 1)} {cy - r + low // (2 * r + 1)}")
        expect.append(str(order))
    selects = [(cases.TIE_SEED, cases.TIE_WIDTH, cx, cy, r) for cx, cy, r, _, _ in cases.TIES]
    selects += [(2, 25, 0, 0, 0), (2, 25, -3, 7, 2), (4, 24, 1000, -500, 2), (2, 25, -70001, -90001, 7), (2, 25, 5, 5, 8), (9, 41, 0, 0, 127), (2, 256, 1, 2, 8),
                (1, 1, 3, 4, 12), (5, 21, (1 << 30) - 1, -(1 << 30), 3)]
    for seed, width, cx, cy, r in selects:
        g = CoordinateField(64, width, 127, seed=seed)
        lines.append(f"s {seed} {width} {cx} {cy} {r}")
        expect.append(" ".join(str(i) for i in sorted(g.selected(cx, cy, r).tolist())))
    return lines, expect


@needs_hipcc
def test_the_host_code_runs_clean_under_asan_and_ubsan_and_the_header_arithmetic_equals_the_definition(tmp_path):
    """tests/host_stub/coordinate_host.cpp and htm_engine.hip (host-only), both with -fsanitize=address,undefined, linked against the
    stub runtime into ONE program that is run directly: nothing is preloaded."""
    from test_likelihood_cpu import _host_objects
    tmp = str(tmp_path)
    san = ["-fsanitize=address,undefined", "-fno-sanitize-recover=undefined"]
    obj, stub, defsym = _host_objects(tmp, san)
    clang = os.path.join(CLANG_DIR, "bin", "clang++")
    exe = os.path.join(tmp, "coordinate_host")
    subprocess.run([clang, "-std=c++17", "-O1", "-g", "-fno-omit-frame-pointer", "-ffp-contract=off"] + san +
                   [os.path.join(ROOT, "tests", "host_stub", "coordinate_host.cpp"), obj, stub, "-ldl", "-o", exe] + defsym, check=True, capture_output=True)
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
    wrong = [(line, g, e) for line, g, e in zip(lines, got, expect) if g != e]
    assert not wrong, wrong[:5]
