"""Field kinds on the CPU (CategoryField, HashedField, date_fields; bithtm_amd/encoders.py is the definition):
hand-computed encodes and decodes, the collision property of hashed fields with the figures DESIGN.md quotes, the table and the
key, the header's text, every case of tests/field_kind_cases.py on the path it names, every refusal of the C ABI and the launch
traces of linear and mixed tables (the host code built host-only against tests/host_stub/hip_stub_runtime.cpp), the compiler's
report for the three new kernels, and the host code under ASan + UBSan as a stand-alone program
(tests/host_stub/field_kinds_host.cpp), which also evaluates the kernel header's arithmetic on the host against the definition."""
import json
import os
import re
import subprocess
import sys

import numpy as np
import pytest

import field_kind_cases as cases

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CLANG_DIR = "/opt/rocm/lib/llvm"
HEADER = os.path.join(ROOT, "include", "bithtm_hip.h")
needs_hipcc = pytest.mark.skipif(not os.path.exists("/opt/rocm/bin/hipcc"), reason="needs hipcc")


def _pos(seed, bits, i):
    """pos(i) worked out in Python integers, not through bithtm_amd._keyed: lowbias32 as htm_rng.h has it."""
    def mix(x):
        x ^= x >> 16
        x = x * 0x7FEB352D & 0xFFFFFFFF
        x ^= x >> 15
        x = x * 0x846CA68B & 0xFFFFFFFF
        return x ^ x >> 16
    base = mix(mix((seed + 7 * 0x9E3779B9) & 0xFFFFFFFF) ^ 0)
    return mix(mix(base ^ i) ^ 0) * bits >> 32


# ---- the definition
def test_category_field_by_hand():
    from bithtm_amd import CategoryField, ScalarEncoder, ScalarField
    c = CategoryField(3, 4, 14)
    assert (c.kind, c.buckets, c.bits, c.width, c.minimum, c.scale, c.periodic) == ("category", 3, 14, 4, 0.0, 1.0, False)
    assert CategoryField(5, 3).bits == 15 and isinstance(c, ScalarField)
    # an unknown id is missing, not clamped; 2.7 is category 2; -0.0 is category 0
    values = [0.0, 1.0, 2.0, -1.0, 3.0, 2.7, -0.0, np.nan, np.inf, -np.inf, -1e-300, 2.9999999, 1e300]
    assert c.bucket(values).tolist() == [0, 1, 2, -1, -1, 2, 0, -1, -1, -1, -1, 2, -1] and c.bucket(values).dtype == np.int32
    assert c.value_of([0, 2]).tolist() == [0.0, 2.0] and np.isnan(c.value_of(-1))
    enc = ScalarEncoder([ScalarField(0, 1, 5, 2), c], 20)
    x = enc.encode([[0.0, 1.0], [np.nan, 2.7], [1.0, 3.0], [0.5, -0.0]])
    assert [np.flatnonzero(r).tolist() for r in x] == [[0, 1, 9, 10, 11, 12], [13, 14, 15, 16], [3, 4], [2, 3, 5, 6, 7, 8]]
    votes = np.zeros((4, 20), np.int64)
    votes[0, [5, 9, 10]] = 3, 2, 2                  # category 0 has 3, category 1 has 4
    votes[1, [6, 13]] = 2, 2                        # a tie between 0 and 2: the lowest
    votes[2, [17, 18, 19]] = 9                      # only the category's unused bits and the row's
    votes[3, 13:17] = 7                             # the last category, all four bits
    bucket, score = enc.decode(votes)
    assert bucket[:, 1].tolist() == [1, 0, -1, 2] and score[:, 1].tolist() == [4, 2, 0, 28]
    for args in ((0, 4), (3, 0), (3, 4, 11)):
        with pytest.raises(ValueError):
            CategoryField(*args)


def test_hashed_field_by_hand():
    from bithtm_amd import HashedField, ScalarEncoder, ScalarField
    f = HashedField(10.0, 20.0, 37, 5, buckets=60, seed=1)
    assert (f.kind, f.buckets, f.bits, f.width, f.periodic, f.seed) == ("hashed", 60, 37, 5, False, 1) and f.scale == 6.0 and isinstance(f, ScalarField)
    assert HashedField(0, 10, 64, 5, resolution=0.3).buckets == 34 and HashedField(0, 10, 64, 5, resolution=2.5).buckets == 4
    # the bucket is a non-periodic linear field's: clamped, NaN missing
    assert f.bucket([10.0, 20.0, 15.0, 9.0, 1e300, -np.inf, np.inf, np.nan, 19.99, 10.17]).tolist() == [0, 59, 30, 0, 59, 0, 59, -1, 59, 1]
    assert f.value_of([0, 59]).tolist() == [10.0 + 0.5 / 6.0, 10.0 + 59.5 / 6.0] and np.isnan(f.value_of(-1))
    pos = [_pos(1, 37, i) for i in range(64)]
    assert f.positions().tolist() == pos and len(pos) == 60 + 5 - 1 and min(pos) >= 0 and max(pos) < 37
    enc = ScalarEncoder([ScalarField(0, 1, 11, 2), f], 50)
    x = enc.encode([[np.nan, 15.0], [np.nan, np.nan], [np.nan, 20.0]])
    assert np.flatnonzero(x[0]).tolist() == sorted({11 + p for p in pos[30:35]}) and not x[1].any()
    assert np.flatnonzero(x[2]).tolist() == sorted({11 + p for p in pos[59:64]})
    # decode: G[i] = votes[pos(i)], a window sums five G's -- a collided position counted once per j
    votes = np.arange(50, dtype=np.int64) * 3 % 17
    G = [int(votes[11 + p]) for p in pos]
    score = [sum(G[b:b + 5]) for b in range(60)]
    bucket, top = enc.decode(votes)
    assert top[1] == max(score) and bucket[1] == score.index(max(score))
    b, p = cases.double_hit(f)
    hot = np.zeros(50, np.int64)
    hot[11 + p] = 1
    bucket, top = enc.decode(hot)
    assert pos[b:b + 5].count(p) == 2 and top[1] == 2 and bucket[1] <= b and bucket[0] == -1
    # bits 1: every position is 0; width above bits is fine
    one = HashedField(0, 1, 1, 3, buckets=10, seed=3)
    assert not one.positions().any() and ScalarEncoder([one]).encode([[0.4]]).tolist() == [[True]]
    assert ScalarEncoder([one]).decode(np.array([4]))[1].tolist() == [12]
    for kw in (dict(width=0, buckets=5), dict(width=257, buckets=5), dict(width=3), dict(width=3, buckets=5, resolution=0.1), dict(width=3, buckets=0),
               dict(width=3, buckets=5, seed=-1), dict(width=3, buckets=5, seed=1 << 29), dict(width=3, resolution=0.0), dict(width=3, buckets=5, bits=0)):
        with pytest.raises(ValueError):
            HashedField(0, 1, **dict(dict(bits=8), **kw))
    with pytest.raises(ValueError):
        HashedField(1, 1, 8, 3, buckets=5)
    assert HashedField(0, 1, 8, 256, buckets=5, seed=(1 << 29) - 1).positions().shape == (260,)


def test_the_collision_property_of_hashed_fields():
    """decode(encode(b)) = b' with score `width`, b' <= b, and the set of b' a subset of the buckets; the worst b - b' and the number
    of buckets with b' != b per parameter set are what DESIGN.md section 23 quotes (tests/field_kind_cases.py CENSUS)."""
    from bithtm_amd import HashedField, ScalarEncoder
    design = open(os.path.join(ROOT, "DESIGN.md")).read()
    for (seed, bits, width, buckets), (worst, off) in cases.CENSUS.items():
        f = HashedField(0, 1, bits, width, buckets=buckets, seed=seed)
        enc = ScalarEncoder([f])
        b = np.arange(buckets)
        v = f.value_of(b)[:, None]
        assert np.array_equal(enc.bucket(v)[:, 0], b)
        back, score = enc.decode(enc.encode(v).astype(np.int32))
        back, score = back[:, 0], score[:, 0]
        assert (score == width).all() and (back <= b).all() and (back >= 0).all() and set(back.tolist()) <= set(b.tolist())
        print(f"(seed {seed}, bits {bits}, width {width}, buckets {buckets}): worst b - b' = {(b - back).max()}, buckets off {(back != b).sum()}"
              f" ({100.0 * (back != b).mean():.1f} %)")
        assert ((b - back).max(), (back != b).sum()) == (worst, off)
        assert worst <= 3
        assert f"| ({seed}, {bits}, {width}, {buckets}) | {worst} | {off} |" in design, (seed, bits, width, buckets)


def test_table_and_key():
    from bithtm_amd import CategoryField, HashedField, ScalarEncoder, ScalarField
    linear = ScalarEncoder([ScalarField(0, 100, 130, 21), ScalarField(0, 24, 96, 11, periodic=True), ScalarField(-5, 5, 70, 1)], 300)
    # a table of linear fields: what it was
    assert [(t.minimum, t.scale, t.offset, t.bits, t.width, t.buckets, t.periodic, t.reserved) for t in linear.table()] == \
        [(0.0, 1.1, 0, 130, 21, 110, 0, 0), (0.0, 4.0, 130, 96, 11, 96, 1, 0), (-5.0, 7.0, 226, 70, 1, 70, 0, 0)]
    assert linear.key() == (300, (0.0, 1.1, 130, 21, False), (0.0, 4.0, 96, 11, True), (-5.0, 7.0, 70, 1, False))
    mixed = lambda seed: ScalarEncoder([ScalarField(0, 100, 130, 21), HashedField(0, 24, 96, 11, buckets=300, seed=seed), CategoryField(4, 9, 40)], 300)
    tab = mixed(5).table()
    assert [(t.minimum, t.scale, t.offset, t.bits, t.width, t.buckets, t.periodic, t.reserved) for t in tab] == \
        [(0.0, 1.1, 0, 130, 21, 110, 0, 0), (0.0, 12.5, 130, 96, 11, 300, 0, 2 | 5 << 2), (0.0, 1.0, 226, 40, 9, 4, 0, 1)]
    assert mixed((1 << 29) - 1).table()[1].reserved == 0x7FFFFFFE
    assert mixed(5).key() == mixed(5).key() and mixed(5).key() != mixed(6).key() and len({mixed(s).key() for s in range(8)}) == 8
    assert mixed(5).key()[2] == (0.0, 12.5, 96, 11, False, "hashed", 300, 5) and mixed(5).key()[3] == (0.0, 1.0, 40, 9, False, "category", 4, 0)
    # the same bits, width and range, other buckets; a category against a linear field of its numbers
    assert ScalarEncoder([HashedField(0, 1, 96, 11, buckets=86)]).key() != ScalarEncoder([ScalarField(0, 1, 96, 11)]).key()
    # check_model: the decode cap of a hashed field is on its positions
    ScalarEncoder([HashedField(0, 1, 9000, 64, buckets=8129)]).check_model(9000, column_dim=2048)
    with pytest.raises(ValueError, match="8192"):
        ScalarEncoder([HashedField(0, 1, 9000, 64, buckets=8130)]).check_model(9000, column_dim=2048)
    ScalarEncoder([HashedField(0, 1, 9000, 64, buckets=8130)]).check_model(9000)
    with pytest.raises(ValueError, match="8192"):
        ScalarEncoder([CategoryField(2, 5, 8193)]).check_model(8193, column_dim=64)


def test_date_fields_and_values():
    from bithtm_amd import ScalarEncoder, date_fields, date_values
    fields = date_fields(time_of_day=(48, 5), day_of_week=(21, 3), weekend=4)
    assert [(f.kind, f.bits, f.width, f.periodic, f.minimum, f.maximum) for f in fields] == \
        [("linear", 48, 5, True, 0.0, 24.0), ("linear", 21, 3, True, 0.0, 7.0), ("category", 8, 4, False, 0.0, 2.0)]
    assert [f.kind for f in date_fields(time_of_day=None)] == ["linear", "category"] and len(date_fields(None, None, 3)) == 1
    times = np.array(["1970-01-01T00:00", "2024-02-29T18:30", "2024-03-02T06:00", "2024-03-03T23:59:59", "2024-03-04T00:00", "NaT", "1969-12-28T12:00"],
                     dtype="datetime64[s]")
    v = date_values(times)
    assert v.shape == (7, 3) and v.dtype == np.float64
    assert v[0].tolist() == [0.0, 3.0, 0.0] and v[1].tolist() == [18.5, 3.0 + 18.5 / 24.0, 0.0] and v[2].tolist() == [6.0, 5.25, 1.0]
    assert v[3, 2] == 1.0 and 6.99 < v[3, 1] < 7.0 and v[4].tolist() == [0.0, 0.0, 0.0] and np.isnan(v[5]).all() and v[6].tolist() == [12.0, 6.5, 1.0]
    assert date_values(times, day_of_week=False).shape == (7, 2) and date_values(times.reshape(7, 1)).shape == (7, 1, 3)
    enc = ScalarEncoder(date_fields(time_of_day=(48, 5), day_of_week=(21, 3), weekend=4))
    x = enc.encode(v)
    assert x.shape == (7, 77) and x[2, 69 + 4:].all() and not x[2, 69:73].any() and not x[5].any() and x[:5].sum(axis=1).tolist() == [12] * 5


def test_header_text():
    from bithtm_amd import _keyed, encoders
    header = open(HEADER).read()
    for line in ("#define HTM_HASHED_MAX_WIDTH 256", "#define HTM_FIELD_CATEGORY 1", "#define HTM_FIELD_HASHED 2", "#define HTM_DECODE_MAX_BITS 8192"):
        assert line in header, line
    assert re.search(r"#define BITHTM_ABI_VERSION\s+4\b", header)
    assert re.search(r"int32_t offset, bits, width, buckets, periodic, reserved;", header)
    comment = header[header.index("Field kinds (DESIGN.md section 23)"):header.index("#define HTM_SCALAR_MAX_FIELDS")]
    for text in ("reserved == 0", "reserved & 3", "reserved >> 2", "NOT clamped", "htm_stream_base(seed, 7, 0)", "kind 3"):
        assert text in comment, text
    rng = open(os.path.join(ROOT, "bithtm_amd", "csrc", "htm_rng.h")).read()
    assert "#define HTM_STREAM_FIELD_HASH 7u" in rng and _keyed.STREAM_FIELD_HASH == 7
    assert (encoders.HASHED_MAX_WIDTH, encoders.FIELD_CATEGORY, encoders.FIELD_HASHED) == (256, 1, 2)
    assert _keyed.draw32(1, 7, 0, np.arange(5)).tolist() == [(_pos(1, 1 << 32, i)) for i in range(5)]


def test_every_case_reaches_the_path_it_names():
    from bithtm_amd.engine import pack_bits  # noqa: F401  (the package imports)
    threads = lambda W: min(256, ((W >> 2) + 63) // 64 * 64)
    words = lambda I: (I + 31) // 32 + 3 & ~3
    assert (threads(words(300)), threads(words(8200)), threads(words(33000))) == (64, 128, 256) and words(33000) // 4 == 258 > 256
    for name, (input_dim, specs, what) in cases.CASES.items():
        enc = cases.encoder(name)
        assert enc.input_dim == input_dim and what
        kinds = [f.kind for f in enc.fields]
        assert "hashed" in kinds and ("category" in kinds or "linear" in kinds)
        assert enc.offsets[-1] + enc.fields[-1].bits < input_dim        # (unused trailing bits)
        v = cases.values(enc, 6, 1)
        b = enc.bucket(v)
        for j, f in enumerate(enc.fields):
            assert (b[:, j] == -1).any() and (b[:, j] == f.buckets - 1).any() and (b[:, j] == 0).any(), (name, j)
            if f.kind == "category":
                assert b[:4, j].tolist() == [0, -1, -1, 2 if f.buckets > 2 else -1] and b[4, j] == 0        # ids 0, -1, categories, 2.7, -0.0
        if name in cases.DECODED:
            enc.check_model(input_dim, column_dim=2048)
            votes = cases.vote_rows(enc, 2048, 3)
            bucket, score = enc.decode(votes)
            assert (bucket[0] == -1).all() and (bucket[8] == -1).all() and not score[0].any()
            assert (bucket[1] >= 0).all() and score[4].max() == 2048 * max(f.width for f in enc.fields)
            for j, f in enumerate(enc.fields):
                if f.kind == "hashed" and cases.double_hit(f):
                    assert score[6, j] >= 2, (name, j)                  # (one vote, counted once per hit)
                if f.kind != "hashed":                                  # (two disjoint windows of 5 votes a bit: a tie, the lowest)
                    assert (bucket[5, j], score[5, j]) == (f.buckets // 5, 5 * f.width) or f.buckets < 3, (name, j)
    enc = cases.encoder("mixed-300")
    assert enc.offsets == (0, 61, 158, 172, 222) and enc.fields[2].bits % enc.fields[2].width
    assert cases.double_hit(enc.fields[4]) is not None and (1, 37, 5, 60) in cases.CENSUS
    big = cases.encoder("mixed-8200")
    assert big.fields[4].width == 256 and big.fields[5].width == 1 and big.fields[1].buckets == 1000 and big.fields[1].bits == 400
    cap = cases.encoder("cap-8200")
    assert cap.fields[0].decode_elements() == 8192 and cap.fields[1].buckets == 1 and cap.fields[2].bits == 1 and cap.fields[3].buckets == 1
    assert not cap.fields[2].positions().any()
    far = cases.encoder("mixed-33000")
    last = far.offsets[-1]
    assert last < 32768 < last + far.fields[-1].bits
    x = far.encode(cases.values(far, 40, 2))
    assert x[:, 32768:].any() and x[:, :32768].any()                    # (bits for the second pass of the store loop)
    with pytest.raises(ValueError):
        far.check_model(33000, column_dim=2048)


# ---- the compiler's report
def test_the_three_new_kernels_have_no_scratch_and_the_older_ones_keep_their_figures():
    from bithtm_amd.build import kernel_resources
    res = kernel_resources()
    if res is None:
        pytest.skip("the library in the tree was not built here")
    new = {re.match(r"_Z\d+(kenc_[a-z]+)", k).group(1): v for k, v in res.items() if re.match(r"_Z\d+kenc_", k)}
    assert sorted(new) == ["kenc_bank", "kenc_finish", "kenc_votes"], sorted(new)
    for name, r in new.items():
        print(name, r)
        assert r["scratch_bytes_per_lane"] == 0 and r["lds_bytes"] <= 64 * 1024 and r["occupancy"] >= 1, (name, r)
    assert new["kenc_finish"]["lds_bytes"] == new["kenc_votes"]["lds_bytes"]
    assert new["kenc_bank"]["lds_bytes"] >= 16 * 256 * 4
    old = {re.match(r"_Z\d+(k[a-z]*_[a-z_0-9]+)", k).group(1) for k in res if not re.match(r"_Z\d+kenc_", k) and re.match(r"_Z\d+k[a-z]*_", k)}
    for name in new:                                # (the budget tests find kernels with re.search: no name inside another)
        assert not [s for s in old if s in name], name
        assert not any(s in name for s in ("k_bank_encode", "k_decode_votes", "klive_"))
    with open(os.path.join(ROOT, "tests", "golden", "kernel_resources_before_likelihood.json")) as f:
        before = json.load(f)
    changed = {k: (before[k], res.get(k)) for k in before if before[k] != res.get(k)}
    assert not changed, changed


# ---- the launch traces and the refusals
@pytest.fixture(scope="module")
def traces(tmp_path_factory):
    from test_launch_trace_cpu import _build
    tmp = str(tmp_path_factory.mktemp("field_kinds_trace"))
    env = dict(os.environ, BITHTM_LIBRARY=_build(tmp), BITHTM_STUB_TRACE=os.path.join(tmp, "trace.txt"))
    for name in ("LD_PRELOAD", "BITHTM_LEAN", "BITHTM_SCAN_LARGE"):
        env.pop(name, None)
    r = subprocess.run([sys.executable, os.path.join(ROOT, "tests", "host_stub", "field_kinds_driver.py")], env=env, capture_output=True, text=True,
                       timeout=600)
    assert r.returncode == 0, (r.stdout + r.stderr)[-4000:]
    return json.loads(r.stdout.splitlines()[-1])


def _kernel(line):
    m = re.match(r"launch _Z(\d+)", line)
    return line[m.end():m.end() + int(m.group(1))] if m else None


def _shape(line):
    """A trace line without its kernel's name: grid, block and LDS of a launch, a copy or memset as it is."""
    m = re.match(r"launch \S+ (grid .*)$", line)
    return m.group(1) if m else line


TWIN = {"k_bank_encode": "kenc_bank", "k_decode_votes": "kenc_votes", "klive_finish": "kenc_finish"}
CALLS = ("bank_encode", "decode_votes", "predicted_value", "recorded", "tick B=1", "tick B=3", "scored B=3")


@needs_hipcc
@pytest.mark.parametrize("call", CALLS)
def test_a_mixed_table_launches_the_twins_at_the_same_places(traces, call):
    linear, mixed = traces["trace"][f"linear {call}"], traces["trace"][f"mixed {call}"]
    if call == "recorded":
        # (how a step of the run selects its winners -- in one launch or in digit passes -- follows the model's history, not the
        # table: the run's own launches are compared by their graph replays, the table's launches and the copies line by line)
        assert [x for x in linear if x == "graph_launch"] == [x for x in mixed if x == "graph_launch"] == ["graph_launch"] * 6
        linear, mixed = ([x for x in lines if not x.startswith("launch ") or _kernel(x) in list(TWIN) + list(TWIN.values())] for lines in (linear, mixed))
        assert len(linear) == 8
    assert [_shape(x) for x in linear] == [_shape(x) for x in mixed], (linear, mixed)         # the same grids, copies and counts
    names, twins = [_kernel(x) for x in linear], [_kernel(x) for x in mixed]
    assert twins == [TWIN.get(k, k) for k in names], (names, twins)
    assert not [k for k in names if k and k.startswith("kenc_")]
    want = {"bank_encode": ["k_bank_encode"], "decode_votes": ["k_decode_votes"], "predicted_value": ["k_decode_votes"], "recorded": ["k_decode_votes"],
            "tick B=1": ["k_bank_encode", "klive_finish"], "tick B=3": ["k_bank_encode", "klive_finish"],
            "scored B=3": ["k_bank_encode", "klive_finish"]}[call]
    assert [k for k in names if k in TWIN] == want, names
    if call.startswith("scored"):
        assert _kernel(linear[-2]) == _kernel(mixed[-2]) == "klik_tick" and _kernel(mixed[-3]) == "kenc_finish"


@needs_hipcc
def test_a_linear_tick_behind_a_mixed_one_launches_the_linear_kernels(traces):
    assert [_kernel(x) for x in traces["after"]] == [_kernel(x) for x in traces["trace"]["linear tick B=3"]]
    assert [_shape(x) for x in traces["after"]] == [_shape(x) for x in traces["trace"]["linear tick B=3"]]


@needs_hipcc
def test_every_refusal_of_the_kinds_is_an_argument_error_and_enqueues_nothing(traces):
    codes = traces["codes"]
    assert len(codes) == 18 * 5 and set(codes.values()) == {-1}, {k: v for k, v in codes.items() if v != -1}
    for entry in ("htm_bank_encode", "htm_decode_votes", "htm_predicted_value", "htm_live_tick", "htm_likelihood_tick"):
        for what in ("reserved < 0", "kind 3", "a seed on a linear field", "a seed on a category", "a periodic category", "a periodic hashed field",
                     "a category without buckets", "a category wider than its bits", "a hashed field without buckets", "a hashed field of width 257"):
            assert codes[f"{what}: {entry}"] == -1
    assert traces["refused"] == []
    # one position above the decode cap: the decoding call's refusal alone; exactly at it both go through
    assert traces["cap"] == [0, -1, 0, 0]


# ---- the host code under ASan + UBSan, as a stand-alone program, and the kernel header's arithmetic on the host
def _arithmetic_cases():
    from bithtm_amd import CategoryField, HashedField, ScalarField
    bits = lambda x: "%016x" % np.float64(x).view(np.uint64)
    rng = np.random.RandomState(5)
    lines, expect = [], []
    for seed, nbits, count in [(0, 1, 4), (1, 37, 64), (1, 400, 1020), (5, 130, 320), ((1 << 29) - 1, 8, 92), (3, 1, 12), (7, 1 << 30, 50), (2, 5000, 8192)]:
        pos = HashedField(0, 1, nbits, 1, buckets=count, seed=seed).positions()
        for i in list(range(min(count, 40))) + rng.randint(0, count, 20).tolist() + [count - 1]:
            lines.append(f"p {seed} {nbits} {i}")
            expect.append(str(int(pos[i])))
    fields = [(HashedField(10.0, 20.0, 37, 5, buckets=60, seed=1), 2 | 1 << 2), (HashedField(-1.0, 1.0, 8, 3, buckets=1, seed=0), 2),
              (HashedField(0.0, 0.3, 400, 21, resolution=0.0003), 2), (CategoryField(3, 4), 1), (CategoryField(1, 2), 1), (CategoryField(1000, 1), 1),
              (ScalarField(0, 100, 130, 21), 0), (ScalarField(0, 24, 96, 11, periodic=True), 0)]
    for f, reserved in fields:
        lo, hi = f.minimum, f.maximum
        special = [lo, hi, np.nextafter(lo, -np.inf), np.nextafter(hi, np.inf), np.nextafter(hi, lo), np.nan, np.inf, -np.inf, 1e300, -1e300, -0.0, 0.0,
                   -1.0, 2.7, float(f.buckets), f.buckets - 1.0, -1e-300, 2.0 ** 31, -2.0 ** 31 - 1]
        for v in special + rng.uniform(lo - 0.3 * (hi - lo), hi + 0.3 * (hi - lo), 30).tolist():
            lines.append(f"b {reserved} {f.buckets} {int(f.periodic)} {bits(f.minimum)} {bits(f.scale)} {bits(v)}")
            expect.append(str(int(f.bucket(v))))
    return lines, expect


@needs_hipcc
def test_the_host_code_runs_clean_under_asan_and_ubsan_and_the_header_arithmetic_equals_the_definition(tmp_path):
    """tests/host_stub/field_kinds_host.cpp and htm_engine.hip (host-only), both with -fsanitize=address,undefined, linked against the
    stub runtime into ONE program that is run directly: nothing is preloaded."""
    from test_likelihood_cpu import _host_objects
    tmp = str(tmp_path)
    san = ["-fsanitize=address,undefined", "-fno-sanitize-recover=undefined"]
    obj, stub, defsym = _host_objects(tmp, san)
    clang = os.path.join(CLANG_DIR, "bin", "clang++")
    exe = os.path.join(tmp, "field_kinds_host")
    subprocess.run([clang, "-std=c++17", "-O1", "-g", "-fno-omit-frame-pointer", "-ffp-contract=off"] + san +
                   [os.path.join(ROOT, "tests", "host_stub", "field_kinds_host.cpp"), obj, stub, "-ldl", "-o", exe] + defsym, check=True, capture_output=True)
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
    assert len(got) == len(expect) > 700
    wrong = [(line, g, e) for line, g, e in zip(lines, got, expect) if g != e]
    assert not wrong, wrong[:5]
