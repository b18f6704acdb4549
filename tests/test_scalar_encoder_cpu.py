"""Scalar streams on the CPU (bithtm_amd/encoders.py, the NumPy definition of htm_bank_encode / htm_decode_votes; DESIGN.md
section 20): the definition on a table of special values per field kind, the shape of an encoded row, decode(encode(v)) ==
bucket(v), ties and empty votes, the constructors' refusals, the C ABI's declarations, and the build's resource report."""

import os
import re

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _layout_a():
    """Three fields at the unaligned offsets 0, 130 and 226 of a 300-bit row, four trailing bits."""
    from bithtm_amd import ScalarEncoder, ScalarField
    return ScalarEncoder([ScalarField(0, 100, 130, 21), ScalarField(0, 24, 96, 11, periodic=True), ScalarField(-5, 5, 70, 1)], 300)


def test_bucket_of_special_values_non_periodic():
    """buckets = 130 - 21 + 1 = 110 over [0, 100]: scale 1.1 per unit."""
    from bithtm_amd import ScalarField
    f = ScalarField(0, 100, 130, 21)
    assert f.buckets == 110 and f.scale == 110.0 / 100.0
    below = np.nextafter(0.0, -1.0)
    values = [50.0, 0.0, 100.0, below, -3.0, np.nan, np.inf, -np.inf, 1e300, -1e300, 99.999999, 0.91]
    want = [55, 0, 109, 0, 0, -1, 109, 0, 109, 0, 109, 1]
    assert f.bucket(values).tolist() == want
    assert f.bucket(values).dtype == np.int32
    assert f.bucket(7.5).shape == ()                                # (any shape, a scalar too)


def test_bucket_of_special_values_periodic():
    """buckets = bits = 96 over a period of 24: four buckets per unit; the value wraps, a value out of int32 reach is missing."""
    from bithtm_amd import ScalarField
    f = ScalarField(0, 24, 96, 11, periodic=True)
    assert f.buckets == 96 and f.scale == 4.0
    values = [12.0, 0.0, 24.0, -1e-300, np.nextafter(0.0, -1.0), -0.25, np.nan, np.inf, -np.inf, 1e300, 24.0 + 5 * 24.0, 24.0 - 7 * 24.0,
              23.99, 2.0 ** 29 - 0.25, 2.0 ** 29, -2.0 ** 29, -2.0 ** 29 - 0.25]
    want = [48, 0, 0, 95, 95, 95, -1, -1, -1, -1, 0, 0,
            95, (2 ** 31 - 1) % 96, -1, (-2 ** 31) % 96, -1]
    assert f.bucket(values).tolist() == want


def test_width_one_and_full_width_fields():
    from bithtm_amd import ScalarEncoder, ScalarField
    one, full = ScalarField(-5, 5, 70, 1), ScalarField(0, 1, 40, 40)
    assert one.buckets == 70 and full.buckets == 1
    assert one.bucket([-5, 5, 0, -5.0001, 4.9999]).tolist() == [0, 69, 35, 0, 69]
    assert full.bucket([0, 1, 0.5, -7, 7, np.nan]).tolist() == [0, 0, 0, 0, 0, -1]
    enc = ScalarEncoder([one, full])
    assert enc.input_dim == 110 and enc.offsets == (0, 70)
    x = enc.encode([[5, 0.3], [np.nan, np.nan]])
    assert x[0, 69] and x[0, :69].sum() == 0 and x[0, 70:].all() and not x[1].any()


def test_encoded_rows_have_width_bits_per_field_or_none():
    enc = _layout_a()
    values = np.array([[50, 12, 0], [0, 0, -5], [100, 24, 5], [-1e-9, -1e-300, -5.0001], [np.nan, 3, np.nan], [np.inf, np.inf, -np.inf],
                       [1e300, 1e300, 1e300], [3, 24 + 24 * 5, 2]])
    x = enc.encode(values)
    assert x.shape == (8, 300) and x.dtype == np.bool_
    b = enc.bucket(values)
    for j, (f, off) in enumerate(zip(enc.fields, enc.offsets)):
        count = x[:, off:off + f.bits].sum(axis=1)
        assert np.array_equal(count, np.where(b[:, j] >= 0, f.width, 0)), j
    assert not x[:, 296:].any()                                     # (trailing bits clear)
    # a non-periodic window is one run starting at its bucket; a periodic wrap sets both ends of the field
    assert np.flatnonzero(x[0, :130]).tolist() == list(range(55, 76))
    wrapped = x[3, 130:226]                                         # (bucket 95 of 96, width 11: bit 95 and bits 0..9)
    assert b[3, 1] == 95 and wrapped[95] and wrapped[:10].all() and wrapped.sum() == 11 and not wrapped[10:95].any()
    assert enc.encode(values[0]).shape == (300,) and enc.encode(values.reshape(2, 4, 3)).shape == (2, 4, 300)


def test_decode_of_encode_is_the_bucket():
    """A few hundred random rows over and beyond every field's range, and the special values: decode(encode(v)) == bucket(v),
    the score the field's width (0 for a missing value)."""
    enc = _layout_a()
    rng = np.random.RandomState(0)
    v = np.stack([rng.uniform(-10, 110, 400), rng.uniform(-50, 50, 400), rng.uniform(-6, 6, 400)], axis=1)
    v[::17, 0], v[::19, 1], v[::23, 2] = np.nan, np.inf, np.nan
    v[5], v[6] = [100.0, 24.0, 5.0], [0.0, -1e-300, -5.0]
    bucket, score = enc.decode(enc.encode(v).astype(np.int32))
    want = enc.bucket(v)
    assert np.array_equal(bucket, want) and bucket.dtype == np.int32 and score.dtype == np.int32
    assert np.array_equal(score, np.where(want >= 0, [f.width for f in enc.fields], 0))
    assert (want == -1).any() and (want[:, 1] > 90).any()


def test_decode_ties_empty_votes_and_value_of():
    from bithtm_amd import ScalarEncoder, ScalarField
    enc = ScalarEncoder([ScalarField(0, 10, 12, 3), ScalarField(0, 8, 8, 3, periodic=True)], 24)
    votes = np.zeros((4, 24), np.int64)
    votes[0, [2, 3, 4, 7, 8, 9]] = 5                                # two equal windows: buckets 2 and 7 -> 2
    votes[0, 12 + 7], votes[0, 12 + 1] = 3, 4                       # periodic: only the window of bucket 7 -- bits 7, 0, 1 -- holds both
    votes[1, 9:12] = 1                                              # a maximum in the last bucket (9 of 10)
    votes[2, 12 + 3] = 2                                            # buckets 1, 2, 3 tie at 2 -> 1; the other field is all zero
    bucket, score = enc.decode(votes)
    assert bucket.tolist() == [[2, 7], [9, -1], [-1, 1], [-1, -1]]
    assert score.tolist() == [[15, 7], [3, 0], [0, 2], [0, 0]]
    value = enc.value_of(bucket)
    assert value[0, 0] == 0.0 + 2.5 / enc.fields[0].scale and value[0, 1] == 7.5 / enc.fields[1].scale
    assert np.isnan(value[3]).all() and np.isnan(enc.fields[0].value_of(-1))
    assert enc.fields[0].value_of(0) == 0.5 and enc.fields[0].value_of(9) == 9.5      # (bucket middles: scale 1)
    with pytest.raises(ValueError):
        enc.decode(np.zeros(23, np.int32))


def test_constructor_refusals():
    from bithtm_amd import ScalarEncoder, ScalarField
    for args in ((0, 1, 8, 0), (0, 1, 8, 9), (0, 1, 0, 1), (1, 1, 8, 2), (2, 1, 8, 2), (np.nan, 1, 8, 2), (0, np.inf, 8, 2), (-np.inf, 0, 8, 2)):
        with pytest.raises(ValueError):
            ScalarField(*args)
    f = ScalarField(0, 1, 8, 2)
    with pytest.raises(ValueError):
        ScalarEncoder([])
    with pytest.raises(ValueError):
        ScalarEncoder([f] * 17)
    with pytest.raises(ValueError):
        ScalarEncoder([f, f], input_dim=15)
    with pytest.raises(ValueError):
        ScalarEncoder([f, "not a field"])
    enc = ScalarEncoder([f] * 16, input_dim=200)
    assert len(enc) == 16 and enc.input_dim == 200 and enc.offsets[-1] == 120
    with pytest.raises(ValueError):
        enc.encode(np.zeros((3, 15)))
    with pytest.raises(ValueError, match="input_dim"):
        enc.check_model(128)
    with pytest.raises(ValueError, match="int32"):
        ScalarEncoder([ScalarField(0, 1, 4096, 2048)]).check_model(4096, column_dim=1 << 20)
    with pytest.raises(ValueError, match="8192"):
        ScalarEncoder([ScalarField(0, 1, 8193, 2)]).check_model(8193, column_dim=64)
    enc.check_model(200, column_dim=2048)


def test_the_field_table_is_the_headers_struct():
    import ctypes as C
    from bithtm_amd import _lib
    assert C.sizeof(_lib.HtmScalarField) == 40 and _lib.HtmScalarField.scale.offset == 8 and _lib.HtmScalarField.offset.offset == 16
    tab = _layout_a().table()
    assert len(tab) == 3
    assert [(t.offset, t.bits, t.width, t.buckets, t.periodic, t.reserved) for t in tab] == \
        [(0, 130, 21, 110, 0, 0), (130, 96, 11, 96, 1, 0), (226, 70, 1, 70, 0, 0)]
    assert tab[1].minimum == 0.0 and tab[1].scale == 4.0 and tab[2].minimum == -5.0 and tab[2].scale == 7.0


def test_header_declares_the_scalar_functions_and_the_abi_stays_4():
    from bithtm_amd import _lib
    header = open(os.path.join(ROOT, "include", "bithtm_hip.h")).read()
    for name in ("htm_bank_encode", "htm_decode_votes", "htm_predicted_value"):
        assert re.search(r"^int " + name + r"\(htm_handle \*h, const htm_scalar_field \*fields, int32_t n_fields,", header, flags=re.M), name
        assert name in _lib.EXPORTS
    assert re.search(r"typedef struct htm_scalar_field \{\s*double minimum, scale;\s*int32_t offset, bits, width, buckets, periodic, reserved;\s*\} htm_scalar_field;",
                     header)
    assert "#define HTM_DECODE_MAX_BITS 8192" in header and "#define HTM_SCALAR_MAX_FIELDS 16" in header
    assert re.search(r"#define BITHTM_ABI_VERSION\s+4\b", header) and _lib.ABI_VERSION == 4
    from bithtm_amd import encoders
    assert encoders.DECODE_MAX_BITS == 8192 and encoders.MAX_FIELDS == 16


def test_record_fields_and_run_record_keep_their_shape():
    from bithtm_amd import RunRecord
    from bithtm_amd.engine import RECORD_FIELDS
    assert RECORD_FIELDS[:4] == ("counters", "active_column", "column_prediction", "predicted_input") and "predicted_value" in RECORD_FIELDS
    rec = RunRecord(np.arange(3), np.zeros((3, 8), np.int32), None, None, np.zeros((3, 5), np.int32))
    assert rec.fields == ("counters", "predicted_input") and rec.predicted_bucket is None and rec.predicted_value is None
    rec = RunRecord(np.arange(2), predicted_bucket=np.zeros((2, 1), np.int32), predicted_score=np.zeros((2, 1), np.int32),
                    predicted_value=np.zeros((2, 1)))
    assert rec.fields == ("predicted_value",)


def test_the_scalar_kernels_use_no_scratch():
    """The build's own resource report: neither kernel spills (a 16-field table indexed at run time must stay in the kernel
    arguments, not become a private array)."""
    from bithtm_amd.build import kernel_resources
    res = kernel_resources()
    if res is None:
        pytest.skip("the library in the tree was not built here")
    mine = {k: v for k, v in res.items() if "k_bank_encode" in k or "k_decode_votes" in k}
    assert len(mine) == 2, sorted(res)
    for name, r in mine.items():
        assert r["scratch_bytes_per_lane"] == 0, (name, r)
        assert r["lds_bytes"] <= 64 * 1024, (name, r)


# ---- which launches and copies the host code makes (the engine's host code over tests/host_stub's runtime; kernels do nothing)

@pytest.fixture(scope="module")
def traces(tmp_path_factory):
    import json
    import subprocess
    import sys
    from test_launch_trace_cpu import _build
    tmp = str(tmp_path_factory.mktemp("scalar_trace"))
    env = dict(os.environ, BITHTM_LIBRARY=_build(tmp), BITHTM_STUB_TRACE=os.path.join(tmp, "trace.txt"))
    for name in ("LD_PRELOAD", "BITHTM_LEAN", "BITHTM_SCAN_LARGE"):
        env.pop(name, None)
    r = subprocess.run([sys.executable, os.path.join(ROOT, "tests", "host_stub", "scalar_driver.py")], env=env, capture_output=True, text=True,
                       timeout=600)
    assert r.returncode == 0, (r.stdout + r.stderr)[-4000:]
    return json.loads(r.stdout.splitlines()[-1])


needs_hipcc = pytest.mark.skipif(not os.path.exists("/opt/rocm/bin/hipcc"), reason="needs hipcc")


def _kernels(lines):
    from test_stream_fork_cpu import _kernels as kernels
    return kernels(lines)


@needs_hipcc
def test_encode_and_decode_are_one_launch_each(traces):
    """htm_bank_encode and htm_decode_votes: one launch, a block per row (one wave for a row of 12 words; 256 threads per row and
    field in the decode), no copy, no memset, no graph."""
    assert len(traces["bank_encode"]) == 1 and re.match(r"launch _Z13k_bank_encode\S+ grid 5 1 block 64 lds 0$", traces["bank_encode"][0])
    assert len(traces["decode_votes"]) == 1 and re.match(r"launch _Z14k_decode_votes\S+ grid 5 3 block 256 lds 0$", traces["decode_votes"][0])


@needs_hipcc
def test_predicted_value_keeps_the_votes_on_the_device(traces):
    """htm_predicted_value: the votes launch, the decode launch over its one row, and one copy of 2 F ints -- no copy of the
    input_dim votes (the memsets are the votes row's, and the zeroing of the two buffers when they are first made)."""
    lines = traces["predicted_value"]
    assert _kernels(lines) == ["k_pin", "k_decode_votes"], lines
    assert [line for line in lines if line.startswith("memcpy")] == ["memcpy 24"] and lines[-1] == "memcpy 24", lines
    assert re.search(r"grid 1 3 block 256", lines[-2])


@needs_hipcc
def test_refused_calls_enqueue_nothing(traces):
    """Every HTM_ERR_ARGUMENT case of the three calls: -1, and not one launch, copy or memset.  The cap of 8 192 bits per field is
    the decoding calls' alone; no rows is HTM_OK; a handle without a Temporal Memory has no state to decode (HTM_ERR_STATE)."""
    assert traces["codes"] and set(traces["codes"]) == {-1}, traces["codes"]
    assert traces["refused"] == []
    assert traces["cap_codes"] == [0, -1, 0, -4]


@needs_hipcc
def test_a_run_over_values_encodes_once_and_decodes_once_per_batch(traces):
    first, second = traces["first_run"], traces["second_run"]
    assert _kernels(first)[0] == "k_bank_encode" and _kernels(first).count("k_bank_encode") == 1
    assert "k_bank_encode" not in _kernels(second) and "k_decode_votes" not in _kernels(first + second)
    # a "predicted_value" record is the "predicted_input" run of the parent commit plus one decode launch behind it
    recorded, with_votes, plain = traces["recorded"], traces["with_votes"], traces["plain"]
    assert re.match(r"launch _Z14k_decode_votes\S+ grid 6 3 block 256 lds 0$", recorded[-1])
    assert recorded[:-1] == plain and with_votes == recorded


@needs_hipcc
def test_a_stack_refuses_predicted_value_with_a_value_error(traces):
    """RegionStack.run has no encoder=: the record field is refused as run() refuses it without one (ValueError, not a KeyError
    from the record shapes), and the other fields go on working (the driver checks that, and ModelGroup.predicted_value's shapes)."""
    assert "encoder" in traces["stack_refusal"] and "predicted_value" in traces["stack_refusal"], traces["stack_refusal"]
