"""CPU: the NumPy definition of the device-side input noise (bithtm_amd.flip_noise / noise_threshold) --
what tests/test_hip_input_noise.py holds the kernel and the noisy runs to -- the integer form of the comparison, the
statistics of keyed stream 6, and the argument checks that need no device."""

import ctypes as C
import os

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_flip_noise_is_the_keyed_draw_below_p():
    from bithtm_amd import flip_noise
    from bithtm_amd._keyed import STREAM_INPUT_NOISE, draw_unit
    assert STREAM_INPUT_NOISE == 6
    for seed, step, I, p in ((0, 0, 300, 0.05), (7, 123, 70, 0.5), (0xFFFFFFFF, 4_000_000_000, 1000, 0.05), (12345, 999, 1024, 0.9)):
        got = flip_noise(seed, step, I, p)
        assert got.dtype == np.bool_ and got.shape == (I,)
        assert np.array_equal(got, draw_unit(seed, 6, step, np.arange(I)) < p)
    # the step enters mod 2^32, as the device's counter does
    assert np.array_equal(flip_noise(3, (1 << 32) + 5, 300, 0.3), flip_noise(3, 5, 300, 0.3))


def test_the_stream_number_is_the_devices():
    src = open(os.path.join(ROOT, "bithtm_amd", "csrc", "htm_rng.h")).read()
    assert "#define HTM_STREAM_INPUT_NOISE 6u" in src
    for taken in ("HTM_STREAM_POPULATE_CELL 4u", "HTM_STREAM_POPULATE_PERM 5u"):
        assert taken in src


def test_no_flips_at_zero_and_all_flips_at_one():
    from bithtm_amd import flip_noise
    for I in (1, 70, 300, 1024):
        for seed, step in ((0, 0), (9, 77)):
            assert not flip_noise(seed, step, I, 0.0).any()
            assert flip_noise(seed, step, I, 1.0).all()


def test_noise_depends_on_seed_step_and_index_only():
    from bithtm_amd import flip_noise
    a = flip_noise(5, 40, 1000, 0.25)
    assert np.array_equal(a, flip_noise(5, 40, 1000, 0.25))            # (stateless: the same call again)
    assert np.array_equal(a[:300], flip_noise(5, 40, 300, 0.25))       # (input i does not depend on input_dim)
    assert not np.array_equal(a, flip_noise(6, 40, 1000, 0.25))
    assert not np.array_equal(a, flip_noise(5, 41, 1000, 0.25))
    assert (a & ~flip_noise(5, 40, 1000, 0.5)).sum() == 0              # (a larger p flips a superset)


def test_the_integer_comparison_is_the_float_one():
    from bithtm_amd import noise_threshold
    assert noise_threshold(0.0) == 0 and noise_threshold(1.0) == 1 << 24
    assert noise_threshold(0.25) == 1 << 22                            # (p * 2^24 an integer: m = p * 2^24 does not flip)
    assert noise_threshold(3 * 2.0 ** -24) == 3
    for p in (0.05, 0.25, 0.5, 1e-9, 2.0 ** -24, 3 * 2.0 ** -24, 1 / 3, 0.999999999, 1.0 - 2.0 ** -25, 1.0):
        t = noise_threshold(p)
        assert 0 <= t <= 1 << 24
        cut = int(p * 2.0 ** 24)
        m = np.unique(np.clip(np.arange(cut - 3, cut + 4), 0, (1 << 24) - 1)).astype(np.int64)
        assert np.array_equal(m * 2.0 ** -24 < p, m < t), p


def test_argument_errors_need_no_device():
    from bithtm_amd import flip_noise, noise_threshold
    from bithtm_amd.networks import _noise_threshold_arg
    for bad in (-0.01, 1.0000001, float("nan"), float("inf"), -1):
        with pytest.raises(ValueError, match="noise"):
            noise_threshold(bad)
        with pytest.raises(ValueError, match="noise"):
            flip_noise(0, 0, 10, bad)
        with pytest.raises(ValueError, match="noise"):
            _noise_threshold_arg(bad)
    with pytest.raises(ValueError, match="noise"):
        _noise_threshold_arg([0.1, 0.2])                # (a list per member is ModelGroup.run's)
    assert _noise_threshold_arg(0) == 0 and _noise_threshold_arg(np.float32(0.5)) == 1 << 23


def test_bank_noise_refuses_a_null_handle():
    import __graft_entry__ as ge
    ge.build()
    from bithtm_amd import _lib
    lib = _lib.load()
    buf = (C.c_uint32 * 8)()
    assert lib.htm_bank_noise(None, buf, 1, buf, 1, 0, 1, 0, 0, None, None) == -1       # HTM_ERR_ARGUMENT


@pytest.mark.parametrize("I", [300, 1000])
def test_stream_six_flips_the_fraction_it_is_asked_for(I):
    """400 rows at p = 0.05 under the seed of the forecast fixture (whose small shape the GPU tests use): the flip fraction of
    the keyed stream is 0.0498 to 0.0501 at both sizes, and no two rows are alike.  Under other seeds the fraction stays
    within five standard deviations of a fair draw of 400 * I inputs, sqrt(p (1 - p) / (400 I)) each."""
    from bithtm_amd import flip_noise
    from forecast_fixture import RUN
    rows = np.stack([flip_noise(RUN["seed"], t, I, 0.05) for t in range(400)])
    print(f"I={I} seed={RUN['seed']}: flip fraction {rows.mean():.5f}")
    assert 0.0498 <= rows.mean() <= 0.0501, rows.mean()
    assert len(np.unique(np.packbits(rows, axis=1), axis=0)) == 400
    sd = np.sqrt(0.05 * 0.95 / (400 * I))
    for seed in (0, 1, 5):
        rows = np.stack([flip_noise(seed, t, I, 0.05) for t in range(400)])
        assert abs(rows.mean() - 0.05) < 5 * sd, (seed, rows.mean())
        assert len(np.unique(np.packbits(rows, axis=1), axis=0)) == 400
