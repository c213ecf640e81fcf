"""Host side of the device resampler (no GPU): the float64 oracle against scipy.signal.resample_poly, the library's design /
taps / length entry points against the oracle, and the wav ingest's rate policies on a small tree of files."""
import ctypes
import os

import numpy as np
import pytest

import resample_cases as RC
import resample_oracle as RO
from speech_recognition_amd import _lib, input_data

ALL_PAIRS = sorted(set(RC.SCIPY_PAIRS) | set(p[:2] for p in RC.PAIRS))


def _design(rate_in, rate_out):
    v = [ctypes.c_int(-7) for _ in range(4)]
    rc = _lib.load().kws_resample_design(rate_in, rate_out, *[ctypes.byref(c) for c in v])
    return rc, tuple(c.value for c in v)


@pytest.mark.parametrize("rate_in,rate_out", RC.SCIPY_PAIRS)
def test_oracle_equals_scipy_resample_poly(rate_in, rate_out):
    signal = pytest.importorskip("scipy.signal")
    up, down, _, _ = RO.design(rate_in, rate_out)
    rng = np.random.RandomState(rate_in % 977)
    for x in (rng.randint(-32768, 32768, 1501).astype(np.float64), RC.alternating_row(700).astype(np.float64),
              np.full(333, -32768.0), np.array([32767.0])):
        want = signal.resample_poly(x, up, down)
        got = RO.resample(x, rate_in, rate_out)
        assert got.shape == want.shape
        if (up, down) == (1, 1):
            assert np.array_equal(got, x)
        err = np.abs(got - want).max() / 32768.0
        print("%d -> %d, n = %d: max |oracle - scipy| / 32768 = %.3g" % (rate_in, rate_out, len(x), err))
        assert err <= 1e-9


@pytest.mark.parametrize("rate_in,rate_out", ALL_PAIRS)
def test_design_matches_the_oracle(rate_in, rate_out):
    rc, got = _design(rate_in, rate_out)
    assert rc == 0 and got == RO.design(rate_in, rate_out)


def test_design_reduces_by_the_gcd_and_skips_null_pointers():
    assert _design(32000, 32000) == (0, (1, 1, 10, 21))
    assert _design(96000, 32000) == (0, (1, 3, 30, 61))
    assert _design(7, 65536) == (0, (65536, 7, 655360, 21))
    up = ctypes.c_int()
    assert _lib.load().kws_resample_design(44100, 16000, ctypes.byref(up), None, None, None) == 0 and up.value == 160


def test_the_case_table_names_the_paths_the_launcher_takes():
    for p in RC.PAIRS:
        assert RO.design(*p[:2])[:2] == p[2:4]
        assert RC.kernel_path(*p[:2]) == RC.EXPECTED_PATHS[p[:2]], p
    assert {v[0] for v in RC.EXPECTED_PATHS.values()} == {'decimate', 'lds', 'global', 'direct', 'copy'}


@pytest.mark.parametrize("rate_in,rate_out", ALL_PAIRS)
def test_taps_are_the_float64_design_rounded_once(rate_in, rate_out):
    """The double design error is far below a float32 ulp, so only a rounding tie may flip: <= 1 ulp."""
    h64 = RO.taps(rate_in, rate_out)
    h = np.full(len(h64), np.nan, dtype=np.float32)
    assert _lib.load().kws_resample_taps(rate_in, rate_out, h.ctypes.data_as(ctypes.c_void_p), h.size) == 0
    want = h64.astype(np.float32)
    ulps = np.abs(h.view(np.int32).astype(np.int64) - want.view(np.int32).astype(np.int64))
    same_sign = (np.signbit(h) == np.signbit(want)) | (want == 0)
    print("%d -> %d: %d taps, %d differ from float32(h64), max %d ulp" % (rate_in, rate_out, h.size, (ulps > 0).sum(), ulps.max()))
    assert same_sign.all() and ulps.max() <= 1
    assert np.array_equal(h, h[::-1])            # symmetric
    # a wrong length is refused and nothing is written
    g = np.full(len(h64) + 1, np.nan, dtype=np.float32)
    assert _lib.load().kws_resample_taps(rate_in, rate_out, g.ctypes.data_as(ctypes.c_void_p), g.size) == -1
    assert np.isnan(g).all()


@pytest.mark.parametrize("rate_in,rate_out", ALL_PAIRS)
def test_out_samples_is_the_ceiling(rate_in, rate_out):
    lib = _lib.load()
    up, down, _, _ = RO.design(rate_in, rate_out)
    ns = {0, 1, 2, 16000, 2 ** 40 + 1}
    for m in (1, 2, 37):
        ns |= {m * down - 1, m * down, m * down + 1}
    for n in sorted(ns):
        assert lib.kws_resample_out_samples(rate_in, rate_out, n) == -(-(n * up) // down) == RO.out_samples(n, rate_in, rate_out)


def test_invalid_rates_are_refused():
    lib = _lib.load()
    h = np.zeros(21, dtype=np.float32)
    for rate_in, rate_out in [(0, 16000), (16000, 0), (-1, 16000), (16000, -16000), (65537, 1), (1, 65537), (65537, 65536)]:
        assert _design(rate_in, rate_out) == (-1, (-7, -7, -7, -7))
        assert lib.kws_resample_taps(rate_in, rate_out, h.ctypes.data_as(ctypes.c_void_p), h.size) == -1
        assert lib.kws_resample_out_samples(rate_in, rate_out, 100) == -1
    assert lib.kws_resample_out_samples(48000, 16000, -1) == -1
    assert _design(65536, 1)[0] == 0 and _design(2 * 65536, 2)[0] == 0          # the limit is on the reduced pair
    assert lib.kws_last_error()


def _wav_tree(root):
    rng = np.random.RandomState(5)
    files = []
    for word, rate, n in [("yes", 16000, 900), ("no", 48000, 2500), ("up", 16000, 1200), ("yes", 48000, 700)]:
        os.makedirs(os.path.join(root, word), exist_ok=True)
        fn = os.path.join(root, word, "%d_%d.wav" % (rate, n))
        input_data.save_wav_file(fn, rng.uniform(-1, 1, n), rate)
        files.append(fn)
    return files


def test_grouping_and_the_error_policy(tmp_path):
    files = _wav_tree(str(tmp_path))
    groups = input_data.group_files_by_rate(files)
    assert [(rate, [k for k, _ in members]) for rate, members in groups] == [(16000, [0, 2]), (48000, [1, 3])]
    for rate, members in groups:
        for k, a in members:
            assert a.dtype == np.int16 and np.array_equal(a, input_data._read_wav_int16(files[k])[0])
    with pytest.raises(ValueError) as e:
        input_data.check_wav_rates(files, 16000)
    assert files[1] in str(e.value) and "48000" in str(e.value)
    input_data.check_wav_rates([files[0], files[2]], 16000)
    # the policy is checked before any device is needed
    with pytest.raises(ValueError) as e:
        input_data.decode_wav_files(files, 1000, 16000, "cpu", rate_policy='error')
    assert files[1] in str(e.value)
    with pytest.raises(ValueError):
        input_data.decode_wav_files(files, 1000, 16000, "cpu", rate_policy='nearest')


def test_decode_wav_policy_is_the_bank_of_today(tmp_path):
    files = _wav_tree(str(tmp_path))
    for policy, subset in (('decode_wav', files), ('error', [files[0], files[2]])):
        got = input_data.decode_wav_files(subset, 1000, 16000, "cpu", rate_policy=policy)
        want = input_data.bank_from_files({fn: k for k, fn in enumerate(subset)}, 1000)
        assert got.dtype.is_floating_point is False and got.numpy().tobytes() == want.tobytes()
    assert input_data.decode_wav_files([], 1000, 16000, "cpu").shape == (0, 1000)


def test_python_op_host_helpers():
    from speech_recognition_amd import resample as rs
    assert rs.design(44100, 16000) == (160, 441, 4410, 56)
    assert rs.resampled_samples(48000, 48000, 16000) == 16000 and rs.resampled_samples(44101, 44100, 16000) == 16001
    assert np.array_equal(rs.taps(8000, 16000), RO.taps(8000, 16000).astype(np.float32)) or \
        np.abs(rs.taps(8000, 16000) - RO.taps(8000, 16000)).max() < 1e-7
    with pytest.raises(ValueError):
        rs.design(0, 16000)
    with pytest.raises(ValueError):
        rs.resampled_samples(10, 65537, 1)
