"""The resampling kernels (csrc/resample.hip, kws_resample_i16 / kws_resample_f32) against the float64 oracle
tests/resample_oracle.py, on every path the launcher has (the decimation loop, table in LDS, table in global memory, the direct kernel, the copy).

Every launch here writes between guard bands, reads from rows whose padding is poison (int16 32767 / float NaN) and runs
twice into separate buffers that must hold equal bits.

  exact    impulses of +-2^k further apart than the filter: every output is ONE product h32[j] 2^k, exact in float32
           whatever the summation order - any slip in phase, offset, tile seam or row edge shows as a wrong number;
  random   |out_f32 - y64| <= (T + 3) 2^-24 sum_j |h[j] x[i_j]|: a float32 inner product of T terms (gamma_T), the
           rounding of the taps to float32 (1 more) and of inputs that are not float32 numbers (none here), with slack 2;
  staged   out_i16 == clamp(rint(out_f32)) from the device's own out_f32, bit for bit."""
import ctypes

import numpy as np
import pytest
import torch

import resample_cases as RC
import resample_oracle as RO
from speech_recognition_amd import _lib
from speech_recognition_amd import resample as rs

pytestmark = pytest.mark.gpu

GUARD = 64                      # elements on both sides of every output (a multiple of 4: the output stays 16-byte aligned)
G16, G32 = -12345, 54321.0


def launch(rate_in, rate_out, rows, keep, dtype=np.int16, pitch_extra=5, lengths_on_device=True, outs="both", misalign=0):
    """rows: list of 1-D host arrays.  Returns (out_f32 or None, out_i16 or None) as host arrays [B, keep] after the guard,
    poison and run-twice checks.  outs: 'both' | 'i16' | 'f32' (the int16 entry point's NULL outputs)."""
    B = len(rows)
    n_in = max(max(len(r) for r in rows), 1)
    pitch = n_in + pitch_extra
    host = np.full((B, pitch), 32767 if dtype == np.int16 else np.nan, dtype=dtype)
    for b, r in enumerate(rows):
        host[b, :len(r)] = r
    x = torch.from_numpy(host).cuda()
    lens = torch.tensor([len(r) for r in rows], dtype=torch.int32).cuda() if lengths_on_device else None
    if not lengths_on_device:
        assert all(len(r) == n_in for r in rows)
    plan = rs._plan(rate_in, rate_out)
    res = []
    for _ in range(2):
        o32 = torch.full((B * keep + 2 * GUARD + 4,), G32, dtype=torch.float32).cuda()
        o16 = torch.full((B * keep + 2 * GUARD + 4,), G16, dtype=torch.int16).cuda()
        p32 = ctypes.c_void_p(o32.data_ptr() + 4 * (GUARD + misalign)) if outs != "i16" else None
        p16 = ctypes.c_void_p(o16.data_ptr() + 2 * (GUARD + misalign)) if outs != "f32" and dtype == np.int16 else None
        if dtype == np.int16:
            _lib.call("kws_resample_i16", plan, _lib.ptr(x), pitch, _lib.ptr(lens), n_in, p16, p32, B, keep, _lib.stream_ptr())
        else:
            _lib.call("kws_resample_f32", plan, _lib.ptr(x), pitch, _lib.ptr(lens), n_in, p32, B, keep, _lib.stream_ptr())
        torch.cuda.synchronize()
        h32, h16 = o32.cpu().numpy(), o16.cpu().numpy()
        lo, hi = GUARD + misalign, GUARD + misalign + B * keep
        for h, g, used in ((h32, G32, p32 is not None), (h16, G16, p16 is not None)):
            assert (h[:lo] == g).all() and (h[hi:] == g).all(), "guard band overwritten"
            if not used:
                assert (h == g).all()
        res.append((h32[lo:hi].reshape(B, keep) if p32 is not None else None,
                    h16[lo:hi].reshape(B, keep) if p16 is not None else None))
    for a, b in zip(res[0], res[1]):
        assert (a is None and b is None) or a.tobytes() == b.tobytes(), "two runs differ"
    assert torch.equal(x.cpu(), torch.from_numpy(host)) or dtype != np.int16     # the input is not written
    return res[0]


def check_rows(rate_in, rate_out, rows, keep, f32, i16, exact=False):
    """Every row of a launch against the oracle; returns the largest error / bound ratio seen."""
    _, _, _, T = RO.design(rate_in, rate_out)
    copy = RC.kernel_path(rate_in, rate_out)[0] == 'copy'
    h32 = rs.taps(rate_in, rate_out).astype(np.float64) if exact else None
    worst = 0.0
    if f32 is not None:
        assert np.isfinite(f32).all(), "poison reached the output"
    for b, r in enumerate(rows):
        y, ya = RO.resample(r, rate_in, rate_out, h=h32, with_abs=True)
        n = min(len(y), keep)
        if f32 is not None:
            got = f32[b].astype(np.float64)
            assert (got[n:] == 0).all(), (b, "tail not zero")
            if exact or copy:
                bad = np.nonzero(got[:n] != y[:n])[0]
                assert bad.size == 0, (b, len(r), bad[:8], got[bad[:8]], y[bad[:8]])
            else:
                bound = (T + 3) * 2.0 ** -24 * ya[:n]
                err = np.abs(got[:n] - y[:n])
                assert (err <= bound).all(), (b, len(r), (err / np.maximum(bound, 1e-300)).max())
                if n:
                    worst = max(worst, float((err / np.maximum(bound, 1e-30))[bound > 0].max(initial=0.0)))
        if i16 is not None:
            assert (i16[b, n:] == 0).all()
            if f32 is not None:
                assert np.array_equal(i16[b], RO.to_int16(f32[b])), (b, "int16 is not the staged float")
            elif exact or copy:
                assert np.array_equal(i16[b, :n], RO.to_int16(y[:n]))
    return worst


def edge_rows(rate_in, rate_out, make):
    return [make(n) for n in RC.edge_lengths(rate_in, rate_out)]


@pytest.mark.parametrize("rate_in,rate_out", [p[:2] for p in RC.FILTER_PAIRS], ids=RC.FILTER_IDS)
def test_impulses_come_out_as_single_exact_products(rate_in, rate_out):
    rows = edge_rows(rate_in, rate_out, lambda n: RC.impulse_row(n, rate_in, rate_out))
    n_max = max(RO.out_samples(len(r), rate_in, rate_out) for r in rows)
    assert sum(int((r != 0).sum()) for r in rows) >= 8
    for keep in (n_max + 7, n_max + 8):                      # scalar stores, vector stores; zero tails everywhere
        f32, i16 = launch(rate_in, rate_out, rows, keep)
        check_rows(rate_in, rate_out, rows, keep, f32, i16, exact=True)
        assert np.count_nonzero(f32) > 0
    frows = [r.astype(np.float32) for r in rows]
    f32, _ = launch(rate_in, rate_out, frows, n_max + 8, dtype=np.float32)
    check_rows(rate_in, rate_out, frows, n_max + 8, f32, None, exact=True)


@pytest.mark.parametrize("rate_in,rate_out", [p[:2] for p in RC.FILTER_PAIRS], ids=RC.FILTER_IDS)
def test_random_and_full_scale_rows_within_the_float32_bound(rate_in, rate_out):
    rng = np.random.RandomState(rate_in % 1000 + 3)
    lens = RC.edge_lengths(rate_in, rate_out)
    rows = [RC.alternating_row(n) if b % 2 else RC.random_row(rng, n) for b, n in enumerate(lens)]
    n_max = max(RO.out_samples(n, rate_in, rate_out) for n in lens)
    tile = RC.kernel_path(rate_in, rate_out)[1] or 256
    worst = 0.0
    # zero tails (odd keep: scalar stores), then a crop inside the first tile's last quad and one at a multiple of 4
    for keep in (n_max + 5, max(tile - 3, 1) if n_max > tile else max(n_max - 3, 1), max(n_max // 8 * 4, 4)):
        f32, i16 = launch(rate_in, rate_out, rows, keep)
        worst = max(worst, check_rows(rate_in, rate_out, rows, keep, f32, i16))
    frows = [RC.random_row(rng, n, np.float32) for n in lens]
    f32, _ = launch(rate_in, rate_out, frows, n_max + 4, dtype=np.float32)
    worst = max(worst, check_rows(rate_in, rate_out, frows, n_max + 4, f32, None))
    print("%d -> %d: largest error / bound = %.3f" % (rate_in, rate_out, worst))


def test_full_scale_saturates_both_ways():
    rows = [RC.alternating_row(300), RC.alternating_row(299)]
    f32, i16 = launch(8000, 16000, rows, 600)
    check_rows(8000, 16000, rows, 600, f32, i16)
    assert ((f32 > 32767.5) & (i16 == 32767)).sum() > 50 and ((f32 < -32768.5) & (i16 == -32768)).sum() > 50


@pytest.mark.parametrize("rate_in,rate_out", [(48000, 16000), (44100, 16000), (999, 1000), (16000, 100), (32000, 32000)],
                         ids=["decimate", "lds", "global", "direct", "copy"])
def test_null_outputs_null_lengths_and_unaligned_outputs(rate_in, rate_out):
    rng = np.random.RandomState(11)
    n = 1300 if rate_out != 100 else 6000
    rows = [RC.random_row(rng, n) for _ in range(3)]
    keep = RO.out_samples(n, rate_in, rate_out) // 4 * 4
    f32, i16 = launch(rate_in, rate_out, rows, keep, pitch_extra=0, lengths_on_device=False)
    check_rows(rate_in, rate_out, rows, keep, f32, i16)
    only32, none16 = launch(rate_in, rate_out, rows, keep, outs="f32")
    none32, only16 = launch(rate_in, rate_out, rows, keep, outs="i16")
    assert none16 is None and none32 is None
    assert only32.tobytes() == f32.tobytes() and only16.tobytes() == i16.tobytes()
    # keep is a multiple of 4 but the output pointers are not 16 / 8-byte aligned: the scalar stores, the same bits
    m32, m16 = launch(rate_in, rate_out, rows, keep, misalign=1)
    assert m32.tobytes() == f32.tobytes() and m16.tobytes() == i16.tobytes()


def test_equal_rates_copy_the_bytes():
    rng = np.random.RandomState(2)
    rows = [RC.random_row(rng, n) for n in (1, 777, 0, 1030)] + [RC.alternating_row(64)]
    f32, i16 = launch(32000, 32000, rows, 1040)
    for b, r in enumerate(rows):
        assert i16[b, :len(r)].tobytes() == r.tobytes() and (i16[b, len(r):] == 0).all()
        assert np.array_equal(f32[b, :len(r)], r.astype(np.float32)) and (f32[b, len(r):] == 0).all()
    f32, i16 = launch(32000, 32000, rows, 500)                         # crop
    for b, r in enumerate(rows):
        assert i16[b, :min(len(r), 500)].tobytes() == r[:500].tobytes()
    frows = [RC.random_row(rng, n, np.float32) for n in (5, 777, 0)]
    frows[1][:4] = [-0.0, 1e-42, 3.4e38, -1e-30]                       # bytes, not values
    f32, _ = launch(32000, 32000, frows, 800, dtype=np.float32)
    for b, r in enumerate(frows):
        assert f32[b, :len(r)].tobytes() == r.tobytes() and (f32[b, len(r):].view(np.int32) == 0).all()


@pytest.mark.parametrize("rate_in,rate_out", [(44100, 16000), (999, 1000)], ids=["lds", "global"])
def test_more_tiles_than_workgroups(rate_in, rate_out):
    """1500 short ragged rows: the grid (4 workgroups per compute unit at most) wraps, a workgroup meets rows of every
    kind - empty, a few samples, zero tiles - one after another on one staged table."""
    rng = np.random.RandomState(4)
    lens = rng.randint(0, 90, 1500)
    lens[[0, 17, 1499]] = [0, 1, 89]
    rows = [RC.alternating_row(n) if b % 7 == 3 else RC.random_row(rng, n) for b, n in enumerate(lens)]
    keep = 40
    f32, i16 = launch(rate_in, rate_out, rows, keep)
    check_rows(rate_in, rate_out, rows, keep, f32, i16)
    # a row inside the batch is the row alone, bit for bit
    for b in (0, 17, 700, 1499):
        if len(rows[b]):
            a32, a16 = launch(rate_in, rate_out, [rows[b]], keep, lengths_on_device=False, pitch_extra=0)
            assert a32.tobytes() == f32[b].tobytes() and a16.tobytes() == i16[b].tobytes()


@pytest.mark.parametrize("rate_in,rate_out", [p[:2] for p in RC.FILTER_PAIRS], ids=RC.FILTER_IDS)
def test_a_row_in_a_batch_is_the_row_alone(rate_in, rate_out):
    rng = np.random.RandomState(8)
    lens = RC.edge_lengths(rate_in, rate_out)
    rows = [RC.random_row(rng, n) for n in lens]
    keep = max(RO.out_samples(n, rate_in, rate_out) for n in lens) + 4
    f32, i16 = launch(rate_in, rate_out, rows, keep)
    for b in (0, 3, len(rows) - 3):
        a32, a16 = launch(rate_in, rate_out, [rows[b]], keep, lengths_on_device=False, pitch_extra=0)
        assert a32.tobytes() == f32[b].tobytes() and a16.tobytes() == i16[b].tobytes()


def test_one_long_row():
    """150 000 samples at 48 kHz, B = 1: 49 tiles of one row."""
    rng = np.random.RandomState(6)
    x = RC.random_row(rng, 150000)
    x[70000:70200] = RC.alternating_row(200)
    keep = 50000
    f32, i16 = launch(48000, 16000, [x], keep, lengths_on_device=False)
    worst = check_rows(48000, 16000, [x], keep, f32, i16)
    print("long row: largest error / bound = %.3f" % worst)
    imp = RC.impulse_row(150000, 48000, 16000)
    f32, i16 = launch(48000, 16000, [imp], keep + 3)
    check_rows(48000, 16000, [imp], keep + 3, f32, i16, exact=True)


def test_bad_arguments_are_refused_before_any_launch():
    lib = _lib.load()
    plan = ctypes.c_void_p()
    assert lib.kws_resample_plan_create(0, 16000, ctypes.byref(plan)) == -1
    assert lib.kws_resample_plan_create(65537, 1, ctypes.byref(plan)) == -1
    assert lib.kws_resample_plan_create(48000, 16000, None) == -1
    p = rs._plan(48000, 16000)
    x = torch.zeros((2, 100), dtype=torch.int16).cuda()
    o = torch.zeros((2, 40), dtype=torch.int16).cuda()
    s = _lib.stream_ptr()
    assert lib.kws_resample_i16(p, _lib.ptr(x), 100, None, 100, None, None, 2, 40, s) == -1       # no output
    assert lib.kws_resample_i16(p, _lib.ptr(x), 99, None, 100, _lib.ptr(o), None, 2, 40, s) == -1  # pitch < n_in
    assert lib.kws_resample_i16(p, None, 100, None, 100, _lib.ptr(o), None, 2, 40, s) == -1
    assert lib.kws_resample_i16(None, _lib.ptr(x), 100, None, 100, _lib.ptr(o), None, 2, 40, s) == -1
    assert lib.kws_resample_i16(p, _lib.ptr(x), 100, None, 100, _lib.ptr(o), None, 0, 40, s) == 0  # nothing to do
    # a plan of its own is created and destroyed
    assert lib.kws_resample_plan_create(22050, 16000, ctypes.byref(plan)) == 0 and plan.value
    assert lib.kws_resample_plan_destroy(plan) == 0 and lib.kws_resample_plan_destroy(None) == 0
