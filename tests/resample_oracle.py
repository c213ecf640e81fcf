"""float64 oracle of the device resampler (csrc/resample.hip): scipy.signal.resample_poly(x, up, down) at its defaults,
restated from its definition in NumPy so that the GPU tests need no scipy (tests/test_resample_cpu.py cross-checks the two).

  g = gcd(rate_out, rate_in), up = rate_out / g, down = rate_in / g, mx = max(up, down), half = 10 mx
  h[j] = up w[j] fc sinc(fc (j - half)) / S, 2 half + 1 taps, fc = 1 / mx, w = np.kaiser(2 half + 1, 5.0), S = sum of w fc sinc
  y[n] = sum_j h[j] xu[n down + half - j], xu[i up] = x[i], zero elsewhere; n_out = ceil(n_in up / down)
"""
import math

import numpy as np


def design(rate_in, rate_out):
    """(up, down, half, T): T = taps that meet a sample per output."""
    g = math.gcd(int(rate_in), int(rate_out))
    up, down = int(rate_out) // g, int(rate_in) // g
    half = 10 * max(up, down)
    return up, down, half, -(-(2 * half + 1) // up)


_TAPS = {}


def taps(rate_in, rate_out):
    """The prototype h[0 .. 2 half] in float64."""
    key = design(rate_in, rate_out)[:2]
    if key not in _TAPS:
        up, down, half, _ = design(rate_in, rate_out)
        fc = 1.0 / max(up, down)
        m = np.arange(2 * half + 1, dtype=np.float64) - half
        h = np.kaiser(2 * half + 1, 5.0) * fc * np.sinc(fc * m)
        _TAPS[key] = up * h / h.sum()
    return _TAPS[key]


def out_samples(n_in, rate_in, rate_out):
    up, down, _, _ = design(rate_in, rate_out)
    return -(-(int(n_in) * up) // down)


def terms(n_in, rate_in, rate_out, n_first=0, n_stop=None):
    """For the outputs [n_first, n_stop) of a row of n_in samples: (j, i, ok) [n, T] - output n sums h[j] x[i] where ok."""
    up, down, half, T = design(rate_in, rate_out)
    n_out = out_samples(n_in, rate_in, rate_out)
    n = np.arange(n_first, n_out if n_stop is None else min(n_stop, n_out), dtype=np.int64)
    p = n * down + half
    q, r = p // up, p % up
    k = np.arange(T, dtype=np.int64)
    j = r[:, None] + k[None, :] * up
    i = q[:, None] - k[None, :]
    ok = (j <= 2 * half) & (i >= 0) & (i < n_in)
    return np.where(ok, j, 0), np.where(ok, i, 0), ok


def resample(x, rate_in, rate_out, h=None, with_abs=False):
    """y64 [n_out] of one row x (any real dtype; computed in float64) with the taps `h` (default: the float64 design).
    with_abs: also sum_j |h[j] x[i_j]| per output, the scale of the float32 error bound."""
    x = np.asarray(x, dtype=np.float64).reshape(-1)
    if design(rate_in, rate_out)[:2] == (1, 1):
        return (x.copy(), np.abs(x)) if with_abs else x.copy()
    h = taps(rate_in, rate_out) if h is None else np.asarray(h, dtype=np.float64)
    n_out = out_samples(len(x), rate_in, rate_out)
    y, ya = np.zeros(n_out), np.zeros(n_out)
    for s in range(0, n_out, 8192):                    # bounded [8192, T] temporaries for the one long row
        j, i, ok = terms(len(x), rate_in, rate_out, s, s + 8192)
        t = np.where(ok, h[j] * x[i], 0.0)
        y[s:s + 8192] = t.sum(1)
        ya[s:s + 8192] = np.abs(t).sum(1)
    return (y, ya) if with_abs else y


def to_int16(v):
    """The staged int16 rule: clamp(rint(v), -32768, 32767), round half to even."""
    return np.clip(np.rint(v), -32768, 32767).astype(np.int16)
