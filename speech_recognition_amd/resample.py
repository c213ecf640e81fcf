"""Rational polyphase resampling on the device (csrc/resample.hip, kws_resample_*): wavs of any sample rate at the model's rate.

The definition is `scipy.signal.resample_poly(x, up, down)` at its defaults (Kaiser(5.0) windowed sinc of 20 max(up, down) + 1
taps, zeros outside the row) with up / down = rate_out / rate_in in lowest terms; equal rates are a copy.  int16 input is
resampled as integers and comes back as int16, rounded half to even and saturated; float32 input comes back as float32."""
import ctypes

import numpy as np
import torch

from . import _lib
from .device_array import DeviceArray, as_device_f32

_PLANS = {}


def _plan(rate_in, rate_out, device=None):
    """The device table of one rate pair, made once per (pair, device)."""
    dev = torch.device(device if device is not None else "cuda:%d" % torch.cuda.current_device())
    key = (int(rate_in), int(rate_out), dev.index or 0)
    if key not in _PLANS:
        plan = ctypes.c_void_p()
        with torch.cuda.device(dev):
            _lib.check(_lib.load().kws_resample_plan_create(key[0], key[1], ctypes.byref(plan)), "kws_resample_plan_create")
        _PLANS[key] = plan
    return _PLANS[key]


def design(rate_in, rate_out):
    """(up, down, half, taps_per_phase) of a rate pair (host only); ValueError for rates the library refuses."""
    v = [ctypes.c_int() for _ in range(4)]
    if _lib.load().kws_resample_design(int(rate_in), int(rate_out), *[ctypes.byref(c) for c in v]) != 0:
        raise ValueError("cannot resample %r -> %r Hz: rates must be >= 1 with max(up, down) <= 65536" % (rate_in, rate_out))
    return tuple(c.value for c in v)


def resampled_samples(n, rate_in, rate_out):
    """Length of n samples after resampling: ceil(n up / down) (host only)."""
    design(rate_in, rate_out)
    r = _lib.load().kws_resample_out_samples(int(rate_in), int(rate_out), int(n))
    if r < 0:
        raise ValueError("resampled_samples: n=%r" % (n,))
    return int(r)


def taps(rate_in, rate_out):
    """The float32 prototype filter the kernels multiply with, in natural order (host only)."""
    half = design(rate_in, rate_out)[2]
    h = np.zeros(2 * half + 1, dtype=np.float32)
    _lib.call("kws_resample_taps", int(rate_in), int(rate_out), h.ctypes.data_as(ctypes.c_void_p), h.size)
    return h


def resample_rows(x, lengths, rate_in, rate_out, keep, want_i16=True, want_f32=False):
    """One launch over a device tensor x [B, pitch] (int16 or float32, contiguous) whose row b holds lengths[b] samples
    (`lengths`: device int32 [B], or None = every row is full).  Returns (out_i16 or None, out_f32 or None), each [B, keep]."""
    B, pitch = x.shape
    i16 = x.dtype == torch.int16
    plan = _plan(rate_in, rate_out, x.device)
    o16 = torch.empty((B, keep), dtype=torch.int16, device=x.device) if i16 and want_i16 else None
    o32 = torch.empty((B, keep), dtype=torch.float32, device=x.device) if (want_f32 or not i16) else None
    with torch.cuda.device(x.device):
        s = _lib.stream_ptr()
        if i16:
            _lib.call("kws_resample_i16", plan, _lib.ptr(x), pitch, _lib.ptr(lengths), pitch, _lib.ptr(o16), _lib.ptr(o32), B,
                      keep, s)
        else:
            _lib.call("kws_resample_f32", plan, _lib.ptr(x), pitch, _lib.ptr(lengths), pitch, _lib.ptr(o32), B, keep, s)
    return o16, o32


def resample(x, rate_in, rate_out, lengths=None, keep=None):
    """x: int16 or float32 samples, 1-D or [B, L] (array / tensor / DeviceArray; other float types are taken as float32).
    lengths: optional [B] valid samples per row (the rest of a row is never read).  Returns a CUDA tensor of x's kind,
    [B, keep] ([1, keep] for 1-D input): the first `keep` resampled samples, zeros behind a row's resampled length;
    keep defaults to resampled_samples(L, rate_in, rate_out)."""
    dev = torch.device("cuda", torch.cuda.current_device())
    if isinstance(x, DeviceArray):
        xd = as_device_f32(x, x.tensor.device)
    elif torch.is_tensor(x):
        xd = x if x.dtype == torch.int16 else x.to(torch.float32)
        xd = xd if xd.is_cuda else xd.to(dev)
    else:
        a = np.asarray(x)
        xd = torch.from_numpy(np.ascontiguousarray(a if a.dtype == np.int16 else a.astype(np.float32))).to(dev)
    if xd.dim() == 1:
        xd = xd.reshape(1, -1)
    if xd.dim() != 2:
        raise ValueError("resample: x must be 1-D or [B, L]")
    xd = xd.contiguous()
    B, L = xd.shape
    if keep is None:
        keep = resampled_samples(L, rate_in, rate_out)
    else:
        design(rate_in, rate_out)
    ld = None
    if lengths is not None:
        ld = torch.as_tensor(np.asarray(lengths.cpu() if torch.is_tensor(lengths) else lengths).astype(np.int32)).to(xd.device)
        if ld.shape != (B,):
            raise ValueError("resample: lengths must have one entry per row")
    o16, o32 = resample_rows(xd, ld, rate_in, rate_out, int(keep))
    return o16 if o16 is not None else o32
