"""kws_pool3s2_fwd_f32 / kws_pool3s2_bwd_f32 (csrc/pool.hip, the kernel set it shares with kws_pool3s2_same_*: VALID is
pad_left = 0 and its own window count) called directly, against float64 NumPy: MaxPool1D(3, strides=2, 'valid') over
relu6(bn(y)), forward and gather-form backward with the BatchNorm partial sums.

The float64 reference takes the device's own decisions where float32 rounding could flip them: activations are recomputed as
the device does (one fused multiply-add per element, rounded to float32), and windows / gates are decided on those.  Inputs
are quantised so that exact ties between unsaturated activations exist (first-max-wins becomes observable: tied saturated
values have shut gates), a share of the BN scales is negative, and every output buffer sits between guard bands.

Bars: z is a selection of float32 values the reference recomputes the same way: exact.  g is a sum of at most two float32
terms times a 0 / 1 gate: one rounding, 2^-23 relative to the larger term (bar 2e-7 of the tensor's maximum).  The folded sums
add up to B * L float32 terms per channel in float32 within a workgroup: relative error up to about sqrt(B L) 2^-24 for
random signs; bar 1e-5 of the sum of magnitudes (B L <= 1.3e5 here: 2e-5 would be the worst case of a plain sum)."""
import numpy as np
import pytest
import torch

import pool_oracle
from speech_recognition_amd import _lib
from pool_oracle import pool_len

pytestmark = pytest.mark.gpu

GUARD = 4096
SHAPES = [(1, 7, 32), (1, 8, 48), (3, 16, 96), (2, 95, 128), (5, 194, 160), (4, 41, 192), (64, 798, 48), (256, 91, 320),
          (1, 3, 256), (2, 4, 32), (1, 5, 1024), (2, 8, 1024)]   # C = 1024: one run per workgroup (R = 1)


def _guarded(n, fill=np.nan):
    buf = torch.full((n + 2 * GUARD,), float(fill), dtype=torch.float32, device='cuda')
    return buf, buf[GUARD:GUARD + n]


def _guards_intact(buf, n):
    return bool(torch.isnan(buf[:GUARD]).all()) and bool(torch.isnan(buf[GUARD + n:]).all())


def _inputs(B, L, C, seed):
    rng = np.random.RandomState(seed)
    y = (rng.randint(-12, 13, size=(B, L, C)) * 0.25).astype(np.float32)     # quantised: exact ties, exact products
    scale = np.where(rng.rand(C) < 0.35, -1.0, 1.0) * rng.choice([0.5, 1.0, 2.0], C)
    shift = rng.choice([0.0, 0.5, 1.0, 3.0], C)
    mean = rng.randn(C) * 0.3
    rstd = 0.5 + rng.rand(C)
    bn = np.concatenate([scale, shift, mean, rstd]).astype(np.float32)
    dz = rng.randn(B, pool_len(L), C).astype(np.float32)
    return y, bn, dz


def _act(y, bn, C):
    """relu6(fma(y, scale, shift)) rounded to float32 as on the device (the double product-sum is exact: one rounding)."""
    pre = (y.astype(np.float64) * bn[:C].astype(np.float64) + bn[C:2 * C].astype(np.float64)).astype(np.float32)
    return pre, np.clip(pre, 0, 6)


def _run_fwd(y, bn, B, L, C):
    yd, bd = torch.from_numpy(y).cuda(), torch.from_numpy(bn).cuda()
    n = B * pool_len(L) * C
    buf, z = _guarded(n)
    _lib.call("kws_pool3s2_fwd_f32", _lib.ptr(yd), _lib.ptr(bd), _lib.ptr(z), B, L, C, _lib.stream_ptr())
    torch.cuda.synchronize()
    return buf, z


def _run_bwd(y, bn, dz, B, L, C):
    lib = _lib.load()
    yd, bd, dzd = torch.from_numpy(y).cuda(), torch.from_numpy(bn).cuda(), torch.from_numpy(dz).cuda()
    rows = lib.kws_pool3s2_bwd_part_rows(B, L, C)
    assert rows > 0 and lib.kws_pool3s2_bwd_part_floats(B, L, C) == rows * 2 * C
    gbuf, g = _guarded(B * L * C)
    pbuf, part = _guarded(rows * 2 * C)
    _lib.call("kws_pool3s2_bwd_f32", _lib.ptr(dzd), _lib.ptr(yd), _lib.ptr(bd), _lib.ptr(g), _lib.ptr(part), B, L, C,
              _lib.stream_ptr())
    torch.cuda.synchronize()
    return gbuf, g, pbuf, part, rows


def _reference_bwd(y, bn, dz, L, C, last=False, on_raw=False, gate=True):
    pre, a = _act(y, bn, C)
    ind = pool_oracle.argmax(y.astype(np.float64) if on_raw else a, pool_len(L), 0, last=last)
    da = pool_oracle.bwd(dz.astype(np.float64), ind, L, 0)
    g = da * ((pre > 0) & (pre <= 6)) if gate else da
    xhat = (y.astype(np.float64) - bn[2 * C:3 * C].astype(np.float64)) * bn[3 * C:].astype(np.float64)
    return g, g.sum(axis=(0, 1)), (g * xhat).sum(axis=(0, 1)), (np.abs(g).sum(axis=(0, 1)), np.abs(g * xhat).sum(axis=(0, 1)))


def test_out_len():
    lib = _lib.load()
    assert [lib.kws_pool3s2_out_len(L) for L in (2, 3, 4, 5, 798, 1598, 16)] == [0, 1, 1, 2, 398, 798, 7]


@pytest.mark.parametrize("B,L,C", SHAPES)
def test_forward_matches_float64(B, L, C):
    y, bn, _ = _inputs(B, L, C, 11 * L + C)
    assert (bn[:C] < 0).any()
    buf, z = _run_fwd(y, bn, B, L, C)
    _, a = _act(y, bn, C)
    ref = pool_oracle.fwd(a, pool_oracle.argmax(a, pool_len(L), 0), 0)
    got = z.cpu().numpy().reshape(ref.shape)
    np.testing.assert_array_equal(got, ref)
    assert _guards_intact(buf, z.numel())
    # pooling the raw output and activating afterwards is a different function here (negative scales)
    wrong = pool_oracle.fwd(a, pool_oracle.argmax(y.astype(np.float64), pool_len(L), 0), 0)
    assert np.abs(wrong - ref).max() > 0.1


@pytest.mark.parametrize("B,L,C", SHAPES)
def test_backward_matches_float64(B, L, C):
    y, bn, dz = _inputs(B, L, C, 13 * L + C)
    gbuf, g, pbuf, part, rows = _run_bwd(y, bn, dz, B, L, C)
    ref, s, sx, (sa, sxa) = _reference_bwd(y, bn, dz, L, C)
    got = g.cpu().numpy().reshape(ref.shape).astype(np.float64)
    gerr = np.abs(got - ref).max() / np.abs(ref).max()
    fold = part.cpu().numpy().astype(np.float64).reshape(rows, 2, C).sum(axis=0)
    serr = (np.abs(fold[0] - s) / np.maximum(sa, 1e-30)).max()
    sxerr = (np.abs(fold[1] - sx) / np.maximum(sxa, 1e-30)).max()
    print("pool bwd B=%d L=%d C=%d: g %.3g, sum g %.3g, sum g xhat %.3g" % (B, L, C, gerr, serr, sxerr))
    assert gerr < 2e-7
    assert serr < 1e-5 and sxerr < 1e-5
    if L % 2 == 0:
        assert not got[:, -1].any()                      # the row no window covers: exact zeros
    assert _guards_intact(gbuf, g.numel()) and _guards_intact(pbuf, part.numel())


@pytest.mark.parametrize("B,L,C", [(2, 4, 32), (1, 8, 48), (3, 16, 96)])
def test_same_padding_of_an_even_length_starts_with_the_valid_windows(B, L, C):
    """Even L: SAME has pad_left = 0, so its first (L - 3) / 2 + 1 windows are VALID's; both entry points run one kernel."""
    y, bn, _ = _inputs(B, L, C, 17 * L + C)
    _, zv = _run_fwd(y, bn, B, L, C)
    lib = _lib.load()
    Ls = lib.kws_pool3s2_same_out_len(L)
    assert Ls == pool_len(L) + 1
    yd, bd = torch.from_numpy(y).cuda(), torch.from_numpy(bn).cuda()
    buf, zs = _guarded(B * Ls * C)
    _lib.call("kws_pool3s2_same_fwd_f32", _lib.ptr(yd), _lib.ptr(bd), _lib.ptr(zs), B, L, C, _lib.stream_ptr())
    torch.cuda.synchronize()
    assert torch.equal(zs.view(B, Ls, C)[:, :pool_len(L)], zv.view(B, pool_len(L), C))
    assert _guards_intact(buf, zs.numel())


def test_backward_negative_controls():
    """The same bar breaks for last-max-wins routing, for winners picked before the activation and for a missing ReLU6 gate."""
    B, L, C = 5, 194, 160
    y, bn, dz = _inputs(B, L, C, 77)
    _, g, _, _, _ = _run_bwd(y, bn, dz, B, L, C)
    got = g.cpu().numpy().reshape(B, L, C).astype(np.float64)
    for kw in ({'last': True}, {'on_raw': True}, {'gate': False}):
        ref = _reference_bwd(y, bn, dz, L, C, **kw)[0]
        assert np.abs(got - ref).max() / np.abs(ref).max() > 1e-2, kw


@pytest.mark.parametrize("B,L,C", [(64, 798, 48), (5, 194, 160)])
def test_repeated_launches_are_bit_identical(B, L, C):
    y, bn, dz = _inputs(B, L, C, 5)
    _, z1 = _run_fwd(y, bn, B, L, C)
    _, z2 = _run_fwd(y, bn, B, L, C)
    assert torch.equal(z1, z2)
    _, g1, _, p1, _ = _run_bwd(y, bn, dz, B, L, C)
    _, g2, _, p2, _ = _run_bwd(y, bn, dz, B, L, C)
    assert torch.equal(g1, g2) and torch.equal(p1, p2)


def test_bad_arguments_are_refused():
    lib = _lib.load()
    t = torch.zeros(4096, device='cuda')
    for B, L, C in ((0, 8, 32), (1, 2, 32), (1, 8, 30), (1, 8, 2048)):
        assert lib.kws_pool3s2_fwd_f32(_lib.ptr(t), _lib.ptr(t), _lib.ptr(t), B, L, C, _lib.stream_ptr()) != 0
        assert lib.kws_pool3s2_bwd_f32(_lib.ptr(t), _lib.ptr(t), _lib.ptr(t), _lib.ptr(t), _lib.ptr(t), B, L, C,
                                       _lib.stream_ptr()) != 0
        assert lib.kws_pool3s2_bwd_part_rows(B, L, C) == 0
    assert lib.kws_pool3s2_fwd_f32(None, _lib.ptr(t), _lib.ptr(t), 1, 8, 32, _lib.stream_ptr()) != 0
