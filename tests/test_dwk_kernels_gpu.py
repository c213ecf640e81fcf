"""kws_dwconvk_* (csrc/dwconvk.hip) called directly, against float64 NumPy (tests/oracle_blocks.py dw_fwd / dw_bwd): the general
depthwise convolution forward, backward and finalize on the six conv_1d_gru geometries and on odd ones (k = 1, k = 64 at stride
16, stride > k, uncovered input rows, C = 1 / 4 / 20 / 448, the direct kernels' k / s > 8), with and without a BatchNorm table
(some scales negative); and the one-channel pointwise pair kws_dwconvk_pw1_*.

Bars are derived from float32 arithmetic, u = 2^-24, and do not depend on the summation order:
  z      a sum of k products of float32 values whose activation carries up to 2 roundings: (k + 4) u sum_j |w_j| |a_j|
  g      the same form over the contributing taps: (k + 4) u sum |w_j| |dz_t|
  sums   n terms in any order: n u sum |terms|, plus the terms' own error (the bar of g, or 4 u |term| for a product of an
         activation / xhat computed in float32)
The ReLU6 gate is compared only where float64 bn(y) is farther than 1e-5 from 0 and from 6 (the excluded share must stay under
0.1 %); the reduced sums take the gate as the device decides it (one fused multiply-add rounded to float32)."""
import numpy as np
import pytest
import torch

from speech_recognition_amd import _lib
from dwk_oracle import LADDER, SPEC
from oracle_blocks import dw_bwd, dw_fwd

pytestmark = pytest.mark.gpu

U = 2.0 ** -24
GUARD = 4096
WIDTHS = [1, 128, 256, 384, 448, 512]
# (B, L_in, C, k, s, pad_l, L_out, bn)
MODEL_CASES = [(3, L, WIDTHS[i], SPEC[i][1], SPEC[i][2], pl, Lo, i > 0) for i, (L, pl, Lo) in enumerate(LADDER)]
ODD_CASES = [(2, 37, 4, 1, 3, 0, 13, True), (2, 300, 20, 64, 16, 24, 19, True), (2, 50, 8, 3, 5, 1, 10, True),
             (2, 90, 448, 7, 4, 2, 20, True), (1, 100, 4, 64, 1, 31, 100, True), (2, 500, 1, 64, 16, 10, 30, True),
             (2, 70, 12, 33, 3, 16, 24, False), (3, 1000, 128, 31, 4, 13, 250, False), (2, 16000, 1, 63, 16, 23, 1000, True),
             (2, 40, 20, 5, 2, 1, 20, False), (5, 63, 384, 7, 4, 2, 16, True)]
CASES = MODEL_CASES + ODD_CASES


def _guarded(n):
    buf = torch.full((n + 2 * GUARD,), float('nan'), dtype=torch.float32, device='cuda')
    return buf, buf[GUARD:GUARD + n]


def _guards_intact(buf, n):
    return bool(torch.isnan(buf[:GUARD]).all()) and bool(torch.isnan(buf[GUARD + n:]).all())


def _inputs(B, L, C, k, Lout, bn, seed):
    rng = np.random.RandomState(seed)
    y = rng.randn(B, L, C).astype(np.float32)
    w = (rng.randn(k, C) / np.sqrt(k)).astype(np.float32)
    dz = rng.randn(B, Lout, C).astype(np.float32)
    tab = None
    if bn:
        scale = (1.0 + 0.1 * rng.randn(C)) * np.where(rng.rand(C) < 0.35, -1.0, 1.0)
        if C > 1:
            scale[0] = -abs(scale[0])
        tab = np.concatenate([scale, 0.5 + 0.3 * rng.randn(C), 0.3 * rng.randn(C), 0.5 + rng.rand(C)]).astype(np.float32)
    return y, w, dz, tab


def _act64(y, tab, C):
    """float64 activation, float64 pre-activation, and the gate as the device decides it (fma rounded to float32)."""
    y64 = y.astype(np.float64)
    if tab is None:
        return y64, None, np.ones(y.shape)
    pre = y64 * tab[:C].astype(np.float64) + tab[C:2 * C].astype(np.float64)
    pre32 = pre.astype(np.float32)
    return np.clip(pre, 0, 6), pre, ((pre32 > 0) & (pre32 <= 6)).astype(np.float64)


def _fwd(y, tab, w, B, L, Lout, C, k, s, pad_l):
    yd, wd = torch.from_numpy(y).cuda(), torch.from_numpy(w).cuda()
    td = torch.from_numpy(tab).cuda() if tab is not None else None
    buf, z = _guarded(B * Lout * C)
    _lib.call("kws_dwconvk_fwd_f32", _lib.ptr(yd), _lib.ptr(td), _lib.ptr(wd), _lib.ptr(z), B, L, Lout, C, k, s, pad_l,
              _lib.stream_ptr())
    torch.cuda.synchronize()
    return buf, z


def _bwd(y, tab, w, dz, B, L, Lout, C, k, s, pad_l):
    lib = _lib.load()
    yd, wd, dzd = torch.from_numpy(y).cuda(), torch.from_numpy(w).cuda(), torch.from_numpy(dz).cuda()
    td = torch.from_numpy(tab).cuda() if tab is not None else None
    rows = lib.kws_dwconvk_bwd_part_rows(B, L, C, k, s)
    assert rows > 0 and lib.kws_dwconvk_bwd_part_floats(B, L, C, k, s) == rows * (2 + k) * C
    gbuf, g = _guarded(B * L * C)
    pbuf, part = _guarded(rows * (2 + k) * C)
    _lib.call("kws_dwconvk_bwd_f32", _lib.ptr(dzd), _lib.ptr(yd), _lib.ptr(td), _lib.ptr(wd), _lib.ptr(g), _lib.ptr(part), B, L, Lout,
              C, k, s, pad_l, _lib.stream_ptr())
    fbuf, fin = _guarded((k + 4) * C)
    dw, dgamma, dbeta, coef = fin[:k * C], fin[k * C:(k + 1) * C], fin[(k + 1) * C:(k + 2) * C], fin[(k + 2) * C:]
    _lib.call("kws_dwconvk_bwd_finalize", _lib.ptr(part), rows, B * L, C, k, _lib.ptr(dw), _lib.ptr(dgamma), _lib.ptr(dbeta),
              _lib.ptr(coef), _lib.stream_ptr())
    torch.cuda.synchronize()
    assert _guards_intact(gbuf, g.numel()) and _guards_intact(pbuf, part.numel()) and _guards_intact(fbuf, fin.numel())
    return g, part, rows, dw, dgamma, dbeta, coef


@pytest.mark.parametrize("B,L,C,k,s,pad_l,Lout,bn", CASES)
def test_forward_matches_float64(B, L, C, k, s, pad_l, Lout, bn):
    y, w, _, tab = _inputs(B, L, C, k, Lout, bn, 7 * L + C + k)
    buf, z = _fwd(y, tab, w, B, L, Lout, C, k, s, pad_l)
    a, _, _ = _act64(y, tab, C)
    w64 = w.astype(np.float64)
    ref = dw_fwd(a, w64, s, pad_l, Lout)
    bar = (k + 4) * U * dw_fwd(np.abs(a), np.abs(w64), s, pad_l, Lout)
    got = z.cpu().numpy().reshape(ref.shape).astype(np.float64)
    err = np.abs(got - ref)
    print("dwconvk fwd %s: worst error / bar %.3g" % ((B, L, C, k, s, pad_l, Lout, bn), (err / np.maximum(bar, 1e-300)).max()))
    assert (err <= bar).all()
    assert _guards_intact(buf, z.numel())
    # negative controls: reversed taps, and pad_l off by one (the odd SAME sample on the left)
    if k >= 3:
        wrong = dw_fwd(a, w64[::-1], s, pad_l, Lout)
        assert (np.abs(got - wrong) / np.maximum(bar, 1e-300)).max() > 100
    if pad_l + 1 < k and s * (Lout - 1) + k - (pad_l + 1) >= 1:
        wrong = dw_fwd(a, w64, s, pad_l + 1, Lout)
        assert (np.abs(got - wrong) / np.maximum(bar, 1e-300)).max() > 100


@pytest.mark.parametrize("B,L,C,k,s,pad_l,Lout,bn", CASES)
def test_backward_and_finalize_match_float64(B, L, C, k, s, pad_l, Lout, bn):
    y, w, dz, tab = _inputs(B, L, C, k, Lout, bn, 13 * L + C + k)
    g, part, rows, dw, dgamma, dbeta, coef = _bwd(y, tab, w, dz, B, L, Lout, C, k, s, pad_l)
    a, pre, gate = _act64(y, tab, C)
    w64, dz64 = w.astype(np.float64), dz.astype(np.float64)
    da, dw_ref = dw_bwd(dz64, a, w64, s, pad_l)
    da_abs, dw_abs = dw_bwd(np.abs(dz64), np.abs(a), np.abs(w64), s, pad_l)
    cover = dw_bwd(np.ones_like(dz64), a, np.ones_like(w64), s, pad_l)[0]
    got = g.cpu().numpy().reshape(B, L, C).astype(np.float64)
    ref = da * gate
    bar_g = (k + 4) * U * da_abs
    far = np.ones(y.shape, bool)
    if bn:
        far = (np.abs(pre) > 1e-5) & (np.abs(pre - 6) > 1e-5)
        assert 1.0 - far.mean() < 1e-3
        f64gate = ((pre > 0) & (pre <= 6)).astype(np.float64)
        assert (f64gate[far] == gate[far]).all()
    err = np.abs(got - ref)
    print("dwconvk bwd %s: g worst error / bar %.3g" % ((B, L, C, k, s, pad_l, Lout, bn), (err[far] / np.maximum(bar_g[far], 1e-300)).max()))
    assert (err[far] <= bar_g[far]).all()
    assert (got[cover == 0] == 0).all()                       # rows no window reaches: exact zeros
    if s > k or s * (Lout - 1) + k - pad_l < L:
        assert (cover == 0).any()
    # tap gradients
    n = B * Lout
    got_dw = dw.cpu().numpy().reshape(k, C).astype(np.float64)
    bar_dw = (n + 4) * U * dw_abs
    assert (np.abs(got_dw - dw_ref) <= bar_dw).all(), (np.abs(got_dw - dw_ref) / np.maximum(bar_dw, 1e-300)).max()
    folded = part.cpu().numpy().astype(np.float64).reshape(rows, 2 + k, C).sum(axis=0)
    assert (np.abs(folded[2:] - dw_ref) <= bar_dw).all()
    if not bn:
        assert not folded[:2].any()                           # no gate, no BatchNorm sums: the part carries only the taps
        return
    # BatchNorm sums on the device's own gate decisions
    n = B * L
    xhat = (y.astype(np.float64) - tab[2 * C:3 * C].astype(np.float64)) * tab[3 * C:].astype(np.float64)
    sg, sgx = ref.sum(axis=(0, 1)), (ref * xhat).sum(axis=(0, 1))
    bar_sg = n * U * np.abs(ref).sum(axis=(0, 1)) + (bar_g * gate).sum(axis=(0, 1))
    bar_sgx = (n + 4) * U * np.abs(ref * xhat).sum(axis=(0, 1)) + (bar_g * gate * np.abs(xhat)).sum(axis=(0, 1))
    got_b, got_g = dbeta.cpu().numpy().astype(np.float64), dgamma.cpu().numpy().astype(np.float64)
    assert (np.abs(got_b - sg) <= bar_sg).all() and (np.abs(got_g - sgx) <= bar_sgx).all()
    cf = coef.cpu().numpy().astype(np.float64)
    assert (np.abs(cf[:C] * n - sg) <= bar_sg + U * np.abs(sg)).all() and (np.abs(cf[C:] * n - sgx) <= bar_sgx + U * np.abs(sgx)).all()


@pytest.mark.parametrize("B,L,C,k,s,pad_l,Lout,bn", [CASES[1], CASES[0], CASES[7], CASES[11], CASES[12]])
def test_repeated_launches_are_bit_identical(B, L, C, k, s, pad_l, Lout, bn):
    y, w, dz, tab = _inputs(B, L, C, k, Lout, bn, 5)
    _, z1 = _fwd(y, tab, w, B, L, Lout, C, k, s, pad_l)
    _, z2 = _fwd(y, tab, w, B, L, Lout, C, k, s, pad_l)
    assert torch.equal(z1, z2)
    r1 = _bwd(y, tab, w, dz, B, L, Lout, C, k, s, pad_l)
    r2 = _bwd(y, tab, w, dz, B, L, Lout, C, k, s, pad_l)
    for t1, t2 in zip((r1[0], r1[1]) + r1[3:], (r2[0], r2[1]) + r2[3:]):
        assert torch.equal(t1, t2)


@pytest.mark.parametrize("M,N", [(3000, 128), (700, 4), (513, 256)])
def test_pointwise_one_channel_pair(M, N):
    lib = _lib.load()
    rng = np.random.RandomState(M + N)
    z, p, dy = rng.randn(M).astype(np.float32), rng.randn(N).astype(np.float32), rng.randn(M, N).astype(np.float32)
    zd, pd, dyd = torch.from_numpy(z).cuda(), torch.from_numpy(p).cuda(), torch.from_numpy(dy).cuda()
    rows = lib.kws_dwconvk_pw1_stats_rows(M)
    ybuf, yv = _guarded(M * N)
    sbuf, st = _guarded(rows * 2 * N)
    _lib.call("kws_dwconvk_pw1_fwd_f32", _lib.ptr(zd), _lib.ptr(pd), _lib.ptr(yv), M, N, _lib.ptr(st), _lib.stream_ptr())
    wsbuf, ws = _guarded(lib.kws_dwconvk_pw1_bwd_workspace_floats(M, N))
    obuf, out = _guarded(M + N)
    dzv, dpv = out[:M], out[M:]
    _lib.call("kws_dwconvk_pw1_bwd_f32", _lib.ptr(dyd), _lib.ptr(zd), _lib.ptr(pd), _lib.ptr(dzv), _lib.ptr(dpv), M, N, _lib.ptr(ws),
              _lib.stream_ptr())
    torch.cuda.synchronize()
    for buf, t in ((ybuf, yv), (sbuf, st), (wsbuf, ws), (obuf, out)):
        assert _guards_intact(buf, t.numel())
    z64, p64, dy64 = z.astype(np.float64), p.astype(np.float64), dy.astype(np.float64)
    ref = z64[:, None] * p64[None, :]
    got = yv.cpu().numpy().reshape(M, N).astype(np.float64)
    assert (np.abs(got - ref) <= U * np.abs(ref)).all()                      # one product, one rounding
    sums = st.cpu().numpy().astype(np.float64).reshape(rows, 2, N).sum(axis=0)
    assert (np.abs(sums[0] - ref.sum(0)) <= (M + 1) * U * np.abs(ref).sum(0)).all()
    assert (np.abs(sums[1] - (ref ** 2).sum(0)) <= (M + 3) * U * (ref ** 2).sum(0)).all()
    assert (np.abs(dzv.cpu().numpy() - dy64 @ p64) <= (N + 1) * U * (np.abs(dy64) @ np.abs(p64))).all()
    assert (np.abs(dpv.cpu().numpy() - z64 @ dy64) <= (M + 1) * U * (np.abs(z64) @ np.abs(dy64))).all()
