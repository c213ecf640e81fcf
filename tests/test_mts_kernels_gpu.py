"""kws_pool3s2_same_* (csrc/pool.hip) and kws_stem_* (csrc/stem.hip) called directly, against float64 NumPy
(tests/pool_oracle.py, tests/mts_cases.py stem_reference), on the conv_1d_multi_time_sliced geometries and on small odd
ones.  Outputs sit in NaN-guarded buffers.

Bars are derived from float32 arithmetic, u = 2^-24, and do not depend on the summation order: a sum of n products is bounded by
(n + 4) u sum |terms|.
  pool fwd   exact: the maximum of float32 values is one of them; the activation is one fused multiply-add rounded to float32
  pool g     a sum of at most two dz values (n = 2), times a gate of 0 or 1
  pool sums  the B L terms of a column in any order: n u sum |g|, plus the terms' own error (g's bar; 4 u |g xhat| for xhat and
             the product computed in float32); on the device's own gate and arg-max decisions
  stem y     3 C triple products w p x: (3 C + 4) u sum |w| |p| |x|
  stem stats M = B (L - 2) values of y in any order: M u sum |y| + sum of y's bars; the squares (M + 4) u sum y^2 + 2 |y| bar
  stem dp    B (L - 2) products of z (3 products) and dy: (M + 3 + 4) u sum |z| |dy|;  dw alike with the N products of dz
g is compared where the float64 pre-activation is farther than 1e-5 from 0 and 6 and the window's two largest activations differ
by more than 1e-6 (tests/mts_cases.py pool_compared; the excluded share stays under 0.1 %, checked on the CPU too)."""
import numpy as np
import pytest
import torch

from speech_recognition_amd import _lib
from mts_cases import (POOL_CASES, STEM_CASES, pool_compared, pool_inputs, pool_pre, stem_inputs, stem_reference)
import pool_oracle

pytestmark = pytest.mark.gpu

U = 2.0 ** -24
GUARD = 4096


def _guarded(n):
    buf = torch.full((n + 2 * GUARD,), float('nan'), dtype=torch.float32, device='cuda')
    return buf, buf[GUARD:GUARD + n]


def _guards_intact(buf, n):
    return bool(torch.isnan(buf[:GUARD]).all()) and bool(torch.isnan(buf[GUARD + n:]).all())


# ---- SAME pool -------------------------------------------------------------------------------------------------------------------
def _pool_fwd(y, tab):
    B, L, C = y.shape
    lib = _lib.load()
    Lp = lib.kws_pool3s2_same_out_len(L)
    assert Lp == pool_oracle.same_geometry(L)[0]
    yd, td = torch.from_numpy(y).cuda(), torch.from_numpy(tab).cuda()
    buf, z = _guarded(B * Lp * C)
    _lib.call("kws_pool3s2_same_fwd_f32", _lib.ptr(yd), _lib.ptr(td), _lib.ptr(z), B, L, C, _lib.stream_ptr())
    torch.cuda.synchronize()
    assert _guards_intact(buf, z.numel())
    return z


def _pool_bwd(y, tab, dz):
    B, L, C = y.shape
    lib = _lib.load()
    rows = lib.kws_pool3s2_same_bwd_part_rows(B, L, C)
    assert rows > 0 and lib.kws_pool3s2_same_bwd_part_floats(B, L, C) == rows * 2 * C
    yd, td, dzd = torch.from_numpy(y).cuda(), torch.from_numpy(tab).cuda(), torch.from_numpy(dz).cuda()
    gbuf, g = _guarded(B * L * C)
    pbuf, part = _guarded(rows * 2 * C)
    _lib.call("kws_pool3s2_same_bwd_f32", _lib.ptr(dzd), _lib.ptr(yd), _lib.ptr(td), _lib.ptr(g), _lib.ptr(part), B, L, C,
              _lib.stream_ptr())
    torch.cuda.synchronize()
    assert _guards_intact(gbuf, g.numel()) and _guards_intact(pbuf, part.numel())
    return g, part, rows


@pytest.mark.parametrize("B,L,C", POOL_CASES)
def test_pool_forward_is_exact(B, L, C):
    y, tab, _ = pool_inputs(B, L, C)
    z = _pool_fwd(y, tab)
    _, pre32 = pool_pre(y, tab)
    act = np.clip(pre32, 0, 6).astype(np.float64)          # the float32-rounded activations
    Lp, pad_l = pool_oracle.same_geometry(L)
    ref = pool_oracle.fwd(act, pool_oracle.argmax(act, Lp, pad_l), pad_l)
    got = z.cpu().numpy().reshape(B, Lp, C).astype(np.float64)
    assert np.array_equal(got, ref)
    # negative controls: pad_left off by one; the maximum taken before the activation (negative scales)
    if L > 2:     # (with two rows both paddings give the one window the same valid rows)
        wrong = pool_oracle.fwd(act, pool_oracle.argmax(act, Lp, 1 - pad_l), 1 - pad_l)
        assert not np.array_equal(got, wrong)
    if L > 3:
        raw = y.astype(np.float64)
        before = pool_oracle.fwd(act, pool_oracle.argmax(raw, Lp, pad_l), pad_l)
        assert not np.array_equal(got, before)


@pytest.mark.parametrize("B,L,C", POOL_CASES)
def test_pool_backward_matches_float64(B, L, C):
    y, tab, dz = pool_inputs(B, L, C)
    g, part, rows = _pool_bwd(y, tab, dz)
    got = g.cpu().numpy().reshape(B, L, C).astype(np.float64)
    assert not np.isnan(got).any()                                               # every element of g is written
    Lp, pad_l = pool_oracle.same_geometry(L)
    pre, pre32 = pool_pre(y, tab)
    dz64 = dz.astype(np.float64)
    # float64 decisions, compared away from kinks and ties
    ind = pool_oracle.argmax(np.clip(pre, 0, 6), Lp, pad_l)
    ref = pool_oracle.bwd(dz64, ind, L, pad_l) * ((pre > 0) & (pre <= 6))
    bar = (2 + 4) * U * pool_oracle.bwd(np.abs(dz64), ind, L, pad_l)
    cmp_ = pool_compared(y, tab)
    share = 1.0 - cmp_.mean()
    err = np.abs(got - ref)
    print("pool_same bwd %s: excluded %.3g %%, worst error / bar %.3g" %
          ((B, L, C), 100 * share, (err[cmp_] / np.maximum(bar[cmp_], 1e-300)).max()))
    assert share < 1e-3
    assert (err[cmp_] <= bar[cmp_]).all()
    # the device's own decisions: exact zeros where a row wins nothing or its gate is shut; the BatchNorm part rows
    act32 = np.clip(pre32, 0, 6).astype(np.float64)
    ind_d = pool_oracle.argmax(act32, Lp, pad_l)
    gate_d = ((pre32 > 0) & (pre32 <= 6)).astype(np.float64)
    ref_d = pool_oracle.bwd(dz64, ind_d, L, pad_l) * gate_d
    wins = pool_oracle.bwd(np.ones_like(dz64), ind_d, L, pad_l)
    assert (got[(wins == 0) | (gate_d == 0)] == 0).all()
    bar_d = (2 + 4) * U * pool_oracle.bwd(np.abs(dz64), ind_d, L, pad_l) * gate_d
    assert (np.abs(got - ref_d) <= bar_d).all()
    n = B * L
    xhat = (y.astype(np.float64) - tab[2 * C:3 * C].astype(np.float64)) * tab[3 * C:].astype(np.float64)
    sums = part.cpu().numpy().astype(np.float64).reshape(rows, 2, C).sum(axis=0)
    sg, sgx = ref_d.sum(axis=(0, 1)), (ref_d * xhat).sum(axis=(0, 1))
    bar_sg = n * U * np.abs(ref_d).sum(axis=(0, 1)) + bar_d.sum(axis=(0, 1))
    bar_sgx = (n + 4) * U * np.abs(ref_d * xhat).sum(axis=(0, 1)) + (bar_d * np.abs(xhat)).sum(axis=(0, 1))
    assert (np.abs(sums[0] - sg) <= bar_sg).all() and (np.abs(sums[1] - sgx) <= bar_sgx).all()
    # negative control: an oracle with pad_left off by one misses by far
    if L > 2:     # (with two rows both paddings give the one window the same valid rows)
        wrong = pool_oracle.bwd(dz64, pool_oracle.argmax(np.clip(pre, 0, 6), Lp, 1 - pad_l), L, 1 - pad_l) * ((pre > 0) & (pre <= 6))
        assert (np.abs(got - wrong)[cmp_] > 100 * np.maximum(bar[cmp_], U)).mean() > 0.05


def test_pool_first_maximum_wins_on_planted_ties():
    """Quantised activations strictly inside the open gate (1, 2, 3): ties abound, the first maximum of a window takes the
    gradient; a last-maximum-wins oracle misses."""
    B, L, C = 3, 37, 16
    rng = np.random.RandomState(4)
    y = rng.randint(1, 4, size=(B, L, C)).astype(np.float32)
    tab = np.concatenate([np.ones(C), np.zeros(C), np.zeros(C), np.ones(C)]).astype(np.float32)
    Lp, pad_l = pool_oracle.same_geometry(L)
    dz = rng.randn(B, Lp, C).astype(np.float32)
    g, _, _ = _pool_bwd(y, tab, dz)
    got = g.cpu().numpy().reshape(B, L, C).astype(np.float64)
    a, dz64 = y.astype(np.float64), dz.astype(np.float64)
    first = pool_oracle.bwd(dz64, pool_oracle.argmax(a, Lp, pad_l), L, pad_l)
    last = pool_oracle.bwd(dz64, pool_oracle.argmax(a, Lp, pad_l, last=True), L, pad_l)
    bar = (2 + 4) * U * pool_oracle.bwd(np.abs(dz64), pool_oracle.argmax(a, Lp, pad_l), L, pad_l)
    assert (np.abs(got - first) <= bar).all()
    assert np.abs(got - last).max() > 0.1
    for Lx in (2, 3, 20):       # and on both parities at the borders, where a window has a padding row
        yx = rng.randint(1, 4, size=(B, Lx, C)).astype(np.float32)
        Lpx, plx = pool_oracle.same_geometry(Lx)
        dzx = rng.randn(B, Lpx, C).astype(np.float32)
        gx = _pool_bwd(yx, tab, dzx)[0].cpu().numpy().reshape(B, Lx, C).astype(np.float64)
        refx = pool_oracle.bwd(dzx.astype(np.float64), pool_oracle.argmax(yx.astype(np.float64), Lpx, plx), Lx, plx)
        assert np.abs(gx - refx).max() <= 6 * U * np.abs(dzx).max() * 2


@pytest.mark.parametrize("B,L,C", [POOL_CASES[1], POOL_CASES[3], POOL_CASES[7]])
def test_pool_repeated_launches_are_bit_identical(B, L, C):
    y, tab, dz = pool_inputs(B, L, C)
    assert torch.equal(_pool_fwd(y, tab), _pool_fwd(y, tab))
    g1, p1, _ = _pool_bwd(y, tab, dz)
    g2, p2, _ = _pool_bwd(y, tab, dz)
    assert torch.equal(g1, g2) and torch.equal(p1, p2)


def test_pool_rejects_shapes_outside_its_domain():
    lib = _lib.load()
    t = torch.zeros(64, device='cuda')
    for B, L, C in ((1, 1, 4), (1, 4, 6), (1, 4, 1028)):
        assert lib.kws_pool3s2_same_fwd_f32(_lib.ptr(t), _lib.ptr(t), _lib.ptr(t), B, L, C, _lib.stream_ptr()) != 0
        assert lib.kws_pool3s2_same_bwd_part_rows(B, L, C) == 0


# ---- stem ------------------------------------------------------------------------------------------------------------------------
def _stem(x, w, p, dy):
    B, L, C = x.shape
    N = p.shape[1]
    lib = _lib.load()
    M = B * (L - 2)
    rows = lib.kws_stem_stats_rows(B, L)
    wsn = lib.kws_stem_bwd_workspace_floats(B, L, C, N)
    assert rows > 0 and wsn > 0
    xd, wd, pd, dyd = (torch.from_numpy(v).cuda() for v in (x, w, p, dy))
    ybuf, y = _guarded(M * N)
    sbuf, st = _guarded(rows * 2 * N)
    _lib.call("kws_stem_fwd_f32", _lib.ptr(xd), _lib.ptr(wd), _lib.ptr(pd), _lib.ptr(y), B, L, C, N, _lib.ptr(st), _lib.stream_ptr())
    wbuf, ws = _guarded(wsn)
    obuf, out = _guarded(3 * C + C * N)
    dw, dp = out[:3 * C], out[3 * C:]
    _lib.call("kws_stem_bwd_f32", _lib.ptr(dyd), _lib.ptr(xd), _lib.ptr(wd), _lib.ptr(pd), _lib.ptr(dw), _lib.ptr(dp), B, L, C, N,
              _lib.ptr(ws), _lib.stream_ptr())
    torch.cuda.synchronize()
    for buf, t in ((ybuf, y), (sbuf, st), (wbuf, ws), (obuf, out)):   # C = 5 and 25: rows that are not 16-byte aligned
        assert _guards_intact(buf, t.numel())
    return y, st, rows, dw, dp


@pytest.mark.parametrize("B,L,C,N", STEM_CASES)
def test_stem_matches_float64(B, L, C, N):
    x, w, p, dy = stem_inputs(B, L, C, N)
    y, st, rows, dw, dp = _stem(x, w, p, dy)
    ref_y, abs_y, ref_dp, abs_dp, ref_dw, abs_dw = stem_reference(x, w, p, dy)
    M = B * (L - 2)
    got = y.cpu().numpy().reshape(B, L - 2, N).astype(np.float64)
    assert not np.isnan(got).any()
    bar_y = (3 * C + 4) * U * abs_y
    err = np.abs(got - ref_y)
    print("stem %s: y worst error / bar %.3g" % ((B, L, C, N), (err / np.maximum(bar_y, 1e-300)).max()))
    assert (err <= bar_y).all()
    sums = st.cpu().numpy().astype(np.float64).reshape(rows, 2, N).sum(axis=0)
    s1, s2 = ref_y.sum(axis=(0, 1)), (ref_y ** 2).sum(axis=(0, 1))
    bar_s1 = M * U * np.abs(ref_y).sum(axis=(0, 1)) + bar_y.sum(axis=(0, 1))
    bar_s2 = (M + 4) * U * s2 + (2 * np.abs(ref_y) * bar_y + bar_y ** 2).sum(axis=(0, 1))
    assert (np.abs(sums[0] - s1) <= bar_s1).all() and (np.abs(sums[1] - s2) <= bar_s2).all()
    got_dp = dp.cpu().numpy().reshape(C, N).astype(np.float64)
    got_dw = dw.cpu().numpy().reshape(3, C).astype(np.float64)
    assert (np.abs(got_dp - ref_dp) <= (M + 3 + 4) * U * abs_dp).all(), (np.abs(got_dp - ref_dp) / np.maximum(abs_dp, 1e-300)).max() / U
    assert (np.abs(got_dw - ref_dw) <= (M + N + 4) * U * abs_dw).all(), (np.abs(got_dw - ref_dw) / np.maximum(abs_dw, 1e-300)).max() / U
    # negative controls: with reversed taps y misses its bar by far and dp misses its bar; dw does not depend on the taps (dz is
    # dy p^T), so its control is the order of the tap gradients: dw back to front misses the bar (the middle tap is its own mirror)
    wrong = stem_reference(x, w[::-1].copy(), p, dy)
    assert (np.abs(got - wrong[0]) / np.maximum(bar_y, 1e-300)).max() > 100
    assert (np.abs(got_dp - wrong[2]) > (M + 3 + 4) * U * abs_dp).any()
    assert (np.abs(got_dw - ref_dw[::-1]) > (M + N + 4) * U * abs_dw[::-1])[[0, 2]].any()


@pytest.mark.parametrize("B,L,C,N", [STEM_CASES[0], STEM_CASES[3], STEM_CASES[5]])
def test_stem_repeated_launches_are_bit_identical(B, L, C, N):
    x, w, p, dy = stem_inputs(B, L, C, N)
    r1, r2 = _stem(x, w, p, dy), _stem(x, w, p, dy)
    for i in (0, 1, 3, 4):
        assert torch.equal(r1[i], r2[i])


def test_stem_rejects_shapes_outside_its_domain():
    lib = _lib.load()
    t = torch.zeros(4096, device='cuda')
    for B, L, C, N in ((1, 2, 4, 16), (1, 8, 33, 16), (1, 8, 4, 6), (1, 8, 4, 68), (1, 8, 0, 16)):
        assert lib.kws_stem_fwd_f32(_lib.ptr(t), _lib.ptr(t), _lib.ptr(t), _lib.ptr(t), B, L, C, N, None, _lib.stream_ptr()) != 0
        assert lib.kws_stem_bwd_workspace_floats(B, L, C, N) == 0
