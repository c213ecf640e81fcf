"""The two operations the 2-D models add - kws_conv2d_* (dense NHWC Conv2D on f32 MFMA: forward with BatchNorm sums, input gradient
split by stride phase, weight gradient) and kws_pool2x2_* (MaxPool2D((2, 2), strides 2, 'valid') over act(bn(y)) with the BatchNorm
backward's partial sums) - against float64 NumPy (tests/conv2d_oracle.py), by the method of test_inception_kernels_gpu.py: every
output sits in a guarded, sentinel-filled allocation and must be written completely and nowhere else; two runs agree bit for bit;
about a third of the BatchNorm scales is negative; the shifts make act(shift) != 0, so a padded tap that leaked would show; no
element is left out of a comparison.

Bars.  kws_conv2d_*: 1e-5 of the tensor's maximum, the siblings' bar.  The largest reductions among the cases are K = 320 (the
10 x 4 window over 8 channels) in a forward pass, 9 x 96 = 864 in an input gradient and 390 rows in a weight gradient; a float32
NumPy restatement of the oracle (tests/test_conv2d_cpu.py::test_float32_restatement_is_under_half_the_kernel_bar runs it) differs
from float64 by at most 5.2e-7 of the tensor's maximum over all cases, forward and both gradients - a tenth of half the bar.  On small-integer inputs with an identity
table float32 is exact, so there Y, every statistics row, dX and dW equal float64 bit for bit.
kws_pool2x2_*: z is a selection of float32 activations the reference recomputes as the device does (one fused multiply-add,
rounded to float32): exact.  g is one float32 dz times a 0 / 1 gate: exact.  The part rows are held to test_stacked_pool_gpu.py's
bar for the BatchNorm sums, 1e-5 of the sum of magnitudes."""
import ctypes

import numpy as np
import pytest
import torch

import conv2d_cases as cases
from conv2d_oracle import conv2d_bwd, conv2d_fwd, pool2_argmax, pool2_bwd, pool2_fwd, pool2_windows
from speech_recognition_amd import _lib

pytestmark = pytest.mark.gpu

GUARD = 4096
SENT = 0x7FC0DEAD
ACTS = {'relu6': _lib.ACT_RELU6, 'relu': _lib.ACT_RELU}
CASES = cases.CONV_CASES
IDS = [cases.conv_id(c) for c in CASES]


class Guarded(object):
    """n floats between two guard bands, all filled with a sentinel"""

    def __init__(self, n):
        self.buf = torch.empty(n + 2 * GUARD, dtype=torch.int32, device="cuda")
        self.buf.fill_(SENT)
        self.view = self.buf[GUARD:GUARD + n].view(torch.float32)

    def check(self, what, holes=None):
        """guards intact; exactly the elements outside `holes` (bool [n]) written"""
        torch.cuda.synchronize()
        assert bool((self.buf[:GUARD] == SENT).all()) and bool((self.buf[-GUARD:] == SENT).all()), "%s wrote outside its output" % what
        written = self.view.view(torch.int32).cpu().numpy() != SENT
        if holes is None:
            assert written.all(), "%s left output elements unwritten" % what
        else:
            assert (written == ~holes.reshape(-1)).all(), "%s wrote where it must not / left an element unwritten" % what

    def numpy(self):
        return self.view.cpu().numpy()


def _desc(c, act='relu6'):
    return _lib.Conv2dDesc(c['B'], c['H'], c['W'], c['Hout'], c['Wout'], c['kh'], c['kw'], c['s'][0], c['s'][1], c['d'][0], c['d'][1],
                           c['pads'][0][0], c['pads'][1][0], c['Cin'], c['F'], ACTS[act])


def _table(rng, C):
    """[4][C]: a third of the scales negative, shifts with act(shift) != 0 (a padded tap must not contribute it)"""
    bn = np.zeros((4, C), np.float32)
    bn[0] = (0.5 + rng.rand(C)) * np.where(rng.rand(C) < 0.33, -1.0, 1.0)
    bn[1] = 0.5 + 0.5 * rng.rand(C)
    bn[2] = rng.randn(C)
    bn[3] = 0.5 + rng.rand(C)
    return bn


def _run(c, tX, tbn, tW, tdY, act='relu6'):
    """-> Y, stats, dX, dW (guarded, checked for complete coverage), stats rows"""
    lib = _lib.load()
    S = _lib.stream_ptr()
    d = _desc(c, act)
    M = c['B'] * c['Hout'] * c['Wout']
    rows = lib.kws_conv2d_stats_rows(ctypes.byref(d))
    assert rows == -(-M // 128)
    Y = Guarded(M * c['F'])
    st = Guarded(rows * 2 * c['F'])
    dX = Guarded(c['B'] * c['H'] * c['W'] * c['Cin'])
    nW = c['kh'] * c['kw'] * c['Cin'] * c['F']
    dW = Guarded(nW)
    ws_n = int(lib.kws_conv2d_wgrad_workspace_floats(ctypes.byref(d)))
    assert ws_n >= nW
    ws = Guarded(ws_n)
    bnp = _lib.ptr(tbn) if tbn is not None else None
    _lib.call("kws_conv2d_fwd_f32", _lib.ptr(tX), bnp, _lib.ptr(tW), _lib.ptr(Y.view), _lib.ptr(st.view), ctypes.byref(d), S)
    _lib.call("kws_conv2d_dgrad_f32", _lib.ptr(tdY), _lib.ptr(tW), _lib.ptr(dX.view), ctypes.byref(d), S)
    _lib.call("kws_conv2d_wgrad_f32", _lib.ptr(tX), bnp, _lib.ptr(tdY), _lib.ptr(dW.view), _lib.ptr(ws.view), ctypes.byref(d), S)
    torch.cuda.synchronize()
    Y.check("conv2d_fwd")
    st.check("conv2d_fwd stats")
    dX.check("conv2d_dgrad")
    dW.check("conv2d_wgrad")
    assert bool((ws.buf[:GUARD] == SENT).all()) and bool((ws.buf[-GUARD:] == SENT).all()), "conv2d_wgrad wrote outside its workspace"
    return Y, st, dX, dW, rows


def _reference(c, x, bn, W, dy, act='relu6'):
    """float64: y [B, Hout, Wout, F], dx (wrt act(x)) [B, H, W, Cin], dW, and which input pixels some window reads"""
    a = x.astype(np.float64)
    if bn is not None:
        b = bn.astype(np.float64)
        a = a * b[0] + b[1]
        a = np.clip(a, 0, 6) if act == 'relu6' else np.maximum(a, 0)
    W64 = W.astype(np.float64)
    y, ap = conv2d_fwd(a, W64, c['s'], c['d'], c['pads'], (c['Hout'], c['Wout']))
    dx, dW = conv2d_bwd(dy.astype(np.float64), ap, W64, c['s'], c['d'], c['pads'], (c['H'], c['W']))
    read = conv2d_bwd(np.ones_like(y[..., :1]), ap[..., :1], np.ones(W.shape[:2] + (1, 1)), c['s'], c['d'], c['pads'], (c['H'], c['W']))[0]
    return y, dx, dW, read[..., 0] > 0


def _inputs(c, rng, integers=False):
    shp_x, shp_w = (c['B'], c['H'], c['W'], c['Cin']), (c['kh'], c['kw'], c['Cin'], c['F'])
    shp_y = (c['B'], c['Hout'], c['Wout'], c['F'])
    if integers:
        x = rng.randint(0, 3, size=shp_x).astype(np.float32)          # in [0, 6]: either activation of the identity table keeps them
        W = rng.randint(-2, 3, size=shp_w).astype(np.float32)
        dy = rng.randint(-2, 3, size=shp_y).astype(np.float32)
    else:
        x = rng.randn(*shp_x).astype(np.float32)
        W = (rng.randn(*shp_w) / np.sqrt(c['kh'] * c['kw'] * c['Cin'])).astype(np.float32)
        dy = rng.randn(*shp_y).astype(np.float32)
    return x, W, dy


def _rel(got, ref):
    return np.abs(got - ref).max() / max(np.abs(ref).max(), 1e-30)


def test_the_cases_cover_what_they_claim():
    by = {cases.conv_id(c): c for c in CASES}
    assert len(by) == len(CASES) == 11
    assert any(c['Cin'] == 1 and c['s'] == (2, 2) for c in CASES)
    assert any(c['B'] * c['Hout'] * c['Wout'] > 128 and c['F'] > 64 for c in CASES)
    assert any(c['d'][0] * (c['kh'] - 1) + 1 > c['H'] for c in CASES)
    assert any(c['kh'] == 1 and c['s'] == (2, 2) for c in CASES) and any(c['s'] == (2, 1) for c in CASES)
    assert any(c['padding'] == 'valid' for c in CASES)
    assert any((c['kh'], c['kw']) == (20, 8) for c in CASES) and any((c['kh'], c['kw']) == (10, 4) for c in CASES)


@pytest.mark.parametrize("mode", ["raw", "relu6", "relu"])
@pytest.mark.parametrize("c", CASES, ids=IDS)
def test_conv2d_matches_float64(c, mode):
    rng = np.random.RandomState(c['H'] * 31 + c['Cin'] + c['kh'] + 7 * len(mode))
    x, W, dy = _inputs(c, rng)
    act = mode if mode != 'raw' else 'relu6'
    bn = _table(rng, c['Cin']) if mode != 'raw' else None
    if bn is not None and mode == 'relu':
        x = x * 8.0                                            # activations above 6 exist: relu and relu6 differ
    tX, tW, tdY = (torch.from_numpy(a).cuda() for a in (x, W, dy))
    tbn = torch.from_numpy(bn).cuda() if bn is not None else None
    Y, st, dX, dW, rows = _run(c, tX, tbn, tW, tdY, act)
    y_ref, dx_ref, dW_ref, read = _reference(c, x, bn, W, dy, act)
    if mode == 'relu':
        assert np.abs(y_ref - _reference(c, x, bn, W, dy, 'relu6')[0]).max() > 1e-3 * np.abs(y_ref).max()
    F = c['F']
    y = Y.numpy().reshape(y_ref.shape)
    dx = dX.numpy().reshape(dx_ref.shape)
    dw = dW.numpy().reshape(dW_ref.shape)
    part = st.numpy().astype(np.float64).reshape(rows, 2, F).sum(0)
    y2 = y_ref.reshape(-1, F)
    print("conv2d %s %s: fwd %.3g, dgrad %.3g, wgrad %.3g (bar 1e-5)" % (cases.conv_id(c), mode, _rel(y, y_ref), _rel(dx, dx_ref),
                                                                       _rel(dw, dW_ref)))
    assert _rel(y, y_ref) < 1e-5
    assert (np.abs(part[0] - y2.sum(0)) <= 1e-5 * np.abs(y2).sum(0) + 1e-30).all()
    assert (np.abs(part[1] - (y2 * y2).sum(0)) <= 1e-5 * (y2 * y2).sum(0) + 1e-30).all()
    assert _rel(dx, dx_ref) < 1e-5
    assert not dx[~read].any()                                  # pixels no window reads: exact zeros
    assert _rel(dw, dW_ref) < 1e-5
    again = _run(c, tX, tbn, tW, tdY, act)                       # run to run: bit for bit
    for a1, a2, what in zip((Y, st, dX, dW), again[:4], ("fwd", "stats", "dgrad", "wgrad")):
        assert torch.equal(a1.buf, a2.buf), what


def test_some_cases_have_pixels_no_window_reads():
    unread = {}
    for c in CASES:
        rng = np.random.RandomState(0)
        x, W, dy = _inputs(c, rng, integers=True)
        unread[cases.conv_id(c)] = int((~_reference(c, x, None, W, dy)[3]).sum())
    assert unread[cases.conv_id(CASES[6])] > 0 and unread[cases.conv_id(CASES[10])] > 0, unread


@pytest.mark.parametrize("c", CASES, ids=IDS)
def test_conv2d_is_exact_on_small_integers(c):
    """Inputs, weights and gradients are small integers and the table is the identity, so every product and every partial sum is
    an integer below 2^24: float32 is exact, whatever the order of the additions.  Y, each statistics row, dX and dW equal float64
    bit for bit - a dropped or doubled padded tap, stride phase or ragged tile cannot hide."""
    rng = np.random.RandomState(c['H'] + 1000)
    x, W, dy = _inputs(c, rng, integers=True)
    bn = np.zeros((4, c['Cin']), np.float32)
    bn[0], bn[3] = 1.0, 1.0
    tX, tW, tdY, tbn = (torch.from_numpy(a).cuda() for a in (x, W, dy, bn))
    for act in ('relu6', 'relu'):
        Y, st, dX, dW, rows = _run(c, tX, tbn, tW, tdY, act)
        y_ref, dx_ref, dW_ref, read = _reference(c, x, bn, W, dy, act)
        F = c['F']
        M = c['B'] * c['Hout'] * c['Wout']
        y2 = np.zeros((rows * 128, F))
        y2[:M] = y_ref.reshape(-1, F)
        tiles = y2.reshape(rows, 128, F)
        st_ref = np.stack([tiles.sum(1), (tiles * tiles).sum(1)], axis=1)        # [rows][2][F]
        for ref in (y_ref, dx_ref, dW_ref, st_ref, np.abs(y2).sum(0)):
            assert np.abs(ref).max() < 2 ** 24                                    # the premise of the exactness argument
        assert np.array_equal(Y.numpy().reshape(y_ref.shape).astype(np.float64), y_ref)
        assert np.array_equal(st.numpy().reshape(rows, 2, F).astype(np.float64), st_ref)
        assert np.array_equal(dX.numpy().reshape(dx_ref.shape).astype(np.float64), dx_ref)
        assert np.array_equal(dW.numpy().reshape(dW_ref.shape).astype(np.float64), dW_ref)


def test_conv2d_stats_are_optional():
    c = CASES[2]
    rng = np.random.RandomState(1)
    x, W, dy = _inputs(c, rng)
    d = _desc(c)
    Y = Guarded(c['B'] * c['Hout'] * c['Wout'] * c['F'])
    tX, tW = torch.from_numpy(x).cuda(), torch.from_numpy(W).cuda()
    _lib.call("kws_conv2d_fwd_f32", _lib.ptr(tX), None, _lib.ptr(tW), _lib.ptr(Y.view), None, ctypes.byref(d), _lib.stream_ptr())
    Y.check("conv2d_fwd without stats")
    y_ref = _reference(c, x, None, W, dy)[0]
    assert _rel(Y.numpy().reshape(y_ref.shape), y_ref) < 1e-5


def test_bad_conv2d_descriptors_are_refused():
    lib = _lib.load()
    good = CASES[2]
    out = Guarded(4096)
    x = torch.zeros(1 << 16, device="cuda")
    S = _lib.stream_ptr()
    fields = ('B', 'H', 'W', 'Hout', 'Wout', 'kh', 'kw', 'sh', 'sw', 'dh', 'dw', 'pad_t', 'pad_l', 'Cin', 'F', 'act')
    for key, val in (('Hout', good['Hout'] + 1), ('Wout', good['Wout'] - 1), ('pad_t', 0), ('pad_l', 2), ('kh', 21), ('kw', 9), ('kh', 0),
                     ('sh', 3), ('sw', 0), ('dh', 3), ('dw', 0), ('Cin', 0), ('F', 0), ('B', 0), ('act', 2)):
        d = _desc(good)
        assert key in fields
        setattr(d, key, val)
        for rc in (lib.kws_conv2d_fwd_f32(_lib.ptr(x), None, _lib.ptr(x), _lib.ptr(out.view), None, ctypes.byref(d), S),
                   lib.kws_conv2d_dgrad_f32(_lib.ptr(x), _lib.ptr(x), _lib.ptr(out.view), ctypes.byref(d), S),
                   lib.kws_conv2d_wgrad_f32(_lib.ptr(x), None, _lib.ptr(x), _lib.ptr(out.view), _lib.ptr(x), ctypes.byref(d), S)):
            assert rc == -1, (key, val)
            assert b'conv2d' in lib.kws_last_error(), (key, val)
        assert lib.kws_conv2d_wgrad_workspace_floats(ctypes.byref(d)) == 0
    d = _desc(CASES[0])                                           # dilation needs stride 1 on that axis
    d.dh = 2
    d.pad_t, d.Hout = 2, 4
    assert lib.kws_conv2d_fwd_f32(_lib.ptr(x), None, _lib.ptr(x), _lib.ptr(out.view), None, ctypes.byref(d), S) == -1
    out.check("a refused call", np.ones(4096, bool))             # nothing was launched


# ---- MaxPool2D((2, 2), strides 2, 'valid') over act(bn(y)) ------------------------------------------------------------------------
def _pool_inputs(B, H, W, C, seed):
    rng = np.random.RandomState(seed)
    y = (rng.randint(-12, 13, size=(B, H, W, C)) * 0.25).astype(np.float32)   # quantised: exact ties, exact products
    scale = np.where(rng.rand(C) < 0.35, -1.0, 1.0) * rng.choice([0.5, 1.0, 2.0, 4.0], C)
    shift = rng.choice([0.0, 0.5, 1.0, 3.0], C)
    mean = rng.randn(C) * 0.3
    rstd = 0.5 + rng.rand(C)
    bn = np.stack([scale, shift, mean, rstd]).astype(np.float32)
    dz = rng.randn(B, H // 2, W // 2, C).astype(np.float32)
    return y, bn, dz


def _pool_act(y, bn, act):
    """the pre-activation and act(.) rounded to float32 as on the device (the double product-sum is exact: one rounding)"""
    pre = (y.astype(np.float64) * bn[0].astype(np.float64) + bn[1].astype(np.float64)).astype(np.float32)
    return pre, (np.clip(pre, 0, 6) if act == 'relu6' else np.maximum(pre, 0))


def _pool_run(y, bn, dz, act):
    lib = _lib.load()
    B, H, W, C = y.shape
    S = _lib.stream_ptr()
    ty, tbn, tdz = (torch.from_numpy(a).cuda() for a in (y, bn, dz))
    rows = lib.kws_pool2x2_bwd_part_rows(B, H, W, C)
    assert rows > 0 and lib.kws_pool2x2_bwd_part_floats(B, H, W, C) == rows * 2 * C
    z, g, part = Guarded(dz.size), Guarded(y.size), Guarded(rows * 2 * C)
    _lib.call("kws_pool2x2_fwd_f32", _lib.ptr(ty), _lib.ptr(tbn), _lib.ptr(z.view), B, H, W, C, ACTS[act], S)
    _lib.call("kws_pool2x2_bwd_f32", _lib.ptr(tdz), _lib.ptr(ty), _lib.ptr(tbn), _lib.ptr(g.view), _lib.ptr(part.view), B, H, W, C,
              ACTS[act], S)
    for t, what in ((z, "pool2x2_fwd"), (g, "pool2x2_bwd"), (part, "pool2x2_bwd part rows")):
        t.check(what)
    return z, g, part, rows


@pytest.mark.parametrize("act", ['relu6', 'relu'])
@pytest.mark.parametrize("B,H,W,C", cases.POOL_CASES)
def test_pool2x2_matches_float64(B, H, W, C, act):
    y, bn, dz = _pool_inputs(B, H, W, C, 11 * H + C + (act == 'relu'))
    y[0, :2, :2, 0] = [[1.0, 0.25], [1.0, 1.0]]   # a three-way tie between unsaturated values (1.5) in the first window, by hand
    bn[0, 0], bn[1, 0] = 1.0, 0.5
    bn[0, -1] = -abs(bn[0, -1])                   # at least one negative scale whatever the draw
    z, g, part, rows = _pool_run(y, bn, dz, act)
    pre, a = _pool_act(y, bn, act)
    a64 = a.astype(np.float64)
    ind = pool2_argmax(a64)
    # forward: a selection of float32 values - exact; pooling the raw output first is a different function (negative scales)
    np.testing.assert_array_equal(z.numpy().reshape(dz.shape), pool2_fwd(a, ind))
    if y.size >= 4096:
        assert np.abs(pool2_fwd(a64, pool2_argmax(y.astype(np.float64))) - pool2_fwd(a64, ind)).max() > 0.1
    # backward: one float32 dz times a 0 / 1 gate - exact; the first maximum in row-major order wins
    gate = ((pre > 0) & (pre <= 6)) if act == 'relu6' else (pre > 0)
    g_ref = pool2_bwd(dz.astype(np.float64), ind, H, W) * gate
    got = g.numpy().reshape(y.shape).astype(np.float64)
    np.testing.assert_array_equal(got, g_ref)
    win = np.sort(pool2_windows(a64), axis=3)[:, :, :, ::-1, :]
    hi = 6.0 if act == 'relu6' else np.inf
    ties = (win[:, :, :, 0] == win[:, :, :, 1]) & (win[:, :, :, 0] > 0) & (win[:, :, :, 0] < hi)
    assert ties.any()                                             # first-wins is observable: open-gated ties exist ...
    g_last = pool2_bwd(dz.astype(np.float64), pool2_argmax(a64, last=True), H, W) * gate
    assert np.abs(got - g_last).max() > 0                         # ... and last-wins routes them elsewhere
    if H % 2:
        assert not got[:, -1].any()                               # the row / column in no window: exact zeros
    if W % 2:
        assert not got[:, :, -1].any()
    # BatchNorm sums: test_stacked_pool_gpu.py's bar
    xhat = (y.astype(np.float64) - bn[2].astype(np.float64)) * bn[3].astype(np.float64)
    fold = part.numpy().astype(np.float64).reshape(rows, 2, C).sum(axis=0)
    s, sx = g_ref.sum(axis=(0, 1, 2)), (g_ref * xhat).sum(axis=(0, 1, 2))
    sa, sxa = np.abs(g_ref).sum(axis=(0, 1, 2)), np.abs(g_ref * xhat).sum(axis=(0, 1, 2))
    serr = (np.abs(fold[0] - s) / np.maximum(sa, 1e-30)).max()
    sxerr = (np.abs(fold[1] - sx) / np.maximum(sxa, 1e-30)).max()
    print("pool2x2 bwd (%d, %d, %d, %d) %s: sum g %.3g, sum g xhat %.3g (bar 1e-5)" % (B, H, W, C, act, serr, sxerr))
    assert serr < 1e-5 and sxerr < 1e-5
    again = _pool_run(y, bn, dz, act)
    for a1, a2 in zip((z, g, part), again[:3]):
        assert torch.equal(a1.buf, a2.buf)


def test_relu_and_relu6_pools_differ_where_values_pass_six():
    B, H, W, C = cases.POOL_CASES[0]
    y, bn, dz = _pool_inputs(B, H, W, C, 5)
    z6, g6 = _pool_run(y, bn, dz, 'relu6')[:2]
    z0, g0 = _pool_run(y, bn, dz, 'relu')[:2]
    assert float(z0.view.max()) > 6.0 and float(z6.view.max()) == 6.0
    assert not torch.equal(g0.view, g6.view)


def test_bad_pool2x2_arguments_are_refused():
    lib = _lib.load()
    out = Guarded(4096)
    t = torch.zeros(4096, device="cuda")
    S = _lib.stream_ptr()
    for B, H, W, C, act in ((0, 4, 4, 8, 0), (1, 1, 4, 8, 0), (1, 4, 1, 8, 0), (1, 4, 4, 6, 0), (1, 4, 4, 2048, 0), (1, 4, 4, 8, 2)):
        assert lib.kws_pool2x2_fwd_f32(_lib.ptr(t), _lib.ptr(t), _lib.ptr(out.view), B, H, W, C, act, S) == -1
        assert b'pool2x2_fwd' in lib.kws_last_error()
        assert lib.kws_pool2x2_bwd_f32(_lib.ptr(t), _lib.ptr(t), _lib.ptr(t), _lib.ptr(out.view), _lib.ptr(out.view), B, H, W, C, act, S) == -1
        assert b'pool2x2_bwd' in lib.kws_last_error()
        if act == 0:
            assert lib.kws_pool2x2_bwd_part_rows(B, H, W, C) == 0
    assert lib.kws_pool2x2_fwd_f32(None, _lib.ptr(t), _lib.ptr(out.view), 1, 4, 4, 8, 0, S) == -1
    out.check("a refused call", np.ones(4096, bool))
