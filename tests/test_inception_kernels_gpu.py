"""The two operations inception_d1 adds - kws_conv1d_* (dense Conv1D with zero padding, dilation and channel windows; forward with
BatchNorm sums, input gradient in both accumulate modes, weight gradient) and kws_avgpool3_same_* (AveragePooling1D(3, 1, 'same'))
- against float64 NumPy (tests/inception_oracle.py).  Every output is a window of a guarded allocation (the method of
test_grouped_conv_gpu.py): columns outside [y0, y0 + F) / [x0, x0 + Cin) and the guard bands keep their sentinel; two runs agree
bit for bit.

Bars.  kws_conv1d_*: 1e-5 of the tensor's maximum, the project's kws_gconv_* bar (K <= 630 there, <= 1488 here).  On small-integer
inputs with an identity table float32 is exact, so there every output - Y, the statistics rows, dX, dW - equals float64 bit for bit.
kws_avgpool3_same_*: forward 6e-6 absolute (at most six float32 roundings on values in [0, 6]); backward 1e-6 * sum |dz_t| / n_t per
element; in accumulate mode the result also equals float32(prior) + (the overwrite-mode result) bit for bit, and the float64
comparison allows the one more float32 rounding of that last addition (6e-8 |prior + gradient|)."""
import ctypes

import numpy as np
import pytest
import torch

from inception_oracle import avgpool_bwd, avgpool_fwd
from oracle_blocks import conv_bwd, conv_fwd, same_geometry
from speech_recognition_amd import _lib

pytestmark = pytest.mark.gpu

GUARD = 4096
SENT = 0x7FC0DEAD


def _case(B, L, Cin, F, k, dil, Cx=None, x0=0, Cy=None, y0=0, valid=False):
    span = dil * (k - 1)
    return dict(B=B, L=L, Cin=Cin, F=F, k=k, dil=dil, Cx=Cx or Cin, x0=x0, Cy=Cy or F, y0=y0,
                pad_l=0 if valid else same_geometry(L, k, 1, dil)[1], Lout=L - span if valid else L)


CASES = [
    _case(3, 6, 48, 64, 3, 2),                                   # every row has a padded tap, half have two
    _case(3, 93, 96, 96, 3, 2),                                  # M = 279 crosses 128-row tiles inside a clip; F = 1.5 column tiles
    _case(2, 47, 256, 192, 3, 1),
    _case(2, 12, 496, 48, 1, 1),
    _case(2, 24, 64, 32, 5, 1),                                  # the 5 taps of the model that is not built yet
    _case(1, 1, 4, 5, 3, 2),                                     # a single row, all but one tap padded
    _case(2, 20, 48, 96, 3, 2, Cx=176, x0=64, Cy=256, y0=128),   # a window on both sides
    _case(2, 30, 20, 24, 3, 2, valid=True),                      # VALID: pad_l = 0, Lout = L - dil * (k - 1)
    _case(2, 9, 12, 7, 4, 3),                                    # even k: SAME pads (4, 5)
]
IDS = ["B%d_L%d_C%d_F%d_k%d_d%d%s" % (c['B'], c['L'], c['Cin'], c['F'], c['k'], c['dil'],
                                      '_win' if c['Cx'] != c['Cin'] else '_valid' if c['Lout'] != c['L'] else '') for c in CASES]


class Guarded(object):
    """n floats between two guard bands, all filled with a sentinel; `prior` (float32 [n], NaN = leave the sentinel) presets values"""

    def __init__(self, n, prior=None):
        self.buf = torch.empty(n + 2 * GUARD, dtype=torch.int32, device="cuda")
        self.buf.fill_(SENT)
        self.view = self.buf[GUARD:GUARD + n].view(torch.float32)
        if prior is not None:
            p = torch.from_numpy(prior.reshape(-1)).cuda()
            keep = ~torch.isnan(p)
            self.view[keep] = p[keep]

    def check(self, what, holes=None):
        """guards intact; exactly the elements outside `holes` (bool [n]) written"""
        torch.cuda.synchronize()
        assert bool((self.buf[:GUARD] == SENT).all()) and bool((self.buf[-GUARD:] == SENT).all()), "%s wrote outside its output" % what
        written = self.view.view(torch.int32).cpu().numpy() != SENT
        if holes is None:
            assert written.all(), "%s left output elements unwritten" % what
        else:
            assert (written == ~holes.reshape(-1)).all(), "%s wrote outside its window / left an element unwritten" % what

    def numpy(self):
        return self.view.cpu().numpy()


def _desc(c):
    return _lib.Conv1dDesc(c['B'], c['L'], c['Lout'], c['k'], c['dil'], c['pad_l'], c['Cx'], c['x0'], c['Cin'], c['Cy'], c['y0'], c['F'])


def _holes(rows, pitch, c0, width):
    h = np.ones((rows, pitch), bool)
    h[:, c0:c0 + width] = False
    return h


def _table(rng, Cx):
    """[4][Cx]: a third of the scales negative, shifts with relu6(shift) != 0 (a padded tap must not contribute it)"""
    bn = np.zeros((4, Cx), np.float32)
    bn[0] = (0.5 + rng.rand(Cx)) * np.where(rng.rand(Cx) < 0.33, -1.0, 1.0)
    bn[1] = 0.5 + 0.5 * rng.rand(Cx)
    bn[2] = rng.randn(Cx)
    bn[3] = 0.5 + rng.rand(Cx)
    return bn


def _run(c, tX, tbn, tW, tdY, prior=None):
    """-> Y, stats, dX (overwrite), dX (accumulate over `prior`), dW, stats rows"""
    lib = _lib.load()
    S = _lib.stream_ptr()
    d = _desc(c)
    rows = lib.kws_conv1d_stats_rows(ctypes.byref(d))
    assert rows == -(-c['B'] * c['Lout'] // 128)
    Y = Guarded(c['B'] * c['Lout'] * c['Cy'])
    st = Guarded(rows * 2 * c['F'])
    dX0 = Guarded(c['B'] * c['L'] * c['Cx'])
    dX1 = Guarded(c['B'] * c['L'] * c['Cx'], prior)
    dW = Guarded(c['k'] * c['Cin'] * c['F'])
    ws_n = int(lib.kws_conv1d_wgrad_workspace_floats(ctypes.byref(d)))
    assert ws_n >= c['k'] * c['Cin'] * c['F']
    ws = Guarded(ws_n)
    bnp = _lib.ptr(tbn) if tbn is not None else None
    _lib.call("kws_conv1d_fwd_f32", _lib.ptr(tX), bnp, _lib.ptr(tW), _lib.ptr(Y.view), _lib.ptr(st.view), ctypes.byref(d), S)
    _lib.call("kws_conv1d_dgrad_f32", _lib.ptr(tdY), _lib.ptr(tW), _lib.ptr(dX0.view), 0, ctypes.byref(d), S)
    _lib.call("kws_conv1d_dgrad_f32", _lib.ptr(tdY), _lib.ptr(tW), _lib.ptr(dX1.view), 1, ctypes.byref(d), S)
    _lib.call("kws_conv1d_wgrad_f32", _lib.ptr(tX), bnp, _lib.ptr(tdY), _lib.ptr(dW.view), _lib.ptr(ws.view), ctypes.byref(d), S)
    torch.cuda.synchronize()
    Y.check("conv1d_fwd", _holes(c['B'] * c['Lout'], c['Cy'], c['y0'], c['F']))
    st.check("conv1d_fwd stats")
    xh = _holes(c['B'] * c['L'], c['Cx'], c['x0'], c['Cin'])
    dX0.check("conv1d_dgrad", xh)
    dX1.check("conv1d_dgrad (accumulate)", xh)
    dW.check("conv1d_wgrad")
    assert bool((ws.buf[:GUARD] == SENT).all()) and bool((ws.buf[-GUARD:] == SENT).all()), "conv1d_wgrad wrote outside its workspace"
    return Y, st, dX0, dX1, dW, rows


def _reference(c, x, bn, W, dy):
    """float64: y [B, Lout, F], dx (wrt act(x)) [B, L, Cin], dW, the activated window"""
    xw = x[:, :, c['x0']:c['x0'] + c['Cin']].astype(np.float64)
    if bn is not None:
        b = bn.astype(np.float64)
        xw = np.clip(xw * b[0, c['x0']:c['x0'] + c['Cin']] + b[1, c['x0']:c['x0'] + c['Cin']], 0, 6)
    W64 = W.astype(np.float64)
    y, ap = conv_fwd(xw, W64, 1, c['dil'], c['pad_l'], c['Lout'])
    dyw = dy[:, :, c['y0']:c['y0'] + c['F']].astype(np.float64)
    dx, dW = conv_bwd(dyw, ap, W64, c['L'], 1, c['dil'], c['pad_l'])
    return y, dx, dW


def _inputs(c, rng, integers=False):
    B, L, Lout = c['B'], c['L'], c['Lout']
    if integers:
        x = rng.randint(0, 3, size=(B, L, c['Cx'])).astype(np.float32)        # in [0, 6]: relu6 of the identity table keeps them
        W = rng.randint(-2, 3, size=(c['k'], c['Cin'], c['F'])).astype(np.float32)
        dy = rng.randint(-2, 3, size=(B, Lout, c['Cy'])).astype(np.float32)
        prior = rng.randint(-4, 5, size=(B, L, c['Cx'])).astype(np.float32)
    else:
        x = rng.randn(B, L, c['Cx']).astype(np.float32)
        W = (rng.randn(c['k'], c['Cin'], c['F']) / np.sqrt(c['k'] * c['Cin'])).astype(np.float32)
        dy = rng.randn(B, Lout, c['Cy']).astype(np.float32)
        prior = rng.randn(B, L, c['Cx']).astype(np.float32)
    prior[:, :, :c['x0']] = np.nan                                            # outside the window the sentinel stays
    prior[:, :, c['x0'] + c['Cin']:] = np.nan
    return x, W, dy, prior


def _rel(got, ref):
    return np.abs(got - ref).max() / max(np.abs(ref).max(), 1e-30)


@pytest.mark.parametrize("with_table", [False, True], ids=["raw", "table"])
@pytest.mark.parametrize("c", CASES, ids=IDS)
def test_conv1d_matches_float64(c, with_table):
    rng = np.random.RandomState(c['L'] * 31 + c['Cin'] + c['k'] + 7 * with_table)
    x, W, dy, prior = _inputs(c, rng)
    bn = _table(rng, c['Cx']) if with_table else None
    tX, tW, tdY = (torch.from_numpy(a).cuda() for a in (x, W, dy))
    tbn = torch.from_numpy(bn).cuda() if with_table else None
    Y, st, dX0, dX1, dW, rows = _run(c, tX, tbn, tW, tdY, prior)
    y_ref, dx_ref, dW_ref = _reference(c, x, bn, W, dy)
    B, L, Lout, F = c['B'], c['L'], c['Lout'], c['F']
    xs, ys = slice(c['x0'], c['x0'] + c['Cin']), slice(c['y0'], c['y0'] + F)
    y = Y.numpy().reshape(B, Lout, c['Cy'])[:, :, ys]
    dx0 = dX0.numpy().reshape(B, L, c['Cx'])[:, :, xs]
    dx1 = dX1.numpy().reshape(B, L, c['Cx'])[:, :, xs]
    acc_ref = prior[:, :, xs].astype(np.float64) + dx_ref
    part = st.numpy().astype(np.float64).reshape(rows, 2, F).sum(0)
    y2 = y_ref.reshape(-1, F)
    print("conv1d %s table=%d: fwd %.3g, dgrad %.3g, dgrad+ %.3g, wgrad %.3g (bar 1e-5)" %
          (c, with_table, _rel(y, y_ref), _rel(dx0, dx_ref), _rel(dx1, acc_ref), _rel(dW.numpy().reshape(dW_ref.shape), dW_ref)))
    assert _rel(y, y_ref) < 1e-5
    assert (np.abs(part[0] - y2.sum(0)) <= 1e-5 * np.abs(y2).sum(0) + 1e-30).all()
    assert (np.abs(part[1] - (y2 * y2).sum(0)) <= 1e-5 * (y2 * y2).sum(0) + 1e-30).all()
    assert _rel(dx0, dx_ref) < 1e-5
    assert _rel(dx1, acc_ref) < 1e-5
    assert np.array_equal(dx1, prior[:, :, xs] + dx0)            # one thread, one addition per element
    assert _rel(dW.numpy().reshape(dW_ref.shape), dW_ref) < 1e-5
    # run to run: bit for bit
    again = _run(c, tX, tbn, tW, tdY, prior)
    for a1, a2, what in zip((Y, st, dX0, dX1, dW), again[:5], ("fwd", "stats", "dgrad", "dgrad accumulate", "wgrad")):
        assert torch.equal(a1.buf, a2.buf), what


@pytest.mark.parametrize("c", [CASES[i] for i in (0, 1, 4, 5, 6, 7, 8)], ids=[IDS[i] for i in (0, 1, 4, 5, 6, 7, 8)])
def test_conv1d_is_exact_on_small_integers(c):
    """Inputs, weights and gradients are small integers and the table is the identity, so every product and every partial sum is
    an integer below 2^24: float32 is exact, whatever the order of the additions.  Y, each statistics row, dX in both modes and dW
    equal float64 bit for bit - a dropped or doubled padded tap or ragged tile cannot hide."""
    rng = np.random.RandomState(c['L'] + 1000)
    x, W, dy, prior = _inputs(c, rng, integers=True)
    bn = np.zeros((4, c['Cx']), np.float32)
    bn[0], bn[3] = 1.0, 1.0
    tX, tW, tdY, tbn = (torch.from_numpy(a).cuda() for a in (x, W, dy, bn))
    Y, st, dX0, dX1, dW, rows = _run(c, tX, tbn, tW, tdY, prior)
    y_ref, dx_ref, dW_ref = _reference(c, x, bn, W, dy)
    B, L, Lout, F = c['B'], c['L'], c['Lout'], c['F']
    xs, ys = slice(c['x0'], c['x0'] + c['Cin']), slice(c['y0'], c['y0'] + F)
    y2 = np.zeros((rows * 128, F))
    y2[:B * Lout] = y_ref.reshape(-1, F)
    tiles = y2.reshape(rows, 128, F)
    st_ref = np.stack([tiles.sum(1), (tiles * tiles).sum(1)], axis=1)        # [rows][2][F]
    for ref in (y_ref, dx_ref, dW_ref, st_ref, np.abs(y2).sum(0), np.abs(prior[:, :, xs]) + np.abs(dx_ref)):
        assert np.abs(ref).max() < 2 ** 24                                    # the premise of the exactness argument
    assert np.array_equal(Y.numpy().reshape(B, Lout, c['Cy'])[:, :, ys].astype(np.float64), y_ref)
    assert np.array_equal(st.numpy().reshape(rows, 2, F).astype(np.float64), st_ref)
    assert np.array_equal(dX0.numpy().reshape(B, L, c['Cx'])[:, :, xs].astype(np.float64), dx_ref)
    assert np.array_equal(dX1.numpy().reshape(B, L, c['Cx'])[:, :, xs].astype(np.float64), prior[:, :, xs].astype(np.float64) + dx_ref)
    assert np.array_equal(dW.numpy().reshape(dW_ref.shape).astype(np.float64), dW_ref)


def test_conv1d_stats_are_optional():
    c = CASES[0]
    rng = np.random.RandomState(1)
    x, W, dy, _ = _inputs(c, rng)
    d = _desc(c)
    Y = Guarded(c['B'] * c['Lout'] * c['Cy'])
    tX, tW = torch.from_numpy(x).cuda(), torch.from_numpy(W).cuda()
    _lib.call("kws_conv1d_fwd_f32", _lib.ptr(tX), None, _lib.ptr(tW), _lib.ptr(Y.view), None, ctypes.byref(d), _lib.stream_ptr())
    Y.check("conv1d_fwd without stats")
    assert _rel(Y.numpy().reshape(c['B'], c['Lout'], c['F']), _reference(c, x, None, W, dy)[0]) < 1e-5


def test_bad_conv1d_descriptors_are_refused():
    lib = _lib.load()
    good = CASES[1]
    bad = []
    for key, val in (('Lout', good['L'] + 3), ('Lout', good['L'] - 5), ('pad_l', 5), ('x0', 1), ('y0', 1), ('k', 8), ('dil', 5), ('dil', 0),
                     ('Cin', 0), ('F', 0)):
        c = dict(good)
        c[key] = val
        bad.append((key, val, _desc(c)))
    out = Guarded(4096)
    x = torch.zeros(1 << 16, device="cuda")
    for key, val, d in bad:
        for rc in (lib.kws_conv1d_fwd_f32(_lib.ptr(x), None, _lib.ptr(x), _lib.ptr(out.view), None, ctypes.byref(d), _lib.stream_ptr()),
                   lib.kws_conv1d_dgrad_f32(_lib.ptr(x), _lib.ptr(x), _lib.ptr(out.view), 0, ctypes.byref(d), _lib.stream_ptr()),
                   lib.kws_conv1d_wgrad_f32(_lib.ptr(x), None, _lib.ptr(x), _lib.ptr(out.view), _lib.ptr(x), ctypes.byref(d),
                                            _lib.stream_ptr())):
            assert rc == -1, (key, val)
            assert b'conv1d' in lib.kws_last_error(), (key, val)
        assert lib.kws_conv1d_wgrad_workspace_floats(ctypes.byref(d)) == 0
    d = _desc(good)
    assert lib.kws_conv1d_dgrad_f32(_lib.ptr(x), _lib.ptr(x), _lib.ptr(out.view), 2, ctypes.byref(d), _lib.stream_ptr()) == -1
    out.check("a refused call", np.ones(4096, bool))             # nothing was launched


# ---- AveragePooling1D(3, 1, 'same') --------------------------------------------------------------------------------------------
POOL_CASES = [(3, 1, 8), (3, 2, 8), (3, 6, 496), (5, 93, 256)]


def _pool_run(x, bn, dz, prior):
    B, L, C = x.shape
    S = _lib.stream_ptr()
    tx, tdz = torch.from_numpy(x).cuda(), torch.from_numpy(dz).cuda()
    tbn = torch.from_numpy(bn).cuda() if bn is not None else None
    z, dx0, dx1 = Guarded(x.size), Guarded(x.size), Guarded(x.size, prior)
    _lib.call("kws_avgpool3_same_fwd_f32", _lib.ptr(tx), _lib.ptr(tbn) if bn is not None else None, _lib.ptr(z.view), B, L, C, S)
    _lib.call("kws_avgpool3_same_bwd_f32", _lib.ptr(tdz), _lib.ptr(dx0.view), 0, B, L, C, S)
    _lib.call("kws_avgpool3_same_bwd_f32", _lib.ptr(tdz), _lib.ptr(dx1.view), 1, B, L, C, S)
    for g, what in ((z, "avgpool fwd"), (dx0, "avgpool bwd"), (dx1, "avgpool bwd (accumulate)")):
        g.check(what)
    return z, dx0, dx1


@pytest.mark.parametrize("with_table", [False, True], ids=["raw", "table"])
@pytest.mark.parametrize("B,L,C", POOL_CASES)
def test_avgpool_matches_float64(B, L, C, with_table):
    rng = np.random.RandomState(L * 7 + C + with_table)
    bn = _table(rng, C) if with_table else None
    x = (rng.randn(B, L, C) * 2.0).astype(np.float32) if with_table else (rng.rand(B, L, C) * 6.0).astype(np.float32)
    dz = rng.randn(B, L, C).astype(np.float32)
    prior = rng.randn(B, L, C).astype(np.float32)
    z, dx0, dx1 = _pool_run(x, bn, dz, prior)
    a = x.astype(np.float64)
    if with_table:
        a = np.clip(a * bn[0].astype(np.float64) + bn[1].astype(np.float64), 0, 6)
    z_ref, dx_ref = avgpool_fwd(a), avgpool_bwd(dz.astype(np.float64))
    bwd_bar = 1e-6 * avgpool_bwd(np.abs(dz).astype(np.float64))              # 1e-6 * sum |dz_t| / n_t
    gz = z.numpy().reshape(B, L, C).astype(np.float64)
    g0 = dx0.numpy().reshape(B, L, C)
    g1 = dx1.numpy().reshape(B, L, C)
    acc_ref = prior.astype(np.float64) + dx_ref
    print("avgpool (%d, %d, %d) table=%d: fwd %.3g (bar 6e-6), bwd / bar %.3g, accumulate / bar %.3g" %
          (B, L, C, with_table, np.abs(gz - z_ref).max(), (np.abs(g0 - dx_ref) / bwd_bar).max(),
           (np.abs(g1 - acc_ref) / (bwd_bar + 6e-8 * np.abs(acc_ref))).max()))
    assert np.abs(gz - z_ref).max() < 6e-6
    assert (np.abs(g0 - dx_ref) <= bwd_bar).all()
    assert np.array_equal(g1, prior + g0)                                    # one thread, one addition per element
    assert (np.abs(g1 - acc_ref) <= bwd_bar + 6e-8 * np.abs(acc_ref)).all()
    # the divisor that counts the padding: wrong at the two ends of a clip (and only there)
    z_bad, dx_bad = avgpool_fwd(a, include_pad=True), avgpool_bwd(dz.astype(np.float64), include_pad=True)
    ends = [0, L - 1]
    assert np.abs(gz - z_bad)[:, ends].max() > 6e-6
    assert (np.abs(g0 - dx_bad) > bwd_bar)[:, ends].any()
    if L > 2:
        assert np.abs(gz - z_bad)[:, 1:-1].max() < 6e-6
    again = _pool_run(x, bn, dz, prior)
    for a1, a2 in zip((z, dx0, dx1), again):
        assert torch.equal(a1.buf, a2.buf)


def test_bad_avgpool_arguments_are_refused():
    lib = _lib.load()
    out = Guarded(4096)
    x = torch.zeros(4096, device="cuda")
    S = _lib.stream_ptr()
    for B, L, C in ((2, 5, 6), (2, 0, 8), (0, 5, 8), (2, 5, 0)):
        assert lib.kws_avgpool3_same_fwd_f32(_lib.ptr(x), None, _lib.ptr(out.view), B, L, C, S) == -1
        assert b'avgpool3_same_fwd' in lib.kws_last_error()
        assert lib.kws_avgpool3_same_bwd_f32(_lib.ptr(x), _lib.ptr(out.view), 0, B, L, C, S) == -1
        assert b'avgpool3_same_bwd' in lib.kws_last_error()
    assert lib.kws_avgpool3_same_bwd_f32(_lib.ptr(x), _lib.ptr(out.view), 3, 2, 5, 8, S) == -1
    out.check("a refused call", np.ones(4096, bool))
