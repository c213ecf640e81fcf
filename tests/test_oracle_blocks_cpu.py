"""The shared layer math of the family oracles (tests/oracle_blocks.py), each primitive directly against torch autograd in float64.
Bars, the family cross-checks': forward 1e-12 absolute, gradients 1e-9 of the tensor's maximum.  Shapes are the smallest that meet
every branch: B 2, L 11 (10 where the total SAME padding has to be odd), a handful of channels."""
import numpy as np
import pytest
import torch
import torch.nn.functional as Fn

from oracle_blocks import (OracleNet, bn_train_bwd, bn_train_fwd, conv_bwd, conv_fwd, dw_bwd, dw_fwd, gconv_bwd, gconv_fwd, glorot,
                           same_geometry)

FWD_ATOL, GRAD_RTOL = 1e-12, 1e-9


def _grad_close(got, want, what):
    want = want.numpy()
    err = np.abs(got - want).max() / max(np.abs(want).max(), 1e-300)
    assert got.shape == want.shape and err < GRAD_RTOL, (what, err)


def _tf_same(L, k, s, dil):
    """TensorFlow's SAME rule, restated: ceil(L / s) outputs, the smaller half of the padding in front"""
    Lout = -(-L // s)
    total = max((Lout - 1) * s + dil * (k - 1) + 1 - L, 0)
    return Lout, total // 2, total - total // 2


# ---- dense Conv1D --------------------------------------------------------------------------------------------------------------
B, L, CIN, F = 2, 11, 3, 4
CONV_SHAPES = [(k, s, d) for k in (1, 3, 5) for s in (1, 2) for d in (1, 2)]


L_ODD_PAD = 10        # with odd k the total SAME padding of L = 11 is even at either stride; at L = 10, stride 2 it is odd


def _conv_geometry(geom, k, s, d):
    """-> (input length, pad_l, Lout, pad_r): VALID, SAME (at L = 11: an even total padding), SAME at L = 10 (an odd one), and a left
    padding with an explicit output length (one window fewer than fits, so rows at the end are read by no tap)"""
    span = d * (k - 1)
    if geom == 'valid':
        return L, 0, None, 0
    if geom == 'left2':
        return L, 2, (L + 2 - span - 1) // s, 0
    Lin = L if geom == 'same' else L_ODD_PAD
    Lout, pl, pr = _tf_same(Lin, k, s, d)
    return Lin, pl, Lout, pr


CONV_CASES = [(g, k, s, d) for g in ('valid', 'same', 'left2') for k, s, d in CONV_SHAPES] + \
             [('same_odd', k, 2, d) for k in (3, 5) for d in (1, 2)]


def test_same_geometry_meets_odd_and_even_paddings():
    totals = {g: [sum(_conv_geometry(g, k, s, d)[1::2]) for gg, k, s, d in CONV_CASES if gg == g] for g in ('same', 'same_odd')}
    assert all(t % 2 == 0 for t in totals['same']) and any(t > 0 for t in totals['same']) and all(t % 2 == 1 for t in totals['same_odd'])
    for Lin in (L, L_ODD_PAD):
        for k, s, d in CONV_SHAPES:
            Lout, pl, pr = _tf_same(Lin, k, s, d)
            assert same_geometry(Lin, k, s, d) == (Lout, pl, pr) and pr - pl in (0, 1)          # the odd sample goes behind
            assert same_geometry(Lin, k, s, d, odd_left=True) == (Lout, pr, pl)


@pytest.mark.parametrize("geom,k,s,d", CONV_CASES)
def test_dense_conv_matches_torch_autograd(geom, k, s, d):
    Lin, pad_l, Lout, pad_r = _conv_geometry(geom, k, s, d)
    rng = np.random.RandomState(100 * k + 10 * s + d)
    a, W = rng.randn(B, Lin, CIN), rng.randn(k, CIN, F)
    y, ap = conv_fwd(a, W, s, d, pad_l, Lout)
    ta, tW = torch.tensor(a, requires_grad=True), torch.tensor(W, requires_grad=True)
    ty = Fn.conv1d(Fn.pad(ta.permute(0, 2, 1), (pad_l, pad_r)), tW.permute(2, 1, 0), stride=s, dilation=d).permute(0, 2, 1)
    if Lout is not None:
        ty = ty[:, :Lout]
    assert y.shape == tuple(ty.shape) and y.shape[1] >= 1
    assert np.abs(y - ty.detach().numpy()).max() < FWD_ATOL
    dy = rng.randn(*y.shape)
    ty.backward(torch.tensor(dy))
    dx, dW = conv_bwd(dy, ap, W, Lin, s, d, pad_l)
    _grad_close(dx, ta.grad, 'dx')
    _grad_close(dW, tW.grad, 'dW')
    assert conv_bwd(dy, ap, W, Lin, s, d, pad_l, need_dx=False)[0] is None


def test_dense_conv_pad_value_fills_the_padding():
    rng = np.random.RandomState(3)
    a, W, v = rng.randn(B, L, CIN), rng.randn(3, CIN, F), rng.randn(CIN)
    y, ap = conv_fwd(a, W, 1, 1, 1, L, pad_value=v)
    want = conv_fwd(np.concatenate([np.broadcast_to(v, (B, 1, CIN)), a, np.broadcast_to(v, (B, 1, CIN))], axis=1), W)[0]
    assert np.array_equal(ap[:, 0], np.broadcast_to(v, (B, CIN))) and np.abs(y - want).max() < FWD_ATOL


def test_grouped_conv_matches_torch_autograd():
    g, gs, Ng, k, s = 2, 3, 2, 3, 2
    rng = np.random.RandomState(5)
    x, Ws = rng.randn(B, L, g * gs + 1), [rng.randn(k, gs, Ng) for _ in range(g)]        # one channel outside every group
    y = gconv_fwd(x, Ws, k, s, gs)
    tx, tWs = torch.tensor(x, requires_grad=True), [torch.tensor(W, requires_grad=True) for W in Ws]
    ty = torch.cat([Fn.conv1d(tx[:, :, q * gs:(q + 1) * gs].permute(0, 2, 1), tW.permute(2, 1, 0), stride=s).permute(0, 2, 1)
                    for q, tW in enumerate(tWs)], dim=2)
    assert np.abs(y - ty.detach().numpy()).max() < FWD_ATOL
    dy = rng.randn(*y.shape)
    ty.backward(torch.tensor(dy))
    dx, dWs = gconv_bwd(dy, x, Ws, k, s, gs)
    _grad_close(dx, tx.grad, 'dx')
    assert not dx[:, :, -1].any()
    for q in range(g):
        _grad_close(dWs[q], tWs[q].grad, 'dW%d' % q)
    assert np.array_equal(gconv_fwd(x, Ws, k, s, gs, reverse=True), np.concatenate([y[:, :, Ng:], y[:, :, :Ng]], axis=2))
    swapped = gconv_bwd(dy, x, Ws, k, s, gs, swap_phase=True)[0]
    assert np.array_equal(swapped[:, 0:10:2], dx[:, 1:10:2]) and np.array_equal(swapped[:, 10], dx[:, 10])


# ---- depthwise Conv1D ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("k,s,L_in,same", [(4, 3, 10, True), (3, 2, 10, False)])
def test_depthwise_conv_matches_torch_autograd(k, s, L_in, same):
    C = 4
    if same:
        Lout, pad_l, pad_r = _tf_same(L_in, k, s, 1)
        assert (pad_l + pad_r) % 2 == 1
    else:
        Lout, pad_l, pad_r = (L_in - k) // s + 1, 0, 0
        assert s * (Lout - 1) + k < L_in                                       # the last row is read by no tap
    rng = np.random.RandomState(k + s)
    a, w, dz = rng.randn(B, L_in, C), rng.randn(k, C), rng.randn(B, Lout, C)
    z = dw_fwd(a, w, s, pad_l, Lout)
    ta, tw = torch.tensor(a, requires_grad=True), torch.tensor(w, requires_grad=True)
    tz = Fn.conv1d(Fn.pad(ta.permute(0, 2, 1), (pad_l, pad_r)), tw.t().reshape(C, 1, k), stride=s, groups=C).permute(0, 2, 1)
    assert z.shape == tuple(tz.shape) == (B, Lout, C)
    assert np.abs(z - tz.detach().numpy()).max() < FWD_ATOL
    tz.backward(torch.tensor(dz))
    da, dw = dw_bwd(dz, a, w, s, pad_l)
    _grad_close(da, ta.grad, 'da')
    _grad_close(dw, tw.grad, 'dw')
    if not same:
        assert not da[:, -1].any()


# ---- BatchNorm + relu6 -------------------------------------------------------------------------------------------------------------
def _bn_net(C, seed=2):
    """An OracleNet with one BatchNormalization: a negative and a positive scale among its channels"""
    net = OracleNet(12, seed)
    n = net.add_bn(C)
    rng = np.random.RandomState(seed)
    net.params['batch_normalization_1/gamma'] = (np.where(np.arange(C) % 2, -1.0, 1.0) * (1.0 + 0.2 * rng.rand(C))).astype(np.float32)
    net.params['batch_normalization_1/beta'] = (3.0 + rng.randn(C)).astype(np.float32)
    return net, n


def _torch_bn_relu6(y, ga, be):
    pre = Fn.batch_norm(y.permute(0, 2, 1), None, None, ga, be, training=True, eps=1e-3).permute(0, 2, 1)
    return pre, torch.clamp(pre, 0, 6)


def test_bn_act_matches_torch_autograd_with_negative_scales():
    C = 5
    net, n = _bn_net(C)
    rng = np.random.RandomState(4)
    y, dout = 2.0 * rng.randn(B, L, C), rng.randn(B, L, C)
    cache = {'batch_stats': {}}
    a = net.bn_act_fwd(n, y, True, cache)
    ty = torch.tensor(y, requires_grad=True)
    tga = torch.tensor(net.params['batch_normalization_1/gamma'].astype(np.float64), requires_grad=True)
    tbe = torch.tensor(net.params['batch_normalization_1/beta'].astype(np.float64), requires_grad=True)
    tpre, ta = _torch_bn_relu6(ty, tga, tbe)
    assert (tga < 0).any() and (tpre < 0).any() and (tpre > 6).any() and ((tpre > 0) & (tpre < 6)).any()
    assert np.abs(a - ta.detach().numpy()).max() < FWD_ATOL
    mean, var = cache['batch_stats'][n]
    assert np.abs(mean - y.mean(axis=(0, 1))).max() < FWD_ATOL and np.abs(var - y.var(axis=(0, 1))).max() < FWD_ATOL
    ta.backward(torch.tensor(dout))
    grads = {}
    dy = net.bn_act_bwd(n, dout, cache, grads)
    _grad_close(dy, ty.grad, 'dy')
    _grad_close(grads['batch_normalization_1/gamma'], tga.grad, 'dgamma')
    _grad_close(grads['batch_normalization_1/beta'], tbe.grad, 'dbeta')
    # a gate handed in replaces the forward pass's own; none at all is the 'no_gate' mutation
    ones = {n: np.ones_like(y)}
    assert np.array_equal(net.bn_act_bwd(n, dout, cache, {}, ones), net.bn_act_bwd(n, dout, cache, {}, gate=False))
    assert np.abs(net.bn_act_bwd(n, dout, cache, {}, ones) - dy).max() > 1e-3
    # inference: the moving statistics
    net.state['batch_normalization_1/moving_mean'] = rng.randn(C).astype(np.float32)
    net.state['batch_normalization_1/moving_variance'] = (1.0 + rng.rand(C)).astype(np.float32)
    tinf = Fn.batch_norm(torch.tensor(y).permute(0, 2, 1), torch.tensor(net.state['batch_normalization_1/moving_mean'].astype(np.float64)),
                         torch.tensor(net.state['batch_normalization_1/moving_variance'].astype(np.float64)), tga.detach(), tbe.detach(),
                         training=False, eps=1e-3).permute(0, 2, 1)
    assert np.abs(net.bn_act_fwd(n, y, False, None) - torch.clamp(tinf, 0, 6).numpy()).max() < FWD_ATOL


def test_relu6_gate_at_exactly_0_and_6():
    """pre > 0 && pre <= 6.  Batch statistics do not land a pre-activation on 0 or 6 exactly, so the forward pass's cached
    pre-activation, which the backward pass gates on, is pinned there and one step to either side."""
    net, n = _bn_net(2)
    rng = np.random.RandomState(8)
    y = rng.randn(B, L, 2)
    cache = {'batch_stats': {}}
    net.bn_act_fwd(n, y, True, cache)
    pre = cache['bn%d' % n]['pre']
    pre[0, 0, 0], pre[0, 1, 0], pre[0, 2, 0], pre[0, 3, 0] = 0.0, 6.0, np.nextafter(0.0, 1.0), np.nextafter(6.0, 7.0)
    keep = net.gate(n, cache)
    assert keep[0, :4, 0].tolist() == [0.0, 1.0, 1.0, 0.0] and np.array_equal(keep, (pre > 0) & (pre <= 6))
    dout = rng.randn(*y.shape)
    assert np.array_equal(net.bn_act_bwd(n, dout, cache, {}), net.bn_act_bwd(n, dout * keep, cache, {}, gate=False))


def test_float32_batchnorm_sums_are_the_float64_sums_cast_down():
    C = 3
    rng = np.random.RandomState(6)
    y = (100.0 + rng.randn(B, 4000, C)).astype(np.float32)       # a float32 running sum of 8000 values near 100 loses digits
    ga, be = (1.0 + rng.rand(C)).astype(np.float32), rng.randn(C).astype(np.float32)
    pre, (mean, var, rstd) = bn_train_fwd(y, ga, be)
    y64 = y.astype(np.float64)
    m64 = y64.mean(axis=(0, 1))
    v64 = ((y - m64) ** 2).mean(axis=(0, 1), dtype=np.float64)
    assert pre.dtype == mean.dtype == var.dtype == rstd.dtype == np.float32
    assert np.array_equal(mean, m64.astype(np.float32)) and np.array_equal(var, v64.astype(np.float32))
    assert np.array_equal(rstd, (1.0 / np.sqrt(v64 + 1e-3)).astype(np.float32))
    dout = rng.randn(B, 4000, C).astype(np.float32)
    dy, dga, dbe = bn_train_bwd(dout, y, ga, (mean, var, rstd))
    xhat = (y - mean) * rstd
    assert dy.dtype == dga.dtype == dbe.dtype == np.float32
    assert np.array_equal(dbe, dout.sum(axis=(0, 1), dtype=np.float64).astype(np.float32))
    assert np.array_equal(dga, (dout * xhat).sum(axis=(0, 1), dtype=np.float64).astype(np.float32))
    # in float64 it is oracle.layers' function
    from oracle import layers as OL
    p64, st64 = bn_train_fwd(y64, ga.astype(np.float64), be.astype(np.float64))
    q64, su64 = OL.bn_train_fwd(y64, ga.astype(np.float64), be.astype(np.float64))
    assert np.array_equal(p64, q64) and all(np.array_equal(u, v) for u, v in zip(st64, su64))
    for u, v in zip(bn_train_bwd(dout.astype(np.float64), y64, ga.astype(np.float64), st64),
                    OL.bn_train_bwd(dout.astype(np.float64), y64, ga.astype(np.float64), su64)):
        assert np.array_equal(u, v)


# ---- glorot, dropout, head -----------------------------------------------------------------------------------------------------------
def test_glorot_is_keras_glorot_uniform_in_draw_order():
    got = glorot(np.random.RandomState(1234), (3, 5, 7), 15, 21)
    rng = np.random.RandomState(1234)
    lim = np.sqrt(6.0 / (15 + 21))
    want = np.array([rng.uniform(-lim, lim) for _ in range(3 * 5 * 7)]).reshape(3, 5, 7).astype(np.float32)
    assert got.dtype == np.float32 and np.array_equal(got, want)
    net = OracleNet(12, 1234)
    assert net.add_kernel('conv1d', (3, 5, 7), 15, 21, l2=True, bias=7) == 'conv1d_1/kernel'
    assert net.add_kernel('conv1d', (1, 7, 2), 7, 2) == 'conv1d_2/kernel' and net.add_bn(2) == 1
    assert np.array_equal(net.params['conv1d_1/kernel'], want) and not net.params['conv1d_1/bias'].any()
    assert list(net.params) == ['conv1d_1/kernel', 'conv1d_1/bias', 'conv1d_2/kernel', 'batch_normalization_1/gamma',
                                'batch_normalization_1/beta']
    assert list(net.state) == ['batch_normalization_1/moving_mean', 'batch_normalization_1/moving_variance']
    assert net.l2_names == ['conv1d_1/kernel'] and net.count_params() == 105 + 7 + 14 + 8


def test_head_matches_torch_autograd():
    net = OracleNet(12, 9)
    kernel = net.add_kernel('conv1d', (2, 3, 12), 6, 24, bias=12)              # a Conv1D kernel used as Dense over its 6 inputs
    net.params['conv1d_1/bias'] = np.random.RandomState(1).randn(12).astype(np.float32)
    rng = np.random.RandomState(2)
    f, y = rng.randn(B, 6), np.eye(12)[[3, 7]]
    p = net.head_fwd(f, kernel, 'conv1d_1/bias')
    tf_, tW, tb = (torch.tensor(v, requires_grad=True) for v in (f, net._p(kernel).reshape(6, 12), net._p('conv1d_1/bias')))
    tp = torch.softmax(tf_ @ tW + tb, dim=1)
    assert np.abs(p - tp.detach().numpy()).max() < FWD_ATOL
    tpn = tp / tp.sum(dim=1, keepdim=True)
    tloss = -(torch.tensor(y) * torch.log(torch.clamp(tpn, 1e-7, 1 - 1e-7))).sum(dim=1).mean()
    tloss.backward()
    grads = {}
    loss, df = net.head_bwd(p, y, f, kernel, 'conv1d_1/bias', grads)
    assert abs(loss - float(tloss.detach())) < FWD_ATOL
    _grad_close(df, tf_.grad, 'df')
    _grad_close(grads[kernel].reshape(6, 12), tW.grad, 'dW')
    _grad_close(grads['conv1d_1/bias'], tb.grad, 'db')
    assert grads[kernel].shape == (2, 3, 12) and list(net.ordered(dict(grads, extra=0))) == list(net.params)
