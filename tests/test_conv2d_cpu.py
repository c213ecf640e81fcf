"""CPU checks of the 2-D family (kws_conv2d_*, kws_pool2x2_*, KWS_NET_CONV_2D_MOBILE / KWS_NET_CONV_2D_FAST): the oracle
(tests/conv2d_oracle.py) against torch's conv2d / max_pool2d / autograd in float64; the fixture recorded from the reference
(tests/golden/conv2d_models.json, made by tests/golden/make_golden_conv2d.py) against the oracle's tables and the native tensor
table - weight names and shapes in Keras order, every pad pair; the speech_model surface; the oracle's mutations; and the float32
runs of the oracle against its float64 self on the GPU tests' own shapes, weights and batches (the figures of the GPU tests'
docstrings)."""
import ctypes
import json
import os

import numpy as np
import pytest
import torch
import torch.nn.functional as Fn

import conv2d_cases as cases
from conv2d_oracle import (ACT, KEEP_LADDER, LADDERS, SGD, Conv2dNet, axis_geom, conv2d_bwd, conv2d_fwd, pool2_argmax, pool2_bwd,
                           pool2_fwd, preprocess)
from net_parity import native_table
from oracle.layers import dropout_key, dropout_mask, sgd_momentum_step
from speech_recognition_amd import _lib

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden', 'conv2d_models.json')
KINDS = {'mobile': 15, 'fast': 16}
IMAGES = {'mobile': [(49, 20), (49, 20), (25, 10), (25, 10), (13, 5), (13, 5), (7, 3), (7, 3)],
          'fast': [(98, 40), (49, 20), (24, 10), (12, 5)]}


def _golden(kind):
    with open(GOLDEN) as f:
        return json.load(f)['conv_2d_' + kind]


def test_kind_constants_and_descriptor():
    assert (_lib.KWS_NET_CONV_2D_MOBILE, _lib.KWS_NET_CONV_2D_FAST) == (15, 16)
    assert (_lib.ACT_RELU6, _lib.ACT_RELU) == (0, 1)
    assert ctypes.sizeof(_lib.Conv2dDesc) == 16 * 4
    assert [f[0] for f in _lib.Conv2dDesc._fields_] == ['B', 'H', 'W', 'Hout', 'Wout', 'kh', 'kw', 'sh', 'sw', 'dh', 'dw', 'pad_t', 'pad_l',
                                                        'Cin', 'F', 'act']


# ---- the op and the pool against torch ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("c", cases.CONV_CASES, ids=[cases.conv_id(c) for c in cases.CONV_CASES])
def test_oracle_conv2d_matches_torch(c):
    rng = np.random.RandomState(1)
    x = rng.randn(c['B'], c['H'], c['W'], c['Cin'])
    W = rng.randn(c['kh'], c['kw'], c['Cin'], c['F'])
    y, ap = conv2d_fwd(x, W, c['s'], c['d'], c['pads'], (c['Hout'], c['Wout']))
    dy = rng.randn(*y.shape)
    dx, dW = conv2d_bwd(dy, ap, W, c['s'], c['d'], c['pads'], (c['H'], c['W']))
    tx = torch.tensor(x).permute(0, 3, 1, 2).requires_grad_(True)
    tw = torch.tensor(W).permute(3, 2, 0, 1).requires_grad_(True)
    (pt, pb), (pl, pr) = c['pads']
    ty = Fn.conv2d(Fn.pad(tx, (pl, pr, pt, pb)), tw, stride=c['s'], dilation=c['d'])
    ty.backward(torch.tensor(dy).permute(0, 3, 1, 2))
    np.testing.assert_allclose(y, ty.detach().permute(0, 2, 3, 1).numpy(), atol=1e-12)
    np.testing.assert_allclose(dx, tx.grad.permute(0, 2, 3, 1).numpy(), atol=1e-12)
    np.testing.assert_allclose(dW, tw.grad.permute(2, 3, 1, 0).numpy(), atol=1e-11)


def test_same_geometry_is_tensorflows():
    assert axis_geom(98, 3, 2) == (49, (0, 1)) and axis_geom(49, 3, 2) == (25, (1, 1)) and axis_geom(40, 3, 2) == (20, (0, 1))
    assert axis_geom(98, 11, 1, 2) == (98, (10, 10)) and axis_geom(24, 20) == (24, (9, 10)) and axis_geom(10, 8) == (10, (3, 4))
    assert axis_geom(7, 1, 2) == (4, (0, 0)) and axis_geom(8, 3, 2, 1, 'valid') == (3, (0, 0)) and axis_geom(1, 3) == (1, (1, 1))


@pytest.mark.parametrize("B,H,W,C", cases.POOL_CASES)
def test_oracle_pool_matches_torch(B, H, W, C):
    rng = np.random.RandomState(H + C)
    a = rng.rand(B, H, W, C) * 8.0                      # distinct values: no ties, torch's choice among equals does not matter
    ta = torch.tensor(a, requires_grad=True)
    tz = Fn.max_pool2d(ta.permute(0, 3, 1, 2), 2, 2).permute(0, 2, 3, 1)
    ind = pool2_argmax(a)
    np.testing.assert_array_equal(pool2_fwd(a, ind), tz.detach().numpy())
    dz = rng.randn(*tz.shape)
    tz.backward(torch.tensor(dz))
    np.testing.assert_array_equal(pool2_bwd(dz, ind, H, W), ta.grad.numpy())
    # first / last maximum of a tied window
    t = np.zeros((1, 2, 2, 1))
    t[0, :, :, 0] = [[1, 3], [3, 3]]
    assert pool2_argmax(t)[0, 0, 0, 0] == 1 and pool2_argmax(t, last=True)[0, 0, 0, 0] == 3


def test_float32_restatement_is_under_half_the_kernel_bar():
    """The oracle's convolution in float32 against float64 on every kernel case (the largest reductions: K = 320 forward, 864 in
    an input gradient, 390 rows in a weight gradient): what the number format alone costs, against the kernel tests' 1e-5 bar."""
    worst = 0.0
    for c in cases.CONV_CASES:
        rng = np.random.RandomState(1)
        x = rng.randn(c['B'], c['H'], c['W'], c['Cin'])
        W = rng.randn(c['kh'], c['kw'], c['Cin'], c['F']) / np.sqrt(c['kh'] * c['kw'] * c['Cin'])
        y, ap = conv2d_fwd(x, W, c['s'], c['d'], c['pads'])
        dy = rng.randn(*y.shape)
        dx, dW = conv2d_bwd(dy, ap, W, c['s'], c['d'], c['pads'], (c['H'], c['W']))
        y32, ap32 = conv2d_fwd(x.astype(np.float32), W.astype(np.float32), c['s'], c['d'], c['pads'])
        dx32, dW32 = conv2d_bwd(dy.astype(np.float32), ap32, W.astype(np.float32), c['s'], c['d'], c['pads'], (c['H'], c['W']))
        worst = max([worst] + [np.abs(a - b).max() / np.abs(b).max() for a, b in ((y32, y), (dx32, dx), (dW32, dW))])
    print("float32 restatement of the convolution: worst %.3g of a tensor's maximum (bar 1e-5)" % worst)
    assert worst < 0.5 * 1e-5


# ---- the fixture, the oracle's tables and the native table ----------------------------------------------------------------------
@pytest.mark.parametrize("kind", cases.KINDS)
def test_fixture_matches_oracle_and_native_table(kind):
    gold = _golden(kind)
    ora = Conv2dNet(kind, num_classes=12)
    lr, momentum = SGD[kind]
    assert (gold['model_name'], gold['optimizer'], gold['lr'], gold['momentum'], gold['loss']) == \
        ('conv_2d_' + kind, 'SGD', lr, momentum, 'categorical_crossentropy')
    assert not gold['nesterov'] and not gold['decay'] and gold['output_shape'] == [12] and gold['input_size'] == 3920
    layers = gold['layers']
    assert layers[0]['class'] == 'Reshape' and layers[0]['output'] == [98, 40, 1]
    assert layers[1]['class'] == 'Lambda' and layers[1]['ops'] == [['add', 0.8], ['div', 7.0], ['clip', -5, 5]]
    convs = [l for l in layers if l['class'] == 'Conv2D']
    assert len(convs) == len(ora.layers) == len(LADDERS[kind])
    assert [tuple(c['output'][:2]) for c in convs] == IMAGES[kind]
    for c, l in zip(convs, ora.layers):                          # geometry: every pad pair and output shape
        assert c['name'] == 'conv2d_%d' % l['idx'] and c['use_bias'] and c['padding'] == 'same' and c['activation'] is None
        assert (c['kernel'], tuple(c['strides']), tuple(c['dilation_rate'])) == ([l['k'][0], l['k'][1], l['C'], l['F']], l['strides'], l['dil'])
        assert (c['input'], c['output']) == ([l['H'], l['W'], l['C']], [l['Hout'], l['Wout'], l['F']])
        assert tuple(map(tuple, c['pads'])) == l['pads'], c['name']
    acts = [l['function'] for l in layers if l['class'] == 'Activation']
    assert acts == [ACT[kind]] * len(convs)
    pools = [l for l in layers if l['class'] == 'MaxPool2D']
    assert len(pools) == sum(l['pool'] for l in ora.layers)
    for pl, l in zip(pools, [l for l in ora.layers if l['pool']]):
        assert (pl['pool_size'], pl['strides'], pl['padding']) == ([2, 2], [2, 2], 'valid')
        assert (pl['input'], pl['output']) == ([l['Hout'], l['Wout'], l['F']], [l['Ho'], l['Wo'], l['F']])
    # where the layers stand: conv -> BN -> activation (-> pool) (-> dropout behind every second one of conv_2d_mobile)
    seq = [l['class'] for l in layers[2:]]
    want = []
    for l in ora.layers:
        want += ['Conv2D', 'BatchNormalization', 'Activation'] + (['MaxPool2D'] if l['pool'] else []) + (['Dropout'] if l['drop_id'] else [])
    want += ['GlobalAveragePooling2D'] + (['Dropout'] if kind == 'mobile' else []) + ['Dense']
    assert seq == want
    rates = [l['rate'] for l in layers if l['class'] == 'Dropout']
    assert rates == ([0.05] * 4 + [0.1] if kind == 'mobile' else [])
    assert [l['drop_id'] for l in ora.layers if l['drop_id']] == ([2, 3, 4, 5] if kind == 'mobile' else [])
    assert abs((1 - KEEP_LADDER) - 0.05) < 1e-12 and abs((1 - ora.keep_tail) - (0.1 if kind == 'mobile' else 0.0)) < 1e-12
    gap = next(l for l in layers if l['class'] == 'GlobalAveragePooling2D')
    assert gap['input'][0] * gap['input'][1] == ora.T and gap['output'] == [ora.C]
    assert (ora.T, ora.C) == ((21, 256) if kind == 'mobile' else (12, 128))
    # weights: names and shapes in Keras order - fixture, oracle, native table
    table = native_table(KINDS[kind], 12, 3920)
    names = [w['name'] for w in gold['weights']]
    assert [t.name.decode() for t in table] == names
    assert names[:6] == ['conv2d_1/kernel', 'conv2d_1/bias', 'batch_normalization_1/gamma', 'batch_normalization_1/beta',
                         'batch_normalization_1/moving_mean', 'batch_normalization_1/moving_variance']
    assert names[-2:] == ['dense_1/kernel', 'dense_1/bias']
    merged = dict(ora.params, **ora.state)
    assert [n for n in names if n in ora.params] == list(ora.params) and [n for n in names if n in ora.state] == list(ora.state)
    for t, w in zip(table, gold['weights']):
        shape = [int(t.shape[k]) for k in range(t.ndim)]
        assert shape == w['shape'] == list(merged[w['name']].shape), w['name']
        assert bool(t.is_state) == bool(w.get('state', False)) and t.l2 == 0.0
        if w['name'].endswith('/kernel') and w['name'].startswith('conv2d'):      # glorot fans kh*kw*Cin / kh*kw*F
            kh, kw, cin, f = w['shape']
            assert (t.fan_in, t.fan_out) == (kh * kw * cin, kh * kw * f)
        if w['name'].endswith('/bias'):
            assert t.fan_in == 0 and t.init == 0.0                               # zeros
    assert sum(t.size for t in table) == ora.count_params()


@pytest.mark.parametrize("kind", cases.KINDS)
def test_native_table_rejects_other_input_sizes(kind):
    lib = _lib.load()
    cfg = _lib.NetConfig(KINDS[kind], 12, 1, 16000, 0, 0)
    h = ctypes.c_void_p()
    assert lib.kws_net_create(ctypes.byref(cfg), ctypes.byref(h)) != 0
    assert b'input_size' in lib.kws_last_error()


@pytest.mark.parametrize("kind", cases.KINDS)
def test_speech_model_surface(monkeypatch, kind):
    """speech_model('conv_2d_mobile' / 'conv_2d_fast') asks for kinds 15 / 16, keras_api.SGD with the reference's lr and momentum,
    the Keras name and 'cce' (the device net itself replaced: no GPU here); another input size is a ValueError; conv_2d itself
    stays unbuilt."""
    from speech_recognition_amd import keras_api, model as M

    class FakeNet(object):
        def __init__(self, k, num_classes, **kw):
            self.kind, self.num_classes, self.kw = k, num_classes, kw

    captured = {}

    def fake_model(net, optimizer, name=None, loss=None):
        captured.update(net=net, optimizer=optimizer, name=name, loss=loss)
        return captured

    monkeypatch.setattr(M, 'DeviceNet', FakeNet)
    monkeypatch.setattr(M, 'Model', fake_model)
    name = 'conv_2d_' + kind
    assert name in M.ACCELERATED and 'conv_2d' not in M.ACCELERATED
    M.speech_model(name, 3920, num_classes=12)
    assert captured['net'].kind == KINDS[kind] and captured['net'].num_classes == 12 and captured['net'].kw['input_size'] == 3920
    assert captured['name'] == name and captured['loss'] == 'cce'
    opt = captured['optimizer']
    lr, momentum = SGD[kind]
    assert isinstance(opt, keras_api.SGD) and abs(float(opt.lr) - lr) < 1e-9 and opt.momentum == momentum
    assert opt.extra_slots(None) == [] and opt.get_scalars() == []       # the velocity is net.slots: checkpoints and broadcasts carry it
    for bad in (16000, 3919):
        with pytest.raises(ValueError):
            M.speech_model(name, bad, num_classes=12)
    with pytest.raises(NotImplementedError) as e:
        M.speech_model('conv_2d', 3920, num_classes=12)
    assert name in str(e.value)


# ---- the oracle nets against torch autograd -----------------------------------------------------------------------------------------
def _torch_loss(ora, x, y, seed, step):
    """The same network in torch float64: F.conv2d over explicitly padded images WITH the bias, F.batch_norm in training mode
    (eps 1e-3), clamp, F.max_pool2d, the oracle's dropout masks, global average, softmax + categorical CE."""
    P = {k: torch.tensor(v.astype(np.float64), requires_grad=True) for k, v in ora.params.items()}
    B = x.shape[0]
    h = torch.tensor(preprocess(x.astype(np.float64))).reshape(B, 1, 98, 40)
    for l in ora.layers:
        n = l['idx']
        (pt, pb), (pl, pr) = l['pads']
        h = Fn.conv2d(Fn.pad(h, (pl, pr, pt, pb)), P['conv2d_%d/kernel' % n].permute(3, 2, 0, 1), P['conv2d_%d/bias' % n],
                      stride=l['strides'], dilation=l['dil'])
        h = Fn.batch_norm(h, None, None, P['batch_normalization_%d/gamma' % n], P['batch_normalization_%d/beta' % n], training=True,
                          eps=1e-3)
        h = h.clamp(0, 6) if ora.act == 'relu6' else h.clamp(min=0)
        if l['pool']:
            h = Fn.max_pool2d(h, 2, 2)
        if l['drop_id']:
            nhwc = h.permute(0, 2, 3, 1)
            keep = dropout_mask(dropout_key(seed, step, l['drop_id']), nhwc.numel(), KEEP_LADDER).reshape(nhwc.shape)
            h = (nhwc * torch.tensor(keep.astype(np.float64)) / KEEP_LADDER).permute(0, 3, 1, 2)
    f = h.mean(dim=(2, 3))
    if ora.keep_tail < 1.0:
        keep = dropout_mask(dropout_key(seed, step, 1), f.numel(), ora.keep_tail).reshape(f.shape)
        f = f * torch.tensor(keep.astype(np.float64)) / ora.keep_tail
    p = torch.softmax(f @ P['dense_1/kernel'] + P['dense_1/bias'], dim=1)
    loss = -(torch.tensor(y.astype(np.float64)) * torch.log(p.clamp(1e-7, 1 - 1e-7))).sum(1).mean()
    loss.backward()
    return float(loss.detach()), p.detach().numpy(), {k: v.grad.numpy() for k, v in P.items()}


@pytest.mark.parametrize("kind", cases.KINDS)
def test_oracle_gradients_match_torch_autograd(kind):
    ora = cases.perturbed(kind)
    assert 0.2 < np.mean([(v < 0).mean() for k, v in ora.params.items() if k.endswith('gamma')]) < 0.45
    x, y = cases.batch(3, seed=7)
    loss, p, grads, cache = ora.loss_and_grads(x, y, seed=3, step=5)
    tl, tp, tg = _torch_loss(ora, x, y, seed=3, step=5)
    assert abs(loss - tl) < 1e-10
    np.testing.assert_allclose(p, tp, atol=1e-12)
    for k, g in grads.items():
        if k.startswith('conv2d_') and k.endswith('bias'):       # zero up to rounding on both sides
            assert np.abs(g).max() < 1e-12 and np.abs(tg[k]).max() < 1e-12, k
            continue
        scale = max(np.abs(tg[k]).max(), 1e-12)
        assert np.abs(g.reshape(tg[k].shape) - tg[k]).max() / scale < 1e-9, k
    assert (np.abs(preprocess(x.astype(np.float64))) == 5).any()          # the clip of Preprocess is exercised


@pytest.mark.parametrize("kind", cases.KINDS)
def test_predict_uses_the_bias_and_the_moving_statistics(kind):
    """Inference runs on moving statistics, where the convolution bias does not cancel: dropping it moves the probabilities."""
    ora = cases.perturbed(kind)
    x, _ = cases.batch(4, seed=2)
    p = ora.forward(x, training=False)
    assert np.abs(p.sum(1) - 1).max() < 1e-12
    nb = cases.perturbed(kind)
    for k in nb.params:
        if k.startswith('conv2d_') and k.endswith('bias'):
            nb.params[k] = np.zeros_like(nb.params[k])
    assert np.abs(nb.forward(x, training=False) - p).max() > 1e-4
    # ... and in training it does cancel
    pt, pn = ora.forward(x, training=True, seed=1), nb.forward(x, training=True, seed=1)
    assert np.abs(pt - pn).max() < 1e-12


@pytest.mark.parametrize("kind,mutate", [('mobile', 'pad_front'), ('fast', 'pad_front')])
def test_mutated_oracle_moves_the_gradients(kind, mutate):
    """Negative control on the oracle itself: each wrong variant moves some gradient by more than 1e-2 relative, far past the 2e-4
    bar of the GPU tests.  (pad_front on conv_2d_fast: its windows are odd at stride 1, the padding is symmetric, nothing moves.)"""
    ora = cases.perturbed(kind)
    x, y = cases.batch(3)
    _, _, good, _ = ora.loss_and_grads(x, y, seed=1, step=0)
    _, _, bad, _ = ora.loss_and_grads(x, y, seed=1, step=0, mutate=mutate)
    err = max(cases.grad_errors(bad, good).values())
    if (kind, mutate) == ('fast', 'pad_front'):
        assert err == 0.0
    else:
        assert err > 1e-2, err


def test_sgd_momentum_rule_is_keras_2_1_2():
    """v' = momentum v - lr g; p' = p + v' (no Nesterov, no decay): two steps by hand."""
    p, v = np.array([1.0, -2.0]), np.zeros(2)
    g = np.array([0.5, 0.25])
    p, v = sgd_momentum_step(p, g, v, 1e-3, 0.95)
    np.testing.assert_allclose(v, -1e-3 * g, rtol=1e-15)
    p2, v2 = sgd_momentum_step(p, g, v, 1e-3, 0.95)
    np.testing.assert_allclose(v2, -1e-3 * g * 1.95, rtol=1e-15)
    np.testing.assert_allclose(p2, np.array([1.0, -2.0]) - 1e-3 * g * 2.95, rtol=1e-15)


# ---- float32 against float64: what the number format alone costs at the GPU tests' cases ----------------------------------------
@pytest.mark.parametrize("kind", cases.KINDS)
def test_float32_oracle_predict_is_within_half_the_gpu_bar(kind):
    x = cases.batch(cases.PREDICT_BATCH, seed=1)[0]
    ref = cases.perturbed(kind).forward(x, training=False)
    p32 = cases.perturbed(kind, np.float32).forward(x, training=False)
    err = np.abs(p32.astype(np.float64) - ref).max()
    print("float32 oracle predict conv_2d_%s B=%d: max |p - float64| = %.3g (bar 2e-5)" % (kind, cases.PREDICT_BATCH, err))
    assert err < 0.5 * 2e-5


@pytest.mark.parametrize("B", cases.TRAIN_BATCHES)
@pytest.mark.parametrize("kind", cases.KINDS)
def test_float32_oracle_train_step_is_within_half_the_gpu_bars(kind, B):
    """The oracle in float32 (on the float64 run's gates and pool winners) against its float64 self, on the GPU tests' weights
    and batches.  Each figure has to stay under half the bar the GPU test applies; the convolution biases' gradients, zero up to
    rounding, are measured in units of their absolute bar (cases.bias_errors)."""
    ora = cases.perturbed(kind)
    x, y = cases.batch(B)
    loss, p, grads, cache = ora.loss_and_grads(x, y, seed=cases.SEED, step=cases.STEP)
    masks, inds = cases.decisions_of(ora, cache)
    o32 = cases.perturbed(kind, np.float32)
    loss32, p32, grads32, cache32 = o32.loss_and_grads(x, y, seed=cases.SEED, step=cases.STEP, relu_masks=masks, pool_ind=inds)
    errs = cases.grad_errors(grads32, grads)
    worst = max(errs, key=errs.get)
    berrs = cases.bias_errors(grads32, grads, cache)
    bworst = max(berrs, key=berrs.get)
    stat = max(max(np.abs(cache32['batch_stats'][i][q].astype(np.float64) - cache['batch_stats'][i][q]).max() for q in (0, 1))
               for i in cache['batch_stats'])
    print("float32 oracle train conv_2d_%s B=%d: probs %.3g (bar 5e-5), loss %.3g (bar 1e-4), worst gradient %s %.3g (bar 2e-4), "
          "worst bias gradient %s %.3g of its bar, batch statistics %.3g" %
          (kind, B, np.abs(p32 - p).max(), abs(float(loss32) - loss), worst, errs[worst], bworst, berrs[bworst], stat))
    assert np.abs(p32 - p).max() < 0.5 * 5e-5
    assert abs(float(loss32) - loss) < 0.5 * 1e-4
    assert errs[worst] < 0.5 * 2e-4, (worst, errs[worst])
    assert berrs[bworst] < 0.5, (bworst, berrs[bworst])
