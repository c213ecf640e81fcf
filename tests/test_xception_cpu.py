"""CPU checks of the attention gate and xception_with_attention: the kind constant and the kws_attn_gate_* symbols, the native tensor
table of kind 13 against the structure recorded from the reference (tests/golden/xception_models.json, made by
tests/golden/make_golden_xception.py) and against the oracle, the model settings, the float64 oracle (tests/xception_oracle.py)
against torch autograd (the gate alone and the whole net at input_size = 4000), its mutations, the host-side planners and domain
checks of kws_attn_gate_*, and the float32-against-float64 figures the GPU tests' bars rest on."""
import ctypes
import os

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from net_parity import native_table
from oracle import layers as L
from speech_recognition_amd import _lib
from test_gru_cpu import _torch_bigru
from gru_oracle import draw_masks
from xception_oracle import (GATE_BWD_KEYS, GATE_CASES, GATE_FWD_KEYS, XC_BLOCKS, XceptionNet, gate_bwd, gate_errors, gate_fwd, gate_inputs,
                             gate_reference, golden, net_float32_figures, perturbed_net)

GATE_SYMBOLS = ['kws_attn_gate_fwd_floats', 'kws_attn_gate_bwd_floats', 'kws_attn_gate_fwd_f32', 'kws_attn_gate_bwd_f32']


def test_kind_constant_and_symbols(repo_root):
    assert _lib.KWS_NET_XCEPTION_ATTENTION == 13
    header = open(os.path.join(repo_root, 'include', 'kws_hip.h')).read()
    assert '#define KWS_NET_XCEPTION_ATTENTION 13' in header and '#define KWS_ABI_VERSION 5' in header
    lib = _lib.load()
    for name in GATE_SYMBOLS:
        assert name in _lib.SIGNATURES and (name + '(') in header and hasattr(lib, name)


def test_accelerated_lists_the_model():
    from speech_recognition_amd.model import ACCELERATED
    assert 'xception_with_attention' in ACCELERATED


def test_fixture_structure():
    gold = golden()
    pools = [l for l in gold['layers'] if l['class'] == 'MaxPool1D']
    assert [(l['pool_size'], l['strides'], l['padding']) for l in pools] == [(3, s, 'same') for _, s in XC_BLOCKS]
    assert [l['output'] for l in pools] == [[200, 128], [100, 256]] + [[100, 256]] * 8 + [[50, 384]]
    dws = [l for l in gold['layers'] if l['class'] == 'DepthwiseConv2D']
    assert len(dws) == 23 and all(l['padding'] == 'same' for l in dws)
    assert [l['kernel'][1] for l in dws] == [3] * 22 + [5] and dws[-1]['output'] == [50, 384]
    sm = [l for l in gold['layers'] if 'softmax_axis' in l]
    assert len(sm) == 1 and sm[0]['softmax_axis'] == 1 and sm[0]['output'] == [50, 1]       # over TIME
    mul = [l for l in gold['layers'] if l['class'] == 'Multiply']
    assert len(mul) == 1 and mul[0]['inputs'] == [[50, 384], [50, 1]]
    bi = [l for l in gold['layers'] if l['class'] == 'Bidirectional'][0]
    assert (bi['units'], bi['dropout'], bi['recurrent_dropout'], bi['input'], bi['output']) == (192, 0.2, 0.2, [50, 384], [384])
    assert (bi['kernel_l2'], bi['recurrent_l2'], bi['bias_l2']) == (1e-5, 0.0, 0.0)
    assert (gold['model_name'], gold['optimizer'], gold['lr'], gold['loss']) == \
        ('xception_with_attention', 'RMSprop', 5e-4, 'categorical_crossentropy')
    assert not any(l['class'] == 'Dropout' for l in gold['layers'])
    small = golden('xception_with_attention_4000')
    assert [l['output'][0] for l in small['layers'] if l['class'] == 'MaxPool1D'] == [50, 25] + [25] * 8 + [13]
    assert [l['input_length'] for l in small['layers'] if l['class'] == 'MaxPool1D'][:2] == [99, 50]
    assert [w['name'] for w in small['weights']] == [w['name'] for w in gold['weights']]


@pytest.mark.parametrize("key", ['xception_with_attention', 'xception_with_attention_4000'])
def test_native_tensor_table_matches_reference_and_oracle(key):
    gold = golden(key)
    table = native_table(_lib.KWS_NET_XCEPTION_ATTENTION, gold['num_classes'], gold['input_size'])
    assert [t.name.decode() for t in table] == [w['name'] for w in gold['weights']]
    for t, w in zip(table, gold['weights']):
        name = w['name']
        assert [int(t.shape[k]) for k in range(t.ndim)] == w['shape'], name
        assert bool(t.is_state) == bool(w.get('state', False)), name
        assert t.l2 == np.float32(w['l2']), name
        if name.endswith('/depthwise_kernel'):
            assert (t.fan_in, t.fan_out) == (w['shape'][1] * w['shape'][2], w['shape'][1]), name
        elif name.endswith('/recurrent_kernel'):
            assert (t.fan_in, t.fan_out) == (0, 0), name          # the host draws it (Orthogonal)
        elif name.endswith('/kernel') and len(w['shape']) == 3:
            assert (t.fan_in, t.fan_out) == (w['shape'][0] * w['shape'][1], w['shape'][0] * w['shape'][2]), name
        elif name.endswith('/kernel'):
            assert (t.fan_in, t.fan_out) == tuple(w['shape']), name
    for state in (0, 1):
        spans = sorted((t.offset, t.offset + t.size) for t in table if t.is_state == state)
        assert all(a[1] <= b[0] for a, b in zip(spans, spans[1:]))
    ora = XceptionNet(num_classes=gold['num_classes'], input_size=gold['input_size'])
    assert [t.name.decode() for t in table if not t.is_state] == list(ora.params)
    assert [t.name.decode() for t in table if t.is_state] == list(ora.state)
    for t in table:
        v = ora.state[t.name.decode()] if t.is_state else ora.params[t.name.decode()]
        assert tuple(int(t.shape[k]) for k in range(t.ndim)) == v.shape
    n_train = sum(int(np.prod(w['shape'])) for w in gold['weights'] if not w.get('state'))
    assert sum(t.size for t in table if not t.is_state) == n_train
    assert sum(t.size for t in table) == ora.count_params()
    # l2 1e-5: every depthwise and pointwise kernel but the shortcuts', the GRU's two `kernel` tensors, dense_1/kernel
    l2 = {t.name.decode() for t in table if t.l2 > 0}
    assert l2 == set(ora.l2_names) == {w['name'] for w in gold['weights'] if w['l2'] > 0}
    assert 'bidirectional_1/forward_gru_1/kernel' in l2 and 'dense_1/kernel' in l2
    assert not any(n.endswith('recurrent_kernel') or n.endswith('bias') for n in l2)


def test_native_table_honours_filter_mult_and_refuses_bad_inputs():
    wide = {t.name.decode(): t for t in native_table(_lib.KWS_NET_XCEPTION_ATTENTION, 12, 16000, 2)}
    assert [int(wide['depthwise_conv2d_23/depthwise_kernel'].shape[k]) for k in range(4)] == [1, 5, 768, 1]
    assert [int(wide['bidirectional_1/forward_gru_1/kernel'].shape[k]) for k in range(2)] == [768, 576]
    lib = _lib.load()
    for size, fm in ((3998, 1), (4001, 1), (16000, 3)):    # too short, odd, a tail wider than the gate's 1024 channels
        cfg = _lib.NetConfig(_lib.KWS_NET_XCEPTION_ATTENTION, 12, fm, size, 0, 0)
        h = ctypes.c_void_p()
        assert lib.kws_net_create(ctypes.byref(cfg), ctypes.byref(h)) != 0, (size, fm)
        assert lib.kws_last_error()


def test_speech_model_settings(monkeypatch):
    from speech_recognition_amd import keras_api, model as M

    class FakeNet(object):
        def __init__(self, kind, num_classes, **kw):
            self.kind, self.num_classes, self.kw = kind, num_classes, kw

    captured = {}

    def fake_model(net, optimizer, name=None, loss=None):
        captured.update(net=net, optimizer=optimizer, name=name, loss=loss)
        return captured

    monkeypatch.setattr(M, 'DeviceNet', FakeNet)
    monkeypatch.setattr(M, 'Model', fake_model)
    M.speech_model('xception_with_attention', 16000, num_classes=12)
    net = captured['net']
    assert net.kind == 13 and net.num_classes == 12 and net.kw['input_size'] == 16000 and net.kw['filter_mult'] == 1
    # name, optimizer class, learning rate and loss are the ones recorded from the reference's own compile() call
    gold = golden()
    assert captured['name'] == gold['model_name']
    assert {'cce': 'categorical_crossentropy'}[captured['loss']] == gold['loss']
    assert type(captured['optimizer']) is getattr(keras_api, gold['optimizer'])
    assert abs(float(captured['optimizer'].lr) - gold['lr']) < 1e-9
    assert net.num_classes == gold['num_classes'] and net.kw['input_size'] == gold['input_size']
    M.xception_with_attention_model(8000, 30, filter_mult=2)
    assert captured['net'].kw == {'filter_mult': 2, 'input_size': 8000}


# ---- the oracle against torch autograd -----------------------------------------------------------------------------------------
def _t_dw(a, w, pad):
    k, C = w.shape
    ap = F.pad(a.permute(0, 2, 1), pad)
    return F.conv1d(ap, w.t().reshape(C, 1, k), groups=C).permute(0, 2, 1)


def _t_bn(y, g, b):
    return F.batch_norm(y.permute(0, 2, 1), None, None, g, b, training=True, eps=1e-3).permute(0, 2, 1)


def _t_gate(x, wa, Wa, gamma, beta, mm, mv, training):
    k = wa.shape[0]
    pl = (k - 1) // 2
    u = _t_dw(x, wa, (pl, k - 1 - pl)) @ Wa
    mean, var = (u.mean(), ((u - u.mean()) ** 2).mean()) if training else (torch.tensor(mm, dtype=u.dtype), torch.tensor(mv, dtype=u.dtype))
    pre = (u - mean) / torch.sqrt(var + 1e-3) * gamma + beta
    return x * torch.softmax(pre.clamp(0, 6), dim=1)[:, :, None], mean, var


@pytest.mark.parametrize("training", [True, False])
@pytest.mark.parametrize("B,T,C,k", GATE_CASES)
def test_gate_oracle_matches_torch_autograd(B, T, C, k, training):
    neg = (B, T, C, k) == GATE_CASES[2]
    x, dy, wa, Wa, gamma, beta, mm, mv = [np.asarray(a, dtype=np.float64) for a in gate_inputs(B, T, C, k, neg)]
    y, c = gate_fwd(x, wa, Wa, gamma, beta, mm, mv, training)
    got = gate_bwd(dy, c)
    tx, twa, tWa = [torch.tensor(a, requires_grad=True) for a in (x, wa, Wa)]
    tg, tb = torch.tensor(float(gamma), dtype=torch.float64, requires_grad=True), torch.tensor(float(beta), dtype=torch.float64, requires_grad=True)
    ty, mean, var = _t_gate(tx, twa, tWa, tg, tb, float(mm), float(mv), training)
    np.testing.assert_allclose(y, ty.detach().numpy(), rtol=1e-9, atol=1e-12)
    assert abs(float(mean.detach()) - c['mean']) <= 1e-9 * max(abs(c['mean']), 1e-12) and abs(float(var.detach()) - c['var']) <= 1e-9 * max(c['var'], 1e-12)
    ty.backward(torch.tensor(dy))
    for nm, g, t in zip(('dx', 'dwa', 'dWa', 'dgamma', 'dbeta'), got, (tx, twa, tWa, tg, tb)):
        ref = t.grad.numpy()
        assert np.abs(g - ref).max() <= 1e-9 * max(np.abs(ref).max(), 1e-12) + 1e-15, nm
    if T > 1:
        assert 0 < L.relu6_mask(c['pre']).mean() < 1 or T == 2      # both sides of a ReLU6 corner are exercised


@pytest.mark.parametrize("mutate", ['softmax_channels', 'no_direct_term'])
def test_every_mutation_moves_a_gradient(mutate):
    x, dy, wa, Wa, gamma, beta, mm, mv = [np.asarray(a, dtype=np.float64) for a in gate_inputs(5, 50, 384, 5)]
    good = gate_bwd(dy, gate_fwd(x, wa, Wa, gamma, beta, mm, mv, True)[1])
    bad = gate_bwd(dy, gate_fwd(x, wa, Wa, gamma, beta, mm, mv, True, mutate)[1], mutate=mutate)
    err = max(np.abs(a - b).max() / max(np.abs(a).max(), 1e-12) for a, b in zip(good, bad))
    assert err > 1e-2, err


def test_oracle_net_matches_torch_autograd():
    """Forward, every gradient, the batch statistics of every BatchNorm and the moving statistics after the step at input_size =
    4000: lengths 200 -> 99 -> 50 -> 25 -> 13, so odd lengths go through the SAME pools and the gate."""
    ora = perturbed_net(4000, att_gamma=-1.5)
    assert [b['Lout'] for b in ora.blocks] == [50, 25] + [25] * 8 + [13] and ora.L0 == 99
    rng = np.random.RandomState(7)
    B = 3
    x = (rng.randn(B, 4000) * 0.3).astype(np.float32)
    y = np.eye(12, dtype=np.float32)[rng.randint(0, 12, B)]
    loss, p, grads, cache = ora.loss_and_grads(x, y, seed=3, step=5)
    P = {k: torch.tensor(v.astype(np.float64), requires_grad=True) for k, v in ora.params.items()}
    stats = {}

    def bn(idx, v):
        stats[idx] = (v.mean(dim=(0, 1)).detach().numpy(), v.var(dim=(0, 1), unbiased=False).detach().numpy())
        return _t_bn(v, P['batch_normalization_%d/gamma' % idx], P['batch_normalization_%d/beta' % idx])

    frames = torch.tensor(L.frame_same(x.astype(np.float64), 40, 20))
    h = bn(ora.first[1], F.conv1d(frames.permute(0, 2, 1), P[ora.first[0]].permute(2, 1, 0), stride=2).permute(0, 2, 1)).clamp(0, 6)
    for blk in ora.blocks:
        if 'short' in blk:
            res = bn(blk['short'][1], h[:, ::blk['stride'], :] @ P[blk['short'][0]][0])
        else:
            res = h
        a = bn(blk['bn1'], _t_dw(h, P[blk['dw1']][0, :, :, 0], (1, 1)) @ P[blk['pw1']][0]).clamp(0, 6)
        a = bn(blk['bn2'], _t_dw(a, P[blk['dw2']][0, :, :, 0], (1, 1)) @ P[blk['pw2']][0]).clamp(0, 6)
        _, pl, pr = L.same_pad(blk['Lin'], 3, blk['stride'])
        pooled = F.max_pool1d(F.pad(a.permute(0, 2, 1), (pl, pr), value=-np.inf), 3, blk['stride']).permute(0, 2, 1)
        h = pooled + res
    gy, mean, var = _t_gate(h, P[ora.att_dw][0, :, :, 0], P[ora.att_pw][0, :, 0], P[ora._bn_name('gamma')][0], P[ora._bn_name('beta')][0],
                            0.0, 1.0, True)
    stats[ora.att_bn] = (np.array([float(mean.detach())]), np.array([float(var.detach())]))
    mx, mh = draw_masks(3, 5, B, ora.I, ora.H, ora.keep, 0, ora.T)
    tws = [tuple(P[b + w] for w in ('kernel', 'recurrent_kernel', 'bias')) for b in ora.gru_names]
    out = _torch_bigru(gy, tws, mx, mh)
    tp = torch.softmax(out @ P['dense_1/kernel'] + P['dense_1/bias'], dim=1)
    tl = -(torch.tensor(y.astype(np.float64)) * torch.log(tp.clamp(1e-7, 1 - 1e-7))).sum(1).mean()
    tl.backward()
    assert abs(loss - float(tl.detach())) < 1e-10
    np.testing.assert_allclose(p, tp.detach().numpy(), atol=1e-12)
    for k, g in grads.items():
        ref = P[k].grad.numpy()
        assert np.abs(g - ref).max() / max(np.abs(ref).max(), 1e-12) < 1e-9, k
    assert set(stats) == set(cache['batch_stats']) and len(stats) == 27
    for idx, (m, v) in stats.items():
        np.testing.assert_allclose(cache['batch_stats'][idx][0], m, rtol=1e-9, atol=1e-12)
        np.testing.assert_allclose(cache['batch_stats'][idx][1], v, rtol=1e-9, atol=1e-12)
    moved = ora.moving_after(cache)
    assert list(moved) == list(ora.state)
    for idx, (m, v) in stats.items():
        for nm, batch in (('moving_mean', m), ('moving_variance', v)):
            name = 'batch_normalization_%d/%s' % (idx, nm)
            old = ora.state[name].astype(np.float64)
            assert np.abs(old - batch).max() > 1e-3, name              # the perturbed state is not already the batch's
            np.testing.assert_allclose(moved[name], 0.99 * old + 0.01 * batch, rtol=1e-9, atol=1e-12, err_msg=name)


# ---- planners and domain ---------------------------------------------------------------------------------------------------------
def test_planners_are_consistent_over_the_domain():
    lib = _lib.load()
    corners = [(B, T, C, k) for B in (1, 37, 1024, 5000) for T in (1, 50, 128) for C in (4, 384, 1024) for k in (3, 5)]
    for B, T, C, k in corners:
        f, b = int(lib.kws_attn_gate_fwd_floats(B, T, C, k)), int(lib.kws_attn_gate_bwd_floats(B, T, C, k))
        rows = -(-B // -(-B // 1024))                     # per-workgroup partial rows of the weight gradients: at most 1024
        assert f >= B and f % 64 == 0, (B, T, C, k)
        assert b % 64 == 0 and b >= B * T + 2 * B + 2 + rows * k * C, (B, T, C, k)
        assert b <= B * T + 2 * B + rows * k * C + 5 * 64, (B, T, C, k)
    assert lib.kws_attn_gate_bwd_floats(8, 50, 384, 5) > lib.kws_attn_gate_bwd_floats(8, 50, 384, 3)
    for B, T, C, k in ((0, 50, 384, 5), (4, 0, 384, 5), (4, 129, 384, 5), (4, 50, 6, 5), (4, 50, 0, 5), (4, 50, 1028, 5), (4, 50, 384, 4),
                       (4, 50, 384, 7), (4, 50, 384, 1)):
        assert lib.kws_attn_gate_fwd_floats(B, T, C, k) == 0 and lib.kws_attn_gate_bwd_floats(B, T, C, k) == 0, (B, T, C, k)


def test_gate_domain_refusals():
    """Host-side checks only: every call is refused before a launch (the pointers are never dereferenced)."""
    lib = _lib.load()
    p = ctypes.c_void_p(4096)

    def fwd(B, T, C, k, x=p):
        return lib.kws_attn_gate_fwd_f32(x, p, p, p, p, p, p, p, p, p, p, p, B, T, C, k, 1, None)

    def bwd(B, T, C, k, dy=p):
        return lib.kws_attn_gate_bwd_f32(dy, p, p, p, p, p, p, p, p, p, p, p, p, p, B, T, C, k, 1, None)

    for B, T, C, k in ((4, 129, 384, 5), (4, 50, 6, 5), (4, 50, 384, 4), (0, 50, 384, 5), (4, 0, 384, 5), (4, 50, 1028, 5)):
        assert fwd(B, T, C, k) == -1, (B, T, C, k)
        assert lib.kws_last_error()
        assert bwd(B, T, C, k) == -1, (B, T, C, k)
    assert b'T=129' in (fwd(4, 129, 384, 5), lib.kws_last_error())[1]
    assert fwd(4, 50, 384, 5, None) == -1 and bwd(4, 50, 384, 5, None) == -1


# ---- what the GPU tests' bars rest on --------------------------------------------------------------------------------------------
def test_gate_float32_figures_stay_under_half_the_gpu_bars():
    """The gate oracle in float32 against itself in float64 at the GPU test's shapes and seeds, on the float64 run's ReLU6 decisions:
    forward values under half of 2e-5, gradients under half of 2e-4; the share of logits within 1e-5 of a ReLU6 corner under 1e-3."""
    worst_f, worst_b, near_n, total = ('', 0.0), ('', 0.0), 0, 0
    for case in GATE_CASES:
        for training in (True, False):
            neg = case == GATE_CASES[2]
            r64 = gate_reference(*case, training, neg)
            r32 = gate_reference(*case, training, neg, dtype=np.float32, mask=L.relu6_mask(r64['pre']).astype(np.float32))
            near = (np.abs(r64['pre']) < 1e-5) | (np.abs(r64['pre'] - 6.0) < 1e-5)
            assert near.sum() <= 1e-3 * near.size, case
            near_n, total = near_n + near.sum(), total + near.size
            e = gate_errors(r32, r64, near)
            for k in GATE_FWD_KEYS:
                worst_f = max(worst_f, ('%s %s' % (k, case), e[k]), key=lambda t: t[1])
            for k in GATE_BWD_KEYS:
                worst_b = max(worst_b, ('%s %s' % (k, case), e[k]), key=lambda t: t[1])
    print("gate float32 vs float64: worst forward %s %.3g, worst gradient %s %.3g, near a corner %d / %d" %
          (worst_f + worst_b + (near_n, total)))
    assert worst_f[1] < 1e-5 and worst_b[1] < 1e-4


@pytest.mark.parametrize("B,input_size", [(8, 16000), (40, 4000)])
def test_net_float32_figures_stay_under_half_the_gpu_bars(B, input_size):
    """The oracle net in float32 against itself in float64 at the two cases of tests/test_xception_models_gpu.py: every figure under
    half its bar there (train probabilities 5e-5, loss 1e-4, gradients 2e-4, moving statistics 5e-6)."""
    f = net_float32_figures(B, input_size)
    print("net float32 vs float64, B %d at %d samples: probs %.3g, loss %.3g, worst gradient %s %.3g, moving statistics %.3g" %
          (B, input_size, f['probs'], f['loss'], f['worst_gradient'], f['gradient'], f['moving']))
    assert f['probs'] < 2.5e-5 and f['loss'] < 5e-5 and f['gradient'] < 1e-4 and f['moving'] < 2.5e-6
