"""CPU checks of the general depthwise ladder conv_1d_gru: the float64 oracle (tests/dwk_oracle.py) against torch autograd, the
native tensor table against the structure recorded from the reference (tests/golden/dwk_models.json, made by
tests/golden/make_golden_dwk.py) and against the oracle, the model settings, and the host-side domain checks of kws_dwconvk_*."""
import ctypes
import json
import os

import numpy as np
import pytest
import torch
import torch.nn.functional as Fn

from net_parity import native_table, perturb
from oracle.layers import dropout_key, dropout_mask
from speech_recognition_amd import _lib
from dwk_oracle import HIDDEN, KEEP, LADDER, SPEC, DwkNet
from oracle_blocks import dw_bwd, dw_fwd, same_geometry

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden', 'dwk_models.json')
WIDTHS = [1, 128, 256, 384, 448, 512, 512]


def _golden():
    with open(GOLDEN) as f:
        return json.load(f)['conv_1d_gru']


def test_kind_constant():
    assert _lib.KWS_NET_CONV_1D_GRU == 10


def test_fixture_has_the_expected_ladder():
    gold = _golden()
    dws = [l for l in gold['layers'] if l['class'] == 'DepthwiseConv2D']
    assert [(l['input_length'], l['pad_left'], l['output'][0]) for l in dws] == LADDER
    assert [(l['kernel'][1], l['strides'], l['padding']) for l in dws] == [(k, s, pad) for _, k, s, pad in SPEC]
    assert [l['kernel'][2] for l in dws] == WIDTHS[:-1]
    assert [c['kernel'] for c in gold['layers'] if c['class'] == 'Conv1D'] == [[1, a, b] for a, b in zip(WIDTHS[:-1], WIDTHS[1:])]
    assert dws[2]['output'][0] == 63          # not the 64 of the reference's comment
    assert (gold['model_name'], gold['optimizer'], gold['lr'], gold['loss']) == \
        ('conv_1d_bigru', 'RMSprop', 1e-3, 'categorical_crossentropy')
    assert [l['rate'] for l in gold['layers'] if l['class'] == 'Dropout'] == [pytest.approx(1 - KEEP)] * 2
    dense = [l for l in gold['layers'] if l['class'] == 'Dense']
    assert [(d['kernel'], d['use_bias'], d['activation']) for d in dense] == [([512, HIDDEN], True, None), ([HIDDEN, 12], True, 'softmax')]
    assert not any('GRU' in l['class'] or 'Bidirectional' in l['class'] for l in gold['layers'])
    # the oracle's own geometry and the TF rule agree with the recording
    for (F, k, s, pad), (L, pad_l, Lout) in zip(SPEC, LADDER):
        if pad == 'same':
            assert same_geometry(L, k, s)[:2] == (Lout, pad_l)


def test_native_tensor_table_matches_reference_and_oracle():
    gold = _golden()
    table = native_table(_lib.KWS_NET_CONV_1D_GRU, gold['num_classes'], gold['input_size'])
    assert [t.name.decode() for t in table] == [w['name'] for w in gold['weights']]
    for t, w in zip(table, gold['weights']):
        assert [int(t.shape[k]) for k in range(t.ndim)] == w['shape'], w['name']
        assert bool(t.is_state) == bool(w.get('state', False)), w['name']
        assert t.l2 == np.float32(w['l2']), w['name']
        if w['name'].endswith('/depthwise_kernel'):
            _, k, C, _ = w['shape']
            assert (t.fan_in, t.fan_out) == (k * C, k), w['name']
        elif w['name'].endswith('/kernel') and len(w['shape']) == 3:
            k, cin, cout = w['shape']
            assert (t.fan_in, t.fan_out) == (k * cin, k * cout), w['name']
        elif w['name'].endswith('/kernel'):
            assert (t.fan_in, t.fan_out) == tuple(w['shape']), w['name']
    for state in (0, 1):
        spans = sorted((t.offset, t.offset + t.size) for t in table if t.is_state == state)
        assert all(a[1] <= b[0] for a, b in zip(spans, spans[1:]))
        assert all(a[0] % 4 == 0 for a in spans)
    n_train = sum(int(np.prod(w['shape'])) for w in gold['weights'] if not w.get('state'))
    assert sum(t.size for t in table if not t.is_state) == n_train == 950539
    ora = DwkNet(num_classes=gold['num_classes'])
    assert [t.name.decode() for t in table if not t.is_state] == list(ora.params)
    assert [t.name.decode() for t in table if t.is_state] == list(ora.state)
    for t in table:
        v = ora.state[t.name.decode()] if t.is_state else ora.params[t.name.decode()]
        assert tuple(int(t.shape[k]) for k in range(t.ndim)) == v.shape
    assert sum(t.size for t in table) == ora.count_params()
    # l2 1e-5 on every depthwise and pointwise kernel, each tensor on its own; none on the Dense layers
    assert {t.name.decode() for t in table if t.l2 > 0} == set(ora.l2_names) and len(ora.l2_names) == 12
    assert all(t.l2 == np.float32(1e-5) for t in table if t.l2 > 0)


def test_native_table_rejects_other_input_sizes():
    lib = _lib.load()
    cfg = _lib.NetConfig(_lib.KWS_NET_CONV_1D_GRU, 12, 1, 8000, 0, 0)
    h = ctypes.c_void_p()
    assert lib.kws_net_create(ctypes.byref(cfg), ctypes.byref(h)) != 0
    assert b'input_size' in lib.kws_last_error()


def test_speech_model_settings(monkeypatch):
    """Name, loss, optimizer class and lr (the device net itself replaced: no GPU here); another input size is refused."""
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
    assert 'conv_1d_gru' in M.ACCELERATED
    M.speech_model('conv_1d_gru', 16000, num_classes=12)
    assert captured['net'].kind == 10 and captured['net'].num_classes == 12 and captured['net'].kw['input_size'] == 16000
    assert captured['name'] == 'conv_1d_bigru' and captured['loss'] == 'cce'
    assert isinstance(captured['optimizer'], keras_api.RMSprop) and abs(float(captured['optimizer'].lr) - 1e-3) < 1e-9   # lr is held in float32, as Keras holds it
    with pytest.raises(ValueError):
        M.speech_model('conv_1d_gru', 8000, num_classes=12)


def _torch_dw(a, w, s, pad_l, Lout):
    """F.conv1d with groups = C and explicit asymmetric zero padding; a [B, L, C], w [k, C]."""
    k, C = w.shape
    pr = max(s * (Lout - 1) + k - pad_l - a.shape[1], 0)
    ap = Fn.pad(a.permute(0, 2, 1), (pad_l, pr))
    return Fn.conv1d(ap, w.t().reshape(C, 1, k), stride=s, groups=C)[:, :, :Lout].permute(0, 2, 1)


@pytest.mark.parametrize("i", range(6))
def test_oracle_depthwise_matches_torch_autograd(i):
    (F, k, s, pad), (L, pad_l, Lout) = SPEC[i], LADDER[i]
    C = min(WIDTHS[i], 8)
    rng = np.random.RandomState(10 + i)
    a, w, dz = rng.randn(2, L, C), rng.randn(k, C), rng.randn(2, Lout, C)
    z = dw_fwd(a, w, s, pad_l, Lout)
    ta, tw = torch.tensor(a, requires_grad=True), torch.tensor(w, requires_grad=True)
    tz = _torch_dw(ta, tw, s, pad_l, Lout)
    assert tuple(tz.shape) == z.shape
    np.testing.assert_allclose(z, tz.detach().numpy(), atol=1e-12)
    tz.backward(torch.tensor(dz))
    da, dw = dw_bwd(dz, a, w, s, pad_l)
    np.testing.assert_allclose(da, ta.grad.numpy(), atol=1e-12)
    np.testing.assert_allclose(dw, tw.grad.numpy(), atol=1e-11)
    # negative controls on the oracle itself: reversed taps, the odd SAME sample on the left
    assert np.abs(dw_fwd(a, w[::-1], s, pad_l, Lout) - z).max() > 0.1
    assert np.abs(dw_fwd(a, w, s, pad_l + 1, Lout) - z).max() > 0.1 if pad_l + 1 < k else True


def _perturbed(seed=5):
    ora = DwkNet(num_classes=12)
    perturb(ora, seed, negative_fraction=0.33, beta=(0.5, 0.3), state=False)
    return ora


def _torch_loss(ora, x, y, seed, step):
    P = {k: torch.tensor(v.astype(np.float64), requires_grad=True) for k, v in ora.params.items()}
    B = x.shape[0]
    a = torch.tensor(x.astype(np.float64))[:, :, None]
    for blk in ora.blocks:
        n = blk['idx']
        z = _torch_dw(a, P['depthwise_conv2d_%d/depthwise_kernel' % n][0, :, :, 0], blk['s'], blk['pad_l'], blk['Lout'])
        yv = z @ P['conv1d_%d/kernel' % n][0]
        a = Fn.batch_norm(yv.permute(0, 2, 1), None, None, P['batch_normalization_%d/gamma' % n],
                          P['batch_normalization_%d/beta' % n], training=True, eps=1e-3).clamp(0, 6).permute(0, 2, 1)
    flat = a.reshape(B, -1)
    k1 = dropout_mask(dropout_key(seed, step, 1), flat.numel(), KEEP).reshape(flat.shape)
    h = (flat * torch.tensor(k1.astype(np.float64)) / KEEP) @ P['dense_1/kernel'] + P['dense_1/bias']
    h = h.clamp(0, 6)
    k2 = dropout_mask(dropout_key(seed, step, 2), h.numel(), KEEP).reshape(h.shape)
    logits = (h * torch.tensor(k2.astype(np.float64)) / KEEP) @ P['dense_2/kernel'] + P['dense_2/bias']
    p = torch.softmax(logits, dim=1)
    loss = -(torch.tensor(y.astype(np.float64)) * torch.log(p.clamp(1e-7, 1 - 1e-7))).sum(1).mean()
    loss.backward()
    return float(loss.detach()), p.detach().numpy(), {k: v.grad.numpy() for k, v in P.items()}


def test_oracle_gradients_match_torch_autograd():
    ora = _perturbed()
    rng = np.random.RandomState(7)
    B = 3
    x = (rng.randn(B, 16000) * 0.3).astype(np.float32)
    y = np.eye(12, dtype=np.float32)[rng.randint(0, 12, B)]
    loss, p, grads, _ = ora.loss_and_grads(x, y, seed=3, step=5)
    tl, tp, tg = _torch_loss(ora, x, y, seed=3, step=5)
    assert abs(loss - tl) < 1e-10
    np.testing.assert_allclose(p, tp, atol=1e-12)
    for k, g in grads.items():
        scale = max(np.abs(tg[k]).max(), 1e-12)
        assert np.abs(g - tg[k]).max() / scale < 1e-9, k


@pytest.mark.parametrize("mutate", ['pad_left', 'reversed_taps'])
def test_mutated_oracle_breaks_the_gradient_bar(mutate):
    ora = _perturbed()
    rng = np.random.RandomState(8)
    x = (rng.randn(3, 16000) * 0.3).astype(np.float32)
    y = np.eye(12, dtype=np.float32)[rng.randint(0, 12, 3)]
    _, _, good, _ = ora.loss_and_grads(x, y, seed=1, step=0)
    _, _, bad, _ = ora.loss_and_grads(x, y, seed=1, step=0, mutate=mutate)
    err = max(np.abs(bad[k] - good[k]).max() / max(np.abs(good[k]).max(), 1e-12) for k in good)
    assert err > 1e-2, err


def test_gate_exclusion_share_is_small():
    """The kernel tests compare the ReLU6 gate only where float64 bn(y) is farther than 1e-5 from 0 and from 6: for normal
    inputs that leaves out about 1e-5 of the elements, far below the 0.1 % the tests allow."""
    rng = np.random.RandomState(0)
    y = rng.randn(1 << 20)
    pre = y * (1.0 + 0.1 * rng.randn(1 << 20)) + 0.5
    share = ((np.abs(pre) < 1e-5) | (np.abs(pre - 6) < 1e-5)).mean()
    assert share < 1e-4


def test_dwconvk_domain_refusals():
    """Host-side checks only: every call is refused before a launch (the pointers are never dereferenced)."""
    lib = _lib.load()
    p = ctypes.c_void_p(4096)

    def fwd(B, L, Lout, C, k, s, pad):
        return lib.kws_dwconvk_fwd_f32(p, None, p, p, B, L, Lout, C, k, s, pad, None)

    def bwd(B, L, Lout, C, k, s, pad):
        return lib.kws_dwconvk_bwd_f32(p, p, None, p, p, p, B, L, Lout, C, k, s, pad, None)

    bad = [(1, 64, 16, 8, 0, 4, 0), (1, 64, 16, 8, 65, 4, 0), (1, 64, 16, 8, 7, 0, 0), (1, 64, 16, 8, 7, 17, 0),
           (1, 64, 16, 8, 7, 4, 7), (1, 64, 16, 8, 7, 4, -1), (1, 64, 16, 6, 7, 4, 2), (1, 64, 16, 2, 7, 4, 2),
           (1, 64, 16, 1028, 7, 4, 2), (1, 64, 18, 8, 7, 4, 0), (0, 64, 16, 8, 7, 4, 2), (1, 0, 16, 8, 7, 4, 2)]
    for args in bad:
        assert fwd(*args) == -1, args
        assert lib.kws_last_error()
        assert bwd(*args) == -1, args
    assert lib.kws_dwconvk_fwd_f32(None, None, p, p, 1, 64, 16, 8, 7, 4, 2, None) == -1
    assert lib.kws_dwconvk_bwd_f32(p, p, None, p, None, p, 1, 64, 16, 8, 7, 4, 2, None) == -1
    # size helpers: 0 outside the domain, rows * (2 + k) * C inside
    assert lib.kws_dwconvk_bwd_part_rows(1, 64, 6, 7, 4) == 0 and lib.kws_dwconvk_bwd_part_rows(1, 64, 8, 65, 4) == 0
    for B, L, C, k, s in ((3, 1000, 128, 31, 4), (3, 16000, 1, 63, 16), (2, 8, 512, 8, 1), (1, 40, 20, 64, 1)):
        rows = lib.kws_dwconvk_bwd_part_rows(B, L, C, k, s)
        assert rows > 0 and lib.kws_dwconvk_bwd_part_floats(B, L, C, k, s) == rows * (2 + k) * C
    assert lib.kws_dwconvk_bwd_finalize(p, 0, 10, 8, 7, p, p, p, p, None) == -1
    assert lib.kws_dwconvk_bwd_finalize(p, 4, 10, 8, 65, p, p, p, p, None) == -1
    # the one-channel pointwise pair: N a power of two, 4 .. 256
    assert lib.kws_dwconvk_pw1_fwd_f32(p, p, p, 100, 96, None, None) == -1
    assert lib.kws_dwconvk_pw1_fwd_f32(p, p, p, 0, 128, None, None) == -1
    assert lib.kws_dwconvk_pw1_bwd_f32(p, p, p, p, p, 100, 512, p, None) == -1
    assert lib.kws_dwconvk_pw1_bwd_workspace_floats(1000, 128) == lib.kws_dwconvk_pw1_stats_rows(1000) * 128 > 0
    assert lib.kws_dwconvk_pw1_bwd_workspace_floats(1000, 96) == 0
