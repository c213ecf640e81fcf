"""CPU checks of the grouped-Conv1D models: the native tensor tables against the structure recorded from the reference
(tests/golden/grouped_models.json, made by tests/golden/make_golden_grouped.py), and the float64 oracle
(tests/grouped_oracle.py) against torch autograd with F.conv1d(groups=g) on the sliced input."""
import json
import os

import numpy as np
import pytest
import torch
import torch.nn.functional as Fn

from net_parity import native_table
from grouped_oracle import FAST_BLOCKS, KEEP, SPEC_BLOCKS, GroupedConvNet
from oracle.layers import dropout_key, dropout_mask
from speech_recognition_amd import _lib

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden', 'grouped_models.json')
KINDS = {'conv_1d_fast': _lib.KWS_NET_CONV_1D_FAST, 'conv_1d_spec': _lib.KWS_NET_CONV_1D_SPEC}


def _golden(name):
    with open(GOLDEN) as f:
        return json.load(f)[name]


@pytest.mark.parametrize("name", sorted(KINDS))
def test_native_tensor_table_matches_reference(name):
    gold = _golden(name)
    table = native_table(KINDS[name], gold['num_classes'], gold['input_size'])
    assert [t.name.decode() for t in table] == [w['name'] for w in gold['weights']]
    for t, w in zip(table, gold['weights']):
        assert [int(t.shape[k]) for k in range(t.ndim)] == w['shape'], w['name']
        assert bool(t.is_state) == bool(w.get('state', False)), w['name']
        assert t.l2 == np.float32(w['l2']), w['name']
        if w['name'].endswith('/kernel') and w['name'].startswith('conv1d'):
            k, cin, cout = w['shape']
            assert (t.fan_in, t.fan_out) == (k * cin, k * cout), w['name']
    # offsets: every tensor inside its buffer, none overlapping
    for state in (0, 1):
        spans = sorted((t.offset, t.offset + t.size) for t in table if t.is_state == state)
        assert all(a[1] <= b[0] for a, b in zip(spans, spans[1:]))


@pytest.mark.parametrize("name,blocks", [('conv_1d_fast', FAST_BLOCKS), ('conv_1d_spec', SPEC_BLOCKS)])
def test_group_slices_and_head_match_reference(name, blocks):
    gold = _golden(name)
    lambdas = [l for l in gold['layers'] if l['class'] == 'Lambda']
    want = []
    for F, k, g, nch, s in blocks:
        gs = nch // g
        want += [[q * gs, (q + 1) * gs] for q in range(g)]
    assert [l['slice'] for l in lambdas] == want
    convs = [l for l in gold['layers'] if l['class'] == 'Conv1D']
    grouped = convs[1:] if name == 'conv_1d_fast' else convs
    strides = [s for F, k, g, nch, s in blocks for _ in range(g)]
    assert [c['strides'] for c in grouped] == strides
    assert all(not c['use_bias'] and c['padding'] == 'valid' for c in convs)
    dense = [l for l in gold['layers'] if l['class'] == 'Dense']
    assert len(dense) == 1 and dense[0]['use_bias'] and dense[0]['activation'] == 'softmax'
    assert [l['rate'] for l in gold['layers'] if l['class'] == 'Dropout'] == [pytest.approx(1 - KEEP)]
    assert gold['loss'] == 'categorical_crossentropy' and gold['optimizer'] == 'RMSprop'
    assert (gold['model_name'], gold['lr']) == {'conv_1d_fast': ('conv_1d_learned_spec', 3e-3),
                                                'conv_1d_spec': ('conv_1d_spec', 2e-3)}[name]
    ora = GroupedConvNet(name.split('_')[-1])
    assert list(ora.params) == [w['name'] for w in gold['weights'] if not w.get('state')]
    assert list(ora.state) == [w['name'] for w in gold['weights'] if w.get('state')]


def _torch_loss(ora, x, y, seed, step):
    """The same network in torch float64: F.conv1d(groups=g) over the channels the groups read, F.batch_norm in training
    mode, clamp(0, 6), the oracle's dropout mask, softmax + categorical CE."""
    P = {k: torch.tensor(v.astype(np.float64), requires_grad=True) for k, v in ora.params.items()}
    B = x.shape[0]
    h = torch.tensor(x.astype(np.float64)).reshape((B,) + ora.in_shape).permute(0, 2, 1)   # [B, C, L]
    if ora.front:
        h = Fn.conv1d(h, P[ora.front].permute(2, 1, 0), stride=160)
    for blk in ora.blocks:
        W = torch.cat([P[n] for n in blk['convs']], dim=2).permute(2, 1, 0)   # [F, gs, k]
        y_ = Fn.conv1d(h[:, :blk['g'] * blk['gs']], W, stride=blk['stride'], groups=blk['g'])
        ga = torch.cat([P['batch_normalization_%d/gamma' % i] for i in blk['bns']])
        be = torch.cat([P['batch_normalization_%d/beta' % i] for i in blk['bns']])
        h = Fn.batch_norm(y_, None, None, ga, be, training=True, eps=1e-3).clamp(0, 6)
    flat = h.permute(0, 2, 1).reshape(B, -1)
    keep = dropout_mask(dropout_key(seed, step, 1), flat.numel(), KEEP).reshape(flat.shape)
    f = flat * torch.tensor(keep.astype(np.float64)) / KEEP
    p = torch.softmax(f @ P['dense_1/kernel'] + P['dense_1/bias'], dim=1)
    loss = -(torch.tensor(y.astype(np.float64)) * torch.log(p.clamp(1e-7, 1 - 1e-7))).sum(1).mean()
    loss.backward()
    return float(loss.detach()), p.detach().numpy(), {k: v.grad.numpy() for k, v in P.items()}


@pytest.mark.parametrize("kind,B", [('fast', 2), ('spec', 3)])
def test_oracle_gradients_match_torch_autograd(kind, B):
    ora = GroupedConvNet(kind, num_classes=12)
    rng = np.random.RandomState(7)
    x = (rng.randn(B, 16000 if kind == 'fast' else 98 * 257) * (0.1 if kind == 'fast' else 1.0)).astype(np.float32)
    y = np.eye(12, dtype=np.float32)[rng.randint(0, 12, B)]
    loss, p, grads, _ = ora.loss_and_grads(x, y, seed=3, step=5)
    tl, tp, tg = _torch_loss(ora, x, y, seed=3, step=5)
    assert abs(loss - tl) < 1e-10
    np.testing.assert_allclose(p, tp, atol=1e-12)
    for k, g in grads.items():
        scale = max(np.abs(tg[k]).max(), 1e-12)
        assert np.abs(g - tg[k]).max() / scale < 1e-9, k


def test_mutated_oracle_breaks_the_gradient_bar():
    """Negative control: the data gradient with its phases swapped moves every gradient below the last block far past the
    2e-4 relative bar the GPU tests apply."""
    ora = GroupedConvNet('spec', num_classes=12)
    rng = np.random.RandomState(8)
    x = rng.randn(3, 98 * 257).astype(np.float32)
    y = np.eye(12, dtype=np.float32)[rng.randint(0, 12, 3)]
    _, _, good, _ = ora.loss_and_grads(x, y, seed=1, step=0)
    _, _, bad, _ = ora.loss_and_grads(x, y, seed=1, step=0, mutate='swap_phase')
    err = max(np.abs(bad[k] - good[k]).max() / max(np.abs(good[k]).max(), 1e-12) for k in good)
    assert err > 1e-2
