"""CPU checks of the dense-Conv1D ladders conv_1d_time_stacked / conv_1d_heavy: the native tensor tables against the structure
recorded from the reference (tests/golden/stacked_models.json, made by tests/golden/make_golden_stacked.py) and against the
float64 oracle (tests/stacked_oracle.py); the oracle against torch autograd and its pool against F.max_pool1d(3, 2)."""
import ctypes
import json
import os

import numpy as np
import pytest
import torch
import torch.nn.functional as Fn

import pool_oracle
from net_parity import native_table, perturb
from oracle.layers import dropout_key, dropout_mask
from pool_oracle import pool_len
from speech_recognition_amd import _lib
from stacked_oracle import HEAD_WIDTH, KEEP1, KEEP2, NETS, StackedConvNet

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden', 'stacked_models.json')
KINDS = {'conv_1d_time_stacked': 8, 'conv_1d_heavy': 9}
# the issue's ladders (conv outputs and pool outputs in order), which the fixture has to reproduce
LADDERS = {'conv_1d_time_stacked': [800, 798, 398, 396, 394, 196, 194, 192, 95, 93, 91, 45, 43, 41, 20, 18, 16, 7, 5, 1],
           'conv_1d_heavy': [1600, 1598, 798, 796, 794, 396, 394, 392, 195, 193, 191, 95, 93, 91, 45, 43, 41, 20, 18, 16, 7, 5,
                             1, 1]}


def _golden(name):
    with open(GOLDEN) as f:
        return json.load(f)[name]


def test_kind_constants():
    assert (_lib.KWS_NET_CONV_1D_TIME_STACKED, _lib.KWS_NET_CONV_1D_HEAVY) == (8, 9)


@pytest.mark.parametrize("name", sorted(KINDS))
def test_fixture_has_the_expected_structure(name):
    gold = _golden(name)
    steps = [l['output'][0] for l in gold['layers'] if l['class'] in ('Conv1D', 'MaxPool1D')]
    assert steps == LADDERS[name]
    assert (gold['model_name'], gold['optimizer'], gold['lr'], gold['loss']) == \
        ('conv_1d_time_stacked', 'Adam', 3e-4, 'categorical_crossentropy')
    assert gold['output_shape'] == [gold['num_classes']]
    pools = [l for l in gold['layers'] if l['class'] == 'MaxPool1D']
    assert all((l['pool_size'], l['strides'], l['padding']) == (3, 2, 'valid') for l in pools)
    convs = [l for l in gold['layers'] if l['class'] == 'Conv1D']
    assert all(c['strides'] == 1 and c['padding'] == 'valid' for c in convs)
    rates = [l['rate'] for l in gold['layers'] if l['class'] == 'Dropout']
    if name == 'conv_1d_heavy':
        assert rates == [pytest.approx(1 - KEEP1), pytest.approx(1 - KEEP2)]
        assert [c['use_bias'] for c in convs[-2:]] == [False, False] and convs[-2]['kernel'] == [5, 320, HEAD_WIDTH]
        assert (convs[-1]['kernel'], convs[-1]['activation']) == ([1, HEAD_WIDTH, gold['num_classes']], 'softmax')
    else:
        assert rates == [pytest.approx(1 - KEEP1)]
        assert convs[-1]['use_bias'] and convs[-1]['activation'] == 'softmax' and convs[-1]['kernel'] == [5, 256, gold['num_classes']]


@pytest.mark.parametrize("name", sorted(KINDS))
def test_native_tensor_table_matches_reference_and_oracle(name):
    gold = _golden(name)
    table = native_table(KINDS[name], gold['num_classes'], gold['input_size'])
    assert [t.name.decode() for t in table] == [w['name'] for w in gold['weights']]
    for t, w in zip(table, gold['weights']):
        assert [int(t.shape[k]) for k in range(t.ndim)] == w['shape'], w['name']
        assert bool(t.is_state) == bool(w.get('state', False)), w['name']
        assert t.l2 == np.float32(w['l2']), w['name']
        if w['name'].endswith('/kernel'):
            k, cin, cout = w['shape']
            assert (t.fan_in, t.fan_out) == (k * cin, k * cout), w['name']
    for state in (0, 1):
        spans = sorted((t.offset, t.offset + t.size) for t in table if t.is_state == state)
        assert all(a[1] <= b[0] for a, b in zip(spans, spans[1:]))
    ora = StackedConvNet(name[len('conv_1d_'):], num_classes=gold['num_classes'])
    assert [t.name.decode() for t in table if not t.is_state] == list(ora.params)
    assert [t.name.decode() for t in table if t.is_state] == list(ora.state)
    for t in table:
        v = ora.state[t.name.decode()] if t.is_state else ora.params[t.name.decode()]
        assert tuple(int(t.shape[k]) for k in range(t.ndim)) == v.shape
    assert sum(t.size for t in table) == ora.count_params()
    # l2 1e-5 on the ladder kernels only
    assert {t.name.decode() for t in table if t.l2 > 0} == set(ora.l2_names)
    assert all(t.l2 == np.float32(1e-5) for t in table if t.l2 > 0)


@pytest.mark.parametrize("kind", sorted(KINDS.values()))
def test_native_table_rejects_other_input_sizes(kind):
    lib = _lib.load()
    cfg = _lib.NetConfig(kind, 12, 1, 8000, 0, 0)
    h = ctypes.c_void_p()
    assert lib.kws_net_create(ctypes.byref(cfg), ctypes.byref(h)) != 0
    assert b'input_size' in lib.kws_last_error()


def test_model_builders_reject_other_input_sizes():
    from speech_recognition_amd.model import ACCELERATED, speech_model
    assert 'conv_1d_time_stacked' in ACCELERATED and 'conv_1d_heavy' in ACCELERATED
    for model_type in ('conv_1d_time_stacked', 'conv_1d_heavy'):
        with pytest.raises(ValueError):
            speech_model(model_type, 8000, num_classes=12)


def test_speech_model_settings(monkeypatch):
    """Name, loss, optimizer class and lr of both builders (the device net itself replaced: no GPU here)."""
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
    for model_type, kind in (('conv_1d_time_stacked', 8), ('conv_1d_heavy', 9)):
        M.speech_model(model_type, 16000, num_classes=12)
        assert captured['net'].kind == kind and captured['net'].num_classes == 12 and captured['net'].kw['input_size'] == 16000
        assert captured['name'] == 'conv_1d_time_stacked' and captured['loss'] == 'cce'
        assert isinstance(captured['optimizer'], keras_api.Adam) and abs(float(captured['optimizer'].lr) - 3e-4) < 1e-9


@pytest.mark.parametrize("L", [7, 8, 16, 95])
def test_oracle_pool_matches_torch_max_pool1d(L):
    rng = np.random.RandomState(L)
    a = np.clip(rng.randn(3, L, 8) * 3.0, 0, 6)       # saturated 0 / 6 values: plenty of ties
    ind = pool_oracle.argmax(a, pool_len(L), 0)
    z = pool_oracle.fwd(a, ind, 0)
    ta = torch.tensor(a, requires_grad=True)
    tz = Fn.max_pool1d(ta.permute(0, 2, 1), 3, 2).permute(0, 2, 1)
    assert tz.shape[1] == pool_len(L)
    np.testing.assert_array_equal(z, tz.detach().numpy())
    dz = rng.randn(*z.shape)
    tz.backward(torch.tensor(dz))
    np.testing.assert_allclose(pool_oracle.bwd(dz, ind, L, 0), ta.grad.numpy(), atol=1e-15)   # torch routes to the first maximum too
    if L % 2 == 0:
        assert not pool_oracle.bwd(np.ones_like(dz), ind, L, 0)[:, -1].any()


def _torch_loss(ora, x, y, seed, step):
    """The same network in torch float64: F.conv1d, F.batch_norm in training mode, clamp(0, 6), F.max_pool1d(3, 2), the
    oracle's dropout masks, softmax + categorical CE."""
    P = {k: torch.tensor(v.astype(np.float64), requires_grad=True) for k, v in ora.params.items()}
    B = x.shape[0]
    h = torch.tensor(x.astype(np.float64)).reshape((B,) + ora.in_shape).permute(0, 2, 1)   # [B, C, L]

    def layer(h, lay):
        h = Fn.conv1d(h, P[lay['conv']].permute(2, 1, 0))
        i = lay['idx']
        h = Fn.batch_norm(h, None, None, P['batch_normalization_%d/gamma' % i], P['batch_normalization_%d/beta' % i],
                          training=True, eps=1e-3).clamp(0, 6)
        return Fn.max_pool1d(h, 3, 2) if lay['pool'] else h

    for lay in ora.layers[:ora.ladder]:
        h = layer(h, lay)
    flat = h.permute(0, 2, 1).reshape(B, -1)
    keep = dropout_mask(dropout_key(seed, step, 1), flat.numel(), KEEP1).reshape(flat.shape)
    f = flat * torch.tensor(keep.astype(np.float64)) / KEEP1
    if ora.kind == 'heavy':
        a = layer(f.reshape(B, 5, -1).permute(0, 2, 1), ora.layers[-1]).reshape(B, HEAD_WIDTH)
        keep2 = dropout_mask(dropout_key(seed, step, 2), a.numel(), KEEP2).reshape(a.shape)
        logits = (a * torch.tensor(keep2.astype(np.float64)) / KEEP2) @ P[ora.out_kernel][0]
    else:
        logits = f @ P[ora.out_kernel].reshape(ora.Dd, ora.nc) + P[ora.out_bias]
    p = torch.softmax(logits, dim=1)
    loss = -(torch.tensor(y.astype(np.float64)) * torch.log(p.clamp(1e-7, 1 - 1e-7))).sum(1).mean()
    loss.backward()
    return float(loss.detach()), p.detach().numpy(), {k: v.grad.numpy() for k, v in P.items()}


def _perturbed(kind, seed=5):
    ora = StackedConvNet(kind, num_classes=12)
    perturb(ora, seed, negative_fraction=0.33, beta=(0.5, 0.3), bias=None, state=False)
    return ora


@pytest.mark.parametrize("kind,B", [('time_stacked', 3), ('heavy', 4)])
def test_oracle_gradients_match_torch_autograd(kind, B):
    ora = _perturbed(kind)
    rng = np.random.RandomState(7)
    x = (rng.randn(B, 16000) * 0.3).astype(np.float32)
    y = np.eye(12, dtype=np.float32)[rng.randint(0, 12, B)]
    loss, p, grads, _ = ora.loss_and_grads(x, y, seed=3, step=5)
    tl, tp, tg = _torch_loss(ora, x, y, seed=3, step=5)
    assert abs(loss - tl) < 1e-10
    np.testing.assert_allclose(p, tp, atol=1e-12)
    for k, g in grads.items():
        scale = max(np.abs(tg[k]).max(), 1e-12)
        assert np.abs(g - tg[k]).max() / scale < 1e-9, k


def test_last_max_routing_differs_on_ties():
    """Inside the nets a tie between two activations is (up to exact float coincidences) a tie of saturated 0 / 6 values,
    whose ReLU6 gates are shut: last-max-wins cannot move a net gradient, so this control works on the pool itself with
    quantised activations strictly inside (0, 6), as test_stacked_pool_gpu.py does on the device."""
    rng = np.random.RandomState(3)
    a = rng.randint(1, 5, size=(4, 33, 16)).astype(np.float64)
    dz = rng.randn(4, pool_len(33), 16)
    good = pool_oracle.bwd(dz, pool_oracle.argmax(a, pool_len(33), 0), 33, 0)
    bad = pool_oracle.bwd(dz, pool_oracle.argmax(a, pool_len(33), 0, last=True), 33, 0)
    assert np.abs(bad - good).max() / np.abs(good).max() > 1e-2


@pytest.mark.parametrize("mutate", ['pool_before_act', 'no_gate'])
def test_mutated_oracle_breaks_the_gradient_bar(mutate):
    """Negative control on the oracle itself: each wrong pool variant moves the gradients far past the 2e-4 relative bar the
    GPU tests apply (inputs with negative BN scales and saturated activations, as there)."""
    ora = _perturbed('time_stacked')
    rng = np.random.RandomState(8)
    x = (rng.randn(3, 16000) * 0.3).astype(np.float32)
    y = np.eye(12, dtype=np.float32)[rng.randint(0, 12, 3)]
    _, _, good, _ = ora.loss_and_grads(x, y, seed=1, step=0)
    _, _, bad, _ = ora.loss_and_grads(x, y, seed=1, step=0, mutate=mutate)
    err = max(np.abs(bad[k] - good[k]).max() / max(np.abs(good[k]).max(), 1e-12) for k in good)
    assert err > 1e-2, err
