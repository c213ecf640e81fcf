"""CPU checks of inception_d1 (KWS_NET_INCEPTION_D1): the fixture recorded from the reference (tests/golden/inception_models.json,
made by tests/golden/make_golden_inception.py) against the model as the issue states it; the native tensor table against the
fixture and the oracle (tests/inception_oracle.py); the speech_model surface; the oracle against torch autograd in float64, its
average pool against F.avg_pool1d(count_include_pad=False), its mutations; and the float32 run of the oracle against its float64
self on the GPU tests' own weights and batches (the figures of test_inception_models_gpu.py's docstring)."""
import ctypes
import json
import os

import numpy as np
import pytest
import torch
import torch.nn.functional as Fn

import inception_cases as cases
from inception_oracle import (BLOCKS, KEEP, InceptionD1Net, avgpool_bwd, avgpool_fwd, same_pool_pad_l)
from net_parity import grad_errors, native_table
from oracle.layers import dropout_key, dropout_mask
from speech_recognition_amd import _lib

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden', 'inception_models.json')
KIND = 14
# conv and pool output lengths of the stem, then the joined tensors' lengths
STEM_LADDER = [800, 798, 398, 396, 394, 196, 194, 192, 95, 93]
MIXED_LENGTHS = [93, 93, 47, 47, 47, 24, 24, 24, 12, 12, 12, 6]
MIXED_DIL = {1: 2, 2: 2, 4: 2, 5: 1, 7: 1, 8: 1, 10: 1, 11: 1}


def _golden():
    with open(GOLDEN) as f:
        return json.load(f)['inception_d1']


def test_kind_constant():
    assert _lib.KWS_NET_INCEPTION_D1 == KIND


def test_fixture_has_the_expected_structure():
    gold = _golden()
    layers = gold['layers']
    by_name = {l['name']: l for l in layers}
    assert (gold['model_name'], gold['optimizer'], gold['lr'], gold['loss']) == ('inception_d1', 'Adam', 1e-3, 'categorical_crossentropy')
    assert gold['output_shape'] == [gold['num_classes']] == [12]
    convs = [l for l in layers if l['class'] == 'Conv1D']
    bns = [l for l in layers if l['class'] == 'BatchNormalization']
    assert (len(convs), len(bns)) == (80, 79)
    assert all(c['strides'] == 1 for c in convs) and not any(c['use_bias'] for c in convs[:-1])
    assert layers[0]['class'] == 'Reshape' and layers[0]['output'] == [800, 20]
    # the stem: lengths, widths, VALID
    first_mixed = next(i for i, l in enumerate(layers) if l['class'] == 'Concatenate')
    stem = [l for l in layers[:first_mixed] if l['class'] in ('Conv1D', 'MaxPool1D') and l['input_length'] > 93]   # (block 1 reads 93 rows)
    assert [l['output'][0] for l in stem] == STEM_LADDER
    assert [c['kernel'] for c in convs[:7]] == [[1, 20, 32], [3, 32, 64], [3, 64, 64], [3, 64, 128], [3, 128, 128], [3, 128, 256],
                                                [3, 256, 256]]
    assert all(c['padding'] == 'valid' for c in convs[1:7])
    stem_pools = [l for l in stem if l['class'] == 'MaxPool1D']
    assert len(stem_pools) == 3 and all((l['pool_size'], l['strides'], l['padding']) == (3, 2, 'valid') for l in stem_pools)
    # the twelve joined tensors
    mixed = [l for l in layers if l['class'] == 'Concatenate']
    assert [m['name'] for m in mixed] == ['mixed%d' % i for i in range(1, 13)]
    assert [m['output'][0] for m in mixed] == MIXED_LENGTHS

    def conv_behind(act_name):     # activation_<n> -> conv1d_<n> record (every BatchNormalization follows its convolution)
        bn = by_name[by_name[act_name]['input_from']]
        return by_name[bn['input_from']]

    n = 7
    for bid, m in enumerate(mixed, 1):
        T = by_name['conv1d_%d' % (n + 1)]['input_length']
        if bid in MIXED_DIL:
            d = MIXED_DIL[bid]
            assert [w for _, w in m['inputs']] == [64, 64, 96, 32] and m['output'][1] == 256
            cs = [by_name['conv1d_%d' % (n + i)] for i in range(1, 8)]     # Keras creation order
            assert [(c['kernel'][0], c['kernel'][2], c['dilation_rate']) for c in cs] == \
                [(1, 64, 1), (1, 48, 1), (3, 64, 2), (1, 64, 1), (3, 96, d), (3, 96, d), (1, 32, 1)]
            assert all(c['padding'] == 'same' and c['output'][0] == T for c in cs)
            assert [c['pad_left'] for c in cs] == [0, 0, 2, 0, d, d, 0] and [c['pad_total'] for c in cs] == [0, 0, 4, 0, 2 * d, 2 * d, 0]
            assert [conv_behind(a)['name'] for a in m['inputs_from']] == ['conv1d_%d' % (n + i) for i in (1, 3, 6, 7)]
            avg = by_name[cs[6]['input_from']]
            assert (avg['class'], avg['pool_size'], avg['strides'], avg['padding']) == ('AveragePooling1D', 3, 1, 'same')
            src = {cs[0]['input_from'], cs[1]['input_from'], cs[3]['input_from'], avg['input_from']}
            assert len(src) == 1                                             # four consumers of the block input
            n += 7
        else:
            cin = by_name['conv1d_%d' % (n + 1)]['kernel'][1]
            assert [w for _, w in m['inputs']] == [192, 48, cin] and m['output'][1] == 496
            cs = [by_name['conv1d_%d' % (n + i)] for i in range(1, 5)]
            assert [(c['kernel'][0], c['kernel'][2], c['dilation_rate'], c['padding']) for c in cs] == \
                [(3, 192, 1, 'same'), (1, 32, 1, 'same'), (3, 48, 1, 'same'), (3, 48, 1, 'same')]
            pools = [by_name[a] for a in m['inputs_from']]
            assert all((p['class'], p['pool_size'], p['strides'], p['padding']) == ('MaxPool1D', 3, 2, 'same') for p in pools)
            assert all(p['pad_left'] == (T & 1) and p['pad_total'] == 1 + (T & 1) for p in pools)
            assert [conv_behind(pools[i]['input_from'])['name'] for i in (0, 1)] == ['conv1d_%d' % (n + 1), 'conv1d_%d' % (n + 4)]
            assert pools[2]['input_from'] == cs[0]['input_from'] == cs[1]['input_from']
            n += 4
    assert n == 79
    assert [l['rate'] for l in layers if l['class'] == 'Dropout'] == [pytest.approx(1 - KEEP)]
    assert convs[-1]['kernel'] == [6, 496, 12] and convs[-1]['use_bias'] and convs[-1]['activation'] == 'softmax'
    assert convs[-1]['padding'] == 'valid' and convs[-1]['output'] == [1, 12]
    kernels = sum(int(np.prod(w['shape'])) for w in gold['weights'] if w['name'].endswith('/kernel'))
    bn_floats = sum(int(np.prod(w['shape'])) for w in gold['weights'] if w['name'].startswith('batch_normalization'))
    assert (kernels - 6 * 496 * 12, bn_floats, 6 * 496 * 12 + 12) == (2074496, 23680, 35724)
    assert sum(int(np.prod(w['shape'])) for w in gold['weights']) == 2133900


def test_native_tensor_table_matches_reference_and_oracle():
    gold = _golden()
    table = native_table(KIND, gold['num_classes'], gold['input_size'])
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
    ora = InceptionD1Net(num_classes=gold['num_classes'])
    assert [t.name.decode() for t in table if not t.is_state] == list(ora.params)
    assert [t.name.decode() for t in table if t.is_state] == list(ora.state)
    for t in table:
        v = ora.state[t.name.decode()] if t.is_state else ora.params[t.name.decode()]
        assert tuple(int(t.shape[k]) for k in range(t.ndim)) == v.shape
    assert sum(t.size for t in table) == ora.count_params() == 2133900
    # l2 1e-5 on the ladder and block kernels only
    assert {t.name.decode() for t in table if t.l2 > 0} == set(ora.l2_names)
    assert all(t.l2 == np.float32(1e-5) for t in table if t.l2 > 0)
    # the oracle's geometry is the fixture's
    by_name = {l['name']: l for l in gold['layers']}
    for c in ora.convs:
        l = by_name['conv1d_%d' % c['idx']]
        assert (l['kernel'], l['dilation_rate'], l['padding'], l['input_length'], l['output'][0]) == \
            ([c['k'], c['C'], c['F']], c['dil'], c['padding'], c['L'], c['Lout']), c['idx']
    assert [k for k, _ in BLOCKS] == ['inc' if len(m['inputs']) == 4 else 'red' for m in gold['layers'] if m['class'] == 'Concatenate']


def test_native_table_rejects_other_input_sizes():
    lib = _lib.load()
    cfg = _lib.NetConfig(KIND, 12, 1, 8000, 0, 0)
    h = ctypes.c_void_p()
    assert lib.kws_net_create(ctypes.byref(cfg), ctypes.byref(h)) != 0
    assert b'input_size' in lib.kws_last_error()


def test_speech_model_surface(monkeypatch):
    """speech_model('inception_d1') asks for kind 14, Adam(1e-3), the Keras name and 'cce' (the device net itself replaced: no GPU
    here); another input size is a ValueError."""
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
    assert 'inception_d1' in M.ACCELERATED
    M.speech_model('inception_d1', 16000, num_classes=12)
    assert captured['net'].kind == KIND and captured['net'].num_classes == 12 and captured['net'].kw['input_size'] == 16000
    assert captured['name'] == 'inception_d1' and captured['loss'] == 'cce'
    assert isinstance(captured['optimizer'], keras_api.Adam) and abs(float(captured['optimizer'].lr) - 1e-3) < 1e-9
    with pytest.raises(ValueError):
        M.speech_model('inception_d1', 8000, num_classes=12)


@pytest.mark.parametrize("L", [1, 2, 6, 93])
def test_oracle_average_pool_matches_torch(L):
    rng = np.random.RandomState(L)
    a = rng.rand(3, L, 8) * 6.0
    ta = torch.tensor(a, requires_grad=True)
    tz = Fn.avg_pool1d(ta.permute(0, 2, 1), 3, 1, padding=1, count_include_pad=False).permute(0, 2, 1)
    np.testing.assert_allclose(avgpool_fwd(a), tz.detach().numpy(), atol=1e-14)
    dz = rng.randn(3, L, 8)
    tz.backward(torch.tensor(dz))
    np.testing.assert_allclose(avgpool_bwd(dz), ta.grad.numpy(), atol=1e-14)
    if L > 1:   # the wrong divisor differs at the two ends only
        bad = avgpool_fwd(a, include_pad=True)
        assert np.abs(bad - avgpool_fwd(a))[:, [0, -1]].min() > 0 and np.array_equal(bad[:, 1:-1], avgpool_fwd(a)[:, 1:-1])


def _torch_loss(ora, x, y, seed, step):
    """The same network in torch float64: F.conv1d with dilation / padding, F.batch_norm in training mode (eps 1e-3),
    clamp(0, 6), F.avg_pool1d(count_include_pad=False), max pools with TensorFlow's SAME padding, the oracle's dropout mask,
    softmax + categorical CE."""
    P = {k: torch.tensor(v.astype(np.float64), requires_grad=True) for k, v in ora.params.items()}
    B = x.shape[0]
    h = torch.tensor(x.astype(np.float64)).reshape(B, 800, 20).permute(0, 2, 1)   # [B, C, L]

    def same_max_pool(h):
        L = h.shape[2]
        Lp = (L + 1) // 2
        pl = same_pool_pad_l(L)
        return Fn.max_pool1d(Fn.pad(h, (pl, 2 * (Lp - 1) + 3 - L - pl), value=float('-inf')), 3, 2)

    def layer(h, c):
        pad = c['dil'] * (c['k'] - 1) // 2 if c['padding'] == 'same' else 0     # (odd k: TF SAME is symmetric at stride 1)
        h = Fn.conv1d(h, P[c['conv']].permute(2, 1, 0), dilation=c['dil'], padding=pad)
        i = c['idx']
        h = Fn.batch_norm(h, None, None, P['batch_normalization_%d/gamma' % i], P['batch_normalization_%d/beta' % i],
                          training=True, eps=1e-3).clamp(0, 6)
        return Fn.max_pool1d(h, 3, 2) if c['pool'] == 'valid' else same_max_pool(h) if c['pool'] == 'same' else h

    for _, c in ora.plan:
        h = layer(h, c)
    for rec in ora.blocks:
        cs = rec['convs']
        if rec['kind'] == 'inc':
            h = torch.cat([layer(h, cs[0]), layer(layer(h, cs[1]), cs[2]), layer(layer(layer(h, cs[3]), cs[4]), cs[5]),
                           layer(Fn.avg_pool1d(h, 3, 1, padding=1, count_include_pad=False), cs[6])], dim=1)
        else:
            h = torch.cat([layer(h, cs[0]), layer(layer(layer(h, cs[1]), cs[2]), cs[3]), same_max_pool(h)], dim=1)
    flat = h.permute(0, 2, 1).reshape(B, -1)
    keep = dropout_mask(dropout_key(seed, step, 1), flat.numel(), KEEP).reshape(flat.shape)
    f = flat * torch.tensor(keep.astype(np.float64)) / KEEP
    logits = f @ P[ora.out_kernel].reshape(ora.D, ora.nc) + P[ora.out_bias]
    p = torch.softmax(logits, dim=1)
    loss = -(torch.tensor(y.astype(np.float64)) * torch.log(p.clamp(1e-7, 1 - 1e-7))).sum(1).mean()
    loss.backward()
    return float(loss.detach()), p.detach().numpy(), {k: v.grad.numpy() for k, v in P.items()}


def test_oracle_gradients_match_torch_autograd():
    ora = cases.perturbed()
    assert 0.25 < np.mean([(v < 0).mean() for k, v in ora.params.items() if k.endswith('gamma')]) < 0.42
    rng = np.random.RandomState(7)
    x = (rng.randn(3, 16000) * 0.3).astype(np.float32)
    y = np.eye(12, dtype=np.float32)[rng.randint(0, 12, 3)]
    loss, p, grads, _ = ora.loss_and_grads(x, y, seed=3, step=5)
    tl, tp, tg = _torch_loss(ora, x, y, seed=3, step=5)
    assert abs(loss - tl) < 1e-10
    np.testing.assert_allclose(p, tp, atol=1e-12)
    for k, g in grads.items():
        scale = max(np.abs(tg[k]).max(), 1e-12)
        assert np.abs(g - tg[k]).max() / scale < 1e-9, k


@pytest.mark.parametrize("mutate", ['avg_count_include_pad', 'ignore_dilation', 'pad_before_act', 'concat_order'])
def test_mutated_oracle_moves_the_gradients(mutate):
    """Negative control on the oracle itself: each wrong variant moves some gradient by more than 1e-2 relative, far past the 2e-4
    bar of the GPU tests."""
    ora = cases.perturbed()
    x, y = cases.batch(3)
    _, _, good, _ = ora.loss_and_grads(x, y, seed=1, step=0)
    _, _, bad, _ = ora.loss_and_grads(x, y, seed=1, step=0, mutate=mutate)
    err = max(grad_errors(bad, good).values())
    assert err > 1e-2, err


def test_float32_oracle_predict_is_within_half_the_gpu_bar():
    ref = cases.perturbed().forward(cases.batch(cases.PREDICT_BATCH, seed=1)[0], training=False)
    p32 = cases.perturbed(np.float32).forward(cases.batch(cases.PREDICT_BATCH, seed=1)[0], training=False)
    err = np.abs(p32.astype(np.float64) - ref).max()
    print("float32 oracle predict B=%d: max |p - float64| = %.3g (bar 2e-5)" % (cases.PREDICT_BATCH, err))
    assert err < 0.5 * 2e-5


@pytest.mark.parametrize("B", cases.TRAIN_BATCHES)
def test_float32_oracle_train_step_is_within_half_the_gpu_bars(B):
    """The oracle in float32 (on the float64 run's gates and pool winners) against its float64 self, on the GPU tests' weights
    and batches: what float32 arithmetic alone costs.  Each figure has to stay under half the bar the GPU test applies."""
    ora = cases.perturbed()
    x, y = cases.batch(B)
    loss, p, grads, cache = ora.loss_and_grads(x, y, seed=cases.SEED, step=cases.STEP)
    masks, inds = cases.decisions_of(ora, cache)
    o32 = cases.perturbed(np.float32)
    loss32, p32, grads32, cache32 = o32.loss_and_grads(x, y, seed=cases.SEED, step=cases.STEP, relu_masks=masks, pool_ind=inds)
    errs = grad_errors(grads32, grads)
    worst = max(errs, key=errs.get)
    stat = max(max(np.abs(cache32['batch_stats'][i][q].astype(np.float64) - cache['batch_stats'][i][q]).max() for q in (0, 1))
               for i in cache['batch_stats'])
    print("float32 oracle train B=%d: probs %.3g (bar 5e-5), loss %.3g (bar 1e-4), worst gradient %s %.3g (bar 2e-4), batch "
          "statistics %.3g" % (B, np.abs(p32 - p).max(), abs(float(loss32) - loss), worst, errs[worst], stat))
    assert np.abs(p32 - p).max() < 0.5 * 5e-5
    assert abs(float(loss32) - loss) < 0.5 * 1e-4
    assert errs[worst] < 0.5 * 2e-4, (worst, errs[worst])
