"""CPU checks of the bidirectional GRU and conv_1d_simple: the kind constant and the kws_gru_* symbols, the native tensor table of
kind 12 against the structure recorded from the reference (tests/golden/gru_models.json, made by tests/golden/make_golden_gru.py) and
against the oracle, the model settings, the orthogonal draw of DeviceNet.initialize, the float64 oracle (tests/gru_oracle.py)
against torch autograd, its mutations, the host-side domain checks of kws_gru_*, and how close the kernel tests' inputs come to the
hard sigmoid's corners."""
import ctypes
import os
from collections import OrderedDict

import numpy as np
import pytest
import torch

from net_parity import native_table
from oracle.layers import dropout_key, dropout_mask
from speech_recognition_amd import _lib
from gru_oracle import (KEEP, KERNEL_CASES, SimpleNet, bigru_bwd, bigru_fwd, draw_masks, golden, kernel_inputs)

GRU_SYMBOLS = ['kws_gru_save_floats', 'kws_gru_workspace_floats', 'kws_gru_masks', 'kws_gru_seq_fwd_f32', 'kws_gru_seq_bwd_f32',
               'kws_gru_fwd_f32', 'kws_gru_bwd_f32']


def test_kind_constant_and_symbols(repo_root):
    assert _lib.KWS_NET_CONV_1D_SIMPLE == 12
    header = open(os.path.join(repo_root, 'include', 'kws_hip.h')).read()
    assert '#define KWS_NET_CONV_1D_SIMPLE 12' in header and '#define KWS_ABI_VERSION 5' in header
    lib = _lib.load()
    for name in GRU_SYMBOLS:
        assert name in _lib.SIGNATURES and (name + '(') in header and hasattr(lib, name)


def test_fixture_structure():
    gold = golden()
    dws = [l for l in gold['layers'] if l['class'] == 'DepthwiseConv2D']
    assert len(dws) == 14 and all(l['padding'] == 'valid' for l in dws)
    assert [l['kernel'][1] for l in dws] == [31] + [3] * 13
    assert [l['strides'] for l in dws] == [16, 1] + [2, 1] * 6
    assert [c['kernel'][2] for c in gold['layers'] if c['class'] == 'Conv1D'] == [32, 32] + [f for f in range(64, 225, 32) for _ in (0, 1)]
    assert dws[-1]['output'] == [10, 224]
    bi = [l for l in gold['layers'] if l['class'] == 'Bidirectional']
    gru = [l for l in gold['layers'] if l['class'] == 'GRU']
    assert len(bi) == 1 and len(gru) == 1
    assert (gru[0]['units'], gru[0]['dropout'], gru[0]['recurrent_dropout'], gru[0]['return_sequences']) == (128, 0.2, 0.2, False)
    assert (gru[0]['activation'], gru[0]['recurrent_activation'], gru[0]['implementation']) == ('tanh', 'hard_sigmoid', 1)
    assert (bi[0]['kernel'], bi[0]['recurrent_kernel'], bi[0]['bias'], bi[0]['output'], bi[0]['merge_mode']) == \
        ([224, 384], [128, 384], [384], [256], 'concat')
    assert (gold['model_name'], gold['optimizer'], gold['lr'], gold['loss']) == ('conv_1d_time_stacked', 'Adam', 1e-3, 'categorical_crossentropy')
    assert not any(l['class'] == 'Dropout' for l in gold['layers'])
    dense = [l for l in gold['layers'] if l['class'] == 'Dense']
    assert [(d['kernel'], d['use_bias'], d['activation']) for d in dense] == [([256, 12], True, 'softmax')]


def test_native_tensor_table_matches_reference_and_oracle():
    gold = golden()
    table = native_table(_lib.KWS_NET_CONV_1D_SIMPLE, gold['num_classes'], gold['input_size'])
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
        assert all(a[0] % 4 == 0 for a in spans)
    names = [w['name'] for w in gold['weights']]
    i0 = names.index('bidirectional_1/forward_gru_1/kernel')
    assert names[i0:] == ['bidirectional_1/%s_gru_1/%s' % (d, w) for d in ('forward', 'backward') for w in ('kernel', 'recurrent_kernel', 'bias')] + \
        ['dense_1/kernel', 'dense_1/bias']
    ora = SimpleNet(num_classes=gold['num_classes'])
    assert [t.name.decode() for t in table if not t.is_state] == list(ora.params)
    assert [t.name.decode() for t in table if t.is_state] == list(ora.state)
    for t in table:
        v = ora.state[t.name.decode()] if t.is_state else ora.params[t.name.decode()]
        assert tuple(int(t.shape[k]) for k in range(t.ndim)) == v.shape
    n_train = sum(int(np.prod(w['shape'])) for w in gold['weights'] if not w.get('state'))
    assert sum(t.size for t in table if not t.is_state) == n_train
    assert sum(t.size for t in table) == ora.count_params()
    # l2 1e-5 on every depthwise and pointwise kernel; none on the GRU or the Dense layer
    assert {t.name.decode() for t in table if t.l2 > 0} == set(ora.l2_names) and len(ora.l2_names) == 28


def test_native_table_rejects_other_input_sizes():
    lib = _lib.load()
    cfg = _lib.NetConfig(_lib.KWS_NET_CONV_1D_SIMPLE, 12, 1, 8000, 0, 0)
    h = ctypes.c_void_p()
    assert lib.kws_net_create(ctypes.byref(cfg), ctypes.byref(h)) != 0
    assert b'input_size' in lib.kws_last_error()


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
    assert 'conv_1d_simple' in M.ACCELERATED
    M.speech_model('conv_1d_simple', 16000, num_classes=12)
    assert captured['net'].kind == 12 and captured['net'].num_classes == 12 and captured['net'].kw['input_size'] == 16000
    assert captured['name'] == 'conv_1d_time_stacked' and captured['loss'] == 'cce'
    opt = captured['optimizer']
    assert isinstance(opt, keras_api.Adam) and abs(float(opt.lr) - 1e-3) < 1e-9
    assert (opt.beta_1, opt.beta_2, opt.epsilon) == (0.9, 0.999, 1e-8)
    with pytest.raises(ValueError):
        M.speech_model('conv_1d_simple', 8000, num_classes=12)


def test_initialize_draws_orthogonal_recurrent_kernels():
    """DeviceNet.initialize on a host stand-in for the device buffers: recurrent kernels have orthonormal rows, every other tensor
    holds what the parent's rule gives it (one RandomState(seed) stream over the tensors with fan_in > 0, in table order)."""
    from speech_recognition_amd.net import DeviceNet, TensorSpec
    table = native_table(_lib.KWS_NET_CONV_1D_SIMPLE)
    net = DeviceNet.__new__(DeviceNet)
    net.tensors = OrderedDict()
    for ti in table:
        s = TensorSpec()
        s.name, s.offset, s.size = ti.name.decode(), int(ti.offset), int(ti.size)
        s.shape = tuple(int(ti.shape[k]) for k in range(ti.ndim))
        s.is_state, s.l2, s.fan_in, s.fan_out, s.init = bool(ti.is_state), float(ti.l2), ti.fan_in, ti.fan_out, float(ti.init)
        net.tensors[s.name] = s
    net.n_params = max(s.offset + s.size for s in net.tensors.values() if not s.is_state)
    net.n_state = max(s.offset + s.size for s in net.tensors.values() if s.is_state)
    net.params, net.state, net.l2 = torch.zeros(net.n_params), torch.zeros(net.n_state), torch.zeros(net.n_params)
    net.slots, net.grads, net.slots2 = torch.zeros(net.n_params), torch.zeros(net.n_params), None
    net.handle = None
    net.initialize(seed=4321)
    p = net.params.numpy()
    rng = np.random.RandomState(4321)
    rec = []
    for s in net.tensors.values():
        if s.is_state:
            continue
        got = p[s.offset:s.offset + s.size]
        if s.name.endswith('/recurrent_kernel'):
            rec.append(got.reshape(s.shape).astype(np.float64))
        elif s.fan_in > 0:
            limit = np.sqrt(6.0 / (s.fan_in + s.fan_out))
            assert np.array_equal(got, rng.uniform(-limit, limit, size=s.size).astype(np.float32)), s.name
        else:
            assert np.all(got == np.float32(s.init)), s.name
    assert len(rec) == 2 and rec[0].shape == (128, 384)
    for q in rec:
        assert np.abs(q @ q.T - np.eye(128)).max() < 1e-5
    assert np.abs(rec[0] - rec[1]).max() > 1e-2       # two draws, not one


# ---- the oracle against torch autograd -----------------------------------------------------------------------------------------
def _torch_bigru(x, ws, mx, mh):
    H = ws[0][1].shape[0]
    outs = []
    for d in range(2):
        W, U, b = ws[d]
        T = x.shape[1]
        h = torch.zeros(x.shape[0], H, dtype=torch.float64)
        for t in (range(T - 1, -1, -1) if d else range(T)):
            m = [torch.tensor(mx[d][g][:, t]) for g in range(3)] if mx is not None else [1.0] * 3
            n = [torch.tensor(mh[d][g][:, t]) for g in range(3)] if mh is not None else [1.0] * 3
            a = [(x[:, t] * m[g]) @ W[:, g * H:(g + 1) * H] + b[g * H:(g + 1) * H] for g in range(3)]
            z = (0.2 * (a[0] + (h * n[0]) @ U[:, :H]) + 0.5).clamp(0, 1)
            r = (0.2 * (a[1] + (h * n[1]) @ U[:, H:2 * H]) + 0.5).clamp(0, 1)
            c = torch.tanh(a[2] + (r * (h * n[2])) @ U[:, 2 * H:])
            h = z * h + (1 - z) * c
        outs.append(h)
    return torch.cat(outs, dim=1)


def _cell_case(T, masked, seed=0, B=4, I=8, H=16):
    rng = np.random.RandomState(seed + T)
    x = rng.randn(B, T, I)
    ws = [(0.6 * rng.randn(I, 3 * H), 0.6 * rng.randn(H, 3 * H), 0.3 * rng.randn(3 * H)) for _ in range(2)]
    dout = rng.randn(B, 2 * H)
    mx, mh = draw_masks(11, 2, B, I, H, KEEP, 0, T) if masked else (None, None)
    return x, ws, dout, mx, mh


@pytest.mark.parametrize("masked", [False, True])
@pytest.mark.parametrize("T", [1, 2, 10])
def test_oracle_cell_gradients_match_torch_autograd(T, masked):
    x, ws, dout, mx, mh = _cell_case(T, masked)
    out, caches = bigru_fwd(x, ws, mx, mh)
    dx, grads = bigru_bwd(dout, x, ws, caches)
    tx = torch.tensor(x, requires_grad=True)
    tws = [tuple(torch.tensor(t, requires_grad=True) for t in w) for w in ws]
    tout = _torch_bigru(tx, tws, mx, mh)
    np.testing.assert_allclose(out, tout.detach().numpy(), atol=1e-12)
    tout.backward(torch.tensor(dout))
    pairs = [('dx', dx, tx.grad.numpy())]
    for d in range(2):
        for nm, g, t in zip(('dW', 'dU', 'db'), grads[d], tws[d]):
            pairs.append(('%s%d' % (nm, d), g, t.grad.numpy() if t.grad is not None else np.zeros_like(g)))
    for nm, g, ref in pairs:
        assert np.abs(g - ref).max() <= 1e-9 * max(np.abs(ref).max(), 1e-12), nm
    sat = sum(((c['z'] <= 0) | (c['z'] >= 1)).sum() for c in caches)
    assert T == 1 or sat > 0       # the inputs reach the flat parts of the hard sigmoid


@pytest.mark.parametrize("mutate", ['reset_after', 'gate_order', 'backward_not_reversed', 'mask_per_step'])
def test_every_mutation_moves_a_gradient(mutate):
    x, ws, dout, mx, mh = _cell_case(10, True, seed=3)
    B, T, I = x.shape
    H = ws[0][1].shape[0]
    good = bigru_bwd(dout, x, ws, bigru_fwd(x, ws, mx, mh)[1])
    if mutate == 'mask_per_step':
        mx2, mh2 = draw_masks(11, 2, B, I, H, KEEP, 0, T, per_step=True)
        bad = bigru_bwd(dout, x, ws, bigru_fwd(x, ws, mx2, mh2)[1])
    else:
        bad = bigru_bwd(dout, x, ws, bigru_fwd(x, ws, mx, mh, mutate)[1], mutate=mutate)
    flat = lambda r: [r[0]] + [t for g in r[1] for t in g]
    err = max(np.abs(a - b).max() / max(np.abs(a).max(), 1e-12) for a, b in zip(flat(good), flat(bad)))
    assert err > 1e-2, err


def _torch_dw(a, w, s, Lout):
    k, C = w.shape
    return torch.nn.functional.conv1d(a.permute(0, 2, 1), w.t().reshape(C, 1, k), stride=s, groups=C)[:, :, :Lout].permute(0, 2, 1)


def test_oracle_net_gradients_match_torch_autograd():
    ora = SimpleNet(num_classes=12)
    rng = np.random.RandomState(5)
    for k in ora.params:
        if k.endswith('gamma'):
            g = 1.0 + 0.1 * rng.randn(*ora.params[k].shape)
            ora.params[k] = (g * np.where(rng.rand(*g.shape) < 0.33, -1.0, 1.0)).astype(np.float32)
        if k.endswith('beta'):
            ora.params[k] = (0.5 + 0.3 * rng.randn(*ora.params[k].shape)).astype(np.float32)
        if k.endswith('bias'):
            ora.params[k] = (0.1 * rng.randn(*ora.params[k].shape)).astype(np.float32)
    B = 3
    x = (rng.randn(B, 16000) * 0.3).astype(np.float32)
    y = np.eye(12, dtype=np.float32)[rng.randint(0, 12, B)]
    loss, p, grads, _ = ora.loss_and_grads(x, y, seed=3, step=5)
    P = {k: torch.tensor(v.astype(np.float64), requires_grad=True) for k, v in ora.params.items()}
    a = torch.tensor(x.astype(np.float64))[:, :, None]
    for blk in ora.blocks:
        n = blk['idx']
        z = _torch_dw(a, P['depthwise_conv2d_%d/depthwise_kernel' % n][0, :, :, 0], blk['s'], blk['Lout'])
        yv = z @ P['conv1d_%d/kernel' % n][0]
        a = torch.nn.functional.batch_norm(yv.permute(0, 2, 1), None, None, P['batch_normalization_%d/gamma' % n],
                                           P['batch_normalization_%d/beta' % n], training=True, eps=1e-3).clamp(0, 6).permute(0, 2, 1)
    mx, mh = draw_masks(3, 5, B, ora.I, ora.H, KEEP, 0, ora.T)
    tws = [tuple(P[b + w] for w in ('kernel', 'recurrent_kernel', 'bias')) for b in ora.gru_names]
    out = _torch_bigru(a, tws, mx, mh)
    tp = torch.softmax(out @ P['dense_1/kernel'] + P['dense_1/bias'], dim=1)
    tl = -(torch.tensor(y.astype(np.float64)) * torch.log(tp.clamp(1e-7, 1 - 1e-7))).sum(1).mean()
    tl.backward()
    assert abs(loss - float(tl.detach())) < 1e-10
    np.testing.assert_allclose(p, tp.detach().numpy(), atol=1e-12)
    for k, g in grads.items():
        ref = P[k].grad.numpy()
        assert np.abs(g - ref).max() / max(np.abs(ref).max(), 1e-12) < 1e-9, k


def test_mask_counter_is_the_dropout_kernels():
    """Rows 8 .. 15 of a 16-row draw are what a shard with row_offset = 8 draws; ids 16 .. 27 are twelve different masks."""
    full_x, full_h = draw_masks(9, 4, 16, 224, 128, KEEP, 0, 1)
    part_x, part_h = draw_masks(9, 4, 8, 224, 128, KEEP, 8, 1)
    seen = set()
    for d in range(2):
        for g in range(3):
            assert np.array_equal(full_x[d][g][8:], part_x[d][g]) and np.array_equal(full_h[d][g][8:], part_h[d][g])
            assert set(np.unique(full_x[d][g])) == {0.0, 1.25}
            seen.add(full_x[d][g].tobytes())
            seen.add(full_h[d][g].tobytes())
    assert len(seen) == 12
    m = dropout_mask(dropout_key(9, 4, 16), 16 * 224, KEEP).reshape(16, 224)
    assert np.array_equal(full_x[0][0][:, 0], m / KEEP)


def test_kernel_test_inputs_stay_clear_of_the_corners():
    """The GPU tests compare gate values only where the float64 pre-activation is farther than 1e-5 from +-2.5 and allow 0.1 % of
    the elements to be left out: for their inputs the share is measured here and must be below 1e-4."""
    near = total = sat = 0
    for B, T, I, H in KERNEL_CASES:
        x, ws, _ = kernel_inputs(B, T, I, H)
        for masked in (False, True):
            mx, mh = draw_masks(1234567, 3, B, I, H, KEEP, 0, T) if masked else (None, None)
            _, caches = bigru_fwd(x.astype(np.float64), [tuple(t.astype(np.float64) for t in w) for w in ws], mx, mh)
            for c in caches:
                for pre in (c['pz'], c['pr']):
                    near += (np.abs(np.abs(pre) - 2.5) <= 1e-5).sum()
                    sat += (np.abs(pre) >= 2.5).sum()
                    total += pre.size
    print("pre-activations within 1e-5 of +-2.5: %d of %d (%.3g); saturated: %.3g" % (near, total, near / total, sat / total))
    assert near / total < 1e-4
    assert sat / total > 0.01      # and the flat parts are exercised


def test_gru_domain_refusals():
    """Host-side checks only: every call is refused before a launch (the pointers are never dereferenced)."""
    lib = _lib.load()
    p = ctypes.c_void_p(4096)

    def fwd(B, T, I, H):
        return lib.kws_gru_fwd_f32(p, p, p, p, p, p, p, None, None, p, None, p, B, T, I, H, None)

    def bwd(B, T, I, H):
        return lib.kws_gru_bwd_f32(p, p, p, p, p, p, None, None, p, p, p, p, p, p, p, p, p, B, T, I, H, None)

    def seq_fwd(B, T, H):
        return lib.kws_gru_seq_fwd_f32(p, 3 * B * T * H, H, 3 * H, p, p, p, p, None, p, None, B, T, H, None)

    def seq_bwd(B, T, H):
        return lib.kws_gru_seq_bwd_f32(p, p, None, p, p, p, B, T, H, None)

    bad = [(0, 10, 224, 128), (4, 0, 224, 128), (4, 1025, 224, 128), (4, 10, 224, 0), (4, 10, 224, 8), (4, 10, 224, 24), (4, 10, 224, 272),
           (4, 10, 224, 120), (4, 10, 0, 128), (4, 10, 6, 128), (4, 10, 223, 128)]
    for B, T, I, H in bad:
        assert fwd(B, T, I, H) == -1, (B, T, I, H)
        assert lib.kws_last_error()
        assert bwd(B, T, I, H) == -1, (B, T, I, H)
        assert lib.kws_gru_workspace_floats(B, T, I, H, 1) == 0
        if I == 224:
            assert seq_fwd(B, T, H) == -1 and seq_bwd(B, T, H) == -1, (B, T, H)
            assert lib.kws_gru_save_floats(B, T, H) == 0
    assert lib.kws_gru_fwd_f32(None, p, p, p, p, p, p, None, None, p, None, p, 4, 10, 224, 128, None) == -1
    assert lib.kws_gru_bwd_f32(p, p, p, p, p, p, None, None, None, p, p, p, p, p, p, p, p, 4, 10, 224, 128, None) == -1
    assert lib.kws_gru_seq_fwd_f32(p, 0, 128, 384, p, p, p, p, None, p, None, 4, 10, 128, None) == -1
    assert lib.kws_gru_masks(p, p, 4, 224, 128, ctypes.c_float(0.0), 1, 0, 0, None) == -1
    assert lib.kws_gru_masks(None, p, 4, 224, 128, ctypes.c_float(0.8), 1, 0, 0, None) == -1
    for B, T, I, H in ((1, 1, 8, 16), (37, 10, 224, 128), (5, 1024, 384, 256)):
        assert lib.kws_gru_save_floats(B, T, H) == 8 * B * T * H
        assert lib.kws_gru_workspace_floats(B, T, I, H, 1) > lib.kws_gru_workspace_floats(B, T, I, H, 0) > 6 * B * T * H
