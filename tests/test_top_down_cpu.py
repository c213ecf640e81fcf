"""CPU checks of conv_1d_top_down (KWS_NET_CONV_1D_TOP_DOWN, csrc/net_grouped.hip) and of the kernel family it brought
(csrc/gdwconv.hip): the header / binding declarations, the speech_model dispatch, the structure recorded from the reference
(tests/golden/top_down_model.json, made by tests/golden/make_golden_top_down.py), the native tensor table against that fixture and
against the float64 oracle (tests/top_down_oracle.py), the input sizes kws_net_create takes, the host-side planner and domain of the
new kernels, and the oracle against torch autograd."""
import ctypes
import json
import os
import re

import numpy as np
import pytest
import torch
import torch.nn.functional as Fn

import gdwconv_cases as GD
from net_parity import native_table, perturb
from oracle.layers import dropout_key, dropout_mask
from speech_recognition_amd import _lib
from top_down_oracle import BLOCKS, FRONT_K, FRONT_N, FRONT_STRIDE, KEEP, MUTATIONS, TopDownNet, front_rows

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden', 'top_down_model.json')
KIND = 19
ROWS = [48, 46, 22, 20, 9, 7, 3, 1]        # at 16000 samples (98 front rows)
ROWS_17600 = [53, 51, 25, 23, 11, 9, 4, 2]  # at 108 front rows
# per block: (first channel read, channels read, filters) of every group - what the DATA FLOW does, not what the slices say
GROUPS = [[(0, 160, 140), (160, 160, 140), (320, 160, 140)], [(0, 420, 210)] * 2,
          [(0, 100, 120), (100, 100, 120), (200, 100, 120)], [(0, 360, 180)] * 2,
          [(0, 120, 100), (120, 120, 100), (240, 120, 100)], [(0, 300, 150)] * 2,
          [(0, 100, 80), (100, 100, 80), (200, 100, 80)], [(0, 240, 120)] * 2]
# by hand: the front kernel and bias; per group a depthwise kernel 3 * cin, a pointwise kernel cin * cout, gamma / beta; Dense
N_TRAINABLE = 479 * 480 + 480 + sum(3 * cin + cin * cout + 2 * cout for blk in GROUPS for _, cin, cout in blk) + 240 * 12 + 12
N_STATE = sum(2 * cout for blk in GROUPS for _, _, cout in blk)


def _golden(L=16000):
    with open(GOLDEN) as f:
        return json.load(f)['conv_1d_top_down_%d' % L]


def _create(input_size, nc=12):
    lib = _lib.load()
    cfg = _lib.NetConfig(KIND, nc, 1, input_size, 0, 0)
    h = ctypes.c_void_p()
    return lib, lib.kws_net_create(ctypes.byref(cfg), ctypes.byref(h)), h


def _gdesc(c):
    d = _lib.GdwconvDesc()
    for k, v in GD.desc_fields(c):
        setattr(d, k, v)
    return d


# ---- the public surface ---------------------------------------------------------------------------------------------------
NEW_ENTRY_POINTS = ["kws_gdwconv_fwd_f32", "kws_gdwconv_bwd_part_rows", "kws_gdwconv_bwd_workspace_floats", "kws_gdwconv_bwd_f32"]


def test_header_defines_the_kind_and_declares_the_new_entry_points(repo_root):
    src = open(os.path.join(repo_root, "include", "kws_hip.h")).read()
    assert re.search(r"#define\s+KWS_NET_CONV_1D_TOP_DOWN\s+19\b", src)
    assert re.search(r"#define\s+KWS_ABI_VERSION\s+5\b", src)              # additive: the version stays
    assert _lib.KWS_NET_CONV_1D_TOP_DOWN == KIND and _lib.ABI_VERSION == 5
    for name, val in (("NONE", 0), ("BN_RELU6", 1), ("BIAS", 2)):
        assert re.search(r"#define\s+KWS_GDW_ACT_%s\s+%d\b" % (name, val), src) and getattr(_lib, "GDW_ACT_" + name) == val
    assert (GD.ACT_NONE, GD.ACT_BN, GD.ACT_BIAS) == (0, 1, 2)
    code = re.sub(r"/\*.*?\*/", "", src, flags=re.S)
    lib = _lib.load()
    for name in NEW_ENTRY_POINTS:
        assert re.search(r"\b%s\s*\(" % name, code), name
        assert name in _lib.SIGNATURES and hasattr(lib, name), name
    members = re.search(r"typedef struct \{([^}]*)\} kws_gdwconv_t;", code).group(1)
    names = re.findall(r"\b([A-Za-z_]\w*)\s*[,;]", members)
    assert names == [f[0] for f in _lib.GdwconvDesc._fields_] == GD.DESC_MEMBERS
    assert ctypes.sizeof(_lib.GdwconvDesc) == 12 * 4 + 8


def test_speech_model_dispatch_and_settings(monkeypatch):
    """Name, loss, optimizer class and lr (the device net itself replaced: no GPU here)."""
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
    assert 'conv_1d_top_down' in M.ACCELERATED and 'conv_1d_top_down' in M.REFERENCE_MODEL_TYPES
    assert len(M.ACCELERATED) == 20 and len(set(M.ACCELERATED)) == 20
    M.speech_model('conv_1d_top_down', 16000, num_classes=12)
    net = captured['net']
    assert net.kind == KIND and net.num_classes == 12 and net.kw == {'input_size': 16000}
    assert captured['name'] == 'conv_1d_top_down' and captured['loss'] == 'cce'
    assert isinstance(captured['optimizer'], keras_api.RMSprop) and abs(float(captured['optimizer'].lr) - 3e-3) < 1e-9
    M.conv_1d_top_down_model(17600, 30)
    assert captured['net'].kw == {'input_size': 17600} and captured['net'].num_classes == 30


# ---- the recorded structure, the native table, the oracle ------------------------------------------------------------------
def test_fixture_has_the_expected_layers():
    gold = _golden()
    assert (gold['model_name'], gold['optimizer'], gold['lr'], gold['loss']) == \
        ('conv_1d_top_down', 'RMSprop', 3e-3, 'categorical_crossentropy')
    layers = gold['layers']
    convs = [l for l in layers if l['class'] == 'Conv1D']
    front = convs[0]
    assert (front['kernel'], front['strides'], front['padding'], front['use_bias'], front['activation'], front['output']) == \
        ([FRONT_K, 1, FRONT_N], FRONT_STRIDE, 'valid', True, None, [98, FRONT_N])
    assert [w['name'] for w in gold['weights'][:2]] == ['conv1d_1/kernel', 'conv1d_1/bias'] and gold['weights'][1]['shape'] == [480]
    assert gold['weights'][0]['l2'] == 0.0                     # no regularizer on the front convolution
    # nothing between the front convolution and the first slices: no BatchNormalization, no Activation
    at = layers.index(front)
    assert layers[at + 1]['class'] == 'Lambda' and layers[at + 1]['reads'] == [front['makes']]
    slices = [l for l in layers if l['class'] == 'Lambda' and 'slice' in l]
    dws = [l for l in layers if l['class'] == 'DepthwiseConv2D']
    want = [g for blk in GROUPS for g in blk]
    assert len(slices) == len(dws) == len(convs) - 1 == len(want) == 20
    made_by = {l['makes']: l for l in layers}
    at = 0
    for i, (blk, (F, g, nch, s, shared)) in enumerate(zip(GROUPS, BLOCKS)):
        for q, (c0, cin, cout) in enumerate(blk):
            sl, dw, pw = slices[at], dws[at], convs[1 + at]
            gs = nch // g
            assert sl['slice'] == sl['requested'] == [q * gs, (q + 1) * gs] and sl['channels'] == gs       # what the slice cuts
            # ... and what the depthwise layer really reads: the expand_dims Lambda in front of it reads the slice in a reduce
            # block and the block's INPUT (what the slice read, too) in a context block, where the slice is dead
            src = made_by[dw['reads'][0]]
            assert src['class'] == 'Lambda' and 'slice' not in src
            assert sl['dead'] == shared
            assert src['reads'] == (sl['reads'] if shared else [sl['makes']])
            assert dw['kernel'] == [1, 3, cin, 1] and dw['strides'] == s and dw['padding'] == 'valid' and not dw['use_bias']
            assert cin == (sl['in_channels'] if shared else gs)
            assert dw['output'] == [ROWS[i], cin]
            assert (pw['kernel'], pw['strides'], pw['use_bias'], pw['output']) == ([1, cin, cout], 1, False, [ROWS[i], cout])
            at += 1
    # the third block cuts 3 x 100 of 420 channels: 120 are never read
    assert [l['slice'] for l in slices[5:8]] == [[0, 100], [100, 200], [200, 300]] and slices[5]['in_channels'] == 420
    assert [l['slice'] for l in slices if l['dead']] == [[0, 210], [210, 420], [0, 180], [180, 360], [0, 150], [150, 300], [0, 120],
                                                         [120, 240]]
    assert len([l for l in layers if l['class'] == 'BatchNormalization']) == 20
    assert len([l for l in layers if l['class'] == 'Concatenate']) == 8
    assert [l['rate'] for l in layers if l['class'] == 'Dropout'] == [pytest.approx(1 - KEEP)]
    dense = [l for l in layers if l['class'] == 'Dense']
    assert [(d['kernel'], d['use_bias'], d['activation']) for d in dense] == [([240, 12], True, 'softmax')]
    l2 = {w['name']: w['l2'] for w in gold['weights']}
    assert all(l2[n] == 1e-5 for n in l2 if 'depthwise' in n or (n.startswith('conv1d_') and n != 'conv1d_1/kernel' and n.endswith('kernel')))
    # 17600 samples: 108 front rows, two rows at the end, Dense over 480
    g2 = _golden(17600)
    assert [l['output'][0] for l in g2['layers'] if l['class'] == 'DepthwiseConv2D'] == [r for r, blk in zip(ROWS_17600, GROUPS) for _ in blk]
    assert [d['kernel'] for d in g2['layers'] if d['class'] == 'Dense'] == [[480, 12]]
    assert [(w['name'], w['shape']) for w in g2['weights'][:-2]] == [(w['name'], w['shape']) for w in gold['weights'][:-2]]


@pytest.mark.parametrize("L", [16000, 17600])
def test_native_tensor_table_matches_reference_and_oracle(L):
    gold = _golden(L)
    table = native_table(KIND, gold['num_classes'], gold['input_size'])
    assert [t.name.decode() for t in table] == [w['name'] for w in gold['weights']]
    for t, w in zip(table, gold['weights']):
        assert [int(t.shape[k]) for k in range(t.ndim)] == w['shape'], w['name']
        assert bool(t.is_state) == bool(w.get('state', False)), w['name']
        assert t.l2 == np.float32(w['l2']), w['name']
        if w['name'].endswith('/depthwise_kernel'):
            assert (t.fan_in, t.fan_out) == (3 * w['shape'][2], 3), w['name']
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
    extra = (480 - 240) * 12 if L == 17600 else 0
    assert sum(t.size for t in table if not t.is_state) == n_train == N_TRAINABLE + extra
    assert sum(t.size for t in table) == N_TRAINABLE + N_STATE + extra
    if L == 16000:
        assert N_TRAINABLE + N_STATE == 872892
    ora = TopDownNet(num_classes=gold['num_classes'], input_size=L)
    assert [t.name.decode() for t in table if not t.is_state] == list(ora.params)
    assert [t.name.decode() for t in table if t.is_state] == list(ora.state)
    for t in table:
        v = ora.state[t.name.decode()] if t.is_state else ora.params[t.name.decode()]
        assert tuple(int(t.shape[k]) for k in range(t.ndim)) == v.shape
    assert sum(t.size for t in table) == ora.count_params()
    # l2 1e-5 on exactly the depthwise and pointwise kernels of the blocks
    assert [t.name.decode() for t in table if t.l2 > 0] == ora.l2_names and len(ora.l2_names) == 40
    assert all(t.l2 == np.float32(1e-5) for t in table if t.l2 > 0)
    # the oracle's windows are the fixture's data flow
    assert [[(c0, w) for c0, w, _ in ora.windows(i)] for i in range(8)] == [[(c0, cin) for c0, cin, _ in blk] for blk in GROUPS]


def test_net_create_input_sizes_and_views():
    """any even size from 14879 samples on (91 front rows, the fewest that leave the last block a row): 14880 is the first"""
    for L, rows, last in ((16000, 98, 1), (14880, 91, 1), (15000, 91, 1), (17600, 108, 2)):
        lib, rc, h = _create(L)
        assert rc == 0, L
        ora = TopDownNet(input_size=L)
        assert ora.rows == front_rows(L) == rows and ora.blocks[-1]['Lout'] == last and ora.D == 240 * last
        off, cnt = ctypes.c_int64(), ctypes.c_int64()
        assert lib.kws_net_debug_view(h, 8, 1, 0, 0, ctypes.byref(off), ctypes.byref(cnt)) == 0 and cnt.value == 8 * rows * 480
        lib.kws_net_destroy(h)
    for L in (14878, 14720, 12000):                            # 90 rows or fewer: the last block would keep no row
        assert front_rows(L) <= 90
        lib, rc, h = _create(L)
        assert rc != 0 and str(L).encode() in lib.kws_last_error()
    for L in (14879, 15001, 0, -16000):                        # odd sizes: the front path loads pairs of samples
        lib, rc, h = _create(L)
        assert rc != 0, L
    lib, rc, h = _create(16000)
    assert rc == 0
    assert lib.kws_net_workspace_bytes(h, 8, 1) > lib.kws_net_workspace_bytes(h, 8, 0) > 0
    off, cnt = ctypes.c_int64(), ctypes.c_int64()
    for i in range(8):
        F, g = BLOCKS[i][0], BLOCKS[i][1]
        assert lib.kws_net_debug_view(h, 8, 1, 0, i + 1, ctypes.byref(off), ctypes.byref(cnt)) == 0 and cnt.value == 8 * ROWS[i] * F
        assert lib.kws_net_debug_view(h, 8, 1, 1, i + 1, ctypes.byref(off), ctypes.byref(cnt)) == 0
        assert cnt.value == 8 * ROWS[i] * sum(cin for _, cin, _ in GROUPS[i])
    offs = []
    for j, Ng in ((0, 140), (2, 140), (3, 210), (4, 210), (5, 120), (19, 120)):
        assert lib.kws_net_debug_view(h, 8, 1, 2, j, ctypes.byref(off), ctypes.byref(cnt)) == 0 and cnt.value == 4 * Ng, j
        offs.append(off.value)
    assert offs[3] - offs[2] == 4 * 210
    assert lib.kws_net_debug_view(h, 8, 1, 0, 9, ctypes.byref(off), ctypes.byref(cnt)) != 0
    assert lib.kws_net_debug_view(h, 8, 1, 1, 0, ctypes.byref(off), ctypes.byref(cnt)) != 0
    assert lib.kws_net_debug_view(h, 8, 1, 2, 20, ctypes.byref(off), ctypes.byref(cnt)) != 0
    assert lib.kws_net_debug_view(h, 8, 1, 3, 0, ctypes.byref(off), ctypes.byref(cnt)) != 0
    lib.kws_net_destroy(h)


# ---- the planner and the domain of the new kernels, on the host ----------------------------------------------------------------
def test_gdwconv_planner_and_domain():
    lib = _lib.load()
    for name, c in GD.CASES.items():
        assert GD.in_domain(c), name
        d = _gdesc(c)
        assert lib.kws_gdwconv_bwd_workspace_floats(ctypes.byref(d)) == GD.workspace_floats(c) > 0, name
        assert lib.kws_gdwconv_bwd_part_rows(ctypes.byref(d)) == GD.part_rows(c) >= 1, name
    assert GD.part_rows(GD.CASES["many_rows"]) >= 2
    whys = " | ".join(why for _, why in GD.REFUSED)
    for needed in ("no taps", "eight taps", "stride 0", "stride 5", "no groups", "nine groups", "gs not a multiple of 4",
                   "C not a multiple of 4", "x0 not a multiple of 4", "x_step not a multiple of 4", "past C", "past L", "unknown act",
                   "bn_group does not divide C", "w_group_stride below"):
        assert needed in whys, needed
    p = ctypes.c_void_p(4096)
    for changes, why in GD.REFUSED:
        bad = GD.refused(changes)
        assert not GD.in_domain(bad), why
        d = _gdesc(bad)
        assert lib.kws_gdwconv_bwd_workspace_floats(ctypes.byref(d)) == 0, why
        assert lib.kws_gdwconv_bwd_part_rows(ctypes.byref(d)) == 0, why
        # refused before any launch: the pointers are never dereferenced
        assert lib.kws_gdwconv_fwd_f32(p, p, p, p, ctypes.byref(d), None) == -1, why
        assert lib.kws_gdwconv_bwd_f32(p, p, p, p, p, p, None, p, ctypes.byref(d), None) == -1, why
    good = _gdesc(GD.CASES["sliced_unread"])
    assert lib.kws_gdwconv_bwd_workspace_floats(None) == 0 and lib.kws_gdwconv_bwd_part_rows(None) == 0
    assert lib.kws_gdwconv_fwd_f32(p, p, p, p, None, None) == -1 and lib.kws_gdwconv_bwd_f32(p, p, p, p, p, p, None, p, None, None) == -1
    # pointers: NULL, a table missing where the mode needs one, a misaligned tensor, a bias gradient outside the bias mode
    odd = ctypes.c_void_p(4100)
    assert lib.kws_gdwconv_fwd_f32(None, None, p, p, ctypes.byref(good), None) == -1
    assert lib.kws_gdwconv_fwd_f32(odd, None, p, p, ctypes.byref(good), None) == -1
    assert lib.kws_gdwconv_fwd_f32(p, None, p, odd, ctypes.byref(good), None) == -1
    assert lib.kws_gdwconv_fwd_f32(p, None, p, p, ctypes.byref(_gdesc(GD.CASES["bias"])), None) == -1
    assert lib.kws_gdwconv_bwd_f32(p, None, p, p, p, p, p, p, ctypes.byref(good), None) == -1
    assert lib.kws_gdwconv_bwd_f32(p, None, p, p, odd, p, None, p, ctypes.byref(good), None) == -1
    assert b'gdwconv' in lib.kws_last_error()
    # the model's own blocks at batch 1024: the first reduce block and the first context block
    c1 = GD._case(1024, 98, 480, 3, 160, 3, 2, act=GD.ACT_BIAS)
    c2 = GD._case(1024, 48, 420, 2, 420, 3, 1, x_step=0, act=GD.ACT_BN, bn_group=140)
    assert (GD.part_rows(c1), GD.part_rows(c2)) == (512, 256)
    assert lib.kws_gdwconv_bwd_workspace_floats(ctypes.byref(_gdesc(c1))) == 512 * 4 * 480
    assert lib.kws_gdwconv_bwd_workspace_floats(ctypes.byref(_gdesc(c2))) == 256 * 4 * 840


# ---- the oracle against torch autograd --------------------------------------------------------------------------------------
def _perturbed(input_size=16000, seed=5):
    ora = TopDownNet(num_classes=12, input_size=input_size)
    perturb(ora, seed, negative_fraction=0.33, beta=(0.5, 0.3), bias=0.1, state=False)
    assert np.abs(ora.params['conv1d_1/bias']).max() > 0
    return ora


def _torch_loss(ora, x, y, seed, step):
    """The same network in torch float64: F.conv1d at stride 160 with the bias for the front layer; per group a depthwise F.conv1d
    (groups = channels) over the channels the group READS, a 1-tap F.conv1d, F.batch_norm in training mode (eps 1e-3), clamp; the
    oracle's dropout mask, softmax + keras categorical CE.  -> loss, probabilities, gradients, the gradient wrt block 2's
    (index 1) concatenated output and the gradient wrt the front convolution's output."""
    P = {k: torch.tensor(v.astype(np.float64), requires_grad=True) for k, v in ora.params.items()}
    B = x.shape[0]
    a = Fn.conv1d(torch.tensor(x.astype(np.float64))[:, None, :], P['conv1d_1/kernel'].permute(2, 1, 0), P['conv1d_1/bias'],
                  stride=FRONT_STRIDE)
    a.retain_grad()
    a0 = a
    dw, conv, bn, kept = 1, 2, 1, None
    for i, (blk, (F, g, nch, s, shared)) in enumerate(zip(GROUPS, BLOCKS)):
        outs = []
        for c0, cin, cout in blk:
            w = P['depthwise_conv2d_%d/depthwise_kernel' % dw][0, :, :, 0].permute(1, 0)[:, None, :]
            z = Fn.conv1d(a[:, c0:c0 + cin], w, stride=s, groups=cin)
            yq = Fn.conv1d(z, P['conv1d_%d/kernel' % conv].permute(2, 1, 0))
            outs.append(Fn.batch_norm(yq, None, None, P['batch_normalization_%d/gamma' % bn], P['batch_normalization_%d/beta' % bn],
                                      training=True, eps=1e-3).clamp(0, 6))
            dw, conv, bn = dw + 1, conv + 1, bn + 1
        a = torch.cat(outs, dim=1)
        if i == 1:
            kept = a
            kept.retain_grad()
    flat = a.permute(0, 2, 1).reshape(B, -1)
    keep = dropout_mask(dropout_key(seed, step, 1), flat.numel(), KEEP).reshape(flat.shape)
    p = torch.softmax((flat * torch.tensor(keep.astype(np.float64)) / KEEP) @ P['dense_1/kernel'] + P['dense_1/bias'], dim=1)
    loss = -(torch.tensor(y.astype(np.float64)) * torch.log(p.clamp(1e-7, 1 - 1e-7))).sum(1).mean()
    loss.backward()
    return (float(loss.detach()), p.detach().numpy(), {k: v.grad.numpy() for k, v in P.items()}, kept.grad.permute(0, 2, 1).numpy(),
            a0.grad.permute(0, 2, 1).numpy())


@pytest.mark.parametrize("input_size", [16000, 17600])
def test_oracle_gradients_match_torch_autograd(input_size):
    ora = _perturbed(input_size)
    rng = np.random.RandomState(7)
    B = 3
    x = (rng.randn(B, input_size) * 0.3).astype(np.float32)
    y = np.eye(12, dtype=np.float32)[rng.randint(0, 12, B)]
    loss, p, grads, cache = ora.loss_and_grads(x, y, seed=3, step=5)
    tl, tp, tg, t_da2, t_da0 = _torch_loss(ora, x, y, seed=3, step=5)
    assert abs(loss - tl) < 1e-10
    np.testing.assert_allclose(p, tp, atol=1e-12)
    assert list(grads) == list(ora.params)
    for k, g in grads.items():
        if k != 'conv1d_1/bias':
            scale = max(np.abs(tg[k]).max(), 1e-12)
            assert np.abs(g - tg[k]).max() / scale < 1e-9, k
    # The front bias reaches the loss only through depthwise -> pointwise -> BatchNormalization on batch statistics, and a
    # constant per channel does not survive the mean subtraction: its gradient, the column sum of the gradient wrt the front
    # output, is ZERO in exact arithmetic.  Oracle and torch agree on the terms and both sums cancel to rounding.
    da0 = cache['da0']
    assert np.abs(da0 - t_da0).max() / np.abs(t_da0).max() < 1e-9
    terms = np.abs(da0).sum(axis=(0, 1)).max()
    assert terms > 1e-3
    assert np.abs(grads['conv1d_1/bias']).max() < 1e-12 * terms and np.abs(tg['conv1d_1/bias']).max() < 1e-12 * terms
    assert np.array_equal(grads['conv1d_1/bias'], da0.sum(axis=(0, 1)))
    # block 3 reads channels 0 .. 299 of block 2's 420: the rest gets an exactly zero gradient, in the oracle and in torch
    da2 = cache['da2']
    assert da2.shape[2] == 420 and np.abs(da2[:, :, :300]).max() > 0
    assert not da2[:, :, 300:].any() and not t_da2[:, :, 300:].any()
    assert np.abs(da2 - t_da2).max() / np.abs(t_da2).max() < 1e-9


@pytest.mark.parametrize("mutate", MUTATIONS)
def test_mutated_oracle_breaks_the_gradient_bar(mutate):
    ora = _perturbed()
    rng = np.random.RandomState(8)
    x = (rng.randn(3, 16000) * 0.3).astype(np.float32)
    y = np.eye(12, dtype=np.float32)[rng.randint(0, 12, 3)]
    _, _, good, _ = ora.loss_and_grads(x, y, seed=1, step=0)
    _, _, bad, _ = ora.loss_and_grads(x, y, seed=1, step=0, mutate=mutate)
    err = max(np.abs(bad[k] - good[k]).max() / max(np.abs(good[k]).max(), 1e-12) for k in good)
    assert err > 1e-2, err
