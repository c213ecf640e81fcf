"""CPU checks of conv_1d_time_sliced (KWS_NET_CONV_1D_TIME_SLICED, csrc/net_time_sliced.hip) and of the two kernel families it
brought (csrc/frame_conv.hip, csrc/gap.hip): the float64 oracle (tests/time_sliced_oracle.py) against torch autograd, the native
tensor table against the structure recorded from the reference (tests/golden/time_sliced_models.json, made by
tests/golden/make_golden_time_sliced.py) and against the oracle for filter_mult 1 and 2, the speech_model dispatch, the header /
binding declarations, the input sizes kws_net_create takes, and the host-side planners of the new kernels."""
import ctypes
import json
import os
import re

import numpy as np
import pytest
import torch
import torch.nn.functional as Fn

import frame_conv_cases as FC
from net_parity import native_table, perturb
from oracle.layers import dropout_key, dropout_mask
from speech_recognition_amd import _lib
from time_sliced_oracle import FRAME, HOP, KEEP1, KEEP2, LENGTHS, SPEC, STRIDE, TAPS, TimeSlicedNet, block_pad

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden', 'time_sliced_models.json')
N_TRAINABLE = {1: 1271008, 2: 5036480}   # by hand from the layer list: 3 * 40 * 32 fm + sum(3 cin + cin cout) + BN pairs + the two Dense


def _golden(fm):
    with open(GOLDEN) as f:
        return json.load(f)['conv_1d_time_sliced_fm%d' % fm]


def _create(fm, input_size, nc=12):
    lib = _lib.load()
    cfg = _lib.NetConfig(_lib.KWS_NET_CONV_1D_TIME_SLICED, nc, fm, input_size, 0, 0)
    h = ctypes.c_void_p()
    return lib, lib.kws_net_create(ctypes.byref(cfg), ctypes.byref(h)), h


# ---- the public surface ---------------------------------------------------------------------------------------------------
NEW_ENTRY_POINTS = ["kws_frame_conv_stats_rows", "kws_frame_conv_fwd_f32", "kws_frame_conv_wgrad_workspace_floats",
                    "kws_frame_conv_wgrad_f32", "kws_gap_drop_fwd_f32", "kws_gap_drop_bwd_part_rows", "kws_gap_drop_bwd_f32"]


def test_header_defines_the_kind_and_declares_the_new_entry_points(repo_root):
    src = open(os.path.join(repo_root, "include", "kws_hip.h")).read()
    assert re.search(r"#define\s+KWS_NET_CONV_1D_TIME_SLICED\s+17\b", src)
    assert re.search(r"#define\s+KWS_ABI_VERSION\s+5\b", src)              # additive: the version stays
    assert _lib.KWS_NET_CONV_1D_TIME_SLICED == 17
    code = re.sub(r"/\*.*?\*/", "", src, flags=re.S)
    lib = _lib.load()
    for name in NEW_ENTRY_POINTS:
        assert re.search(r"\b%s\s*\(" % name, code), name
        assert name in _lib.SIGNATURES and hasattr(lib, name), name
    assert "kws_frame_conv_t" in code
    # the descriptor's binding has the header's members, in order
    members = re.search(r"typedef struct \{([^}]*)\} kws_frame_conv_t;", code).group(1)
    names = re.findall(r"\b([A-Za-z_]\w*)\s*[,;]", members)
    assert names == [f[0] for f in _lib.FrameConvDesc._fields_]
    assert ctypes.sizeof(_lib.FrameConvDesc) == 48


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
    assert 'conv_1d_time_sliced' in M.ACCELERATED and 'conv_1d_time_sliced' in M.REFERENCE_MODEL_TYPES
    M.speech_model('conv_1d_time_sliced', 16000, num_classes=12)
    net = captured['net']
    assert net.kind == 17 and net.num_classes == 12 and net.kw['input_size'] == 16000 and net.kw['filter_mult'] == 1
    assert captured['name'] == 'conv_1d_time_sliced' and captured['loss'] == 'cce'
    assert isinstance(captured['optimizer'], keras_api.RMSprop) and abs(float(captured['optimizer'].lr) - 1e-3) < 1e-9
    M.conv_1d_time_sliced_model(12000, 30, filter_mult=2)
    assert captured['net'].kw == {'filter_mult': 2, 'input_size': 12000} and captured['net'].num_classes == 30
    # the models that are still missing keep saying so
    for missing in ('conv_2d', 'conv_1d_time_sliced_group'):
        with pytest.raises(NotImplementedError):
            M.speech_model(missing, 16000, num_classes=12)


# ---- the recorded structure, the native table, the oracle ------------------------------------------------------------------
@pytest.mark.parametrize("fm", [1, 2])
def test_fixture_has_the_expected_layers(fm):
    gold = _golden(fm)
    assert (gold['model_name'], gold['optimizer'], gold['lr'], gold['loss']) == \
        ('conv_1d_time_sliced', 'RMSprop', 1e-3, 'categorical_crossentropy')
    patches = [l['patches'] for l in gold['layers'] if 'patches' in l]
    assert patches == [{'class': 'extract_image_patches', 'ksize': FRAME, 'stride': HOP, 'padding': 'SAME', 'input_length': 16000,
                        'pad_left': 10, 'output': [800, FRAME]}]
    convs = [l for l in gold['layers'] if l['class'] == 'Conv1D']
    assert (convs[0]['kernel'], convs[0]['strides'], convs[0]['padding'], convs[0]['output']) == \
        ([TAPS, FRAME, 32 * fm], STRIDE, 'valid', [399, 32 * fm])
    dws = [l for l in gold['layers'] if l['class'] == 'DepthwiseConv2D']
    assert [(l['strides'], l['padding']) for l in dws] == [(s, 'same' if s == 2 else 'valid') for s, _ in SPEC]
    assert [l['kernel'] for l in dws] == [[1, 3, c * fm, 1] for c in [32] + [F for _, F in SPEC[:-1]]]
    assert [c['kernel'][2] for c in convs[1:]] == [F * fm for _, F in SPEC]
    assert [399] + [l['output'][0] for l in dws] == LENGTHS[16000]
    # the oracle's geometry is the recording's: both SAME parities occur (pad 1 | 1 on odd lengths, 0 | 1 on even ones)
    for l in dws:
        assert block_pad(l['input_length'], l['strides'])[0] == l['pad_left']
    assert {l['input_length'] % 2 for l in dws if l['strides'] == 2} == {0, 1}
    assert [l['rate'] for l in gold['layers'] if l['class'] == 'Dropout'] == [pytest.approx(1 - KEEP1), pytest.approx(1 - KEEP2)]
    dense = [l for l in gold['layers'] if l['class'] == 'Dense']
    assert [(d['kernel'], d['use_bias'], d['activation']) for d in dense] == \
        [([512 * fm, 256 * fm], False, None), ([256 * fm, 12], False, 'softmax')]
    pool = [l for l in gold['layers'] if l['class'] == 'GlobalAveragePooling1D']
    assert len(pool) == 1 and pool[0]['input'] == [3, 512 * fm]


@pytest.mark.parametrize("fm", [1, 2])
def test_native_tensor_table_matches_reference_and_oracle(fm):
    gold = _golden(fm)
    table = native_table(_lib.KWS_NET_CONV_1D_TIME_SLICED, gold['num_classes'], gold['input_size'], fm)
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
    assert sum(t.size for t in table if not t.is_state) == n_train == N_TRAINABLE[fm]
    ora = TimeSlicedNet(num_classes=gold['num_classes'], filter_mult=fm)
    assert [t.name.decode() for t in table if not t.is_state] == list(ora.params)
    assert [t.name.decode() for t in table if t.is_state] == list(ora.state)
    for t in table:
        v = ora.state[t.name.decode()] if t.is_state else ora.params[t.name.decode()]
        assert tuple(int(t.shape[k]) for k in range(t.ndim)) == v.shape
    assert sum(t.size for t in table) == ora.count_params()
    # l2 1e-5 on the first convolution, every depthwise and pointwise kernel and the last Dense kernel; none on dense_1
    assert {t.name.decode() for t in table if t.l2 > 0} == set(ora.l2_names) and len(ora.l2_names) == 1 + 13 + 13 + 1
    assert all(t.l2 == np.float32(1e-5) for t in table if t.l2 > 0)
    assert ora.lengths() == LENGTHS[16000] and (ora.T, ora.C, ora.H) == (3, 512 * fm, 256 * fm)


def test_net_create_takes_12000_and_refuses_8000():
    lib, rc, h = _create(1, 12000)
    assert rc == 0
    lib.kws_net_destroy(h)
    ora = TimeSlicedNet(input_size=12000)
    assert ora.lengths() == LENGTHS[12000] and ora.T == 1
    lib, rc, h = _create(1, 8000)                       # the last block would keep no row
    assert rc != 0 and b'8000' in lib.kws_last_error()
    with pytest.raises(AssertionError):
        TimeSlicedNet(input_size=8000)
    for fm, size in ((3, 16000), (0, 16000), (1, 16002), (1, 20)):
        lib, rc, h = _create(fm, size)
        assert rc != 0, (fm, size)
    # the split step stays the attention net's
    lib, rc, h = _create(2, 16000)
    assert rc == 0 and lib.kws_net_num_blocks(h) == 0 and lib.kws_net_grad_ready_offset(h, 3) == -1
    # gemm mode 2 is accepted and ignored, as for the other kinds
    assert lib.kws_net_set_gemm_mode(h, 2) == 0 and lib.kws_net_get_gemm_mode(h) == 2
    assert lib.kws_net_workspace_bytes(h, 8, 1) > lib.kws_net_workspace_bytes(h, 8, 0) > 0
    off, cnt = ctypes.c_int64(), ctypes.c_int64()
    assert lib.kws_net_debug_view(h, 8, 1, 4, 0, ctypes.byref(off), ctypes.byref(cnt)) == 0 and cnt.value == 8 * 512
    assert lib.kws_net_debug_view(h, 8, 1, 0, 13, ctypes.byref(off), ctypes.byref(cnt)) == 0 and cnt.value == 8 * 3 * 1024
    assert lib.kws_net_debug_view(h, 8, 1, 1, 12, ctypes.byref(off), ctypes.byref(cnt)) == 0 and cnt.value == 8 * 3 * 1024
    assert lib.kws_net_debug_view(h, 8, 1, 1, 11, ctypes.byref(off), ctypes.byref(cnt)) == 0 and cnt.value == 8 * 5 * 768
    assert lib.kws_net_debug_view(h, 8, 1, 2, 0, ctypes.byref(off), ctypes.byref(cnt)) == 0 and cnt.value == 4 * 64
    assert lib.kws_net_debug_view(h, 8, 1, 0, 14, ctypes.byref(off), ctypes.byref(cnt)) != 0
    assert lib.kws_net_debug_view(h, 8, 1, 3, 0, ctypes.byref(off), ctypes.byref(cnt)) != 0
    lib.kws_net_destroy(h)


# ---- the planners of the new kernels, on the host ---------------------------------------------------------------------------
def test_frame_conv_case_table_and_planners():
    lib = _lib.load()
    reached = set()
    for name, c in list(FC.CASES.items()) + list(FC.FLOAT_CASES.items()):
        assert FC.in_domain(c), name
        assert c['corners'] <= FC.edges(c), (name, c['corners'] - FC.edges(c))
        reached |= c['corners']
        d = _lib.FrameConvDesc(**FC.desc_fields(c))
        assert lib.kws_frame_conv_stats_rows(ctypes.byref(d)) == FC.stats_rows(c) > 0, name
        assert lib.kws_frame_conv_wgrad_workspace_floats(ctypes.byref(d)) == FC.workspace_floats(c) > 0, name
    assert reached == FC.CORNERS
    for changes, why in FC.REFUSED:
        bad = FC.refused(changes)
        assert not FC.in_domain(bad), why
        d = _lib.FrameConvDesc(**FC.desc_fields(bad))
        assert lib.kws_frame_conv_stats_rows(ctypes.byref(d)) == 0, why
        assert lib.kws_frame_conv_wgrad_workspace_floats(ctypes.byref(d)) == 0, why
        # refused before any launch: the pointers are never dereferenced
        p = ctypes.c_void_p(4096)
        assert lib.kws_frame_conv_fwd_f32(p, p, p, p, ctypes.byref(d), None) == -1, why
        assert lib.kws_frame_conv_wgrad_f32(p, p, p, p, ctypes.byref(d), None) == -1, why
    assert lib.kws_frame_conv_stats_rows(None) == 0 and lib.kws_frame_conv_wgrad_workspace_floats(None) == 0
    # the model's own layer at batch 1024: 7 tiles per clip; 1024 statistics rows, 1024 slabs of [80][N]
    for N in (32, 64):
        c = FC._case(1024, 16000, 0, N=N)
        d = _lib.FrameConvDesc(**FC.desc_fields(c))
        assert (c['Lout'], c['pad_l']) == (399, 10)
        assert lib.kws_frame_conv_stats_rows(ctypes.byref(d)) == 1024
        assert lib.kws_frame_conv_wgrad_workspace_floats(ctypes.byref(d)) == 1024 * 80 * N


def test_gap_drop_planner_and_domain():
    lib = _lib.load()
    for B, T, C, rows in ((1, 1, 4, 1), (5, 3, 4, 1), (257, 2, 4, 2), (5, 4, 512, 3), (1024, 3, 512, 512), (5, 16, 1024, 5),
                          (64, 1, 1024, 64)):
        assert lib.kws_gap_drop_bwd_part_rows(B, T, C) == rows, (B, T, C)
    p = ctypes.c_void_p(4096)
    for B, T, C in ((2, 17, 8), (2, 2, 6), (2, 0, 8), (0, 2, 8), (2, 2, 1028)):
        assert lib.kws_gap_drop_bwd_part_rows(B, T, C) == 0
        assert lib.kws_gap_drop_fwd_f32(p, p, p, p, B, T, C, 0.5, 1, 0, 1, 0, None) == -1
        assert lib.kws_gap_drop_bwd_f32(p, p, p, p, p, B, T, C, 0.5, 1, 0, 1, 0, None) == -1
    assert lib.kws_gap_drop_fwd_f32(p, p, p, p, 2, 2, 8, 0.0, 1, 0, 1, 0, None) == -1
    assert lib.kws_gap_drop_fwd_f32(p, p, p, p, 2, 2, 8, 0.5, 1, 0, 1, -1, None) == -1


# ---- the oracle against torch autograd --------------------------------------------------------------------------------------
def _perturbed(fm=1, input_size=16000, seed=5):
    ora = TimeSlicedNet(num_classes=12, filter_mult=fm, input_size=input_size)
    perturb(ora, seed, negative_fraction=0.33, beta=(0.5, 0.3), bias=None, state=False)
    return ora


def _torch_loss(ora, x, y, seed, step):
    """The same network in torch float64: unfold for the frames, F.conv1d for the first and the pointwise convolutions, a grouped
    F.conv1d over explicitly padded inputs for the depthwise ones, F.batch_norm in training mode (eps 1e-3), clamp, the oracle's
    dropout masks, the mean over time, softmax + keras categorical CE."""
    P = {k: torch.tensor(v.astype(np.float64), requires_grad=True) for k, v in ora.params.items()}
    B, L = x.shape
    n = -(-L // HOP)
    total = (n - 1) * HOP + FRAME - L
    xp = Fn.pad(torch.tensor(x.astype(np.float64)), (total // 2, total - total // 2))
    a = xp.unfold(1, FRAME, HOP).permute(0, 2, 1)                                  # [B, 40, frames]
    a = Fn.conv1d(a, P['conv1d_1/kernel'].permute(2, 1, 0), stride=STRIDE)          # [B, C1, L1]

    def bn(a, i):
        return Fn.batch_norm(a, None, None, P['batch_normalization_%d/gamma' % i], P['batch_normalization_%d/beta' % i],
                             training=True, eps=1e-3).clamp(0, 6)
    a = bn(a, 1)
    for blk in ora.blocks:
        C = blk['C']
        w = P['depthwise_conv2d_%d/depthwise_kernel' % blk['dw']][0, :, :, 0]      # [3, C]
        a = Fn.conv1d(Fn.pad(a, block_pad(blk['L'], blk['s'])), w.t().reshape(C, 1, 3), stride=blk['s'], groups=C)
        a = Fn.conv1d(a, P['conv1d_%d/kernel' % blk['bn']].permute(2, 1, 0))
        a = bn(a, blk['bn'])
    feat = a.mean(dim=2)
    k1 = dropout_mask(dropout_key(seed, step, 1), feat.numel(), KEEP1).reshape(feat.shape)
    h = ((feat * torch.tensor(k1.astype(np.float64)) / KEEP1) @ P['dense_1/kernel']).clamp(0, 6)
    k2 = dropout_mask(dropout_key(seed, step, 2), h.numel(), KEEP2).reshape(h.shape)
    p = torch.softmax((h * torch.tensor(k2.astype(np.float64)) / KEEP2) @ P['dense_2/kernel'], dim=1)
    loss = -(torch.tensor(y.astype(np.float64)) * torch.log(p.clamp(1e-7, 1 - 1e-7))).sum(1).mean()
    loss.backward()
    return float(loss.detach()), p.detach().numpy(), {k: v.grad.numpy() for k, v in P.items()}


@pytest.mark.parametrize("fm,input_size", [(1, 16000), (2, 12000)])
def test_oracle_gradients_match_torch_autograd(fm, input_size):
    ora = _perturbed(fm, input_size)
    rng = np.random.RandomState(7)
    B = 3
    x = (rng.randn(B, input_size) * 0.3).astype(np.float32)
    y = np.eye(12, dtype=np.float32)[rng.randint(0, 12, B)]
    loss, p, grads, _ = ora.loss_and_grads(x, y, seed=3, step=5)
    tl, tp, tg = _torch_loss(ora, x, y, seed=3, step=5)
    assert abs(loss - tl) < 1e-10
    np.testing.assert_allclose(p, tp, atol=1e-12)
    assert list(grads) == list(ora.params)
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
