"""CPU checks of conv_1d_learned_spec (KWS_NET_CONV_1D_LEARNED_SPEC, csrc/net_grouped.hip) and of the kernel family it brought
(csrc/fbank_conv.hip): the header / binding declarations, the speech_model dispatch, the structure recorded from the reference
(tests/golden/learned_spec_model.json, made by tests/golden/make_golden_learned_spec.py), the native tensor table against that
fixture and against the float64 oracle (tests/learned_spec_oracle.py), the input sizes kws_net_create takes, the host-side planner
of the new kernels, and the oracle against torch autograd."""
import ctypes
import json
import os
import re

import numpy as np
import pytest
import torch
import torch.nn.functional as Fn

import fbank_conv_cases as FB
from learned_spec_oracle import BLOCKS, FRONT_K, FRONT_N, FRONT_STRIDE, KEEP, MUTATIONS, LearnedSpecNet, padded, same_pads
from net_parity import native_table, perturb
from oracle.layers import dropout_key, dropout_mask
from speech_recognition_amd import _lib

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden', 'learned_spec_model.json')
KIND = 18
# by hand from the layer list: six front kernels of 40 filters; per block the groups' kernels 3 * cin * cout and a gamma / beta
# pair per output channel; Dense [480, 12] with bias
N_TRAINABLE = (40 * (479 + 383 + 319 + 255 + 191 + 161)
               + 3 * (3 * 80 * 100) + 2 * 300 + (3 * 180 * 150 + 3 * 120 * 150) + 2 * 300
               + 3 * (3 * 100 * 120) + 2 * 360 + 2 * (3 * 180 * 180) + 2 * 360
               + 3 * (3 * 80 * 140) + 2 * 420 + 2 * (3 * 210 * 210) + 2 * 420
               + 3 * (3 * 140 * 160) + 2 * 480 + 2 * (3 * 240 * 240) + 2 * 480
               + 480 * 12 + 12)
ROWS = [49, 47, 23, 21, 10, 8, 3, 1]
# per block: (slice start, slice stop, kernel shape) of every group
GROUPS = [[(0, 80, [3, 80, 100]), (80, 160, [3, 80, 100]), (160, 240, [3, 80, 100])],
          [(0, 180, [3, 180, 150]), (180, 300, [3, 120, 150])],
          [(0, 100, [3, 100, 120]), (100, 200, [3, 100, 120]), (200, 300, [3, 100, 120])],
          [(0, 180, [3, 180, 180]), (180, 360, [3, 180, 180])],
          [(0, 80, [3, 80, 140]), (80, 160, [3, 80, 140]), (160, 240, [3, 80, 140])],
          [(0, 210, [3, 210, 210]), (210, 420, [3, 210, 210])],
          [(0, 140, [3, 140, 160]), (140, 280, [3, 140, 160]), (280, 420, [3, 140, 160])],
          [(0, 240, [3, 240, 240]), (240, 480, [3, 240, 240])]]


def _golden(L=16000):
    with open(GOLDEN) as f:
        return json.load(f)['conv_1d_learned_spec_%d' % L]


def _create(input_size, nc=12):
    lib = _lib.load()
    cfg = _lib.NetConfig(KIND, nc, 1, input_size, 0, 0)
    h = ctypes.c_void_p()
    return lib, lib.kws_net_create(ctypes.byref(cfg), ctypes.byref(h)), h


def _fdesc(c, w_off=None):
    d = _lib.FbankConvDesc()
    for k, v in FB.desc_fields(c, w_off):
        if isinstance(v, list):
            for i, e in enumerate(v):
                getattr(d, k)[i] = e
        else:
            setattr(d, k, v)
    return d


# ---- the public surface ---------------------------------------------------------------------------------------------------
NEW_ENTRY_POINTS = ["kws_fbank_conv_fwd_f32", "kws_fbank_conv_wgrad_workspace_floats", "kws_fbank_conv_wgrad_f32"]


def test_header_defines_the_kind_and_declares_the_new_entry_points(repo_root):
    src = open(os.path.join(repo_root, "include", "kws_hip.h")).read()
    assert re.search(r"#define\s+KWS_NET_CONV_1D_LEARNED_SPEC\s+18\b", src)
    assert re.search(r"#define\s+KWS_ABI_VERSION\s+5\b", src)              # additive: the version stays
    assert _lib.KWS_NET_CONV_1D_LEARNED_SPEC == KIND and _lib.ABI_VERSION == 5
    code = re.sub(r"/\*.*?\*/", "", src, flags=re.S)
    lib = _lib.load()
    for name in NEW_ENTRY_POINTS:
        assert re.search(r"\b%s\s*\(" % name, code), name
        assert name in _lib.SIGNATURES and hasattr(lib, name), name
    # the descriptor's binding has the header's members, in order
    members = re.search(r"typedef struct \{([^}]*)\} kws_fbank_conv_t;", code).group(1)
    names = re.findall(r"\b([A-Za-z_]\w*)\s*(?:\[\d+\])?\s*[,;]", members)
    assert names == [f[0] for f in _lib.FbankConvDesc._fields_] == FB.DESC_MEMBERS
    assert re.findall(r"\b(\w+)\[(\d+)\]", members) == [("ksize", "8"), ("pad_l", "8"), ("w_off", "8")]
    assert ctypes.sizeof(_lib.FbankConvDesc) == 6 * 4 + 2 * 8 * 4 + 8 * 8 + 8


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
    assert 'conv_1d_learned_spec' in M.ACCELERATED and 'conv_1d_learned_spec' in M.REFERENCE_MODEL_TYPES
    M.speech_model('conv_1d_learned_spec', 16000, num_classes=12)
    net = captured['net']
    assert net.kind == KIND and net.num_classes == 12 and net.kw == {'input_size': 16000}
    assert captured['name'] == 'conv_1d_learned_spec' and captured['loss'] == 'cce'
    assert isinstance(captured['optimizer'], keras_api.RMSprop) and abs(float(captured['optimizer'].lr) - 2e-3) < 1e-9
    M.conv_1d_learned_spec_model(15000, 30)
    assert captured['net'].kw == {'input_size': 15000} and captured['net'].num_classes == 30
    # conv_1d_fast keeps its kind (and the Keras name it shares with this model)
    M.speech_model('conv_1d_fast', 16000, num_classes=12)
    assert captured['net'].kind == _lib.KWS_NET_CONV_1D_FAST and captured['name'] == 'conv_1d_learned_spec'
    assert abs(float(captured['optimizer'].lr) - 3e-3) < 1e-9
    # the models that are still missing keep saying so
    for missing in ('conv_2d', 'conv_1d_time_sliced_group'):
        with pytest.raises(NotImplementedError):
            M.speech_model(missing, 16000, num_classes=12)


# ---- the recorded structure, the native table, the oracle ------------------------------------------------------------------
def test_fixture_has_the_expected_layers():
    gold = _golden()
    assert (gold['model_name'], gold['optimizer'], gold['lr'], gold['loss']) == \
        ('conv_1d_learned_spec', 'RMSprop', 2e-3, 'categorical_crossentropy')
    convs = [l for l in gold['layers'] if l['class'] == 'Conv1D']
    front = convs[:6]
    assert [l['kernel'] for l in front] == [[k, 1, 40] for k in FRONT_K]
    assert all((l['padding'], l['strides'], l['use_bias'], l['output']) == ('same', 160, False, [100, 40]) for l in front)
    assert [l['pad_left'] for l in front] == [159, 111, 79, 47, 15, 0]
    assert [l['name'] for l in front] == ['conv1d_%d' % i for i in range(1, 7)]
    cat = [l for l in gold['layers'] if l['class'] == 'Concatenate']
    assert cat[0]['inputs'] == [[100, 40]] * 6 and len(cat) == 9
    slices = [l for l in gold['layers'] if l['class'] == 'Lambda' and 'slice' in l]
    want = [g for blk in GROUPS for g in blk]
    assert [(l['slice'][0], l['slice'][1]) for l in slices] == [(a, b) for a, b, _ in want]
    assert [l['channels'] for l in slices] == [b - a for a, b, _ in want]
    ragged = [l for l in slices if l['requested'] != l['slice']]
    assert [(l['requested'], l['slice'], l['channels']) for l in ragged] == [([180, 360], [180, 300], 120)]
    assert [l['kernel'] for l in convs[6:]] == [k for _, _, k in want]
    assert all(l['padding'] == 'valid' and not l['use_bias'] for l in convs[6:])
    rows = [l['output'][0] for l in convs[6:]]
    at = 0
    for blk, r, (F, k, g, nch, s) in zip(GROUPS, ROWS, BLOCKS):
        assert rows[at:at + len(blk)] == [r] * len(blk) and len(blk) == g
        assert all(l['strides'] == s for l in convs[6 + at:6 + at + g])
        at += g
    assert len([l for l in gold['layers'] if l['class'] == 'BatchNormalization']) == 20
    assert [l['rate'] for l in gold['layers'] if l['class'] == 'Dropout'] == [pytest.approx(1 - KEEP)]
    dense = [l for l in gold['layers'] if l['class'] == 'Dense']
    assert [(d['kernel'], d['use_bias'], d['activation']) for d in dense] == [([480, 12], True, 'softmax')]
    # 15000 samples: 94 rows, the front pads from the TF rule
    front = [l for l in _golden(15000)['layers'] if l['class'] == 'Conv1D'][:6]
    assert [l['output'] for l in front] == [[94, 40]] * 6
    assert [l['pad_left'] for l in front] == same_pads(15000)[1] == LearnedSpecNet(input_size=15000).pads == [179, 131, 99, 67, 35, 20]


@pytest.mark.parametrize("L", [16000, 15000])
def test_native_tensor_table_matches_reference_and_oracle(L):
    gold = _golden(L)
    table = native_table(KIND, gold['num_classes'], gold['input_size'])
    assert [t.name.decode() for t in table] == [w['name'] for w in gold['weights']]
    for t, w in zip(table, gold['weights']):
        assert [int(t.shape[k]) for k in range(t.ndim)] == w['shape'], w['name']
        assert bool(t.is_state) == bool(w.get('state', False)), w['name']
        assert t.l2 == np.float32(w['l2']), w['name']
        if w['name'].endswith('/kernel') and len(w['shape']) == 3:
            k, cin, cout = w['shape']
            assert (t.fan_in, t.fan_out) == (k * cin, k * cout), w['name']
        elif w['name'].endswith('/kernel'):
            assert (t.fan_in, t.fan_out) == tuple(w['shape']), w['name']
    for state in (0, 1):
        spans = sorted((t.offset, t.offset + t.size) for t in table if t.is_state == state)
        assert all(a[1] <= b[0] for a, b in zip(spans, spans[1:]))
        assert all(a[0] % 4 == 0 for a in spans)
    n_train = sum(int(np.prod(w['shape'])) for w in gold['weights'] if not w.get('state'))
    assert sum(t.size for t in table if not t.is_state) == n_train == N_TRAINABLE
    ora = LearnedSpecNet(num_classes=gold['num_classes'], input_size=L)
    assert [t.name.decode() for t in table if not t.is_state] == list(ora.params)
    assert [t.name.decode() for t in table if t.is_state] == list(ora.state)
    for t in table:
        v = ora.state[t.name.decode()] if t.is_state else ora.params[t.name.decode()]
        assert tuple(int(t.shape[k]) for k in range(t.ndim)) == v.shape
    assert sum(t.size for t in table) == ora.count_params()
    # l2 1e-4 on exactly the six front kernels
    assert [t.name.decode() for t in table if t.l2 > 0] == ora.l2_names == ['conv1d_%d/kernel' % i for i in range(1, 7)]
    assert all(t.l2 == np.float32(1e-4) for t in table if t.l2 > 0)


def test_net_create_input_sizes_and_views():
    for L, rows in ((16000, 100), (14560, 91), (15000, 94)):
        lib, rc, h = _create(L)
        assert rc == 0, L
        ora = LearnedSpecNet(input_size=L)
        assert ora.rows == rows and ora.blocks[-1]['Lout'] == 1 and ora.D == 480
        assert ora.pads == [max((rows - 1) * 160 + k - L, 0) // 2 for k in FRONT_K]
        off, cnt = ctypes.c_int64(), ctypes.c_int64()
        assert lib.kws_net_debug_view(h, 8, 1, 0, 0, ctypes.byref(off), ctypes.byref(cnt)) == 0 and cnt.value == 8 * rows * 240
        lib.kws_net_destroy(h)
    assert LearnedSpecNet(input_size=15000).pads != LearnedSpecNet(input_size=16000).pads
    for L in (14400, 12000):                             # 90 and 75 rows: the last block would keep no row
        lib, rc, h = _create(L)
        assert rc != 0 and str(L).encode() in lib.kws_last_error()
    for L in (15001, 0, -16000):
        lib, rc, h = _create(L)
        assert rc != 0, L
    lib, rc, h = _create(16000)
    assert rc == 0
    assert lib.kws_net_workspace_bytes(h, 8, 1) > lib.kws_net_workspace_bytes(h, 8, 0) > 0
    off, cnt = ctypes.c_int64(), ctypes.c_int64()
    for index, r, F in [(i + 1, ROWS[i], BLOCKS[i][0]) for i in range(8)]:
        assert lib.kws_net_debug_view(h, 8, 1, 0, index, ctypes.byref(off), ctypes.byref(cnt)) == 0 and cnt.value == 8 * r * F, index
    # batch_normalization_4 and _5 are the ragged block's: 150 columns each, 600 floats apart in one table [2][4][150]
    offs = []
    for j, Ng in ((0, 100), (2, 100), (3, 150), (4, 150), (5, 120), (19, 240)):
        assert lib.kws_net_debug_view(h, 8, 1, 2, j, ctypes.byref(off), ctypes.byref(cnt)) == 0 and cnt.value == 4 * Ng, j
        offs.append(off.value)
    assert offs[3] - offs[2] == 4 * 150
    assert lib.kws_net_debug_view(h, 8, 1, 0, 9, ctypes.byref(off), ctypes.byref(cnt)) != 0
    assert lib.kws_net_debug_view(h, 8, 1, 2, 20, ctypes.byref(off), ctypes.byref(cnt)) != 0
    assert lib.kws_net_debug_view(h, 8, 1, 1, 0, ctypes.byref(off), ctypes.byref(cnt)) != 0
    lib.kws_net_destroy(h)


# ---- the planner of the new kernels, on the host ----------------------------------------------------------------------------
def test_fbank_conv_case_table_and_planner():
    lib = _lib.load()
    reached = set()
    for name, c in list(FB.CASES.items()) + list(FB.FLOAT_CASES.items()):
        assert FB.in_domain(c), name
        assert c['corners'] <= FB.edges(c), (name, c['corners'] - FB.edges(c))
        reached |= c['corners']
        assert lib.kws_fbank_conv_wgrad_workspace_floats(ctypes.byref(_fdesc(c))) == FB.workspace_floats(c) > 0, name
        assert FB.plan(c)['lds_bytes'] <= 160 * 1024, name
    assert reached == FB.CORNERS
    whys = " | ".join(why for _, why in FB.REFUSED)
    for needed in ("no banks", "nine banks", "without taps", "pad_l = ksize", "negative pad_l", "multiple of 4", "odd stride", "span",
                   "x_batch_stride below L"):
        assert needed in whys, needed
    p = ctypes.c_void_p(4096)
    for changes, why in FB.REFUSED:
        bad = FB.refused(changes)
        assert not FB.in_domain(bad), why
        d = _fdesc(bad, FB.packed_offsets(bad)[:8])
        assert lib.kws_fbank_conv_wgrad_workspace_floats(ctypes.byref(d)) == 0, why
        # refused before any launch: the pointers are never dereferenced
        assert lib.kws_fbank_conv_fwd_f32(p, p, p, ctypes.byref(d), None) == -1, why
        assert lib.kws_fbank_conv_wgrad_f32(p, p, p, p, ctypes.byref(d), None) == -1, why
    assert lib.kws_fbank_conv_wgrad_workspace_floats(None) == 0
    assert lib.kws_fbank_conv_fwd_f32(p, p, p, None, None) == -1 and lib.kws_fbank_conv_wgrad_f32(p, p, p, p, None, None) == -1
    # the model's own layer at batch 1024: one tile per clip, 288 accumulator tiles, 256 slabs
    c = FB._case(1024, 16000, 0, 40, FB.MODEL_BANKS)
    pl = FB.plan(c)
    assert (pl['R'], pl['tpc'], pl['T'], pl['S'], pl['P']) == (100, 1, 288, 256, 164)
    assert lib.kws_fbank_conv_wgrad_workspace_floats(ctypes.byref(_fdesc(c))) == 256 * 288 * 256
    # the K ranges multiply 4584 * 16 taps where 1788 * 40 exist
    assert sum(b - a for a, b in zip(pl['k0'], pl['k1'])) == 4584 and sum(FB.MODEL_BANKS) == 1788


# ---- the oracle against torch autograd --------------------------------------------------------------------------------------
def _perturbed(input_size=16000, seed=5):
    ora = LearnedSpecNet(num_classes=12, input_size=input_size)
    perturb(ora, seed, negative_fraction=0.33, beta=(0.5, 0.3), bias=None, state=False)
    return ora


def _torch_loss(ora, x, y, seed, step):
    """The same network in torch float64: F.conv1d at stride 160 over explicitly padded clips for the six front layers, F.conv1d
    over channel slices for the groups, F.batch_norm in training mode (eps 1e-3), clamp, the oracle's dropout mask, softmax + keras
    categorical CE.  -> loss, probabilities, gradients, and the gradient wrt block 4's (index 3) concatenated output."""
    P = {k: torch.tensor(v.astype(np.float64), requires_grad=True) for k, v in ora.params.items()}
    B, L = x.shape
    rows, pads = same_pads(L)
    banks = []
    for q, k in enumerate(FRONT_K):
        xp = torch.tensor(padded(x.astype(np.float64), pads[q], (rows - 1) * FRONT_STRIDE + k))
        banks.append(Fn.conv1d(xp[:, None, :], P['conv1d_%d/kernel' % (q + 1)].permute(2, 1, 0), stride=FRONT_STRIDE))
    a = torch.cat(banks, dim=1)                                                    # [B, 240, rows]
    conv, bn, kept = 7, 1, None
    for i, (F, k, g, nch, s) in enumerate(BLOCKS):
        gs, C = nch // g, a.shape[1]
        outs = []
        for q in range(g):
            yq = Fn.conv1d(a[:, min(q * gs, C):min((q + 1) * gs, C)], P['conv1d_%d/kernel' % conv].permute(2, 1, 0), stride=s)
            outs.append(Fn.batch_norm(yq, None, None, P['batch_normalization_%d/gamma' % bn], P['batch_normalization_%d/beta' % bn],
                                      training=True, eps=1e-3).clamp(0, 6))
            conv, bn = conv + 1, bn + 1
        a = torch.cat(outs, dim=1)
        if i == 3:
            kept = a
            kept.retain_grad()
    flat = a.permute(0, 2, 1).reshape(B, -1)
    keep = dropout_mask(dropout_key(seed, step, 1), flat.numel(), KEEP).reshape(flat.shape)
    p = torch.softmax((flat * torch.tensor(keep.astype(np.float64)) / KEEP) @ P['dense_1/kernel'] + P['dense_1/bias'], dim=1)
    loss = -(torch.tensor(y.astype(np.float64)) * torch.log(p.clamp(1e-7, 1 - 1e-7))).sum(1).mean()
    loss.backward()
    return float(loss.detach()), p.detach().numpy(), {k: v.grad.numpy() for k, v in P.items()}, kept.grad.permute(0, 2, 1).numpy()


@pytest.mark.parametrize("input_size", [16000, 15000])
def test_oracle_gradients_match_torch_autograd(input_size):
    ora = _perturbed(input_size)
    rng = np.random.RandomState(7)
    B = 3
    x = (rng.randn(B, input_size) * 0.3).astype(np.float32)
    y = np.eye(12, dtype=np.float32)[rng.randint(0, 12, B)]
    loss, p, grads, cache = ora.loss_and_grads(x, y, seed=3, step=5)
    tl, tp, tg, t_da4 = _torch_loss(ora, x, y, seed=3, step=5)
    assert abs(loss - tl) < 1e-10
    np.testing.assert_allclose(p, tp, atol=1e-12)
    assert list(grads) == list(ora.params)
    for k, g in grads.items():
        scale = max(np.abs(tg[k]).max(), 1e-12)
        assert np.abs(g - tg[k]).max() / scale < 1e-9, k
    # block 5 reads channels 0 .. 239 of block 4's 360: the rest gets an exactly zero gradient, in the oracle and in torch
    da4 = cache['da4']
    assert da4.shape[2] == 360 and np.abs(da4[:, :, :240]).max() > 0
    assert not da4[:, :, 240:].any() and not t_da4[:, :, 240:].any()
    assert np.abs(da4 - t_da4).max() / np.abs(t_da4).max() < 1e-9


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
