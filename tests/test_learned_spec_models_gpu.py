"""GPU parity of the conv_1d_learned_spec network program (KWS_NET_CONV_1D_LEARNED_SPEC: the banked front convolution of
csrc/fbank_conv.hip, the grouped ladder with its ragged second block) against the float64 oracle tests/learned_spec_oracle.py -
the method and the bars of test_grouped_models_gpu.py, whose nets run the same ladder kernels at the same depths: the device's
ReLU6 decisions are read back (debug views 0 and 2) and handed to the oracle's backward pass."""
import json
import os

import numpy as np
import pytest
import torch

import net_parity as NP
from learned_spec_oracle import MUTATIONS, LearnedSpecNet
from speech_recognition_amd import _lib
from speech_recognition_amd.net import DeviceNet

pytestmark = pytest.mark.gpu

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden', 'learned_spec_model.json')


def _pair(L=16000, nc=12, seed=5):
    ora = LearnedSpecNet(num_classes=nc, input_size=L)
    NP.perturb(ora, seed)
    net = DeviceNet(_lib.KWS_NET_CONV_1D_LEARNED_SPEC, nc, input_size=L)
    net.set_weights(dict(ora.params, **ora.state))
    return ora, net


def _decisions(net, ora, B):
    masks = {}
    for i, blk in enumerate(ora.blocks):
        y = net.debug_view(B, 0, i + 1).reshape(B, blk['Lout'], blk['F']).astype(np.float64)
        Ng = blk['Ng']
        for q, idx in enumerate(blk['bns']):
            bn = net.debug_view(B, 2, idx - 1).astype(np.float64)
            assert bn.size == 4 * Ng
            pre = (y[:, :, q * Ng:(q + 1) * Ng] * bn[:Ng] + bn[Ng:2 * Ng]).astype(np.float32)
            masks[idx] = ((pre > 0) & (pre <= 6)).astype(np.float64)
    return masks


def test_tensor_table_matches_oracle_and_reference():
    ora, net = _pair()
    assert [s.name for s in net.tensors.values() if not s.is_state] == list(ora.params.keys())
    assert [s.name for s in net.tensors.values() if s.is_state] == list(ora.state.keys())
    for k, v in list(ora.params.items()) + list(ora.state.items()):
        assert net.tensors[k].shape == v.shape, k
    assert net.count_params() == ora.count_params()
    with open(GOLDEN) as f:
        gold = json.load(f)['conv_1d_learned_spec_16000']
    assert [s.name for s in net.tensors.values()] == [w['name'] for w in gold['weights']]


@pytest.mark.parametrize("L", [16000, 15000])
def test_predict_matches_oracle(L):
    ora, net = _pair(L)
    x, _ = NP.waveform_batch(5, 12, 1, L=L)
    p = net.predict(torch.from_numpy(x).cuda()).cpu().numpy()
    ref = ora.forward(x.astype(np.float64), training=False)
    assert np.abs(p - ref).max() < 2e-5
    assert np.array_equal(p.argmax(1), ref.argmax(1))


@pytest.mark.parametrize("L,B", [(16000, 3), (16000, 10), (15000, 4), (14560, 3)])
def test_train_fwd_bwd_matches_oracle(L, B):
    ora, net = _pair(L)
    x, y = NP.waveform_batch(B, 12, B, L=L)
    probs = net.train_fwd_bwd(torch.from_numpy(x).cuda(), torch.from_numpy(y).cuda(), seed=77, step=2)
    torch.cuda.synchronize()
    masks = _decisions(net, ora, B)
    loss, p, grads, cache = ora.loss_and_grads(x.astype(np.float64), y.astype(np.float64), seed=77, step=2, relu_masks=masks)
    # the front convolution's output, straight in the joined tensor
    y0 = net.debug_view(B, 0, 0).reshape(B, ora.rows, 240)
    assert np.abs(y0 - cache['x0']).max() < 2e-6 * max(np.abs(cache['x0']).max(), 1.0)
    got = probs.cpu().numpy()
    assert np.abs(got - p).max() < 5e-5
    assert np.array_equal(got.argmax(1), p.argmax(1))
    m = net.metrics.cpu().numpy()
    assert abs(m[0] / B - loss) < 1e-4
    assert m[1] == (p.argmax(1) == y.argmax(1)).sum()
    g = net.grads_dict()
    worst = {}
    for k, ref in grads.items():
        ref = ref.reshape(g[k].shape)
        worst[k] = np.abs(g[k] - ref).max() / max(np.abs(ref).max(), 1e-7)
    print("\nconv_1d_learned_spec L=%d B=%d: worst gradient error %.3e (%s)" % (L, B, max(worst.values()), max(worst, key=worst.get)))
    for k, err in worst.items():
        assert err < 2e-4, (k, err)
    w = net.get_weights()
    for idx, (mean, var) in cache['batch_stats'].items():
        for nm, batch in (('moving_mean', mean), ('moving_variance', var)):
            old = ora.state['batch_normalization_%d/%s' % (idx, nm)].astype(np.float64)
            np.testing.assert_allclose(w['batch_normalization_%d/%s' % (idx, nm)], old - (old - batch) * 0.01, atol=5e-6, rtol=1e-5)
    if (L, B) == (16000, 3):       # the device agrees with neither mutated oracle
        for mutate in MUTATIONS:
            _, _, wrong, _ = ora.loss_and_grads(x.astype(np.float64), y.astype(np.float64), seed=77, step=2, relu_masks=masks,
                                                mutate=mutate)
            assert max(np.abs(g[k] - r.reshape(g[k].shape)).max() / max(np.abs(r).max(), 1e-7) for k, r in wrong.items()) > 1e-2, mutate


def test_train_step_is_bit_reproducible():
    ora, net = _pair()
    x, y = NP.waveform_batch(64, 12, 3)
    xd, yd = torch.from_numpy(x).cuda(), torch.from_numpy(y).cuda()
    state0 = net.state.clone()
    net.train_fwd_bwd(xd, yd, seed=1, step=0)
    g1, s1 = net.grads.clone(), net.state.clone()
    net.state.copy_(state0)
    net.train_fwd_bwd(xd, yd, seed=1, step=0)
    assert torch.equal(g1, net.grads) and torch.equal(s1, net.state)


def test_speech_model_trains():
    from speech_recognition_amd.model import ACCELERATED, speech_model
    assert 'conv_1d_learned_spec' in ACCELERATED
    model = speech_model('conv_1d_learned_spec', 16000, num_classes=12)
    assert model.name == 'conv_1d_learned_spec' and model.loss == 'cce' and abs(float(model.optimizer.lr) - 2e-3) < 1e-9
    x, y = NP.waveform_batch(32, 12, 100)
    losses = [float(model.train_on_batch(x, y)[0]) for _ in range(12)]
    assert np.all(np.isfinite(losses)) and min(losses[2:]) < 0.7 * losses[0]
