"""GPU parity of the conv_1d_learned_spec network program (KWS_NET_CONV_1D_LEARNED_SPEC: the banked front convolution of
csrc/fbank_conv.hip, the grouped ladder with its ragged second block) against the float64 oracle tests/learned_spec_oracle.py on
the harness and the bars (FAMILY_BARS) of tests/net_parity.py - the bars of test_grouped_models_gpu.py, whose nets run the same
ladder kernels at the same depths: the device's ReLU6 decisions are read back (debug views 0 and 2) and handed to the oracle's
backward pass."""
import json
import os

import numpy as np
import pytest
import torch

import net_parity as NP
from learned_spec_oracle import MUTATIONS, LearnedSpecNet
from speech_recognition_amd import _lib

pytestmark = pytest.mark.gpu

BARS = NP.FAMILY_BARS
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden', 'learned_spec_model.json')


def _pair(L=16000, nc=12, seed=5):
    ora = LearnedSpecNet(num_classes=nc, input_size=L)
    NP.perturb(ora, seed)
    return NP.device_pair(ora, _lib.KWS_NET_CONV_1D_LEARNED_SPEC, nc, input_size=L)


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
    NP.check_tensor_table(ora, net, shapes=True)
    with open(GOLDEN) as f:
        gold = json.load(f)['conv_1d_learned_spec_16000']
    assert [s.name for s in net.tensors.values()] == [w['name'] for w in gold['weights']]


@pytest.mark.parametrize("L", [16000, 15000])
def test_predict_matches_oracle(L):
    ora, net = _pair(L)
    x, _ = NP.waveform_batch(5, 12, 1, L=L)
    p = net.predict(torch.from_numpy(x).cuda()).cpu().numpy()
    NP.check_predict(p, ora.forward(x.astype(np.float64), training=False), BARS, 'conv_1d_learned_spec L=%d' % L)


@pytest.mark.parametrize("L,B", [(16000, 3), (16000, 10), (15000, 4), (14560, 3)])
def test_train_fwd_bwd_matches_oracle(L, B):
    ora, net = _pair(L)
    x, y = NP.waveform_batch(B, 12, B, L=L)
    dev = NP.device_step(net, x, y, seed=77, step=2)
    x64, y64, kw = x.astype(np.float64), y.astype(np.float64), dict(seed=77, step=2, relu_masks=_decisions(net, ora, B))
    ref = ora.loss_and_grads(x64, y64, **kw)
    # the front convolution's output, straight in the joined tensor
    y0, x0 = net.debug_view(B, 0, 0).reshape(B, ora.rows, 240), ref[3]['x0']
    assert np.abs(y0 - x0).max() < 2e-6 * max(np.abs(x0).max(), 1.0)
    NP.check_train_step(dev, y, ref, ora, BARS, "conv_1d_learned_spec L=%d B=%d" % (L, B))
    if (L, B) == (16000, 3):       # the device agrees with neither mutated oracle
        for mutate in MUTATIONS:
            wrong = ora.loss_and_grads(x64, y64, mutate=mutate, **kw)[2]
            assert max(NP.grad_errors(dev['grads'], wrong).values()) > NP.MUTATED_ORACLE_BAR, mutate


def test_train_step_is_bit_reproducible():
    ora, net = _pair()
    NP.assert_bit_reproducible(net, *NP.waveform_batch(64, 12, 3))


def test_speech_model_trains():
    from speech_recognition_amd.model import ACCELERATED, speech_model
    assert 'conv_1d_learned_spec' in ACCELERATED
    model = speech_model('conv_1d_learned_spec', 16000, num_classes=12)
    assert model.name == 'conv_1d_learned_spec' and model.loss == 'cce' and abs(float(model.optimizer.lr) - 2e-3) < 1e-9
    x, y = NP.waveform_batch(32, 12, 100)
    losses = [float(model.train_on_batch(x, y)[0]) for _ in range(12)]
    assert np.all(np.isfinite(losses)) and min(losses[2:]) < 0.7 * losses[0]
