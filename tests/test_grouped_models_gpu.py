"""GPU parity of the conv_1d_fast / conv_1d_spec network programs (KWS_NET_CONV_1D_FAST / KWS_NET_CONV_1D_SPEC) against the
float64 oracle tests/grouped_oracle.py on the harness of tests/net_parity.py (bars: its FAMILY_BARS): the device's ReLU6
decisions are read back (debug views 0 and 2) and handed to the oracle's backward pass."""
import json
import os

import numpy as np
import pytest
import torch

import net_parity as NP
from grouped_oracle import GroupedConvNet
from speech_recognition_amd import _lib

pytestmark = pytest.mark.gpu

BARS = NP.FAMILY_BARS
KIND = {'fast': _lib.KWS_NET_CONV_1D_FAST, 'spec': _lib.KWS_NET_CONV_1D_SPEC}
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden', 'grouped_models.json')


def _pair(kind, nc=12, seed=5):
    ora = GroupedConvNet(kind, num_classes=nc)
    NP.perturb(ora, seed, bias=0.05, bias_names=('dense_1/bias',))
    return NP.device_pair(ora, KIND[kind], nc, input_size=16000 if kind == 'fast' else 98 * 257)


def _batch(kind, B, nc, seed):
    if kind == 'fast':
        return NP.waveform_batch(B, nc, seed)
    rng = np.random.RandomState(seed)
    lab = rng.randint(0, nc, B)
    x = np.abs(rng.randn(B, 98, 257)) * (1.0 + 0.1 * lab[:, None, None])
    return x.reshape(B, -1).astype(np.float32), np.eye(nc, dtype=np.float32)[lab]


def _decisions(net, ora, B):
    """Every block's BatchNorms gate their own column slice of the block's raw output."""
    masks = {}
    stage0 = 1 if ora.front else 0
    for i, blk in enumerate(ora.blocks):
        y = net.debug_view(B, 0, i + stage0).reshape(B, blk['Lout'], blk['F']).astype(np.float64)
        Ng = blk['Ng']
        for q, idx in enumerate(blk['bns']):
            bn = net.debug_view(B, 2, idx - 1).astype(np.float64)
            pre = (y[:, :, q * Ng:(q + 1) * Ng] * bn[:Ng] + bn[Ng:2 * Ng]).astype(np.float32)
            masks[idx] = ((pre > 0) & (pre <= 6)).astype(np.float64)
    return masks


@pytest.mark.parametrize("kind", ['fast', 'spec'])
def test_tensor_table_matches_oracle_and_reference(kind):
    ora, net = _pair(kind)
    NP.check_tensor_table(ora, net, shapes=True)
    with open(GOLDEN) as f:
        gold = json.load(f)['conv_1d_' + kind]
    assert [s.name for s in net.tensors.values()] == [w['name'] for w in gold['weights']]
    l2 = {s.name: s.l2 for s in net.tensors.values() if s.l2 > 0}
    assert l2 == ({'conv1d_1/kernel': np.float32(1e-4)} if kind == 'fast' else {})


@pytest.mark.parametrize("kind", ['fast', 'spec'])
def test_predict_matches_oracle(kind):
    ora, net = _pair(kind)
    x, _ = _batch(kind, 5, 12, 1)
    p = net.predict(torch.from_numpy(x).cuda()).cpu().numpy()
    NP.check_predict(p, ora.forward(x.astype(np.float64), training=False), BARS, 'conv_1d_' + kind)


@pytest.mark.parametrize("kind,B", [('fast', 3), ('fast', 10), ('fast', 1024), ('spec', 3), ('spec', 10), ('spec', 1024)])
def test_train_fwd_bwd_matches_oracle(kind, B):
    ora, net = _pair(kind)
    x, y = _batch(kind, B, 12, B)
    dev = NP.device_step(net, x, y, seed=77, step=2)
    ref = ora.loss_and_grads(x.astype(np.float64), y.astype(np.float64), seed=77, step=2, relu_masks=_decisions(net, ora, B))
    NP.check_train_step(dev, y, ref, ora, BARS, "conv_1d_%s B=%d" % (kind, B))


@pytest.mark.parametrize("kind", ['fast', 'spec'])
def test_train_step_is_bit_reproducible(kind):
    ora, net = _pair(kind)
    NP.assert_bit_reproducible(net, *_batch(kind, 64, 12, 3))


@pytest.mark.parametrize("model_type,name,lr", [('conv_1d_fast', 'conv_1d_learned_spec', 3e-3),
                                                ('conv_1d_spec', 'conv_1d_spec', 2e-3)])
def test_speech_model_trains(model_type, name, lr):
    from speech_recognition_amd.model import ACCELERATED, speech_model
    assert model_type in ACCELERATED
    model = speech_model(model_type, 16000, num_classes=12)
    assert model.name == name and model.loss == 'cce' and abs(float(model.optimizer.lr) - lr) < 1e-9
    x, y = _batch('fast' if model_type == 'conv_1d_fast' else 'spec', 32, 12, 100)
    losses = [float(model.train_on_batch(x, y)[0]) for _ in range(12)]
    assert np.all(np.isfinite(losses)) and min(losses[2:]) < 0.7 * losses[0]


def test_conv_1d_spec_on_the_spec_generator(repo_root):
    """conv_1d_spec as train.py drives it: AudioProcessor(output_representation='spec') -> data_gen -> speech_model ->
    train_on_batch, then Model.fit_generator for one short epoch."""
    gen, model, _ = NP.generator_model('conv_1d_spec', 'spec', repo_root)
    losses = []
    for _ in range(12):
        X, y = next(gen)
        assert np.asarray(X).shape == (64, 98 * 257)
        losses.append(float(model.train_on_batch(X, y)[0]))
    assert np.all(np.isfinite(losses)) and np.mean(losses[-3:]) < np.mean(losses[:3])
    hist = model.fit_generator(gen, steps_per_epoch=4, epochs=1, verbose=0)
    assert np.isfinite(hist.history['loss'][-1])
