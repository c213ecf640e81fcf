"""GPU parity of the conv_1d_time_stacked / conv_1d_heavy network programs (KWS_NET_CONV_1D_TIME_STACKED / KWS_NET_CONV_1D_HEAVY)
against the float64 oracle tests/stacked_oracle.py on the harness of tests/net_parity.py: the device's ReLU6 and pool arg-max
decisions are read back (debug views 0 and 2) and handed to the oracle's backward pass.  A third of the BatchNorm scales is
negative, so pooling before the normalisation would not pass.

Bars: net_parity.FAMILY_BARS - predict 2e-5, train probabilities 5e-5, loss 1e-4, gradients 2e-4 of the tensor's maximum, moving
statistics atol 5e-6 / rtol 1e-5; class indices and the correct-count exact."""
import numpy as np
import pytest
import torch

import net_parity as NP
from speech_recognition_amd import _lib
from stacked_oracle import StackedConvNet

pytestmark = pytest.mark.gpu

BARS = NP.FAMILY_BARS
KIND = {'time_stacked': _lib.KWS_NET_CONV_1D_TIME_STACKED, 'heavy': _lib.KWS_NET_CONV_1D_HEAVY}
HEAVY_BATCH = 512   # conv_1d_heavy's large parity batch: its float64 oracle holds about 2.5 GB of activations and takes about a minute


def _pair(kind, nc=12, seed=5):
    ora = StackedConvNet(kind, num_classes=nc)
    NP.perturb(ora, seed, negative_fraction=0.33, beta=(0.3, 0.2), bias=0.05)
    return NP.device_pair(ora, KIND[kind], nc, input_size=16000)


def _step(ora, net, B, batch_seed, seed=77, step=2, row_offset=0):
    """One device step and what the oracle needs to repeat it on the device's ReLU6 gates and pool winners"""
    x, y = NP.waveform_batch(B, 12, batch_seed)
    dev = NP.device_step(net, x, y, seed, step, row_offset)
    masks, inds = NP.gates_and_winners(net, B, [(lay['idx'], lay['Lout'], lay['F'], (lay['Lp'], 0) if lay['pool'] else None)
                                                for lay in ora.layers])
    return dev, y, (x.astype(np.float64), y.astype(np.float64)), dict(seed=seed, step=step, relu_masks=masks, pool_ind=inds)


@pytest.mark.parametrize("kind", ['time_stacked', 'heavy'])
def test_tensor_table_matches_oracle(kind):
    NP.check_tensor_table(*_pair(kind))


@pytest.mark.parametrize("kind", ['time_stacked', 'heavy'])
def test_predict_matches_oracle(kind):
    ora, net = _pair(kind)
    x, _ = NP.waveform_batch(5, 12, 1)
    p = net.predict(torch.from_numpy(x).cuda()).cpu().numpy()
    NP.check_predict(p, ora.forward(x.astype(np.float64), training=False), BARS, kind)


@pytest.mark.parametrize("kind,B", [('time_stacked', 3), ('time_stacked', 10), ('time_stacked', 1024), ('heavy', 3), ('heavy', 10),
                                    ('heavy', HEAVY_BATCH)])
def test_train_fwd_bwd_matches_oracle(kind, B):
    ora, net = _pair(kind)
    dev, y, xy, kw = _step(ora, net, B, B)
    NP.check_train_step(dev, y, ora.loss_and_grads(*xy, **kw), ora, BARS, "%s B=%d" % (kind, B))


@pytest.mark.parametrize("mutate", ['pool_before_act', 'no_gate'])
def test_wrong_pool_variants_break_the_gradient_bar(mutate):
    """Negative controls: against an oracle that picks the pool winners before the activation, or drops the pooled layers'
    ReLU6 gate, the device's gradients miss the 2e-4 bar by far.  (Last-max-wins routing cannot move a NET gradient - tied
    activations are saturated ones, whose gates are shut; test_stacked_pool_gpu.py shows that control on the kernel.)"""
    ora, net = _pair('time_stacked')
    dev, _, xy, kw = _step(ora, net, 6, 9)
    NP.check_mutated_oracle(dev['grads'], ora.loss_and_grads(*xy, **kw)[2], ora.loss_and_grads(*xy, mutate=mutate, **kw)[2], BARS,
                            far=NP.MUTATED_ORACLE_BAR)


@pytest.mark.parametrize("kind", ['time_stacked', 'heavy'])
def test_train_step_is_bit_reproducible(kind):
    ora, net = _pair(kind)
    NP.assert_bit_reproducible(net, *NP.waveform_batch(64, 12, 3))


def test_data_parallel_shards_use_the_global_dropout_rows():
    """Both dropout layers of conv_1d_heavy index their masks by the global row: a shard with row_offset reproduces the
    oracle run with drop_offset."""
    ora, net = _pair('heavy')
    dev, _, xy, kw = _step(ora, net, 4, 21, seed=5, step=3, row_offset=37)
    NP.check_shard(dev, ora.loss_and_grads(*xy, drop_offset=37, **kw), BARS)


@pytest.mark.parametrize("model_type", ['conv_1d_time_stacked', 'conv_1d_heavy'])
def test_speech_model_trains(model_type):
    from speech_recognition_amd.keras_api import Adam
    from speech_recognition_amd.model import ACCELERATED, speech_model
    assert model_type in ACCELERATED
    model = speech_model(model_type, 16000, num_classes=12)
    assert model.name == 'conv_1d_time_stacked' and model.loss == 'cce'
    assert isinstance(model.optimizer, Adam) and abs(float(model.optimizer.lr) - 3e-4) < 1e-9
    x, y = NP.waveform_batch(32, 12, 100)
    losses = [float(model.train_on_batch(x, y)[0]) for _ in range(12)]
    print("%s losses on a fixed batch: %s" % (model_type, ' '.join('%.4f' % v for v in losses)))
    assert np.all(np.isfinite(losses)) and np.mean(losses[-3:]) < np.mean(losses[:3])
    with pytest.raises(ValueError):
        speech_model(model_type, 8000, num_classes=12)


def test_adam_checkpoint_round_trip_on_conv_1d_heavy(tmp_path):
    """save -> load -> one more step equals the uninterrupted run bit for bit (weights, moving statistics, both Adam moments,
    `iterations`)."""
    from speech_recognition_amd.model import speech_model
    NP.check_checkpoint_round_trip(lambda: speech_model('conv_1d_heavy', 16000, num_classes=12),
                                   [NP.waveform_batch(16, 12, 200 + i) for i in range(4)], str(tmp_path / "heavy.npz"),
                                   slots=('slots', 'slots2'), iterations=True)


def test_conv_1d_time_stacked_on_the_raw_generator(repo_root):
    """conv_1d_time_stacked as train.py drives it: AudioProcessor(output_representation='raw') -> data_gen -> speech_model ->
    train_on_batch, then Model.fit_generator for one short epoch."""
    gen, model, _ = NP.generator_model('conv_1d_time_stacked', 'raw', repo_root)
    losses = []
    for _ in range(12):
        X, y = next(gen)
        assert tuple(X.shape) == (64, 16000)
        losses.append(float(model.train_on_batch(X, y)[0]))
    assert np.all(np.isfinite(losses))
    hist = model.fit_generator(gen, steps_per_epoch=4, epochs=1, verbose=0)
    assert np.isfinite(hist.history['loss'][-1])
