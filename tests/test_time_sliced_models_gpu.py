"""GPU parity of the conv_1d_time_sliced network program (KWS_NET_CONV_1D_TIME_SLICED, csrc/net_time_sliced.hip) against the
float64 oracle tests/time_sliced_oracle.py on the harness of tests/net_parity.py: the device's ReLU6 decisions (debug views
0 / 2 / 4) are handed to the oracle's backward pass.  A third of the BatchNorm scales is negative.

Bars: net_parity.FAMILY_BARS - predict 2e-5, train probabilities 5e-5, loss 1e-4, gradients 2e-4 of the tensor's maximum, moving
statistics atol 5e-6 / rtol 1e-5; class indices and the correct-count exact."""
import numpy as np
import pytest
import torch

import net_parity as NP
from speech_recognition_amd import _lib
from time_sliced_oracle import TimeSlicedNet

pytestmark = pytest.mark.gpu

BARS = NP.FAMILY_BARS


def _pair(nc=12, fm=1, input_size=16000, seed=5):
    ora = TimeSlicedNet(num_classes=nc, filter_mult=fm, input_size=input_size)
    NP.perturb(ora, seed, negative_fraction=0.33, beta=(0.3, 0.2), bias=None)
    return NP.device_pair(ora, _lib.KWS_NET_CONV_1D_TIME_SLICED, nc, filter_mult=fm, input_size=input_size)


def _decisions(net, ora, B):
    """The device's ReLU6 gates: the fourteen BatchNorms from their raw inputs and tables, the hidden layer from h."""
    shapes = {0: (B, ora.L1, ora.C1)}
    shapes.update({blk['bn'] - 1: (B, blk['Lout'], blk['F']) for blk in ora.blocks})
    masks0, _ = NP.relu_masks(net, B, shapes)
    masks = {i + 1: m for i, m in masks0.items()}
    h = net.debug_view(B, 4, 0).reshape(B, ora.H)
    masks['hidden'] = ((h > 0) & (h <= 6)).astype(np.float64)
    return masks


def _step(ora, net, B, batch_seed, seed=77, step=2, row_offset=0, L=16000):
    """One device step and what the oracle needs to repeat it on the device's gates"""
    x, y = NP.waveform_batch(B, 12, batch_seed, L=L)
    dev = NP.device_step(net, x, y, seed, step, row_offset)
    return dev, y, (x.astype(np.float64), y.astype(np.float64)), dict(seed=seed, step=step, relu_masks=_decisions(net, ora, B))


@pytest.mark.parametrize("fm", [1, 2])
def test_tensor_table_matches_oracle(fm):
    NP.check_tensor_table(*_pair(fm=fm))


def test_predict_matches_oracle():
    ora, net = _pair()
    x, _ = NP.waveform_batch(5, 12, 1)
    p = net.predict(torch.from_numpy(x).cuda()).cpu().numpy()
    NP.check_predict(p, ora.forward(x.astype(np.float64), training=False), BARS, 'conv_1d_time_sliced')


def test_forward_views_match_oracle():
    """Debug views 0 and 1: the first convolution's output and every block's depthwise output against the oracle's forward in
    training mode."""
    ora, net = _pair()
    B = 4
    x, y = NP.waveform_batch(B, 12, 2)
    NP.device_step(net, x, y, seed=3, step=1)
    cache = {}
    ora.forward(x.astype(np.float64), training=True, seed=3, step=1, cache=cache)
    y0 = net.debug_view(B, 0, 0).reshape(B, ora.L1, ora.C1)
    assert np.abs(y0 - cache['y1']).max() < 2e-5 * np.abs(cache['y1']).max()
    for i, blk in enumerate(ora.blocks):
        z = net.debug_view(B, 1, i).reshape(B, blk['Lout'], blk['C'])
        ref = cache['z%d' % blk['bn']]
        assert np.abs(z - ref).max() < 2e-4 * max(np.abs(ref).max(), 1e-7), i


@pytest.mark.parametrize("B,input_size,fm", [(8, 16000, 1), (4, 12000, 2)])
def test_train_fwd_bwd_matches_oracle(B, input_size, fm):
    ora, net = _pair(fm=fm, input_size=input_size)
    assert ora.T == (3 if input_size == 16000 else 1)
    dev, y, xy, kw = _step(ora, net, B, B, L=input_size)
    ref = ora.loss_and_grads(*xy, **kw)
    errs = NP.check_train_step(dev, y, ref, ora, BARS, "conv_1d_time_sliced B=%d L=%d fm=%d" % (B, input_size, fm))
    assert list(errs) == list(ora.params)
    assert len(ref[3]['batch_stats']) == 14


@pytest.mark.parametrize("mutate", ['pad_left', 'reversed_taps'])
def test_mutated_oracle_misses_the_gradient_bar(mutate):
    """Negative controls: against an oracle that puts the odd SAME sample on the left, or applies the taps back to front, the
    device's gradients miss the 2e-4 bar by far."""
    ora, net = _pair()
    dev, _, xy, kw = _step(ora, net, 6, 9)
    NP.check_mutated_oracle(dev['grads'], ora.loss_and_grads(*xy, **kw)[2], ora.loss_and_grads(*xy, mutate=mutate, **kw)[2], BARS,
                            far=NP.MUTATED_ORACLE_BAR)


def test_gemm_mode_1_gives_the_same_bits():
    """separate input- / weight-gradient launches (mode 1) and the fused pair (mode 0) run the same code on the same data"""
    ora, net = _pair()
    x, y = NP.waveform_batch(16, 12, 4)
    xd, yd = torch.from_numpy(x).cuda(), torch.from_numpy(y).cuda()
    state0 = net.state.clone()
    net.train_fwd_bwd(xd, yd, seed=1, step=0)
    g0 = net.grads.clone()
    net.state.copy_(state0)
    net.set_gemm_mode(1)
    net.train_fwd_bwd(xd, yd, seed=1, step=0)
    assert torch.equal(g0, net.grads)


def test_train_step_is_bit_reproducible():
    ora, net = _pair()
    NP.assert_bit_reproducible(net, *NP.waveform_batch(64, 12, 3))


def test_data_parallel_shard_uses_the_global_dropout_rows():
    ora, net = _pair()
    dev, _, xy, kw = _step(ora, net, 4, 21, seed=5, step=3, row_offset=37)
    NP.check_shard(dev, ora.loss_and_grads(*xy, drop_offset=37, **kw), BARS)
    # ... and not the local ones
    _, p0, _, _ = ora.loss_and_grads(*xy, drop_offset=0, **kw)
    assert np.abs(dev['probs'] - p0).max() > 1e-3


def test_speech_model_trains():
    from speech_recognition_amd.keras_api import RMSprop
    from speech_recognition_amd.model import ACCELERATED, speech_model
    assert 'conv_1d_time_sliced' in ACCELERATED
    model = speech_model('conv_1d_time_sliced', 16000, num_classes=12)
    assert model.name == 'conv_1d_time_sliced' and model.loss == 'cce'
    assert isinstance(model.optimizer, RMSprop) and abs(float(model.optimizer.lr) - 1e-3) < 1e-9
    x, y = NP.waveform_batch(32, 12, 100)
    losses = [float(model.train_on_batch(x, y)[0]) for _ in range(12)]
    print("conv_1d_time_sliced losses on a fixed batch: %s" % ' '.join('%.4f' % v for v in losses))
    assert np.all(np.isfinite(losses)) and np.mean(losses[-3:]) < np.mean(losses[:3])
    with pytest.raises(_lib.KwsError):
        speech_model('conv_1d_time_sliced', 8000, num_classes=12)


def test_checkpoint_round_trip(tmp_path):
    """save -> load -> one more step equals the uninterrupted run bit for bit (weights, moving statistics, RMSprop slots)."""
    from speech_recognition_amd.model import speech_model
    NP.check_checkpoint_round_trip(lambda: speech_model('conv_1d_time_sliced', 16000, num_classes=12),
                                   [NP.waveform_batch(16, 12, 200 + i) for i in range(4)], str(tmp_path / "tsl.npz"), slots=('slots',))
