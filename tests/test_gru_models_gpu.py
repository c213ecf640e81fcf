"""GPU parity of the conv_1d_simple network program (KWS_NET_CONV_1D_SIMPLE, csrc/net_dwk.hip + csrc/gru.hip) against the float64
oracle tests/gru_oracle.py on the harness of tests/net_parity.py: the device's ReLU6 decisions (debug views 0 / 2) and its
hard-sigmoid decisions (view 5: a gate is in its linear region iff its saved value is strictly between 0 and 1) are handed to the
oracle's backward pass.  A third of the BatchNorm scales is negative.

Bars: net_parity.FAMILY_BARS - predict 2e-5, train probabilities 5e-5, loss 1e-4, gradients 2e-4 of the tensor's maximum, moving
statistics atol 5e-6 / rtol 1e-5; class indices and the correct-count exact.  Before relying on them the oracle net was run in
float32 against itself in float64 on the CPU (same weights and batches as below, the float32 run on the float64 run's ReLU6 and
hard-sigmoid decisions): B = 8: train probabilities 1.2e-6, loss 1.7e-6, worst gradient 1.5e-5 (conv1d_13/kernel); B = 40: train
probabilities 3.0e-6, loss 1.1e-6, worst gradient 2.3e-5 (batch_normalization_11/gamma).  Each is under half its bar, so the bars
stand.  (The inference pass of that float32 run is promoted to float64 by the oracle's moving-statistics arithmetic and says
nothing; the training-mode forward figure, 3.0e-6 against the 2e-5 predict bar, is the one that bears on it.)"""
import numpy as np
import pytest
import torch

import adam_oracle as SO
import net_parity as NP
from speech_recognition_amd import _lib
from gru_oracle import SimpleNet

pytestmark = pytest.mark.gpu

BARS = NP.FAMILY_BARS


def _pair(nc=12, seed=5):
    ora = SimpleNet(num_classes=nc)
    NP.perturb(ora, seed, negative_fraction=0.33, beta=(0.3, 0.2), bias=0.05)
    return NP.device_pair(ora, _lib.KWS_NET_CONV_1D_SIMPLE, nc, input_size=16000)


def _decisions(net, ora, B):
    shapes = {blk['idx'] - 1: (B, blk['Lout'], blk['F']) for blk in ora.blocks}
    masks0, _ = NP.relu_masks(net, B, shapes)
    masks = {i + 1: m for i, m in masks0.items()}
    save = net.debug_view(B, 5, 0).reshape(2, 4, B, ora.T, ora.H)
    gates = {(d, k): (save[d, q] > 0) & (save[d, q] < 1) for d in range(2) for q, k in enumerate('zr')}
    return masks, gates, save


def _step(ora, net, x, y, seed=77, step=2, row_offset=0):
    """One device step and what the oracle needs to repeat it on the device's gates; the saved GRU gates besides"""
    dev = NP.device_step(net, x, y, seed, step, row_offset)
    masks, gates, save = _decisions(net, ora, x.shape[0])
    return dev, (x.astype(np.float64), y.astype(np.float64)), dict(seed=seed, step=step, relu_masks=masks, decisions=gates), save


def test_tensor_table_matches_oracle():
    NP.check_tensor_table(*_pair())


def test_predict_matches_oracle():
    ora, net = _pair()
    x, _ = NP.waveform_batch(5, 12, 1)
    p = net.predict(torch.from_numpy(x).cuda()).cpu().numpy()
    NP.check_predict(p, ora.forward(x.astype(np.float64), training=False), BARS, 'conv_1d_simple')


@pytest.mark.parametrize("B", [8, 40])
def test_train_fwd_bwd_matches_oracle(B):
    ora, net = _pair()
    x, y = NP.waveform_batch(B, 12, B)
    dev, xy, kw, save = _step(ora, net, x, y)
    ref = ora.loss_and_grads(*xy, **kw)
    cache = ref[3]
    gout = net.debug_view(B, 6, 0).reshape(B, 2 * ora.H)
    NP.check_train_step(dev, y, ref, ora, BARS, "conv_1d_simple B=%d" % B, lead="gru out %.3g, " % np.abs(gout - cache['gru_out']).max())
    # saved gates against the oracle's, away from the corners of the hard sigmoid
    left = total = 0
    for d in range(2):
        for q, k in enumerate('zr'):
            pre = cache['gru'][d]['p' + k]
            far = np.abs(np.abs(pre) - 2.5) > 1e-5
            left += (~far).sum()
            total += far.size
            assert np.abs(save[d, q] - cache['gru'][d][k])[far].max() < 5e-5, (d, k)
    assert left <= 1e-3 * total
    assert np.abs(gout - cache['gru_out']).max() < 5e-5


def test_reset_after_oracle_misses_the_gradient_bar():
    """Negative control: against the reset_after cell (r applied after the product) the device's gradients miss the bar by far."""
    ora, net = _pair()
    dev, xy, kw, _ = _step(ora, net, *NP.waveform_batch(6, 12, 9))
    NP.check_mutated_oracle(dev['grads'], ora.loss_and_grads(*xy, **kw)[2], ora.loss_and_grads(*xy, mutate='reset_after', **kw)[2], BARS,
                            far=NP.MUTATED_ORACLE_BAR)


def test_train_step_is_bit_reproducible():
    ora, net = _pair()
    NP.assert_bit_reproducible(net, *NP.waveform_batch(40, 12, 3))


def test_data_parallel_shard_draws_the_global_rows_masks():
    """row_offset = 8 on rows 8 .. 15 reproduces what those rows see inside the 16-row batch, on the GRU output (view 6).  Batch
    statistics differ between the two runs, so the shard is compared with the oracle at drop_offset = 8, and the oracle's masks
    of the shard with rows 8 .. 15 of the full draw."""
    from gru_oracle import draw_masks
    ora, net = _pair()
    x, y = NP.waveform_batch(16, 12, 21)
    dev, (xs, ys), kw, _ = _step(ora, net, x[8:], y[8:], seed=5, step=3, row_offset=8)
    gout = net.debug_view(8, 6, 0).reshape(8, 2 * ora.H)
    cache = {}
    ora.forward(xs, training=True, seed=5, step=3, cache=cache, drop_offset=8)
    assert np.abs(gout - cache['gru_out']).max() < 5e-5
    wrong = {}
    ora.forward(xs, training=True, seed=5, step=3, cache=wrong, drop_offset=0)
    assert np.abs(gout - wrong['gru_out']).max() > 1e-2
    full = draw_masks(5, 3, 16, ora.I, ora.H, ora.keep, 0, 1)
    part = draw_masks(5, 3, 8, ora.I, ora.H, ora.keep, 8, 1)
    for d in range(2):
        for g in range(3):
            assert np.array_equal(full[0][d][g][8:], part[0][d][g]) and np.array_equal(full[1][d][g][8:], part[1][d][g])
    NP.check_shard(dev, ora.loss_and_grads(xs, ys, drop_offset=8, **kw), BARS)


def test_two_adam_steps_move_the_weights_as_the_oracle_says():
    """Model.train_on_batch twice: after each step the weights are the float64 Keras-2.1.2 Adam rule applied to the device's own
    gradient (plus the l2 term 2 c w the optimizer folds in).  A step moves a weight by about lr = 1e-3; the bar is 1e-6: a
    relative error of 1e-3 of the step, far above f32 rounding of the update and of the weights themselves (6e-8)."""
    from speech_recognition_amd.keras_api import Adam
    from speech_recognition_amd.model import ACCELERATED, speech_model
    assert 'conv_1d_simple' in ACCELERATED
    model = speech_model('conv_1d_simple', 16000, num_classes=12)
    assert model.name == 'conv_1d_time_stacked' and model.loss == 'cce' and isinstance(model.optimizer, Adam)
    net = model.net
    l2 = net.l2.cpu().numpy().astype(np.float64)
    m = np.zeros(net.n_params)
    v = np.zeros(net.n_params)
    for t in (1, 2):
        x, y = NP.waveform_batch(16, 12, 300 + t)
        p0 = net.params.cpu().numpy().astype(np.float64)
        model.train_on_batch(x, y)
        g = net.grads.cpu().numpy().astype(np.float64) + 2.0 * l2 * p0
        ref, m, v = SO.adam_step(p0, g, m, v, float(np.float32(1e-3)), t)
        got = net.params.cpu().numpy()
        moved = np.abs(got - p0).max()
        print("adam step %d: max |w - oracle| = %.3g, largest move %.3g" % (t, np.abs(got - ref).max(), moved))
        assert np.abs(got - ref).max() < 1e-6
        assert 1e-4 < moved < 2e-3


def test_speech_model_trains_through_fit_generator(repo_root):
    """conv_1d_simple as train.py drives it: AudioProcessor(output_representation='raw') -> data_gen -> speech_model ->
    Model.fit_generator; the loss on a fixed batch falls over a few steps."""
    from speech_recognition_amd.model import speech_model
    model = speech_model('conv_1d_simple', 16000, num_classes=12)
    x, y = NP.waveform_batch(32, 12, 100)
    losses = [float(model.train_on_batch(x, y)[0]) for _ in range(12)]
    print("conv_1d_simple losses on a fixed batch: %s" % ' '.join('%.4f' % v for v in losses))
    assert np.all(np.isfinite(losses)) and np.mean(losses[-3:]) < np.mean(losses[:3])
    with pytest.raises(ValueError):
        speech_model('conv_1d_simple', 8000, num_classes=12)
    gen, model, _ = NP.generator_model('conv_1d_simple', 'raw', repo_root)
    hist = model.fit_generator(gen, steps_per_epoch=4, epochs=1, verbose=0)
    assert np.isfinite(hist.history['loss'][-1])


def test_checkpoint_round_trip(tmp_path):
    """save -> load -> one more step equals the uninterrupted run bit for bit (weights, moving statistics, both Adam moments)."""
    from speech_recognition_amd.model import speech_model
    NP.check_checkpoint_round_trip(lambda: speech_model('conv_1d_simple', 16000, num_classes=12),
                                   [NP.waveform_batch(16, 12, 200 + i) for i in range(3)], str(tmp_path / "simple.npz"),
                                   slots=('slots', 'slots2'), iterations=True)
