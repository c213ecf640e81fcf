"""GPU parity of the xception_with_attention network program (KWS_NET_XCEPTION_ATTENTION: csrc/net_logmfcc.hip + csrc/attgate.hip +
csrc/gru.hip) against the float64 oracle tests/xception_oracle.py on the harness of tests/net_parity.py: the device's discrete
decisions are handed to the oracle's backward pass: the ReLU6 masks of every BatchNorm (debug views 0 / 2; the one-channel
attention BatchNorm from views 4 / 9), the winners of the 3-wide max-pool windows, and the hard-sigmoid decisions of the GRU (view
7: a gate is in its linear region iff its saved value is strictly between 0 and 1).

Bars: net_parity.FAMILY_BARS - predict 2e-5, train probabilities 5e-5, loss 1e-4, gradients 2e-4 of the tensor's maximum, moving
statistics atol 5e-6 / rtol 1e-5; class indices and the correct-count exact.  Before relying on them the oracle net was run in
float32 against itself in float64 on the CPU (xception_oracle.net_float32_figures: same weights and batches as below, the float32
run on the float64 run's ReLU6, pool and hard-sigmoid decisions; gru_oracle's recurrence keeps its state in float64, so from the
GRU on that run is float64 and the figures for probabilities and loss are lower bounds).  scripts/measure_xception_f32.py prints
both cases, tests/test_xception_cpu.py asserts them: B = 8 at 16000 samples: train probabilities 6.1e-8, loss 3.4e-8,
worst gradient 1.0e-5 (batch_normalization_2/beta), moving statistics 8.3e-8; B = 40 at 4000 samples: train probabilities 1.7e-7,
loss 5.5e-8, worst gradient 2.5e-5 (batch_normalization_27/beta, the one-channel BatchNorm's: a sum of softmax gradients that
cancel), moving statistics 7.3e-8.  Each is under half its bar, so the bars stand."""
import numpy as np
import pytest
import torch

import net_parity as NP
from oracle import layers as OL
from speech_recognition_amd import _lib
from xception_oracle import perturbed_net

pytestmark = pytest.mark.gpu

BARS = NP.FAMILY_BARS


def _pair(nc=12, seed=5, input_size=16000):
    return NP.device_pair(perturbed_net(input_size, num_classes=nc, seed=seed), _lib.KWS_NET_XCEPTION_ATTENTION, nc, input_size=input_size)


def _decisions(net, ora, B):
    shapes = {ora.first[1]: (B, ora.L0, ora.C0)}
    for blk in ora.blocks:
        shapes[blk['bn1']] = (B, blk['Lin'], blk['nf'])
        shapes[blk['bn2']] = (B, blk['Lin'], blk['nf'])
    masks, pre_of = NP.relu_masks(net, B, shapes)
    args = {}
    for i, blk in enumerate(ora.blocks):
        a = np.minimum(np.maximum(pre_of[blk['bn2']], np.float32(0)), np.float32(6))
        Lout, pl, pr = OL.same_pad(blk['Lin'], 3, blk['stride'])
        ap = np.pad(a, [[0, 0], [pl, pr], [0, 0]], constant_values=-np.inf)
        win = np.stack([ap[:, j:j + blk['stride'] * Lout:blk['stride'], :] for j in range(3)], axis=2)
        args[i] = win.argmax(axis=2)
    u, tab = net.debug_view(B, 4, 0), net.debug_view(B, 9, 0)
    pre = (u.astype(np.float64) * np.float64(tab[0]) + np.float64(tab[1])).astype(np.float32)
    masks[ora.att_bn] = ((pre > 0) & (pre <= 6)).astype(np.float64).reshape(B, ora.T)
    save = net.debug_view(B, 7, 0).reshape(2, 4, B, ora.T, ora.H)
    gates = {(d, k): (save[d, q] > 0) & (save[d, q] < 1) for d in range(2) for q, k in enumerate('zr')}
    return masks, args, gates, save


def _step(ora, net, x, y, seed=77, step=2, row_offset=0):
    """One device step and what the oracle needs to repeat it on the device's decisions; the saved GRU gates besides"""
    dev = NP.device_step(net, x, y, seed, step, row_offset)
    masks, args, gates, save = _decisions(net, ora, x.shape[0])
    kw = dict(seed=seed, step=step, relu_masks=masks, pool_args=args, decisions=gates)
    return dev, (x.astype(np.float64), y.astype(np.float64)), kw, save


def test_tensor_table_matches_oracle():
    ora, net = _pair()
    NP.check_tensor_table(ora, net, shapes=True)
    assert {s.name for s in net.tensors.values() if s.l2 > 0} == set(ora.l2_names)


def test_predict_matches_oracle():
    ora, net = _pair()
    x, _ = NP.waveform_batch(5, 12, 1)
    p = net.predict(torch.from_numpy(x).cuda()).cpu().numpy()
    NP.check_predict(p, ora.forward(x.astype(np.float64), training=False), BARS, 'xception_with_attention')


@pytest.mark.parametrize("B,input_size", [(8, 16000), (40, 4000)])
def test_train_fwd_bwd_matches_oracle(B, input_size):
    ora, net = _pair(input_size=input_size)
    assert ora.T == {16000: 50, 4000: 13}[input_size]
    x, y = NP.waveform_batch(B, 12, B, L=input_size)
    dev, xy, kw, save = _step(ora, net, x, y)
    ref = ora.loss_and_grads(*xy, **kw)
    cache = ref[3]
    gc = cache['gate']
    u, att = net.debug_view(B, 4, 0).reshape(B, ora.T), net.debug_view(B, 3, 0).reshape(B, ora.T)
    gy = net.debug_view(B, 6, 0).reshape(B, ora.T, ora.C)
    gout = net.debug_view(B, 8, 0).reshape(B, 2 * ora.H)
    tab = net.debug_view(B, 9, 0)
    assert ora.att_bn in cache['batch_stats']
    NP.check_train_step(dev, y, ref, ora, BARS, "xception B=%d L=%d" % (B, input_size),
                        lead="u %.3g, att %.3g, gate out %.3g, gru out %.3g, " %
                        (np.abs(u - gc['u']).max() / np.abs(gc['u']).max(), np.abs(att - gc['att']).max(),
                         np.abs(gy - cache['gate_out']).max(), np.abs(gout - cache['gru_out']).max()))
    assert np.abs(u - gc['u']).max() < 5e-5 * np.abs(gc['u']).max()
    np.testing.assert_allclose(tab, [gc['scale'], gc['shift'], gc['mean'], gc['rstd']], rtol=5e-5, atol=5e-6)
    assert np.abs(att - gc['att']).max() < 5e-5
    assert np.abs(gy - cache['gate_out']).max() < 5e-5
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


def test_oracle_without_the_direct_term_misses_the_gradient_bar():
    """Negative control: against the gate whose dx lacks the dy att term the device's gradients miss the bar by far."""
    ora, net = _pair(input_size=4000)
    dev, xy, kw, _ = _step(ora, net, *NP.waveform_batch(6, 12, 9, L=4000))
    NP.check_mutated_oracle(dev['grads'], ora.loss_and_grads(*xy, **kw)[2], ora.loss_and_grads(*xy, mutate='no_direct_term', **kw)[2],
                            BARS, far=NP.MUTATED_ORACLE_BAR)


def test_train_step_is_bit_reproducible():
    ora, net = _pair()
    NP.assert_bit_reproducible(net, *NP.waveform_batch(40, 12, 3))


def test_data_parallel_shard_draws_the_global_rows_masks():
    """row_offset = 8 on rows 8 .. 15 reproduces what those rows see inside the 16-row batch, on the GRU output (view 8).  Batch
    statistics differ between the two runs, so the shard is compared with the oracle at drop_offset = 8."""
    ora, net = _pair(input_size=4000)
    x, y = NP.waveform_batch(16, 12, 21, L=4000)
    dev, (xs, ys), kw, _ = _step(ora, net, x[8:], y[8:], seed=5, step=3, row_offset=8)
    gout = net.debug_view(8, 8, 0).reshape(8, 2 * ora.H)
    cache = {}
    ora.forward(xs, training=True, seed=5, step=3, cache=cache, drop_offset=8)
    assert np.abs(gout - cache['gru_out']).max() < 5e-5
    wrong = {}
    ora.forward(xs, training=True, seed=5, step=3, cache=wrong, drop_offset=0)
    assert np.abs(gout - wrong['gru_out']).max() > 1e-2
    NP.check_shard(dev, ora.loss_and_grads(xs, ys, drop_offset=8, **kw), BARS)


def test_two_rmsprop_steps_move_the_weights_as_the_oracle_says():
    """Model.train_on_batch twice: after each step the weights are the float64 Keras-2.1.2 RMSprop rule applied to the device's own
    gradient plus the l2 term 2 c w the optimizer folds in.  A step moves a weight by up to lr / sqrt(1 - rho) = 1.6e-3; the bar is
    1e-6, far above f32 rounding of the update and of the weights themselves (6e-8)."""
    from speech_recognition_amd.keras_api import RMSprop
    from speech_recognition_amd.model import ACCELERATED, speech_model
    assert 'xception_with_attention' in ACCELERATED
    model = speech_model('xception_with_attention', 16000, num_classes=12)
    assert model.name == 'xception_with_attention' and model.loss == 'cce' and isinstance(model.optimizer, RMSprop)
    assert abs(float(model.optimizer.lr) - 5e-4) < 1e-9
    net = model.net
    l2 = net.l2.cpu().numpy().astype(np.float64)
    acc = np.zeros(net.n_params)
    for t in (1, 2):
        x, y = NP.waveform_batch(16, 12, 300 + t)
        p0 = net.params.cpu().numpy().astype(np.float64)
        model.train_on_batch(x, y)
        g = net.grads.cpu().numpy().astype(np.float64) + 2.0 * l2 * p0
        ref, acc = OL.rmsprop_step(p0, g, acc, float(np.float32(5e-4)))
        got = net.params.cpu().numpy()
        moved = np.abs(got - p0).max()
        print("rmsprop step %d: max |w - oracle| = %.3g, largest move %.3g" % (t, np.abs(got - ref).max(), moved))
        assert np.abs(got - ref).max() < 1e-6
        assert 1e-4 < moved < 2e-3


def test_speech_model_trains_through_fit_generator(repo_root):
    """xception_with_attention as train.py drives it: AudioProcessor(output_representation='raw') -> data_gen -> speech_model ->
    Model.fit_generator; the loss on a fixed batch falls over a few steps."""
    from speech_recognition_amd.model import speech_model
    model = speech_model('xception_with_attention', 16000, num_classes=12)
    x, y = NP.waveform_batch(32, 12, 100)
    losses = [float(model.train_on_batch(x, y)[0]) for _ in range(12)]
    print("xception_with_attention losses on a fixed batch: %s" % ' '.join('%.4f' % v for v in losses))
    assert np.all(np.isfinite(losses)) and np.mean(losses[-3:]) < np.mean(losses[:3])
    with pytest.raises(_lib.KwsError):
        speech_model('xception_with_attention', 3999, num_classes=12)
    gen, model, _ = NP.generator_model('xception_with_attention', 'raw', repo_root)
    hist = model.fit_generator(gen, steps_per_epoch=4, epochs=1, verbose=0)
    assert np.isfinite(hist.history['loss'][-1])


def test_checkpoint_round_trip(tmp_path):
    """save -> load -> one more step equals the uninterrupted run bit for bit (weights, moving statistics, the RMSprop slots)."""
    from speech_recognition_amd.model import speech_model
    NP.check_checkpoint_round_trip(lambda: speech_model('xception_with_attention', 16000, num_classes=12),
                                   [NP.waveform_batch(16, 12, 200 + i) for i in range(3)], str(tmp_path / "xception.npz"), slots=('slots',))
