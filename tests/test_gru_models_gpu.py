"""GPU parity of the conv_1d_simple network program (KWS_NET_CONV_1D_SIMPLE, csrc/net_dwk.hip + csrc/gru.hip) against the float64
oracle tests/gru_oracle.py - the method of test_dwk_models_gpu.py: the device's ReLU6 decisions (debug views 0 / 2) and its
hard-sigmoid decisions (view 5: a gate is in its linear region iff its saved value is strictly between 0 and 1) are handed to the
oracle's backward pass.  A third of the BatchNorm scales is negative.

Bars (the siblings', unchanged): predict 2e-5, train probabilities 5e-5, loss 1e-4, gradients 2e-4 of the tensor's maximum, moving
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
from net_parity import relu_masks, waveform_batch
from speech_recognition_amd import _lib
from speech_recognition_amd.net import DeviceNet
from gru_oracle import SimpleNet

pytestmark = pytest.mark.gpu


def _pair(nc=12, seed=5):
    ora = SimpleNet(num_classes=nc)
    rng = np.random.RandomState(seed)
    for k in ora.params:
        if k.endswith('gamma'):   # about a third of the scales negative
            g = 1.0 + 0.1 * rng.randn(*ora.params[k].shape)
            ora.params[k] = (g * np.where(rng.rand(*g.shape) < 0.33, -1.0, 1.0)).astype(np.float32)
        if k.endswith('beta'):
            ora.params[k] = (0.3 + 0.2 * rng.randn(*ora.params[k].shape)).astype(np.float32)
        if k.endswith('bias'):
            ora.params[k] = (0.05 * rng.randn(*ora.params[k].shape)).astype(np.float32)
    for k in ora.state:
        if k.endswith('moving_mean'):
            ora.state[k] = (0.05 * rng.randn(*ora.state[k].shape)).astype(np.float32)
        else:
            ora.state[k] = (1.0 + 0.2 * rng.rand(*ora.state[k].shape)).astype(np.float32)
    net = DeviceNet(_lib.KWS_NET_CONV_1D_SIMPLE, nc, input_size=16000)
    net.set_weights(dict(ora.params, **ora.state))
    return ora, net


def _decisions(net, ora, B):
    shapes = {blk['idx'] - 1: (B, blk['Lout'], blk['F']) for blk in ora.blocks}
    masks0, _ = relu_masks(net, B, shapes)
    masks = {i + 1: m for i, m in masks0.items()}
    save = net.debug_view(B, 5, 0).reshape(2, 4, B, ora.T, ora.H)
    gates = {(d, k): (save[d, q] > 0) & (save[d, q] < 1) for d in range(2) for q, k in enumerate('zr')}
    return masks, gates, save


def _grad_errors(g, grads):
    return {k: np.abs(g[k] - ref.reshape(g[k].shape)).max() / max(np.abs(ref).max(), 1e-7) for k, ref in grads.items()}


def test_tensor_table_matches_oracle():
    ora, net = _pair()
    assert [s.name for s in net.tensors.values() if not s.is_state] == list(ora.params.keys())
    assert [s.name for s in net.tensors.values() if s.is_state] == list(ora.state.keys())
    assert net.count_params() == ora.count_params()


def test_predict_matches_oracle():
    ora, net = _pair()
    x, _ = waveform_batch(5, 12, 1)
    p = net.predict(torch.from_numpy(x).cuda()).cpu().numpy()
    ref = ora.forward(x.astype(np.float64), training=False)
    print("predict conv_1d_simple: max |p - oracle| = %.3g" % np.abs(p - ref).max())
    assert np.abs(p - ref).max() < 2e-5
    assert np.array_equal(p.argmax(1), ref.argmax(1))


@pytest.mark.parametrize("B", [8, 40])
def test_train_fwd_bwd_matches_oracle(B):
    ora, net = _pair()
    x, y = waveform_batch(B, 12, B)
    probs = net.train_fwd_bwd(torch.from_numpy(x).cuda(), torch.from_numpy(y).cuda(), seed=77, step=2)
    torch.cuda.synchronize()
    masks, gates, save = _decisions(net, ora, B)
    loss, p, grads, cache = ora.loss_and_grads(x.astype(np.float64), y.astype(np.float64), seed=77, step=2, relu_masks=masks, decisions=gates)
    got = probs.cpu().numpy()
    m = net.metrics.cpu().numpy()
    errs = _grad_errors(net.grads_dict(), grads)
    worst = max(errs, key=errs.get)
    gout = net.debug_view(B, 6, 0).reshape(B, 2 * ora.H)
    print("train conv_1d_simple B=%d: gru out %.3g, probs %.3g, loss %.3g, worst gradient %s %.3g" %
          (B, np.abs(gout - cache['gru_out']).max(), np.abs(got - p).max(), abs(m[0] / B - loss), worst, errs[worst]))
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
    assert np.abs(got - p).max() < 5e-5
    assert np.array_equal(got.argmax(1), p.argmax(1))
    assert abs(m[0] / B - loss) < 1e-4
    assert m[1] == (p.argmax(1) == y.argmax(1)).sum()
    for k, err in errs.items():
        assert err < 2e-4, (k, err)
    w = net.get_weights()
    for idx, (mean, var) in cache['batch_stats'].items():
        for nm, batch in (('moving_mean', mean), ('moving_variance', var)):
            old = ora.state['batch_normalization_%d/%s' % (idx, nm)].astype(np.float64)
            np.testing.assert_allclose(w['batch_normalization_%d/%s' % (idx, nm)], old - (old - batch) * 0.01, atol=5e-6, rtol=1e-5)


def test_reset_after_oracle_misses_the_gradient_bar():
    """Negative control: against the reset_after cell (r applied after the product) the device's gradients miss the bar by far."""
    ora, net = _pair()
    B = 6
    x, y = waveform_batch(B, 12, 9)
    net.train_fwd_bwd(torch.from_numpy(x).cuda(), torch.from_numpy(y).cuda(), seed=77, step=2)
    torch.cuda.synchronize()
    masks, gates, _ = _decisions(net, ora, B)
    x64, y64 = x.astype(np.float64), y.astype(np.float64)
    good = ora.loss_and_grads(x64, y64, seed=77, step=2, relu_masks=masks, decisions=gates)[2]
    bad = ora.loss_and_grads(x64, y64, seed=77, step=2, relu_masks=masks, decisions=gates, mutate='reset_after')[2]
    g = net.grads_dict()
    assert max(_grad_errors(g, good).values()) < 2e-4
    assert max(_grad_errors(g, bad).values()) > 1e-2


def test_train_step_is_bit_reproducible():
    ora, net = _pair()
    x, y = waveform_batch(40, 12, 3)
    xd, yd = torch.from_numpy(x).cuda(), torch.from_numpy(y).cuda()
    state0 = net.state.clone()
    net.train_fwd_bwd(xd, yd, seed=1, step=0)
    g1, s1 = net.grads.clone(), net.state.clone()
    net.state.copy_(state0)
    net.train_fwd_bwd(xd, yd, seed=1, step=0)
    assert torch.equal(g1, net.grads) and torch.equal(s1, net.state)


def test_data_parallel_shard_draws_the_global_rows_masks():
    """row_offset = 8 on rows 8 .. 15 reproduces what those rows see inside the 16-row batch, on the GRU output (view 6).  Batch
    statistics differ between the two runs, so the shard is compared with the oracle at drop_offset = 8, and the oracle's masks
    of the shard with rows 8 .. 15 of the full draw."""
    from gru_oracle import draw_masks
    ora, net = _pair()
    x, y = waveform_batch(16, 12, 21)
    xs, ys = x[8:], y[8:]
    probs = net.train_fwd_bwd(torch.from_numpy(xs).cuda(), torch.from_numpy(ys).cuda(), seed=5, step=3, row_offset=8)
    torch.cuda.synchronize()
    gout = net.debug_view(8, 6, 0).reshape(8, 2 * ora.H)
    masks, gates, _ = _decisions(net, ora, 8)
    cache = {}
    ora.forward(xs.astype(np.float64), training=True, seed=5, step=3, cache=cache, drop_offset=8)
    assert np.abs(gout - cache['gru_out']).max() < 5e-5
    wrong = {}
    ora.forward(xs.astype(np.float64), training=True, seed=5, step=3, cache=wrong, drop_offset=0)
    assert np.abs(gout - wrong['gru_out']).max() > 1e-2
    full = draw_masks(5, 3, 16, ora.I, ora.H, ora.keep, 0, 1)
    part = draw_masks(5, 3, 8, ora.I, ora.H, ora.keep, 8, 1)
    for d in range(2):
        for g in range(3):
            assert np.array_equal(full[0][d][g][8:], part[0][d][g]) and np.array_equal(full[1][d][g][8:], part[1][d][g])
    _, p, grads, _ = ora.loss_and_grads(xs.astype(np.float64), ys.astype(np.float64), seed=5, step=3, drop_offset=8, relu_masks=masks,
                                        decisions=gates)
    assert np.abs(probs.cpu().numpy() - p).max() < 5e-5
    assert max(_grad_errors(net.grads_dict(), grads).values()) < 2e-4


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
        x, y = waveform_batch(16, 12, 300 + t)
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
    import sys
    sys.path.insert(0, repo_root)
    import bench
    from speech_recognition_amd.input_data import AudioProcessor, prepare_words_list
    from speech_recognition_amd.model import prepare_model_settings, speech_model
    from speech_recognition_amd.utils import data_gen
    model = speech_model('conv_1d_simple', 16000, num_classes=12)
    x, y = waveform_batch(32, 12, 100)
    losses = [float(model.train_on_batch(x, y)[0]) for _ in range(12)]
    print("conv_1d_simple losses on a fixed batch: %s" % ' '.join('%.4f' % v for v in losses))
    assert np.all(np.isfinite(losses)) and np.mean(losses[-3:]) < np.mean(losses[:3])
    with pytest.raises(ValueError):
        speech_model('conv_1d_simple', 8000, num_classes=12)
    dev = torch.device("cuda", 0)
    settings = prepare_model_settings(label_count=len(prepare_words_list(bench.WANTED)), sample_rate=16000,
                                      clip_duration_ms=1000, window_size_ms=30.0, window_stride_ms=10.0,
                                      dct_coefficient_count=80, num_log_mel_features=60, output_representation='raw')
    proc = AudioProcessor(bench.build_synthetic(dev, 8192, seed=59185), 13.0, 60.0, bench.WANTED, 10.0, 0.0, settings,
                          output_representation='raw', device=dev)
    np.random.seed(1234)
    gen = data_gen(proc, None, batch_size=64, mode='training')
    model = speech_model('conv_1d_simple', settings['fingerprint_size'], num_classes=settings['label_count'], **settings)
    hist = model.fit_generator(gen, steps_per_epoch=4, epochs=1, verbose=0)
    assert np.isfinite(hist.history['loss'][-1])


def test_checkpoint_round_trip(tmp_path):
    """save -> load -> one more step equals the uninterrupted run bit for bit (weights, moving statistics, both Adam moments)."""
    from speech_recognition_amd.model import speech_model
    a = speech_model('conv_1d_simple', 16000, num_classes=12)
    batches = [waveform_batch(16, 12, 200 + i) for i in range(3)]
    for xb, yb in batches[:2]:
        a.train_on_batch(xb, yb)
    path = str(tmp_path / "simple.npz")
    a.save(path)
    b = speech_model('conv_1d_simple', 16000, num_classes=12)
    b.load_weights(path)
    la, lb = a.train_on_batch(*batches[2]), b.train_on_batch(*batches[2])
    assert la == lb
    assert torch.equal(a.net.params, b.net.params) and torch.equal(a.net.state, b.net.state)
    assert torch.equal(a.net.slots, b.net.slots) and torch.equal(a.net.slots2, b.net.slots2)
