"""GPU parity of the conv_1d_time_stacked / conv_1d_heavy network programs (KWS_NET_CONV_1D_TIME_STACKED / KWS_NET_CONV_1D_HEAVY)
against the float64 oracle tests/stacked_oracle.py - the method of test_grouped_models_gpu.py: the device's ReLU6 and pool
arg-max decisions are read back (debug views 0 and 2) and handed to the oracle's backward pass.  A third of the BatchNorm
scales is negative, so pooling before the normalisation would not pass.

Bars (those of test_grouped_models_gpu.py): predict 2e-5, train probabilities 5e-5, loss 1e-4, gradients 2e-4 of the tensor's
maximum, moving statistics atol 5e-6 / rtol 1e-5; class indices and the correct-count exact."""
import numpy as np
import pytest
import torch

import pool_oracle
from speech_recognition_amd import _lib
from speech_recognition_amd.net import DeviceNet
from stacked_oracle import StackedConvNet

pytestmark = pytest.mark.gpu

KIND = {'time_stacked': _lib.KWS_NET_CONV_1D_TIME_STACKED, 'heavy': _lib.KWS_NET_CONV_1D_HEAVY}
HEAVY_BATCH = 512   # conv_1d_heavy's large parity batch: its float64 oracle holds about 2.5 GB of activations and takes about a minute


def _pair(kind, nc=12, seed=5):
    ora = StackedConvNet(kind, num_classes=nc)
    rng = np.random.RandomState(seed)
    for k in ora.params:
        if k.endswith('gamma'):   # about a third of the scales negative
            g = 1.0 + 0.1 * rng.randn(*ora.params[k].shape)
            ora.params[k] = (g * np.where(rng.rand(*g.shape) < 0.33, -1.0, 1.0)).astype(np.float32)
        if k.endswith('beta'):
            ora.params[k] = (0.3 + 0.2 * rng.randn(*ora.params[k].shape)).astype(np.float32)
        if k.endswith('bias'):
            ora.params[k] = (0.05 * rng.randn(nc)).astype(np.float32)
    for k in ora.state:
        if k.endswith('moving_mean'):
            ora.state[k] = (0.05 * rng.randn(*ora.state[k].shape)).astype(np.float32)
        else:
            ora.state[k] = (1.0 + 0.2 * rng.rand(*ora.state[k].shape)).astype(np.float32)
    assert any((v < 0).any() for k, v in ora.params.items() if k.endswith('gamma'))
    net = DeviceNet(KIND[kind], nc, input_size=16000)
    net.set_weights(dict(ora.params, **ora.state))
    return ora, net


def _batch(B, nc, seed):
    rng = np.random.RandomState(seed)
    lab = rng.randint(0, nc, B)
    t = np.arange(16000) / 16000.0
    x = rng.randn(B, 16000) * 0.0774 + 0.05 * np.sin(2 * np.pi * 200.0 * (1 + lab)[:, None] * t[None, :])
    return x.astype(np.float32), np.eye(nc, dtype=np.float32)[lab]


def _decisions(net, ora, B):
    """The device's ReLU6 gates and pool winners, from its raw conv outputs and BN tables (float32 fused multiply-add)."""
    masks, inds = {}, {}
    for lay in ora.layers:
        idx, F = lay['idx'], lay['F']
        y = net.debug_view(B, 0, idx - 1).reshape(B, lay['Lout'], F).astype(np.float64)
        bn = net.debug_view(B, 2, idx - 1).astype(np.float64)
        pre = (y * bn[:F] + bn[F:2 * F]).astype(np.float32)
        masks[idx] = (pre > 0) & (pre <= 6)
        if lay['pool']:
            inds[idx] = pool_oracle.argmax(np.clip(pre, 0, 6), lay['Lp'], 0)
    return masks, inds


def _grad_errors(g, grads):
    return {k: np.abs(g[k] - ref.reshape(g[k].shape)).max() / max(np.abs(ref).max(), 1e-7) for k, ref in grads.items()}


@pytest.mark.parametrize("kind", ['time_stacked', 'heavy'])
def test_tensor_table_matches_oracle(kind):
    ora, net = _pair(kind)
    assert [s.name for s in net.tensors.values() if not s.is_state] == list(ora.params.keys())
    assert [s.name for s in net.tensors.values() if s.is_state] == list(ora.state.keys())
    assert net.count_params() == ora.count_params()


@pytest.mark.parametrize("kind", ['time_stacked', 'heavy'])
def test_predict_matches_oracle(kind):
    ora, net = _pair(kind)
    x, _ = _batch(5, 12, 1)
    p = net.predict(torch.from_numpy(x).cuda()).cpu().numpy()
    ref = ora.forward(x.astype(np.float64), training=False)
    print("predict %s: max |p - oracle| = %.3g" % (kind, np.abs(p - ref).max()))
    assert np.abs(p - ref).max() < 2e-5
    assert np.array_equal(p.argmax(1), ref.argmax(1))


@pytest.mark.parametrize("kind,B", [('time_stacked', 3), ('time_stacked', 10), ('time_stacked', 1024), ('heavy', 3), ('heavy', 10),
                                    ('heavy', HEAVY_BATCH)])
def test_train_fwd_bwd_matches_oracle(kind, B):
    ora, net = _pair(kind)
    x, y = _batch(B, 12, B)
    probs = net.train_fwd_bwd(torch.from_numpy(x).cuda(), torch.from_numpy(y).cuda(), seed=77, step=2)
    torch.cuda.synchronize()
    masks, inds = _decisions(net, ora, B)
    loss, p, grads, cache = ora.loss_and_grads(x.astype(np.float64), y.astype(np.float64), seed=77, step=2, relu_masks=masks,
                                               pool_ind=inds)
    got = probs.cpu().numpy()
    m = net.metrics.cpu().numpy()
    errs = _grad_errors(net.grads_dict(), grads)
    worst = max(errs, key=errs.get)
    print("train %s B=%d: probs %.3g, loss %.3g, worst gradient %s %.3g" %
          (kind, B, np.abs(got - p).max(), abs(m[0] / B - loss), worst, errs[worst]))
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
            np.testing.assert_allclose(w['batch_normalization_%d/%s' % (idx, nm)], old - (old - batch) * 0.01,
                                       atol=5e-6, rtol=1e-5)


@pytest.mark.parametrize("mutate", ['pool_before_act', 'no_gate'])
def test_wrong_pool_variants_break_the_gradient_bar(mutate):
    """Negative controls: against an oracle that picks the pool winners before the activation, or drops the pooled layers'
    ReLU6 gate, the device's gradients miss the 2e-4 bar by far.  (Last-max-wins routing cannot move a NET gradient - tied
    activations are saturated ones, whose gates are shut; test_stacked_pool_gpu.py shows that control on the kernel.)"""
    ora, net = _pair('time_stacked')
    B = 6
    x, y = _batch(B, 12, 9)
    net.train_fwd_bwd(torch.from_numpy(x).cuda(), torch.from_numpy(y).cuda(), seed=77, step=2)
    torch.cuda.synchronize()
    masks, inds = _decisions(net, ora, B)
    x64, y64 = x.astype(np.float64), y.astype(np.float64)
    good = ora.loss_and_grads(x64, y64, seed=77, step=2, relu_masks=masks, pool_ind=inds)[2]
    bad = ora.loss_and_grads(x64, y64, seed=77, step=2, relu_masks=masks, pool_ind=inds, mutate=mutate)[2]
    g = net.grads_dict()
    assert max(_grad_errors(g, good).values()) < 2e-4
    assert max(_grad_errors(g, bad).values()) > 1e-2


@pytest.mark.parametrize("kind", ['time_stacked', 'heavy'])
def test_train_step_is_bit_reproducible(kind):
    ora, net = _pair(kind)
    x, y = _batch(64, 12, 3)
    xd, yd = torch.from_numpy(x).cuda(), torch.from_numpy(y).cuda()
    state0 = net.state.clone()
    net.train_fwd_bwd(xd, yd, seed=1, step=0)
    g1, s1 = net.grads.clone(), net.state.clone()
    net.state.copy_(state0)
    net.train_fwd_bwd(xd, yd, seed=1, step=0)
    assert torch.equal(g1, net.grads) and torch.equal(s1, net.state)


def test_data_parallel_shards_use_the_global_dropout_rows():
    """Both dropout layers of conv_1d_heavy index their masks by the global row: a shard with row_offset reproduces the
    oracle run with drop_offset."""
    ora, net = _pair('heavy')
    B, off = 4, 37
    x, y = _batch(B, 12, 21)
    probs = net.train_fwd_bwd(torch.from_numpy(x).cuda(), torch.from_numpy(y).cuda(), seed=5, step=3, row_offset=off)
    torch.cuda.synchronize()
    masks, inds = _decisions(net, ora, B)
    _, p, grads, _ = ora.loss_and_grads(x.astype(np.float64), y.astype(np.float64), seed=5, step=3, drop_offset=off,
                                        relu_masks=masks, pool_ind=inds)
    assert np.abs(probs.cpu().numpy() - p).max() < 5e-5
    assert max(_grad_errors(net.grads_dict(), grads).values()) < 2e-4


@pytest.mark.parametrize("model_type", ['conv_1d_time_stacked', 'conv_1d_heavy'])
def test_speech_model_trains(model_type):
    from speech_recognition_amd.keras_api import Adam
    from speech_recognition_amd.model import ACCELERATED, speech_model
    assert model_type in ACCELERATED
    model = speech_model(model_type, 16000, num_classes=12)
    assert model.name == 'conv_1d_time_stacked' and model.loss == 'cce'
    assert isinstance(model.optimizer, Adam) and abs(float(model.optimizer.lr) - 3e-4) < 1e-9
    x, y = _batch(32, 12, 100)
    losses = [float(model.train_on_batch(x, y)[0]) for _ in range(12)]
    print("%s losses on a fixed batch: %s" % (model_type, ' '.join('%.4f' % v for v in losses)))
    assert np.all(np.isfinite(losses)) and np.mean(losses[-3:]) < np.mean(losses[:3])
    with pytest.raises(ValueError):
        speech_model(model_type, 8000, num_classes=12)


def test_adam_checkpoint_round_trip_on_conv_1d_heavy(tmp_path):
    """save -> load -> one more step equals the uninterrupted run bit for bit (weights, moving statistics, both Adam moments,
    `iterations`)."""
    from speech_recognition_amd.model import speech_model
    a = speech_model('conv_1d_heavy', 16000, num_classes=12)
    batches = [_batch(16, 12, 200 + i) for i in range(4)]
    for xb, yb in batches[:3]:
        a.train_on_batch(xb, yb)
    path = str(tmp_path / "heavy.npz")
    a.save(path)
    b = speech_model('conv_1d_heavy', 16000, num_classes=12)
    b.load_weights(path)
    assert b.optimizer.iterations == 3
    assert torch.equal(a.net.slots, b.net.slots) and torch.equal(a.net.slots2, b.net.slots2)
    la, lb = a.train_on_batch(*batches[3]), b.train_on_batch(*batches[3])
    assert la == lb
    assert torch.equal(a.net.params, b.net.params) and torch.equal(a.net.state, b.net.state)
    assert torch.equal(a.net.slots, b.net.slots) and torch.equal(a.net.slots2, b.net.slots2)


def test_conv_1d_time_stacked_on_the_raw_generator(repo_root):
    """conv_1d_time_stacked as train.py drives it: AudioProcessor(output_representation='raw') -> data_gen -> speech_model ->
    train_on_batch, then Model.fit_generator for one short epoch."""
    import sys
    sys.path.insert(0, repo_root)
    import bench
    from speech_recognition_amd.input_data import AudioProcessor, prepare_words_list
    from speech_recognition_amd.model import prepare_model_settings, speech_model
    from speech_recognition_amd.utils import data_gen
    dev = torch.device("cuda", 0)
    settings = prepare_model_settings(label_count=len(prepare_words_list(bench.WANTED)), sample_rate=16000,
                                      clip_duration_ms=1000, window_size_ms=30.0, window_stride_ms=10.0,
                                      dct_coefficient_count=80, num_log_mel_features=60, output_representation='raw')
    proc = AudioProcessor(bench.build_synthetic(dev, 8192, seed=59185), 13.0, 60.0, bench.WANTED, 10.0, 0.0, settings,
                          output_representation='raw', device=dev)
    np.random.seed(1234)
    gen = data_gen(proc, None, batch_size=64, mode='training')
    model = speech_model('conv_1d_time_stacked', settings['fingerprint_size'], num_classes=settings['label_count'], **settings)
    losses = []
    for _ in range(12):
        X, y = next(gen)
        assert tuple(X.shape) == (64, 16000)
        losses.append(float(model.train_on_batch(X, y)[0]))
    assert np.all(np.isfinite(losses))
    hist = model.fit_generator(gen, steps_per_epoch=4, epochs=1, verbose=0)
    assert np.isfinite(hist.history['loss'][-1])
