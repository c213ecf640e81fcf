"""GPU parity of the conv_1d_time_sliced network program (KWS_NET_CONV_1D_TIME_SLICED, csrc/net_time_sliced.hip) against the
float64 oracle tests/time_sliced_oracle.py - test_dwk_models_gpu.py's template with tests/net_parity.py's batch and mask
read-back: the device's ReLU6 decisions (debug views 0 / 2 / 4) are handed to the oracle's backward pass.  A third of the
BatchNorm scales is negative.

Bars (test_dwk_models_gpu.py's, unchanged): predict 2e-5, train probabilities 5e-5, loss 1e-4, gradients 2e-4 of the tensor's
maximum, moving statistics atol 5e-6 / rtol 1e-5; class indices and the correct-count exact."""
import numpy as np
import pytest
import torch

from net_parity import relu_masks, waveform_batch
from speech_recognition_amd import _lib
from speech_recognition_amd.net import DeviceNet
from time_sliced_oracle import TimeSlicedNet

pytestmark = pytest.mark.gpu


def _pair(nc=12, fm=1, input_size=16000, seed=5):
    ora = TimeSlicedNet(num_classes=nc, filter_mult=fm, input_size=input_size)
    rng = np.random.RandomState(seed)
    for k in ora.params:
        if k.endswith('gamma'):   # about a third of the scales negative
            g = 1.0 + 0.1 * rng.randn(*ora.params[k].shape)
            ora.params[k] = (g * np.where(rng.rand(*g.shape) < 0.33, -1.0, 1.0)).astype(np.float32)
        if k.endswith('beta'):
            ora.params[k] = (0.3 + 0.2 * rng.randn(*ora.params[k].shape)).astype(np.float32)
    for k in ora.state:
        if k.endswith('moving_mean'):
            ora.state[k] = (0.05 * rng.randn(*ora.state[k].shape)).astype(np.float32)
        else:
            ora.state[k] = (1.0 + 0.2 * rng.rand(*ora.state[k].shape)).astype(np.float32)
    assert any((v < 0).any() for k, v in ora.params.items() if k.endswith('gamma'))
    net = DeviceNet(_lib.KWS_NET_CONV_1D_TIME_SLICED, nc, filter_mult=fm, input_size=input_size)
    net.set_weights(dict(ora.params, **ora.state))
    return ora, net


def _decisions(net, ora, B):
    """The device's ReLU6 gates: the fourteen BatchNorms from their raw inputs and tables, the hidden layer from h."""
    shapes = {0: (B, ora.L1, ora.C1)}
    shapes.update({blk['bn'] - 1: (B, blk['Lout'], blk['F']) for blk in ora.blocks})
    masks0, _ = relu_masks(net, B, shapes)
    masks = {i + 1: m for i, m in masks0.items()}
    h = net.debug_view(B, 4, 0).reshape(B, ora.H)
    masks['hidden'] = ((h > 0) & (h <= 6)).astype(np.float64)
    return masks


def _grad_errors(g, grads):
    return {k: np.abs(g[k] - ref.reshape(g[k].shape)).max() / max(np.abs(ref).max(), 1e-7) for k, ref in grads.items()}


@pytest.mark.parametrize("fm", [1, 2])
def test_tensor_table_matches_oracle(fm):
    ora, net = _pair(fm=fm)
    assert [s.name for s in net.tensors.values() if not s.is_state] == list(ora.params.keys())
    assert [s.name for s in net.tensors.values() if s.is_state] == list(ora.state.keys())
    assert net.count_params() == ora.count_params()


def test_predict_matches_oracle():
    ora, net = _pair()
    x, _ = waveform_batch(5, 12, 1)
    p = net.predict(torch.from_numpy(x).cuda()).cpu().numpy()
    ref = ora.forward(x.astype(np.float64), training=False)
    print("predict conv_1d_time_sliced: max |p - oracle| = %.3g" % np.abs(p - ref).max())
    assert np.abs(p - ref).max() < 2e-5
    assert np.array_equal(p.argmax(1), ref.argmax(1))


def test_forward_views_match_oracle():
    """Debug views 0 and 1: the first convolution's output and every block's depthwise output against the oracle's forward in
    training mode."""
    ora, net = _pair()
    B = 4
    x, y = waveform_batch(B, 12, 2)
    net.train_fwd_bwd(torch.from_numpy(x).cuda(), torch.from_numpy(y).cuda(), seed=3, step=1)
    torch.cuda.synchronize()
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
    x, y = waveform_batch(B, 12, B, L=input_size)
    probs = net.train_fwd_bwd(torch.from_numpy(x).cuda(), torch.from_numpy(y).cuda(), seed=77, step=2)
    torch.cuda.synchronize()
    masks = _decisions(net, ora, B)
    loss, p, grads, cache = ora.loss_and_grads(x.astype(np.float64), y.astype(np.float64), seed=77, step=2, relu_masks=masks)
    got = probs.cpu().numpy()
    m = net.metrics.cpu().numpy()
    errs = _grad_errors(net.grads_dict(), grads)
    worst = max(errs, key=errs.get)
    print("train conv_1d_time_sliced B=%d L=%d fm=%d: probs %.3g, loss %.3g, worst gradient %s %.3g" %
          (B, input_size, fm, np.abs(got - p).max(), abs(m[0] / B - loss), worst, errs[worst]))
    assert np.abs(got - p).max() < 5e-5
    assert np.array_equal(got.argmax(1), p.argmax(1))
    assert abs(m[0] / B - loss) < 1e-4
    assert m[1] == (p.argmax(1) == y.argmax(1)).sum()
    assert list(errs) == list(ora.params)
    for k, err in errs.items():
        assert err < 2e-4, (k, err)
    w = net.get_weights()
    assert len(cache['batch_stats']) == 14
    for idx, (mean, var) in cache['batch_stats'].items():
        for nm, batch in (('moving_mean', mean), ('moving_variance', var)):
            old = ora.state['batch_normalization_%d/%s' % (idx, nm)].astype(np.float64)
            np.testing.assert_allclose(w['batch_normalization_%d/%s' % (idx, nm)], old - (old - batch) * 0.01,
                                       atol=5e-6, rtol=1e-5)


@pytest.mark.parametrize("mutate", ['pad_left', 'reversed_taps'])
def test_mutated_oracle_misses_the_gradient_bar(mutate):
    """Negative controls: against an oracle that puts the odd SAME sample on the left, or applies the taps back to front, the
    device's gradients miss the 2e-4 bar by far."""
    ora, net = _pair()
    B = 6
    x, y = waveform_batch(B, 12, 9)
    net.train_fwd_bwd(torch.from_numpy(x).cuda(), torch.from_numpy(y).cuda(), seed=77, step=2)
    torch.cuda.synchronize()
    masks = _decisions(net, ora, B)
    x64, y64 = x.astype(np.float64), y.astype(np.float64)
    good = ora.loss_and_grads(x64, y64, seed=77, step=2, relu_masks=masks)[2]
    bad = ora.loss_and_grads(x64, y64, seed=77, step=2, relu_masks=masks, mutate=mutate)[2]
    g = net.grads_dict()
    assert max(_grad_errors(g, good).values()) < 2e-4
    assert max(_grad_errors(g, bad).values()) > 1e-2


def test_gemm_mode_1_gives_the_same_bits():
    """separate input- / weight-gradient launches (mode 1) and the fused pair (mode 0) run the same code on the same data"""
    ora, net = _pair()
    x, y = waveform_batch(16, 12, 4)
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
    x, y = waveform_batch(64, 12, 3)
    xd, yd = torch.from_numpy(x).cuda(), torch.from_numpy(y).cuda()
    state0 = net.state.clone()
    net.train_fwd_bwd(xd, yd, seed=1, step=0)
    g1, s1 = net.grads.clone(), net.state.clone()
    net.state.copy_(state0)
    net.train_fwd_bwd(xd, yd, seed=1, step=0)
    assert torch.equal(g1, net.grads) and torch.equal(s1, net.state)


def test_data_parallel_shard_uses_the_global_dropout_rows():
    ora, net = _pair()
    B, off = 4, 37
    x, y = waveform_batch(B, 12, 21)
    probs = net.train_fwd_bwd(torch.from_numpy(x).cuda(), torch.from_numpy(y).cuda(), seed=5, step=3, row_offset=off)
    torch.cuda.synchronize()
    masks = _decisions(net, ora, B)
    _, p, grads, _ = ora.loss_and_grads(x.astype(np.float64), y.astype(np.float64), seed=5, step=3, drop_offset=off, relu_masks=masks)
    assert np.abs(probs.cpu().numpy() - p).max() < 5e-5
    assert max(_grad_errors(net.grads_dict(), grads).values()) < 2e-4
    # ... and not the local ones
    _, p0, _, _ = ora.loss_and_grads(x.astype(np.float64), y.astype(np.float64), seed=5, step=3, drop_offset=0, relu_masks=masks)
    assert np.abs(probs.cpu().numpy() - p0).max() > 1e-3


def test_speech_model_trains():
    from speech_recognition_amd.keras_api import RMSprop
    from speech_recognition_amd.model import ACCELERATED, speech_model
    assert 'conv_1d_time_sliced' in ACCELERATED
    model = speech_model('conv_1d_time_sliced', 16000, num_classes=12)
    assert model.name == 'conv_1d_time_sliced' and model.loss == 'cce'
    assert isinstance(model.optimizer, RMSprop) and abs(float(model.optimizer.lr) - 1e-3) < 1e-9
    x, y = waveform_batch(32, 12, 100)
    losses = [float(model.train_on_batch(x, y)[0]) for _ in range(12)]
    print("conv_1d_time_sliced losses on a fixed batch: %s" % ' '.join('%.4f' % v for v in losses))
    assert np.all(np.isfinite(losses)) and np.mean(losses[-3:]) < np.mean(losses[:3])
    with pytest.raises(_lib.KwsError):
        speech_model('conv_1d_time_sliced', 8000, num_classes=12)


def test_checkpoint_round_trip(tmp_path):
    """save -> load -> one more step equals the uninterrupted run bit for bit (weights, moving statistics, RMSprop slots)."""
    from speech_recognition_amd.model import speech_model
    a = speech_model('conv_1d_time_sliced', 16000, num_classes=12)
    batches = [waveform_batch(16, 12, 200 + i) for i in range(4)]
    for xb, yb in batches[:3]:
        a.train_on_batch(xb, yb)
    path = str(tmp_path / "tsl.npz")
    a.save(path)
    b = speech_model('conv_1d_time_sliced', 16000, num_classes=12)
    b.load_weights(path)
    assert torch.equal(a.net.slots, b.net.slots)
    la, lb = a.train_on_batch(*batches[3]), b.train_on_batch(*batches[3])
    assert la == lb
    assert torch.equal(a.net.params, b.net.params) and torch.equal(a.net.state, b.net.state)
    assert torch.equal(a.net.slots, b.net.slots)
