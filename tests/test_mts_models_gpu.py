"""GPU parity of the conv_1d_multi_time_sliced network program (KWS_NET_CONV_1D_MULTI_TIME_SLICED, csrc/net_mts.hip) against the
float64 oracle tests/mts_oracle.py - the method of test_dwk_models_gpu.py / test_stacked_models_gpu.py: the device's ReLU6 and
pool arg-max decisions are read back (debug views 0 and 2, blocks in creation order) and handed to the oracle's backward pass.  A
third of the BatchNorm scales is negative.

Bars: the sibling nets', unchanged - predict 2e-5, train probabilities 5e-5, loss 1e-4, gradients 2e-4 of the tensor's maximum,
moving statistics atol 5e-6 / rtol 1e-5; class indices and the correct-count exact.  This net is twice as deep as any sibling and
its last BatchNorms see only B rows, so the oracle net was first run in float32 on the CPU (torch, tests/mts_torch.py, on its own
decisions) against its float64 self with these weights and batches: batch 8 - probabilities 8.8e-7, loss 4.9e-7, worst gradient
7.7e-6 of its tensor's maximum; batch 64 - probabilities 1.7e-6, loss 2.8e-7, worst gradient 7.7e-6.  Every figure is under half
the sibling bar, so no bar is widened."""
import numpy as np
import pytest
import torch

import pool_oracle
from net_parity import perturb, waveform_batch
from speech_recognition_amd import _lib
from speech_recognition_amd.net import DeviceNet
from mts_oracle import MtsNet

pytestmark = pytest.mark.gpu

NC = 12


def _perturb(ora, seed=5):
    perturb(ora, seed, negative_fraction=0.33, beta=(0.3, 0.2), bias=0.05)
    assert any((v < 0).any() for k, v in ora.params.items() if k.endswith('gamma'))


def _pair(zero=None):
    ora = MtsNet(num_classes=NC)
    _perturb(ora)
    if zero is not None:
        ora.params[zero] = np.zeros_like(ora.params[zero])
    net = DeviceNet(_lib.KWS_NET_CONV_1D_MULTI_TIME_SLICED, NC, input_size=16000)
    net.set_weights(dict(ora.params, **ora.state))
    return ora, net


def _decisions(net, ora, B):
    """The device's ReLU6 gates and pool winners, from its raw pointwise outputs and BN tables (float32 fused multiply-add)."""
    masks, inds = {}, {}
    for blk in ora.blocks:
        idx, F = blk['idx'], blk['F']
        y = net.debug_view(B, 0, idx - 1).reshape(B, blk['Lout'], F).astype(np.float64)
        bn = net.debug_view(B, 2, idx - 1).astype(np.float64)
        pre = (y * bn[:F] + bn[F:2 * F]).astype(np.float32)
        masks[idx] = ((pre > 0) & (pre <= 6)).astype(np.float64)
        if blk['pool'] is not None:
            inds[idx] = pool_oracle.argmax(np.clip(pre, 0, 6).astype(np.float64), blk['pool']['Lp'], blk['pool']['pad_l'])
    return masks, inds


def _grad_errors(g, grads):
    return {k: np.abs(g[k] - ref.reshape(g[k].shape)).max() / max(np.abs(ref).max(), 1e-7) for k, ref in grads.items()}


def _step(ora, net, B, batch_seed, seed=77, step=2, row_offset=0):
    x, y = waveform_batch(B, NC, batch_seed)
    probs = net.train_fwd_bwd(torch.from_numpy(x).cuda(), torch.from_numpy(y).cuda(), seed=seed, step=step, row_offset=row_offset)
    torch.cuda.synchronize()
    masks, inds = _decisions(net, ora, B)
    return x.astype(np.float64), y.astype(np.float64), probs.cpu().numpy(), masks, inds


@pytest.fixture(scope='module')
def step8():
    """One device step at batch 8, the device's decisions and the oracle's step on them: shared, left unchanged."""
    ora, net = _pair()
    x, y, probs, masks, inds = _step(ora, net, 8, 8)
    ref = ora.loss_and_grads(x, y, seed=77, step=2, relu_masks=masks, pool_ind=inds)
    return {'ora': ora, 'x': x, 'y': y, 'probs': probs, 'masks': masks, 'inds': inds, 'ref': ref, 'grads': net.grads_dict(),
            'metrics': net.metrics.cpu().numpy(), 'weights': net.get_weights()}


def _check(ora, B, y, probs, metrics, g, weights, ref, tag):
    loss, p, grads, cache = ref
    errs = _grad_errors(g, grads)
    worst = max(errs, key=errs.get)
    print("train conv_1d_multi_time_sliced %s: probs %.3g, loss %.3g, worst gradient %s %.3g" %
          (tag, np.abs(probs - p).max(), abs(metrics[0] / B - loss), worst, errs[worst]))
    assert np.abs(probs - p).max() < 5e-5
    assert np.array_equal(probs.argmax(1), p.argmax(1))
    assert abs(metrics[0] / B - loss) < 1e-4
    assert metrics[1] == (p.argmax(1) == y.argmax(1)).sum()
    for k, err in errs.items():
        assert err < 2e-4, (k, err)
    for idx, (mean, var) in cache['batch_stats'].items():
        for nm, batch in (('moving_mean', mean), ('moving_variance', var)):
            old = ora.state['batch_normalization_%d/%s' % (idx, nm)].astype(np.float64)
            np.testing.assert_allclose(weights['batch_normalization_%d/%s' % (idx, nm)], old - (old - batch) * 0.01, atol=5e-6,
                                       rtol=1e-5)


def test_tensor_table_matches_oracle():
    ora, net = _pair()
    assert [s.name for s in net.tensors.values() if not s.is_state] == list(ora.params.keys())
    assert [s.name for s in net.tensors.values() if s.is_state] == list(ora.state.keys())
    assert net.count_params() == ora.count_params()
    for s in net.tensors.values():
        assert s.shape == (ora.state if s.is_state else ora.params)[s.name].shape


def test_predict_matches_oracle():
    ora, net = _pair()
    x, _ = waveform_batch(5, NC, 1)
    p = net.predict(torch.from_numpy(x).cuda()).cpu().numpy()
    ref = ora.forward(x.astype(np.float64), training=False)
    print("predict conv_1d_multi_time_sliced: max |p - oracle| = %.3g" % np.abs(p - ref).max())
    assert np.abs(p - ref).max() < 2e-5
    assert np.array_equal(p.argmax(1), ref.argmax(1))


def test_train_fwd_bwd_matches_oracle_batch_8(step8):
    s = step8
    _check(s['ora'], 8, s['y'], s['probs'], s['metrics'], s['grads'], s['weights'], s['ref'], 'B=8')


def test_train_fwd_bwd_matches_oracle_batch_64():
    ora, net = _pair()
    x, y, probs, masks, inds = _step(ora, net, 64, 64)
    ref = ora.loss_and_grads(x, y, seed=77, step=2, relu_masks=masks, pool_ind=inds)
    _check(ora, 64, y, probs, net.metrics.cpu().numpy(), net.grads_dict(), net.get_weights(), ref, 'B=64')


def test_two_consumer_tensors_pass_both_gradients_upstream(step8):
    """The blocks that produce the 28- and 22-step tensors (8 and 20) and what lies upstream of them meet the bar; an oracle that
    drops the tap's gradient at the fork misses it there, and only there."""
    s = step8
    ora = s['ora']
    assert ora.forks == [8, 20]
    errs = _grad_errors(s['grads'], s['ref'][2])
    up = ['%s_%d/%s' % (a, i, b) for i in (1, 7, 8, 13, 19, 20)
          for a, b in (('conv1d', 'kernel'), ('depthwise_conv2d', 'depthwise_kernel'), ('batch_normalization', 'gamma'))]
    assert max(errs[k] for k in up) < 2e-4
    bad = ora.loss_and_grads(s['x'], s['y'], seed=77, step=2, relu_masks=s['masks'], pool_ind=s['inds'], mutate='drop_fork')[2]
    bad_errs = _grad_errors(s['grads'], bad)
    assert min(bad_errs['conv1d_8/kernel'], bad_errs['conv1d_20/kernel']) > 1e-2
    assert max(bad_errs[k] for k in bad_errs if k.split('/')[0].split('_')[-1] in ('10', '11', '12', '22', '23', '24', '32', '33')) < 2e-4


def test_pool_padding_side_control(step8):
    """An oracle with the pool's odd padding sample on the wrong side breaks the gradient bar."""
    s = step8
    bad = s['ora'].loss_and_grads(s['x'], s['y'], seed=77, step=2, relu_masks=s['masks'], mutate='pool_pad_side')[2]
    assert max(_grad_errors(s['grads'], bad).values()) > 1e-2


def test_concatenation_keeps_the_other_ends_apart():
    """conv1d_21's kernel (branch end xs5a) zeroed in both nets: the other four ends' gradients stay within the bar, and nothing
    flows back through the zeroed end's pointwise layer."""
    ora, net = _pair(zero='conv1d_21/kernel')
    x, y, probs, masks, inds = _step(ora, net, 8, 8)
    grads = ora.loss_and_grads(x, y, seed=77, step=2, relu_masks=masks, pool_ind=inds)[2]
    g = net.grads_dict()
    errs = _grad_errors(g, grads)
    for end in (9, 12, 24, 31):
        for name in ('conv1d_%d/kernel' % end, 'depthwise_conv2d_%d/depthwise_kernel' % end, 'batch_normalization_%d/gamma' % end):
            assert errs[name] < 2e-4, (name, errs[name])
            assert np.abs(g[name]).max() > 0
    assert max(errs.values()) < 2e-4
    assert not g['depthwise_conv2d_21/depthwise_kernel'].any()


def test_train_step_is_bit_reproducible():
    ora, net = _pair()
    x, y = waveform_batch(16, NC, 3)
    xd, yd = torch.from_numpy(x).cuda(), torch.from_numpy(y).cuda()
    state0 = net.state.clone()
    net.train_fwd_bwd(xd, yd, seed=1, step=0)
    g1, s1 = net.grads.clone(), net.state.clone()
    net.state.copy_(state0)
    net.train_fwd_bwd(xd, yd, seed=1, step=0)
    assert torch.equal(g1, net.grads) and torch.equal(s1, net.state)


def test_data_parallel_shard_uses_the_global_dropout_rows():
    ora, net = _pair()
    off = 37
    x, y, probs, masks, inds = _step(ora, net, 4, 21, seed=5, step=3, row_offset=off)
    _, p, grads, _ = ora.loss_and_grads(x, y, seed=5, step=3, drop_offset=off, relu_masks=masks, pool_ind=inds)
    assert np.abs(probs - p).max() < 5e-5
    assert max(_grad_errors(net.grads_dict(), grads).values()) < 2e-4


def test_speech_model_fits():
    from speech_recognition_amd.keras_api import RMSprop
    from speech_recognition_amd.model import ACCELERATED, speech_model
    assert 'conv_1d_multi_time_sliced' in ACCELERATED
    model = speech_model('conv_1d_multi_time_sliced', 16000, num_classes=NC)
    assert model.name == 'conv_1d_multi_time_sliced' and model.loss == 'cce'
    assert isinstance(model.optimizer, RMSprop) and abs(float(model.optimizer.lr) - 3e-3) < 1e-9
    batches = [waveform_batch(32, NC, 100 + i) for i in range(8)]
    def gen():
        while True:
            for b in batches:
                yield b

    hist = model.fit_generator(gen(), steps_per_epoch=8, epochs=3, verbose=0)
    losses = hist.history['loss']
    print("conv_1d_multi_time_sliced fit on 8 batches of 32: epoch losses %s" % ' '.join('%.4f' % v for v in losses))
    assert np.all(np.isfinite(losses)) and losses[-1] < losses[0]
    with pytest.raises(ValueError):
        speech_model('conv_1d_multi_time_sliced', 8000, num_classes=NC)


def test_checkpoint_round_trip(tmp_path):
    """save -> load -> one more step equals the uninterrupted run bit for bit (weights, moving statistics, RMSprop slots)."""
    from speech_recognition_amd.model import speech_model
    a = speech_model('conv_1d_multi_time_sliced', 16000, num_classes=NC)
    batches = [waveform_batch(16, NC, 200 + i) for i in range(4)]
    for xb, yb in batches[:3]:
        a.train_on_batch(xb, yb)
    path = str(tmp_path / "mts.npz")
    a.save(path)
    b = speech_model('conv_1d_multi_time_sliced', 16000, num_classes=NC)
    b.load_weights(path)
    wa, wb = a.net.get_weights(), b.net.get_weights()
    assert list(wa) == list(wb) and all(np.array_equal(wa[k], wb[k]) for k in wa)
    assert torch.equal(a.net.slots, b.net.slots)
    la, lb = a.train_on_batch(*batches[3]), b.train_on_batch(*batches[3])
    assert la == lb
    assert torch.equal(a.net.params, b.net.params) and torch.equal(a.net.state, b.net.state)
    assert torch.equal(a.net.slots, b.net.slots)
