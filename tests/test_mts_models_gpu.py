"""GPU parity of the conv_1d_multi_time_sliced network program (KWS_NET_CONV_1D_MULTI_TIME_SLICED, csrc/net_mts.hip) against the
float64 oracle tests/mts_oracle.py on the harness of tests/net_parity.py: the device's ReLU6 and pool arg-max decisions are read
back (debug views 0 and 2, blocks in creation order) and handed to the oracle's backward pass.  A third of the BatchNorm scales is
negative.

Bars: net_parity.FAMILY_BARS - predict 2e-5, train probabilities 5e-5, loss 1e-4, gradients 2e-4 of the tensor's maximum,
moving statistics atol 5e-6 / rtol 1e-5; class indices and the correct-count exact.  This net is twice as deep as any sibling and
its last BatchNorms see only B rows, so the oracle net was first run in float32 on the CPU (torch, tests/mts_torch.py, on its own
decisions) against its float64 self with these weights and batches: batch 8 - probabilities 8.8e-7, loss 4.9e-7, worst gradient
7.7e-6 of its tensor's maximum; batch 64 - probabilities 1.7e-6, loss 2.8e-7, worst gradient 7.7e-6.  Every figure is under half
the sibling bar, so no bar is widened."""
import numpy as np
import pytest
import torch

import net_parity as NP
from speech_recognition_amd import _lib
from mts_oracle import MtsNet

pytestmark = pytest.mark.gpu

BARS = NP.FAMILY_BARS
NC = 12


def _pair(zero=None):
    ora = MtsNet(num_classes=NC)
    NP.perturb(ora, 5, negative_fraction=0.33, beta=(0.3, 0.2), bias=0.05)
    if zero is not None:
        ora.params[zero] = np.zeros_like(ora.params[zero])
    return NP.device_pair(ora, _lib.KWS_NET_CONV_1D_MULTI_TIME_SLICED, NC, input_size=16000)


def _step(ora, net, B, batch_seed, seed=77, step=2, row_offset=0):
    """One device step and what the oracle needs to repeat it on the device's ReLU6 gates and pool winners"""
    x, y = NP.waveform_batch(B, NC, batch_seed)
    dev = NP.device_step(net, x, y, seed, step, row_offset)
    masks, inds = NP.gates_and_winners(net, B, [(blk['idx'], blk['Lout'], blk['F'], blk['pool'] and (blk['pool']['Lp'], blk['pool']['pad_l']))
                                                for blk in ora.blocks])
    return dev, y, (x.astype(np.float64), y.astype(np.float64)), dict(seed=seed, step=step, relu_masks=masks, pool_ind=inds)


@pytest.fixture(scope='module')
def step8():
    """One device step at batch 8, the device's decisions and the oracle's step on them: shared, left unchanged."""
    ora, net = _pair()
    dev, y, xy, kw = _step(ora, net, 8, 8)
    return {'ora': ora, 'dev': dev, 'y': y, 'xy': xy, 'kw': kw, 'ref': ora.loss_and_grads(*xy, **kw)}


def test_tensor_table_matches_oracle():
    NP.check_tensor_table(*_pair(), shapes=True)


def test_predict_matches_oracle():
    ora, net = _pair()
    x, _ = NP.waveform_batch(5, NC, 1)
    p = net.predict(torch.from_numpy(x).cuda()).cpu().numpy()
    NP.check_predict(p, ora.forward(x.astype(np.float64), training=False), BARS, 'conv_1d_multi_time_sliced')


def test_train_fwd_bwd_matches_oracle_batch_8(step8):
    s = step8
    NP.check_train_step(s['dev'], s['y'], s['ref'], s['ora'], BARS, 'conv_1d_multi_time_sliced B=8')


def test_train_fwd_bwd_matches_oracle_batch_64():
    ora, net = _pair()
    dev, y, xy, kw = _step(ora, net, 64, 64)
    NP.check_train_step(dev, y, ora.loss_and_grads(*xy, **kw), ora, BARS, 'conv_1d_multi_time_sliced B=64')


def test_two_consumer_tensors_pass_both_gradients_upstream(step8):
    """The blocks that produce the 28- and 22-step tensors (8 and 20) and what lies upstream of them meet the bar; an oracle that
    drops the tap's gradient at the fork misses it there, and only there."""
    s = step8
    ora, g = s['ora'], s['dev']['grads']
    assert ora.forks == [8, 20]
    errs = NP.grad_errors(g, s['ref'][2])
    up = ['%s_%d/%s' % (a, i, b) for i in (1, 7, 8, 13, 19, 20)
          for a, b in (('conv1d', 'kernel'), ('depthwise_conv2d', 'depthwise_kernel'), ('batch_normalization', 'gamma'))]
    assert max(errs[k] for k in up) < BARS['grad']
    bad_errs = NP.grad_errors(g, ora.loss_and_grads(*s['xy'], mutate='drop_fork', **s['kw'])[2])
    assert min(bad_errs['conv1d_8/kernel'], bad_errs['conv1d_20/kernel']) > NP.MUTATED_ORACLE_BAR
    assert max(bad_errs[k] for k in bad_errs
               if k.split('/')[0].split('_')[-1] in ('10', '11', '12', '22', '23', '24', '32', '33')) < BARS['grad']


def test_pool_padding_side_control(step8):
    """An oracle with the pool's odd padding sample on the wrong side breaks the gradient bar."""
    s = step8
    kw = dict(s['kw'], pool_ind=None)
    bad = s['ora'].loss_and_grads(*s['xy'], mutate='pool_pad_side', **kw)[2]
    assert max(NP.grad_errors(s['dev']['grads'], bad).values()) > NP.MUTATED_ORACLE_BAR


def test_concatenation_keeps_the_other_ends_apart():
    """conv1d_21's kernel (branch end xs5a) zeroed in both nets: the other four ends' gradients stay within the bar, and nothing
    flows back through the zeroed end's pointwise layer."""
    ora, net = _pair(zero='conv1d_21/kernel')
    dev, _, xy, kw = _step(ora, net, 8, 8)
    g = dev['grads']
    errs = NP.grad_errors(g, ora.loss_and_grads(*xy, **kw)[2])
    for end in (9, 12, 24, 31):
        for name in ('conv1d_%d/kernel' % end, 'depthwise_conv2d_%d/depthwise_kernel' % end, 'batch_normalization_%d/gamma' % end):
            assert errs[name] < BARS['grad'], (name, errs[name])
            assert np.abs(g[name]).max() > 0
    assert max(errs.values()) < BARS['grad']
    assert not g['depthwise_conv2d_21/depthwise_kernel'].any()


def test_train_step_is_bit_reproducible():
    ora, net = _pair()
    NP.assert_bit_reproducible(net, *NP.waveform_batch(16, NC, 3))


def test_data_parallel_shard_uses_the_global_dropout_rows():
    ora, net = _pair()
    dev, _, xy, kw = _step(ora, net, 4, 21, seed=5, step=3, row_offset=37)
    NP.check_shard(dev, ora.loss_and_grads(*xy, drop_offset=37, **kw), BARS)


def test_speech_model_fits():
    from speech_recognition_amd.keras_api import RMSprop
    from speech_recognition_amd.model import ACCELERATED, speech_model
    assert 'conv_1d_multi_time_sliced' in ACCELERATED
    model = speech_model('conv_1d_multi_time_sliced', 16000, num_classes=NC)
    assert model.name == 'conv_1d_multi_time_sliced' and model.loss == 'cce'
    assert isinstance(model.optimizer, RMSprop) and abs(float(model.optimizer.lr) - 3e-3) < 1e-9
    batches = [NP.waveform_batch(32, NC, 100 + i) for i in range(8)]
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
    NP.check_checkpoint_round_trip(lambda: speech_model('conv_1d_multi_time_sliced', 16000, num_classes=NC),
                                   [NP.waveform_batch(16, NC, 200 + i) for i in range(4)], str(tmp_path / "mts.npz"), slots=('slots',))
