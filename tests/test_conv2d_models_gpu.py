"""GPU parity of the two 2-D network programs (KWS_NET_CONV_2D_MOBILE / KWS_NET_CONV_2D_FAST, csrc/net_conv2d.hip) against the
float64 oracle tests/conv2d_oracle.py on the harness of tests/net_parity.py: the device's activation gates and max-pool winners
are read back (debug views 0 and 2: every Conv2D's raw output and its BatchNorm table) and handed to the oracle's backward
pass.  About a third of the BatchNorm scales is negative; every bias, the convolutions' included, is non-zero.

Bars: net_parity.FAMILY_BARS - predict 2e-5, train probabilities 5e-5, loss 1e-4, gradients 2e-4 of the tensor's maximum, moving
statistics atol 5e-6 / rtol 1e-5; class indices and the correct-count exact.  The convolution biases stand in front of a
BatchNormalization, so the oracle's gradient for them is zero up to rounding and the device writes exact zeros: they are held to the
absolute bar of conv2d_cases.bias_errors (16 float32 roundings of the terms that cancel).  The oracle nets were first run in float32
on the CPU (NumPy, column sums in float64 as the device adds them; on the float64 run's gates and winners;
tests/conv2d_cases.py holds the weights and batches of both sides; test_conv2d_cpu.py repeats the run) against their float64
selves:
  conv_2d_mobile  predict, batch 5: probabilities 8.1e-8
                  train, batch 3:   probabilities 1.3e-7, loss 7.4e-8, worst gradient 1.2e-6 of its tensor's maximum
                                    (batch_normalization_6/gamma), worst bias gradient 0.20 of its bar
                  train, batch 16:  probabilities 2.6e-7, loss 8.4e-8, worst gradient 1.3e-6 (batch_normalization_1/beta), bias 0.21
  conv_2d_fast    predict, batch 5: probabilities 1.0e-7
                  train, batch 3:   probabilities 2.2e-7, loss 2.7e-7, worst gradient 1.9e-6 (conv2d_3/kernel), bias 0.30
                  train, batch 16:  probabilities 3.3e-7, loss 2.4e-7, worst gradient 1.5e-6 (batch_normalization_1/beta), bias 0.40
Every figure is under half its bar at the first batches chosen."""
import numpy as np
import pytest
import torch

import conv2d_cases as cases
import net_parity as NP
from conv2d_oracle import SGD, pool2_argmax, pool2_fwd
from oracle.layers import sgd_momentum_step
from speech_recognition_amd import _lib

pytestmark = pytest.mark.gpu

BARS = NP.FAMILY_BARS
NC = cases.NC
KIND = {'mobile': _lib.KWS_NET_CONV_2D_MOBILE, 'fast': _lib.KWS_NET_CONV_2D_FAST}


def _pair(kind):
    return NP.device_pair(cases.perturbed(kind), KIND[kind], NC, input_size=3920)


def _decisions(net, ora, B):
    """The device's activation gates and pool winners, from its raw conv outputs and BN tables (float32 fused multiply-add)."""
    masks, inds = {}, {}
    for l in ora.layers:
        n, F = l['idx'], l['F']
        y = net.debug_view(B, 0, n - 1).reshape(B, l['Hout'], l['Wout'], F).astype(np.float64)
        bn = net.debug_view(B, 2, n - 1).reshape(4, F).astype(np.float64)
        pre = (y * bn[0] + bn[1]).astype(np.float32)
        if ora.act == 'relu6':
            masks[n] = (pre > 0) & (pre <= 6)
            a = np.clip(pre, 0, 6)
        else:
            masks[n] = pre > 0
            a = np.maximum(pre, 0)
        if l['pool']:
            inds[n] = pool2_argmax(a.astype(np.float64))
            out = net.debug_view(B, 1, n - 1).reshape(B, l['Ho'], l['Wo'], F)          # the pooled tensor the device kept
            assert np.array_equal(out, pool2_fwd(a, inds[n]))
    return masks, inds


def _step(ora, net, B, batch_seed=None, seed=cases.SEED, step=cases.STEP, row_offset=0):
    """One device step and what the oracle needs to repeat it on the device's gates and winners"""
    x, y = cases.batch(B, seed=batch_seed)
    dev = NP.device_step(net, x, y, seed, step, row_offset)
    masks, inds = _decisions(net, ora, B)
    return dict(dev, ora=ora, x=x, y=y, xy=(x.astype(np.float64), y.astype(np.float64)),
                kw=dict(seed=seed, step=step, relu_masks=masks, pool_ind=inds))


def _check_step(kind, B, d, ora, ref):
    loss, p, grads, cache = ref
    NP.check_train_step(d, d['y'], (loss, p, cases.relative(grads), cache), ora, BARS, "conv_2d_%s B=%d" % (kind, B))
    berrs = cases.bias_errors(d['grads'], grads, cache)
    bworst = max(berrs, key=berrs.get)
    print("conv_2d_%s B=%d: worst bias gradient %s %.3g of its bar" % (kind, B, bworst, berrs[bworst]))
    for k, err in berrs.items():
        assert err < 1.0, (k, err)
        assert not np.asarray(d['grads'][k]).any(), k             # the device's convolution-bias gradients are exact zeros
    # the batch mean the moving mean was held to INCLUDES the convolution bias: without it the moving mean would miss that bar
    w = d['weights']
    b1 = ora.params['conv2d_1/bias'].astype(np.float64)
    old = ora.state['batch_normalization_1/moving_mean'].astype(np.float64)
    no_bias = old - (old - (cache['batch_stats'][1][0] - b1)) * 0.01
    assert np.abs(w['batch_normalization_1/moving_mean'] - no_bias).max() > 1e-4


@pytest.fixture(scope="module", params=cases.KINDS)
def step3(request):
    kind = request.param
    ora, net = _pair(kind)
    d = _step(ora, net, 3)
    d['kind'] = kind
    d['oracle'] = ora.loss_and_grads(*d['xy'], **d['kw'])
    return d


@pytest.mark.parametrize("kind", cases.KINDS)
def test_tensor_table_matches_oracle(kind):
    NP.check_tensor_table(*_pair(kind))


@pytest.mark.parametrize("kind", cases.KINDS)
def test_predict_matches_oracle_and_rows_do_not_see_each_other(kind):
    ora, net = _pair(kind)
    x, _ = cases.batch(cases.PREDICT_BATCH, seed=1)
    p = net.predict(torch.from_numpy(x).cuda()).cpu().numpy()
    NP.check_predict(p, ora.forward(x.astype(np.float64), training=False), BARS, 'conv_2d_' + kind)
    for r in range(cases.PREDICT_BATCH):     # a predict at batch 1 agrees with the same row of the batch of 5
        p1 = net.predict(torch.from_numpy(x[r:r + 1]).cuda()).cpu().numpy()
        assert np.abs(p1[0] - p[r]).max() < 1e-6, r
    # inference runs on moving statistics, where the convolution bias does not cancel: an oracle without it misses the bar
    nb = cases.perturbed(kind)
    for k in nb.params:
        if k.startswith('conv2d_') and k.endswith('bias'):
            nb.params[k] = np.zeros_like(nb.params[k])
    assert np.abs(p - nb.forward(x.astype(np.float64), training=False)).max() > BARS['predict']


def test_train_fwd_bwd_matches_oracle_batch_3(step3):
    _check_step(step3['kind'], 3, step3, step3['ora'], step3['oracle'])


@pytest.mark.parametrize("kind", cases.KINDS)
def test_train_fwd_bwd_matches_oracle_batch_16(kind):
    B = cases.TRAIN_BATCHES[1]
    ora, net = _pair(kind)
    d = _step(ora, net, B)
    _check_step(kind, B, d, ora, ora.loss_and_grads(*d['xy'], **d['kw']))


def test_wrong_padding_oracle_misses_the_gradient_bar(step3):
    """Negative control: against an oracle that puts the odd SAME padding in front, conv_2d_mobile's gradients miss the 2e-4 bar
    (conv_2d_fast's windows are odd at stride 1: its padding is symmetric and the variant is the same function)."""
    bad = step3['ora'].loss_and_grads(*step3['xy'], mutate='pad_front', **step3['kw'])[2]
    worst = max(cases.grad_errors(step3['grads'], bad).values())
    print("conv_2d_%s against the pad_front oracle: worst gradient %.3g" % (step3['kind'], worst))
    assert worst > BARS['grad'] if step3['kind'] == 'mobile' else worst < BARS['grad']


@pytest.mark.parametrize("kind", cases.KINDS)
def test_train_step_is_bit_reproducible(kind):
    ora, net = _pair(kind)
    NP.assert_bit_reproducible(net, *cases.batch(24, seed=3))


@pytest.mark.parametrize("kind", cases.KINDS)
def test_data_parallel_shard_uses_the_global_dropout_rows_and_loss_batch(kind):
    """row_offset indexes every dropout mask by the global row (the oracle's drop_offset); loss_batch divides the loss gradient by
    the global batch (a shard of half the batch: every gradient halves - a power of two, exact but for underflow)."""
    ora, net = _pair(kind)
    B, off = 4, 37
    d = _step(ora, net, B, batch_seed=21, seed=5, step=3, row_offset=off)
    loss, p, grads, cache = ora.loss_and_grads(*d['xy'], drop_offset=off, **d['kw'])
    NP.check_shard(d, (loss, p, cases.relative(grads), cache), BARS)
    if kind == 'mobile':     # the masks of row 0 are not those of row 37: the same oracle without the offset misses the bar
        g0 = ora.loss_and_grads(*d['xy'], drop_offset=0, **d['kw'])[2]
        assert max(cases.grad_errors(d['grads'], g0).values()) > BARS['grad']
    g1 = net.grads.clone()
    net.set_weights(dict(ora.params, **ora.state))
    net.train_fwd_bwd(torch.from_numpy(d['x']).cuda(), torch.from_numpy(d['y']).cuda(), seed=5, step=3, row_offset=off, loss_batch=2 * B)
    np.testing.assert_allclose(2.0 * net.grads.cpu().numpy(), g1.cpu().numpy(), rtol=1e-6, atol=1e-12)


@pytest.mark.parametrize("kind", cases.KINDS)
def test_sgd_steps_move_the_weights_as_the_oracle_says(kind):
    """Model.train_on_batch on a fixed batch: after each of the first two steps the weights are the float64 Keras-2.1.2 SGD rule
    (v' = momentum v - lr g, p' = p + v'; no l2 in these models) applied to the device's own gradient, to the siblings' update bar
    1e-6, and the velocity is what the checkpoint and the data-parallel broadcast carry (net.slots); over twelve steps the loss
    falls."""
    from speech_recognition_amd import keras_api
    from speech_recognition_amd.model import ACCELERATED, speech_model
    name = 'conv_2d_' + kind
    assert name in ACCELERATED
    model = speech_model(name, 3920, num_classes=NC)
    lr, momentum = SGD[kind]
    assert model.name == name and model.loss == 'cce'
    assert isinstance(model.optimizer, keras_api.SGD) and abs(float(model.optimizer.lr) - lr) < 1e-9 and model.optimizer.momentum == momentum
    net = model.net
    assert not net.l2.cpu().numpy().any()
    v = np.zeros(net.n_params)
    x, y = cases.batch(32, seed=100)
    losses = []
    for t in range(1, 13):
        p0 = net.params.cpu().numpy().astype(np.float64)
        losses.append(float(model.train_on_batch(x, y)[0]))
        if t <= 2:
            g = net.grads.cpu().numpy().astype(np.float64)
            ref, v = sgd_momentum_step(p0, g, v, float(np.float32(lr)), momentum)
            got = net.params.cpu().numpy()
            print("sgd step %d: max |w - oracle| = %.3g, max |velocity - oracle| = %.3g, largest move %.3g" %
                  (t, np.abs(got - ref).max(), np.abs(net.slots.cpu().numpy() - v).max(), np.abs(got - p0).max()))
            assert np.abs(got - ref).max() < 1e-6
            assert np.abs(net.slots.cpu().numpy() - v).max() < 1e-6 * max(np.abs(v).max(), 1e-3)
            assert np.abs(got - p0).max() > 1e-6
    print("%s losses on a fixed batch: %s" % (name, ' '.join('%.4f' % q for q in losses)))
    assert np.all(np.isfinite(losses)) and np.mean(losses[-3:]) < np.mean(losses[:3])
    with pytest.raises(ValueError):
        speech_model(name, 16000, num_classes=NC)
    with pytest.raises(NotImplementedError):
        speech_model('conv_2d', 3920, num_classes=NC)


def test_checkpoint_round_trip_carries_the_velocity(tmp_path):
    """save -> load -> one more step equals the uninterrupted run bit for bit (weights, moving statistics, the SGD velocity)."""
    from speech_recognition_amd.model import speech_model
    NP.check_checkpoint_round_trip(lambda: speech_model('conv_2d_mobile', 3920, num_classes=NC),
                                   [cases.batch(8, seed=200 + i) for i in range(3)], str(tmp_path / "conv2d.npz"), slots=('slots',))


def test_conv_2d_mobile_on_the_mfcc_generator(repo_root):
    """The product's own objects end to end: AudioProcessor(output_representation='mfcc') -> data_gen -> speech_model('conv_2d_mobile',
    3920, 12) -> two train_on_batch calls on the same batch (the loss is finite and falls) and a predict.

    train_on_batch reports the loss of the weights it was called with, under that step's dropout draw.  The model has five Dropout
    layers and its first SGD step (lr 1e-3, zero velocity) lowers the loss by about 1e-3 |g|^2, less than what a fresh draw of the
    masks moves it by at batch 64: with each call on its own draw the two losses were 2.51081 -> 2.55654 on the card, and the twelve
    fixed-batch steps of test_sgd_steps_move_the_weights_as_the_oracle_says wobble by +-0.07 on their way down.  So the second call
    repeats the first call's draw as well as its batch (the step counter that keys the masks is set back): then the two losses are
    one function at two points, and a descent step has to lower it."""
    gen, model, settings = NP.generator_model('conv_2d_mobile', 'mfcc', repo_root, dct=40, mel=40, settings_to_model=False)
    assert settings['fingerprint_size'] == 3920 and settings['label_count'] == 12
    X, y = next(gen)
    assert np.asarray(X).shape == (64, 3920)
    step0 = model._step
    l1 = float(model.train_on_batch(X, y)[0])
    assert model._step == step0 + 1
    model._step = step0                                           # the same dropout masks for the repeated batch
    l2 = float(model.train_on_batch(X, y)[0])
    print("conv_2d_mobile on mfcc features: loss %.5f -> %.5f" % (l1, l2))
    assert np.isfinite(l1) and np.isfinite(l2) and l2 < l1
    p = np.asarray(model.predict(X))
    assert p.shape == (64, 12) and np.isfinite(p).all() and np.abs(p.sum(1) - 1).max() < 1e-5


@pytest.mark.parametrize("training", [0, 1])
@pytest.mark.parametrize("kind", cases.KINDS)
def test_workspace_bytes_is_honoured_and_one_byte_less_is_refused(kind, training):
    """A step in a workspace of exactly workspace_bytes leaves the guard bands around it alone; one byte less is KWS_E_WORKSPACE
    with a message, and nothing runs."""
    ora, net = _pair(kind)
    NP.check_workspace_refusal(net, *cases.batch(3), training=training)
