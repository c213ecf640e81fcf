"""GPU parity of the steffeNet network program (reference model.py:1663-1726) against
oracle/net.py:SteffeNet - same method as tests/test_logmfcc_gpu.py: the device's discrete decisions (ReLU6 masks,
the positions of the global maxima) are read back and handed to the oracle's backward pass."""
import numpy as np
import pytest
import torch

from oracle.net import SteffeNet
from speech_recognition_amd import _lib
from speech_recognition_amd.net import DeviceNet

from net_parity import check_residual_step, perturb, relu_masks, waveform_batch

pytestmark = pytest.mark.gpu


def _pair(nc=12, seed=5):
    ora = SteffeNet(num_classes=nc, dtype=np.float64)
    perturb(ora, seed)
    net = DeviceNet(_lib.KWS_NET_STEFFE, nc, input_size=16000)
    net.set_weights(dict(ora.params, **ora.state))
    return ora, net


def _batch(B, nc, seed):
    return waveform_batch(B, nc, seed)


def _decisions(net, ora, B):
    shapes = {ora.first[1]: (B, ora.L0, ora.C0), ora.ctx[2]: (B, ora.L0, ora.C0)}
    for blk in ora.blocks:
        shapes[blk['bn1']] = (B, blk['Lout'], blk['nf'])
        shapes[blk['bn2']] = (B, blk['Lout'], blk['nf'])
    masks, _ = relu_masks(net, B, shapes)
    h = net.debug_view(B, 5, 0).reshape(B, ora.T, ora.C)
    ind = (h == h.max(axis=1, keepdims=True)).astype(np.float64)
    return masks, ind


def test_tensor_table_matches_oracle():
    ora, net = _pair()
    assert [s.name for s in net.tensors.values() if not s.is_state] == list(ora.params.keys())
    for k, v in list(ora.params.items()) + list(ora.state.items()):
        assert net.tensors[k].shape == v.shape, k
    assert net.count_params() == ora.count_params()


def test_predict_matches_oracle():
    ora, net = _pair()
    x, _ = _batch(5, 12, 1)
    p = net.predict(torch.from_numpy(x).cuda()).cpu().numpy()
    ref = ora.forward(x.astype(np.float64), training=False)
    assert np.abs(p - ref).max() < 2e-5
    assert np.array_equal(p.argmax(1), ref.argmax(1))


@pytest.mark.parametrize("B", [3, 10])
def test_train_fwd_bwd_matches_oracle(B):
    ora, net = _pair()
    x, y = _batch(B, 12, B)
    probs = net.train_fwd_bwd(torch.from_numpy(x).cuda(), torch.from_numpy(y).cuda(), seed=77, step=2)
    torch.cuda.synchronize()
    masks, ind = _decisions(net, ora, B)
    ref = ora.loss_and_grads(x.astype(np.float64), y.astype(np.float64), seed=77, step=2,
                             relu_masks=masks, pool_ind=ind)
    check_residual_step(ora, net, probs, y, ref, probs_atol=5e-5, loss_atol=1e-4, grad_rtol=2e-4,
               moving_mean_atol=5e-6)


def test_speech_model_trains():
    from speech_recognition_amd.model import speech_model
    model = speech_model('steffeNet', 16000, num_classes=12)
    assert model.name == 'steffeNet' and model.loss == 'smooth_cce'
    losses = []
    x, y = _batch(32, 12, 100)
    for i in range(12):
        losses.append(float(model.train_on_batch(x, y)[0]))
    # RMSprop(1e-3) with Dropout(.5) on a 1536-wide net is noisy from step to step; the fit of a fixed batch is not
    assert np.all(np.isfinite(losses)) and min(losses[2:]) < 0.7 * losses[0]
