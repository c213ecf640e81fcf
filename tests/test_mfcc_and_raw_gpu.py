"""GPU parity of the conv_1d_mfcc_and_raw network program (reference model.py:1563-1660) against
oracle/net.py:MfccAndRawNet, and the model on the generator's 'mfcc_and_raw' output."""
import numpy as np
import pytest
import torch

from oracle import layers as OL
from oracle.net import MfccAndRawNet
from speech_recognition_amd import _lib
from speech_recognition_amd.net import DeviceNet

from net_parity import check_residual_step, perturb, relu_masks

pytestmark = pytest.mark.gpu
T, F, LRAW = 98, 60, 16000


def _pair(nc=12, seed=5):
    ora = MfccAndRawNet(num_classes=nc, spectrogram_length=T, num_features=F, raw_size=LRAW, dtype=np.float64)
    perturb(ora, seed)
    net = DeviceNet(_lib.KWS_NET_MFCC_AND_RAW, nc, input_size=T * F + LRAW, spectrogram_length=T, num_features=F)
    net.set_weights(dict(ora.params, **ora.state))
    return ora, net


def _batch(B, nc, seed):
    rng = np.random.RandomState(seed)
    lab = rng.randint(0, nc, B)
    t = np.arange(LRAW) / 16000.0
    raw = rng.randn(B, LRAW) * 0.0774 + 0.05 * np.sin(2 * np.pi * 200.0 * (1 + lab)[:, None] * t[None, :])
    mf = rng.randn(B, T, F) * 2.0 - 0.7 + 0.5 * np.sin(np.arange(F)[None, None, :] * (1 + lab)[:, None, None] * 0.1)
    return mf.reshape(B, -1).astype(np.float32), raw.astype(np.float32), np.eye(nc, dtype=np.float32)[lab]


def _decisions(net, ora, B):
    shapes = {ora.first_m[1]: (B, ora.L0, ora.Cm), ora.first_r[1]: (B, ora.L0, ora.Cr)}
    pools = {}
    for i, blk in enumerate(ora.blocks):
        shapes[blk['bn1']] = (B, blk['Lin'], blk['nf'])
        shapes[blk['bn2']] = (B, blk['Lin'], blk['nf'])
        pools[i] = blk['bn2']
    masks, pre_of = relu_masks(net, B, shapes)
    args = {}
    for i, idx in pools.items():
        blk = ora.blocks[i]
        a = np.minimum(np.maximum(pre_of[idx], np.float32(0)), np.float32(6))
        Lout, pl, pr = OL.same_pad(blk['Lin'], 3, blk['stride'])
        ap = np.pad(a, [[0, 0], [pl, pr], [0, 0]], constant_values=-np.inf)
        win = np.stack([ap[:, j:j + blk['stride'] * Lout:blk['stride'], :] for j in range(3)], axis=2)
        args[i] = win.argmax(axis=2)
    return masks, args


def test_tensor_table_and_predict_match_oracle():
    ora, net = _pair()
    assert [s.name for s in net.tensors.values() if not s.is_state] == list(ora.params.keys())
    for k, v in list(ora.params.items()) + list(ora.state.items()):
        assert net.tensors[k].shape == v.shape, k
    mf, raw, _ = _batch(5, 12, 1)
    x = torch.from_numpy(np.concatenate([mf, raw], axis=1)).cuda()
    p = net.predict(x).cpu().numpy()
    ref = ora.forward([mf.astype(np.float64), raw.astype(np.float64)], training=False)
    assert np.abs(p - ref).max() < 2e-5
    assert np.array_equal(p.argmax(1), ref.argmax(1))


@pytest.mark.parametrize("B", [3, 9])
def test_train_fwd_bwd_matches_oracle(B):
    ora, net = _pair()
    mf, raw, y = _batch(B, 12, B)
    x = torch.from_numpy(np.concatenate([mf, raw], axis=1)).cuda()
    probs = net.train_fwd_bwd(x, torch.from_numpy(y).cuda(), seed=77, step=2)
    torch.cuda.synchronize()
    masks, args = _decisions(net, ora, B)
    ref = ora.loss_and_grads([mf.astype(np.float64), raw.astype(np.float64)], y.astype(np.float64),
                             seed=77, step=2, relu_masks=masks, pool_args=args)
    # the correct count and the moving means: the bars of the other three residual-family files (same native program)
    check_residual_step(ora, net, probs, y, ref, probs_atol=5e-5, loss_atol=1e-4, grad_rtol=2e-4,
               moving_mean_atol=5e-6)


def test_model_on_the_mfcc_and_raw_generator(repo_root):
    """train.py-style: AudioProcessor(output_representation='mfcc_and_raw') -> data_gen -> speech_model(
    'conv_1d_mfcc_and_raw', fingerprint_size, **model_settings) -> train_on_batch([mfcc, raw], y)."""
    import sys
    sys.path.insert(0, repo_root)
    import bench
    from speech_recognition_amd.input_data import AudioProcessor, prepare_words_list
    from speech_recognition_amd.model import prepare_model_settings, speech_model
    from speech_recognition_amd.utils import data_gen
    dev = torch.device("cuda", 0)
    settings = prepare_model_settings(label_count=len(prepare_words_list(bench.WANTED)), sample_rate=16000,
                                      clip_duration_ms=1000, window_size_ms=30.0, window_stride_ms=10.0,
                                      dct_coefficient_count=80, num_log_mel_features=60,
                                      output_representation='mfcc_and_raw')
    proc = AudioProcessor(bench.build_synthetic(dev, 8192, seed=59185), 13.0, 60.0, bench.WANTED, 10.0, 0.0, settings,
                          output_representation='mfcc_and_raw', device=dev)
    np.random.seed(1234)
    gen = data_gen(proc, None, batch_size=64, mode='training')
    model = speech_model('conv_1d_mfcc_and_raw', settings['fingerprint_size'], num_classes=settings['label_count'],
                         **settings)
    assert model.name == 'conv_1d_mfcc_and_raw' and model.loss == 'cce'
    losses = []
    for _ in range(12):
        X, y = next(gen)
        assert isinstance(X, list) and len(X) == 2
        losses.append(float(model.train_on_batch(X, y)[0]))
    assert np.all(np.isfinite(losses)) and np.mean(losses[-3:]) < np.mean(losses[:3])
    p = model.predict_on_batch(X)
    assert p.shape == (64, settings['label_count']) and np.allclose(p.sum(1), 1.0, atol=1e-4)
