"""SHA-256 digests of what one library build computes for the eight models whose BatchNorm bookkeeping is csrc/bncols.hip: per
model one predict and one train_fwd_bwd at batch 3, then a second train_fwd_bwd at batch 16, each digest over the raw bytes of
probs, grads, state and metrics (and whether all of them are finite).  Weights come from a fixed NumPy seed, with gammas of both signs and moving statistics off 0 / 1
(tests/net_parity.perturb's idea).  Two builds that agree on every digest compute the same bits; a digest says nothing across
compiler versions, which is why this is a comparison tool and not a test.
--set ladder: the two nets on the shared 3-tap depthwise ladder (csrc/net_dw3ladder.hip) instead - the raw-waveform attention net under
GEMM modes 0, 1 and 2 (modes 0 and 1 also as the split step at blocks 1 and 6, with the gradients that are final between the parts)
and conv_1d_time_sliced under modes 0 and 1.
--set pools: the six models that run the pooling kernels with [2][C] partial rows (csrc/part_rows.h): pool.hip's four, conv_2d_fast
for pool2d.hip and conv_1d_time_sliced for gap.hip.
--set flat_tail: the twelve configs of the five programs on the flat-tail skeleton (FlatTailProgram, csrc/net_internal.h): the eight
models above, conv_1d_learned_spec, conv_1d_top_down and conv_1d_time_sliced at filter_mult 1 / 16000 and filter_mult 2 / 12000.
--set residual: the eight residual-family configs of tests/golden/make_golden_net_tables.py (LmProgram, csrc/net_logmfcc.hip), each under
GEMM modes 0 and 1 (mode 1, the reference schedule, takes the unfused, unpaired branches) and log_mfcc_32 under mode 2 as well.
usage: [KWS_LIB_PATH=other/libkws_hip.so] python3 scripts/step_digests.py [--set bncols|ladder|pools|flat_tail|residual] [--out FILE]"""
import argparse
import hashlib
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np  # noqa: E402
import torch  # noqa: E402

from speech_recognition_amd import _lib  # noqa: E402
from speech_recognition_amd.net import DeviceNet  # noqa: E402

MODELS = [  # (name, kind, input_size)
    ('conv_1d_fast', _lib.KWS_NET_CONV_1D_FAST, 16000),
    ('conv_1d_spec', _lib.KWS_NET_CONV_1D_SPEC, 98 * 257),
    ('conv_1d_time_stacked', _lib.KWS_NET_CONV_1D_TIME_STACKED, 16000),
    ('conv_1d_heavy', _lib.KWS_NET_CONV_1D_HEAVY, 16000),
    ('conv_1d_gru', _lib.KWS_NET_CONV_1D_GRU, 16000),
    ('conv_1d_simple', _lib.KWS_NET_CONV_1D_SIMPLE, 16000),
    ('conv_1d_multi_time_sliced', _lib.KWS_NET_CONV_1D_MULTI_TIME_SLICED, 16000),
    ('inception_d1', _lib.KWS_NET_INCEPTION_D1, 16000),
]
LADDER = [  # (name, kind, filter_mult, input_size, gemm modes, split step)
    ('ts_attention_fm1_16000', _lib.KWS_NET_TS_ATTENTION, 1, 16000, (0, 1, 2), True),
    ('ts_attention_fm2_16000', _lib.KWS_NET_TS_ATTENTION, 2, 16000, (0, 1, 2), True),   # the first convolution's gathered-GEMM fall-back
    ('ts_attention_fm1_12000', _lib.KWS_NET_TS_ATTENTION, 1, 12000, (0, 1, 2), True),
    ('conv_1d_time_sliced_fm1_16000', _lib.KWS_NET_CONV_1D_TIME_SLICED, 1, 16000, (0, 1), False),
    ('conv_1d_time_sliced_fm2_12000', _lib.KWS_NET_CONV_1D_TIME_SLICED, 2, 12000, (0, 1), False),
]
POOL_NAMES = ('conv_1d_time_stacked', 'conv_1d_heavy', 'conv_1d_multi_time_sliced', 'inception_d1')
POOLS = [m + (1,) for m in MODELS if m[0] in POOL_NAMES] + [  # (name, kind, input_size, filter_mult)
    ('conv_2d_fast', _lib.KWS_NET_CONV_2D_FAST, 3920, 1),
    ('conv_1d_time_sliced', _lib.KWS_NET_CONV_1D_TIME_SLICED, 16000, 1),
]
FLAT_TAIL = [m + (1,) for m in MODELS] + [  # (name, kind, input_size, filter_mult)
    ('conv_1d_learned_spec', _lib.KWS_NET_CONV_1D_LEARNED_SPEC, 16000, 1),
    ('conv_1d_top_down', _lib.KWS_NET_CONV_1D_TOP_DOWN, 16000, 1),
    ('conv_1d_time_sliced_fm1_16000', _lib.KWS_NET_CONV_1D_TIME_SLICED, 16000, 1),
    ('conv_1d_time_sliced_fm2_12000', _lib.KWS_NET_CONV_1D_TIME_SLICED, 12000, 2),
]
RESIDUAL = [  # (name, kind, num_classes, filter_mult, input_size, spectrogram_length, num_features, gemm modes)
    ('log_mfcc_32', _lib.KWS_NET_LOG_MFCC, 32, 1, 98 * 40, 98, 40, (0, 1, 2)),
    ('log_mfcc_65x40', _lib.KWS_NET_LOG_MFCC, 12, 1, 65 * 40, 65, 40, (0, 1)),
    ('spectrogram', _lib.KWS_NET_LOG_MFCC, 12, 1, 98 * 257, 98, 257, (0, 1)),
    ('steffe', _lib.KWS_NET_STEFFE, 12, 1, 16000, 0, 0, (0, 1)),
    ('residual', _lib.KWS_NET_RESIDUAL, 12, 1, 16000, 0, 0, (0, 1)),
    ('residual_x2', _lib.KWS_NET_RESIDUAL, 12, 2, 16000, 0, 0, (0, 1)),
    ('mfcc_and_raw', _lib.KWS_NET_MFCC_AND_RAW, 12, 1, 98 * 40 + 16000, 98, 40, (0, 1)),
    ('xception_with_attention', _lib.KWS_NET_XCEPTION_ATTENTION, 12, 1, 16000, 0, 0, (0, 1)),
]
SPLITS = (1, 6)
NC = 12


def perturbed_weights(net, seed):
    rng = np.random.RandomState(seed)
    w = net.get_weights()
    for k in w:
        shp = w[k].shape
        if k.endswith('gamma'):      # both signs, away from 0
            w[k] = ((1.0 + 0.1 * rng.randn(*shp)) * np.where(rng.rand(*shp) < 0.3, -1.0, 1.0)).astype(np.float32)
        elif k.endswith('beta') or k.endswith('bias'):
            w[k] = (0.1 * rng.randn(*shp)).astype(np.float32)
        elif k.endswith('moving_mean'):
            w[k] = (0.05 * rng.randn(*shp)).astype(np.float32)
        elif k.endswith('moving_variance'):
            w[k] = (1.0 + 0.2 * rng.rand(*shp)).astype(np.float32)
    return w


def sha(t):
    return hashlib.sha256(t.detach().cpu().numpy().tobytes()).hexdigest()


def digests(net, probs):
    torch.cuda.synchronize()
    finite = all(bool(torch.isfinite(t).all()) for t in (probs, net.grads, net.state, net.metrics))
    return {'probs': sha(probs), 'grads': sha(net.grads), 'state': sha(net.state), 'metrics': sha(net.metrics), 'finite': finite}


def batch(B, input_size, seed, nc=NC):
    rng = np.random.RandomState(seed)
    x = (rng.randn(B, input_size) * 0.0774).astype(np.float32)
    y = np.eye(nc, dtype=np.float32)[rng.randint(0, nc, B)]
    return torch.from_numpy(x).cuda(), torch.from_numpy(y).cuda()


def model_digests(name, kind, input_size, filter_mult=1, gemm_mode=0, split=False, nc=NC, spectrogram_length=0, num_features=0):
    net = DeviceNet(kind, nc, filter_mult=filter_mult, input_size=input_size, spectrogram_length=spectrogram_length,
                    num_features=num_features, seed=1234, gemm_mode=gemm_mode)
    net.set_weights(perturbed_weights(net, 99))
    out = {}
    x, y = batch(3, input_size, 7, nc)
    out['predict_b3'] = digests(net, net.predict(x))
    out['train_b3'] = digests(net, net.train_fwd_bwd(x, y, seed=5, step=1))
    x, y = batch(16, input_size, 8, nc)
    out['train_b16'] = digests(net, net.train_fwd_bwd(x, y, seed=5, step=2))
    if split:
        x, y = batch(3, input_size, 9)
        for k, sb in enumerate(SPLITS):
            net.train_fwd_bwd_part(1, sb, x, y, seed=5, step=3 + k)
            torch.cuda.synchronize()
            ready = sha(net.grads[net.grad_ready_offset(sb):])
            out['split%d_b3' % sb] = dict(digests(net, net.train_fwd_bwd_part(2, sb, x, y, seed=5, step=3 + k)), ready_grads=ready)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--out', default=None)
    ap.add_argument('--set', default='bncols', choices=('bncols', 'ladder', 'pools', 'flat_tail', 'residual'))
    a = ap.parse_args()
    torch.cuda.set_device(0)
    if a.set == 'ladder':
        res = dict(('%s_mode%d' % (name, m), model_digests(name, kind, size, fm, m, split and m != 2))
                   for name, kind, fm, size, modes, split in LADDER for m in modes)
    elif a.set == 'residual':
        res = dict(('%s_mode%d' % (name, m), model_digests(name, kind, size, fm, m, nc=nc, spectrogram_length=T, num_features=F))
                   for name, kind, nc, fm, size, T, F, modes in RESIDUAL for m in modes)
    elif a.set in ('pools', 'flat_tail'):
        res = dict((name, model_digests(name, kind, size, fm)) for name, kind, size, fm in (POOLS if a.set == 'pools' else FLAT_TAIL))
    else:
        res = dict((name, model_digests(name, kind, size)) for name, kind, size in MODELS)
    text = json.dumps(res, indent=1, sort_keys=True)
    print(text)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, 'w') as f:
            f.write(text + '\n')


if __name__ == '__main__':
    main()
