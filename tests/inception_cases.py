"""Weights and batches shared by the inception_d1 tests (CPU float32-against-float64 run and GPU parity): the same nets and
clips on both sides, so that the figures in test_inception_models_gpu.py's docstring are those of the GPU cases."""
import numpy as np

from inception_oracle import InceptionD1Net
from net_parity import perturb, waveform_batch

NC = 12
TRAIN_BATCHES = (3, 16)
PREDICT_BATCH = 5
SEED, STEP = 77, 2


def perturbed(dtype=np.float64, nc=NC, seed=5):
    """About a third of the BatchNorm scales negative, shifts that make relu6(shift) != 0, moving statistics off their
    initial values."""
    ora = InceptionD1Net(num_classes=nc, dtype=dtype)
    perturb(ora, seed, negative_fraction=0.33, beta=(0.3, 0.2), bias=0.05)
    return ora


def batch(B, nc=NC, seed=None):
    return waveform_batch(B, nc, B if seed is None else seed)


def decisions_of(ora, cache):
    """ReLU6 gates and pool winners of a cached oracle run, in the form loss_and_grads takes them."""
    masks = {c['idx']: (cache[c['idx']]['pre'] > 0) & (cache[c['idx']]['pre'] <= 6) for c in ora.convs}
    inds = {c['idx']: cache[c['idx']]['ind'] for c in ora.convs if c['pool']}
    inds.update({'mixed%d' % r['id']: cache['mixed%d' % r['id']] for r in ora.blocks if r['kind'] == 'red'})
    return masks, inds
