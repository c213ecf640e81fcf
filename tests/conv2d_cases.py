"""Weights, batches and kernel cases shared by the 2-D family's tests (CPU float32-against-float64 runs and GPU parity): the same
nets, clips and shapes on both sides, so that the figures in the GPU tests' docstrings are those of the GPU cases."""
import numpy as np

from conv2d_oracle import Conv2dNet, axis_geom
import net_parity
from net_parity import perturb

NC = 12
KINDS = ('mobile', 'fast')
TRAIN_BATCHES = (3, 16)
PREDICT_BATCH = 5
SEED, STEP = 77, 2


def perturbed(kind, dtype=np.float64, nc=NC, seed=5):
    """About a third of the BatchNorm scales negative, shifts that make act(shift) != 0, non-zero convolution and dense biases,
    moving statistics off their initial values."""
    ora = Conv2dNet(kind, num_classes=nc, dtype=dtype)
    perturb(ora, seed, negative_fraction=0.33, beta=(0.3, 0.2), bias=0.05)
    assert all(np.abs(v).max() > 0 for k, v in ora.params.items() if k.endswith('bias'))
    return ora


def batch(B, nc=NC, seed=None):
    """mfcc-like images [B, 98 * 40]: a class-dependent ripple under noise wide enough that Preprocess clips a few values"""
    rng = np.random.RandomState(B if seed is None else seed)
    lab = rng.randint(0, nc, B)
    tt, ff = np.meshgrid(np.arange(98) / 98.0, np.arange(40) / 40.0, indexing='ij')
    ripple = np.sin(2 * np.pi * ((1 + lab)[:, None, None] * tt[None] + (1 + lab % 5)[:, None, None] * ff[None]))
    x = rng.randn(B, 98, 40) * 12.0 + 6.0 * ripple - 0.8
    return x.reshape(B, 3920).astype(np.float32), np.eye(nc, dtype=np.float32)[lab]


def relative(ref):
    """The reference gradients held to the relative bar: all but the convolution biases, whose reference is zero up to rounding
    and which are held to an absolute bar instead (bias_errors)"""
    return {k: r for k, r in ref.items() if not (k.startswith('conv2d_') and k.endswith('bias'))}


def grad_errors(g, ref):
    """net_parity.grad_errors over relative(ref)"""
    return net_parity.grad_errors(g, relative(ref))


BIAS_BAR_ROUNDINGS = 16


def bias_errors(g, ref, cache):
    """The convolution biases stand in front of a BatchNormalization: their gradient is the sum over the rows of
    dy = gamma rstd (g - dbeta / n - xhat dgamma / n), which is zero in exact arithmetic, so the bar is absolute.  Its unit is
    one float32 rounding of the terms that cancel, per channel: 2^-24 * |gamma rstd| * sum over the rows of (|g| + |dbeta| / n +
    |xhat| |dgamma| / n) (the oracle's `bias_terms`).  A float32 evaluation rounds each row about ten times on the way (xhat: a
    difference and a product; dgamma / n and dbeta / n; the product with xhat; two differences; gamma rstd and the product with
    it; the sum): the float32 run of the oracle (test_conv2d_cpu.py) measures up to 6.4 such units, and the bar is
    BIAS_BAR_ROUNDINGS = 16 of them, the next power of two over twice that.  -> |g - ref| in units of the bar: a figure below 1
    passes.  The device writes exact zeros, so its figure is the float64 oracle's own rounding."""
    out = {}
    for k, r in ref.items():
        if k.startswith('conv2d_') and k.endswith('bias'):
            n = int(k.split('/')[0].split('_')[1])
            bar = BIAS_BAR_ROUNDINGS * 2.0 ** -24 * np.asarray(cache[n]['bias_terms'], np.float64)
            out[k] = (np.abs(np.asarray(g[k], np.float64) - np.asarray(r, np.float64)) / np.maximum(bar, 1e-300)).max()
    return out


def decisions_of(ora, cache):
    """Gates and pool winners of a cached oracle run, in the form loss_and_grads takes them."""
    from oracle_blocks import act_mask
    masks = {l['idx']: act_mask(cache[l['idx']]['pre'], ora.act) for l in ora.layers}
    inds = {l['idx']: cache[l['idx']]['ind'] for l in ora.layers if l['pool']}
    return masks, inds


# ---- kernel cases: B, (H, W), Cin -> F, (kh, kw), strides, dilation, padding ------------------------------------------------------
def conv_case(B, H, W, Cin, F, kh, kw, s=(1, 1), d=(1, 1), padding='same'):
    Ho, ph = axis_geom(H, kh, s[0], d[0], padding)
    Wo, pw = axis_geom(W, kw, s[1], d[1], padding)
    return dict(B=B, H=H, W=W, Cin=Cin, F=F, kh=kh, kw=kw, s=tuple(s), d=tuple(d), padding=padding, Hout=Ho, Wout=Wo, pads=(ph, pw))


CONV_CASES = [
    conv_case(2, 7, 5, 1, 32, 3, 3, s=(2, 2)),            # Cin = 1, odd sizes, pads (1, 1)
    conv_case(2, 8, 6, 4, 8, 3, 3, s=(2, 2)),             # pads (0, 1): padding at the far edge only
    conv_case(3, 13, 5, 32, 96, 3, 3),                    # M = 195 crosses a 128-row tile inside an image row; 1.5 column tiles
    conv_case(2, 12, 5, 1, 16, 11, 5, d=(2, 1)),          # the window spans more than H
    conv_case(2, 9, 6, 16, 32, 5, 3, d=(2, 1)),           # dilation with wider channels
    conv_case(1, 1, 1, 4, 5, 3, 3),                       # a single pixel
    conv_case(2, 7, 3, 20, 24, 1, 1, s=(2, 2)),           # dX rows nobody reads: exact zeros
    conv_case(2, 9, 8, 8, 8, 3, 3, s=(2, 1)),             # unequal strides
    conv_case(1, 24, 10, 1, 8, 20, 8),                    # even taps: pads (9, 10), (3, 4)
    conv_case(1, 12, 6, 8, 8, 10, 4),                     # conv_2d's second form
    conv_case(2, 8, 7, 6, 10, 3, 3, s=(2, 2), padding='valid'),   # no padding; the last row is read by no window
]
assert CONV_CASES[0]['pads'] == ((1, 1), (1, 1)) and CONV_CASES[1]['pads'] == ((0, 1), (0, 1))
assert CONV_CASES[8]['pads'] == ((9, 10), (3, 4))


def conv_id(c):
    return "B%d_%dx%d_C%d_F%d_k%dx%d_s%d%d_d%d%d_%s" % (c['B'], c['H'], c['W'], c['Cin'], c['F'], c['kh'], c['kw'], c['s'][0], c['s'][1],
                                                        c['d'][0], c['d'][1], c['padding'])


POOL_CASES = [(2, 49, 20, 16), (3, 5, 5, 8), (2, 2, 2, 4), (1, 3, 2, 12)]
