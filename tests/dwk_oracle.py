"""Float64 NumPy oracle of the general depthwise ladder conv_1d_gru (reference model.py:470-512; no recurrent layer): forward,
loss and every gradient, restated layer by layer for the GPU parity tests, and the stand-alone depthwise convolution
`dw_fwd` / `dw_bwd` the kernel tests compare kws_dwconvk_* with.

TEST INFRASTRUCTURE ONLY.  A block is DepthwiseConv2D((1, k), strides=s, SAME or VALID, no bias) -> Conv1D(F, 1, no bias) ->
BatchNormalization -> relu6; SAME padding is TensorFlow's (the odd sample on the right) and pads the ACTIVATED input.  The head
is Flatten -> Dropout(.3) -> Dense(256) -> relu6 -> Dropout(.3) -> Dense -> softmax with oracle/layers.py's counter-based
dropout masks (layer ids 1 and 2), as on the device.

`relu_masks` hands the device's own ReLU6 decisions to the backward pass ({block number 1..6: mask, 'hidden': mask}); `mutate`
names a deliberately wrong variant for the negative controls:
  'pad_left'       SAME padding with the odd sample on the LEFT (pad_l one too large where the total padding is odd)
  'reversed_taps'  the depthwise kernels applied back to front
"""
from collections import OrderedDict

import numpy as np

from oracle.layers import (bn_infer_fwd, bn_train_bwd, bn_train_fwd, cce_fwd_bwd, dropout_key, dropout_mask, relu6, relu6_mask,
                           softmax, softmax_bwd)

# (filters, taps, stride, padding) of the six blocks; the expected (L_in, pad_l, L_out) ladder for 16000 samples
SPEC = [(128, 63, 16, 'same'), (256, 31, 4, 'same'), (384, 15, 4, 'same'), (448, 7, 4, 'same'), (512, 5, 2, 'same'),
        (512, 8, 1, 'valid')]
LADDER = [(16000, 23, 1000), (1000, 13, 250), (250, 6, 63), (63, 2, 16), (16, 1, 8), (8, 0, 1)]
HIDDEN = 256
KEEP = 0.7   # both Dropout(0.3)


def same_geometry(L, k, s, odd_left=False):
    """TensorFlow SAME: output length and left padding (the odd sample goes to the right unless odd_left)."""
    Lout = -(-L // s)
    p = max((Lout - 1) * s + k - L, 0)
    return Lout, (p - p // 2) if odd_left else p // 2


def _padded(a, k, s, pad_l, Lout):
    need = s * (Lout - 1) + k
    pr = max(need - pad_l - a.shape[1], 0)
    return np.pad(a, ((0, 0), (pad_l, pr), (0, 0)))


def dw_fwd(a, w, s, pad_l, Lout):
    """a [B, L, C] (already activated), w [k, C] -> z [B, Lout, C]; zeros outside [0, L)."""
    k = w.shape[0]
    ap = _padded(a, k, s, pad_l, Lout)
    span = s * (Lout - 1) + 1
    z = np.zeros((a.shape[0], Lout, a.shape[2]), np.result_type(a, w))
    for j in range(k):
        z += w[j] * ap[:, j:j + span:s, :]
    return z


def dw_bwd(dz, a, w, s, pad_l):
    """-> (gradient wrt a [B, L, C], gradient wrt w [k, C])."""
    k, Lout, L = w.shape[0], dz.shape[1], a.shape[1]
    ap = _padded(a, k, s, pad_l, Lout)
    span = s * (Lout - 1) + 1
    dap = np.zeros(ap.shape, np.result_type(dz, w))
    dw = np.zeros(w.shape, dap.dtype)
    for j in range(k):
        dap[:, j:j + span:s, :] += w[j] * dz
        dw[j] = (ap[:, j:j + span:s, :] * dz).sum(axis=(0, 1))
    return dap[:, pad_l:pad_l + L, :], dw


def glorot(rng, shape, fan_in, fan_out):
    lim = np.sqrt(6.0 / (fan_in + fan_out))
    return rng.uniform(-lim, lim, size=shape).astype(np.float32)


class DwkNet(object):
    """conv_1d_gru; input [B, 16000] raw samples."""

    def __init__(self, num_classes=12, seed=1234, input_size=16000):
        rng = np.random.RandomState(seed)
        self.nc = num_classes
        P, S = OrderedDict(), OrderedDict()
        self.blocks = []
        L, C = input_size, 1
        for i, (F, k, s, pad) in enumerate(SPEC):
            n = i + 1
            P['depthwise_conv2d_%d/depthwise_kernel' % n] = glorot(rng, (1, k, C, 1), k * C, k)
            P['conv1d_%d/kernel' % n] = glorot(rng, (1, C, F), C, F)
            base = 'batch_normalization_%d/' % n
            P[base + 'gamma'] = np.ones(F, np.float32)
            P[base + 'beta'] = np.zeros(F, np.float32)
            S[base + 'moving_mean'] = np.zeros(F, np.float32)
            S[base + 'moving_variance'] = np.ones(F, np.float32)
            if pad == 'same':
                Lout, pad_l = same_geometry(L, k, s)
            else:
                Lout, pad_l = (L - k) // s + 1, 0
            self.blocks.append({'idx': n, 'k': k, 's': s, 'same': pad == 'same', 'C': C, 'F': F, 'L': L, 'Lout': Lout, 'pad_l': pad_l})
            L, C = Lout, F
        assert L == 1
        self.D = C
        P['dense_1/kernel'] = glorot(rng, (C, HIDDEN), C, HIDDEN)
        P['dense_1/bias'] = np.zeros(HIDDEN, np.float32)
        P['dense_2/kernel'] = glorot(rng, (HIDDEN, num_classes), HIDDEN, num_classes)
        P['dense_2/bias'] = np.zeros(num_classes, np.float32)
        self.l2_names = [k for k in P if k.endswith('depthwise_kernel') or k.startswith('conv1d_')]
        self.params, self.state = P, S

    def count_params(self):
        return sum(v.size for v in self.params.values()) + sum(v.size for v in self.state.values())

    def _p(self, name):
        return self.params[name].astype(np.float64)

    def _taps(self, blk, mutate):
        w = self._p('depthwise_conv2d_%d/depthwise_kernel' % blk['idx'])[0, :, :, 0]
        return w[::-1] if mutate == 'reversed_taps' else w

    def _pad_l(self, blk, mutate):
        if mutate == 'pad_left' and blk['same']:
            return same_geometry(blk['L'], blk['k'], blk['s'], odd_left=True)[1]
        return blk['pad_l']

    def forward(self, x, training=False, seed=0, step=0, cache=None, drop_offset=0, mutate=None):
        B = x.shape[0]
        a = x.astype(np.float64)[:, :, None]
        if cache is not None:
            cache['batch_stats'] = {}
        for blk in self.blocks:
            n = blk['idx']
            z = dw_fwd(a, self._taps(blk, mutate), blk['s'], self._pad_l(blk, mutate), blk['Lout'])
            y = z @ self._p('conv1d_%d/kernel' % n)[0]
            ga, be = self._p('batch_normalization_%d/gamma' % n), self._p('batch_normalization_%d/beta' % n)
            if training:
                pre, st = bn_train_fwd(y, ga, be)
            else:
                st = None
                pre = bn_infer_fwd(y, ga, be, self.state['batch_normalization_%d/moving_mean' % n].astype(np.float64),
                                   self.state['batch_normalization_%d/moving_variance' % n].astype(np.float64))
            if cache is not None:
                cache['a%d' % n], cache['z%d' % n], cache['y%d' % n], cache['st%d' % n] = a, z, y, st
                if training:
                    cache['batch_stats'][n] = (st[0], st[1])
            a = relu6(pre)
        flat = a.reshape(B, self.D)
        keep1 = keep2 = None
        if training:
            keep1 = dropout_mask(dropout_key(seed, step, 1), B * self.D, KEEP, offset=drop_offset * self.D).reshape(B, self.D)
            flat = flat * keep1 / KEEP
        hpre = flat @ self._p('dense_1/kernel') + self._p('dense_1/bias')
        h = relu6(hpre)
        if training:
            keep2 = dropout_mask(dropout_key(seed, step, 2), B * HIDDEN, KEEP, offset=drop_offset * HIDDEN).reshape(B, HIDDEN)
            h = h * keep2 / KEEP
        p = softmax(h @ self._p('dense_2/kernel') + self._p('dense_2/bias'))
        if cache is not None:
            cache.update(flat=flat, hpre=hpre, h=h, keep1=keep1, keep2=keep2, p=p)
        return p

    def loss_and_grads(self, x, y_onehot, seed=0, step=0, drop_offset=0, relu_masks=None, mutate=None):
        """Data loss (batch mean) and its gradients (no L2 term)."""
        cache = {}
        B = x.shape[0]
        p = self.forward(x, training=True, seed=seed, step=step, cache=cache, drop_offset=drop_offset, mutate=mutate)
        loss, per, dp = cce_fwd_bwd(p, y_onehot.astype(np.float64))
        dl = softmax_bwd(dp, p)
        grads = OrderedDict()
        grads['dense_2/kernel'] = cache['h'].T @ dl
        grads['dense_2/bias'] = dl.sum(axis=0)
        dh = (dl @ self._p('dense_2/kernel').T) * cache['keep2'] / KEEP
        hmask = relu_masks['hidden'] if relu_masks is not None and 'hidden' in relu_masks else relu6_mask(cache['hpre'])
        dh = dh * hmask
        grads['dense_1/kernel'] = cache['flat'].T @ dh
        grads['dense_1/bias'] = dh.sum(axis=0)
        da = ((dh @ self._p('dense_1/kernel').T) * cache['keep1'] / KEEP).reshape(B, 1, self.D)
        for blk in reversed(self.blocks):
            n = blk['idx']
            y, st = cache['y%d' % n], cache['st%d' % n]
            ga = self._p('batch_normalization_%d/gamma' % n)
            if relu_masks is not None and n in relu_masks:
                mask = relu_masks[n]
            else:
                mask = relu6_mask(y * (st[2] * ga) + (self._p('batch_normalization_%d/beta' % n) - st[0] * st[2] * ga))
            dy, dga, dbe = bn_train_bwd(da * mask, y, ga, st)
            grads['batch_normalization_%d/gamma' % n] = dga
            grads['batch_normalization_%d/beta' % n] = dbe
            W = self._p('conv1d_%d/kernel' % n)[0]
            z = cache['z%d' % n]
            grads['conv1d_%d/kernel' % n] = (z.reshape(-1, z.shape[2]).T @ dy.reshape(-1, dy.shape[2]))[None]
            dz = dy @ W.T
            da, dw = dw_bwd(dz, cache['a%d' % n], self._taps(blk, mutate), blk['s'], self._pad_l(blk, mutate))
            if mutate == 'reversed_taps':
                dw = dw[::-1]
            grads['depthwise_conv2d_%d/depthwise_kernel' % n] = dw[None, :, :, None]
        ordered = OrderedDict((k, grads[k]) for k in self.params)
        return loss, p, ordered, cache
