"""Float64 NumPy oracle of conv_1d_time_sliced (reference model.py:716-772): forward, loss and every gradient, built layer by
layer from oracle/layers.py for the GPU parity tests.

TEST INFRASTRUCTURE ONLY.  overlapping_time_slice_stack(x, 40, 20) SAME -> Conv1D(32 fm, 3, strides=2, VALID, no bias) ->
BatchNormalization -> relu6 -> thirteen blocks DepthwiseConv2D((1, 3), strides=s, no bias) -> Conv1D(F, 1, no bias) ->
BatchNormalization -> relu6 (stride 2: SAME, TensorFlow's padding with the odd sample on the right, over the ACTIVATED input;
stride 1: VALID) -> GlobalAveragePooling1D -> Dropout(.4) -> Dense(256 fm, no bias) -> relu6 -> Dropout(.3) -> Dense(no bias) ->
softmax, keras categorical_crossentropy; oracle/layers.py's counter-based dropout masks (layer ids 1 and 2), as on the device.

`relu_masks` hands the device's own ReLU6 decisions to the backward pass ({BatchNormalization number 1..14: mask, 'hidden':
mask}); `mutate` names a deliberately wrong variant for the negative controls:
  'pad_left'       SAME padding with the odd sample on the LEFT (where the total padding is odd: the even-length inputs)
  'reversed_taps'  the depthwise kernels applied back to front
"""
from collections import OrderedDict

import numpy as np

from oracle.layers import (bn_infer_fwd, bn_train_bwd, bn_train_fwd, cce_fwd_bwd, conv1d_bwd, conv1d_fwd, dropout_key, dropout_mask,
                           dwconv_bwd, dwconv_fwd, frame_same, pw_bwd, pw_fwd, relu6, relu6_mask, same_pad, softmax, softmax_bwd)

# (stride, filters / filter_mult) of the thirteen blocks; the expected lengths behind the first convolution and each block
SPEC = [(1, 64), (2, 128), (1, 128), (2, 192), (1, 192), (2, 256), (1, 256), (2, 320), (1, 320), (2, 384), (1, 384), (2, 512),
        (1, 512)]
LENGTHS = {16000: [399, 397, 199, 197, 99, 97, 49, 47, 24, 22, 11, 9, 5, 3], 12000: [299, 297, 149, 147, 74, 72, 36, 34, 17, 15, 8, 6, 3, 1]}
FRAME, HOP, TAPS, STRIDE = 40, 20, 3, 2
KEEP1, KEEP2 = 0.6, 0.7   # Dropout(0.4), Dropout(0.3)


def glorot(rng, shape, fan_in, fan_out):
    lim = np.sqrt(6.0 / (fan_in + fan_out))
    return rng.uniform(-lim, lim, size=shape).astype(np.float32)


def block_pad(L, stride, odd_left=False):
    """(pad_l, pad_r) of a 3-tap depthwise layer: stride 2 SAME, stride 1 VALID"""
    if stride == 1:
        return 0, 0
    _, pl, pr = same_pad(L, 3, 2)
    return (pr, pl) if odd_left else (pl, pr)


class TimeSlicedNet(object):
    """conv_1d_time_sliced; input [B, input_size] raw samples."""

    def __init__(self, num_classes=12, filter_mult=1, input_size=16000, seed=1234):
        rng = np.random.RandomState(seed)
        fm = filter_mult
        self.nc, self.fm, self.input_size = num_classes, fm, input_size
        P, S = OrderedDict(), OrderedDict()

        def add_bn(n, C):
            base = 'batch_normalization_%d/' % n
            P[base + 'gamma'] = np.ones(C, np.float32)
            P[base + 'beta'] = np.zeros(C, np.float32)
            S[base + 'moving_mean'] = np.zeros(C, np.float32)
            S[base + 'moving_variance'] = np.ones(C, np.float32)

        self.C1 = 32 * fm
        P['conv1d_1/kernel'] = glorot(rng, (TAPS, FRAME, self.C1), TAPS * FRAME, TAPS * self.C1)
        add_bn(1, self.C1)
        frames = same_pad(input_size, FRAME, HOP)[0]
        L, C = (frames - TAPS) // STRIDE + 1, self.C1
        self.L1 = L
        self.blocks = []
        for i, (s, F) in enumerate(SPEC):
            F *= fm
            P['depthwise_conv2d_%d/depthwise_kernel' % (i + 1)] = glorot(rng, (1, 3, C, 1), 3 * C, 3)
            P['conv1d_%d/kernel' % (i + 2)] = glorot(rng, (1, C, F), C, F)
            add_bn(i + 2, F)
            pl, pr = block_pad(L, s)
            Lout = (L + pl + pr - 3) // s + 1
            assert Lout >= 1, "input_size %d: block %d keeps no row" % (input_size, i)
            self.blocks.append({'dw': i + 1, 'bn': i + 2, 's': s, 'C': C, 'F': F, 'L': L, 'Lout': Lout})
            L, C = Lout, F
        self.T, self.C, self.H = L, C, 256 * fm
        P['dense_1/kernel'] = glorot(rng, (C, self.H), C, self.H)
        P['dense_2/kernel'] = glorot(rng, (self.H, num_classes), self.H, num_classes)
        self.l2_names = [k for k in P if k.endswith('depthwise_kernel') or k.startswith('conv1d_')] + ['dense_2/kernel']
        self.params, self.state = P, S

    def lengths(self):
        return [self.L1] + [b['Lout'] for b in self.blocks]

    def count_params(self):
        return sum(v.size for v in self.params.values()) + sum(v.size for v in self.state.values())

    def _p(self, name):
        return self.params[name].astype(np.float64)

    def _taps(self, blk, mutate):
        w = self._p('depthwise_conv2d_%d/depthwise_kernel' % blk['dw'])[0, :, :, 0]
        return w[::-1] if mutate == 'reversed_taps' else w

    def _bn(self, n, y, training, cache):
        ga, be = self._p('batch_normalization_%d/gamma' % n), self._p('batch_normalization_%d/beta' % n)
        if training:
            pre, st = bn_train_fwd(y, ga, be)
        else:
            st = None
            pre = bn_infer_fwd(y, ga, be, self.state['batch_normalization_%d/moving_mean' % n].astype(np.float64),
                               self.state['batch_normalization_%d/moving_variance' % n].astype(np.float64))
        if cache is not None:
            cache['y%d' % n], cache['st%d' % n] = y, st
            if training:
                cache['batch_stats'][n] = (st[0], st[1])
        return relu6(pre)

    def forward(self, x, training=False, seed=0, step=0, cache=None, drop_offset=0, mutate=None):
        B = x.shape[0]
        if cache is not None:
            cache['batch_stats'] = {}
        F = frame_same(x.astype(np.float64), FRAME, HOP)
        y, cols = conv1d_fwd(F, self._p('conv1d_1/kernel'), stride=STRIDE)
        if cache is not None:
            cache['cols1'], cache['frames_shape'] = cols, F.shape
        a = self._bn(1, y, training, cache)
        for blk in self.blocks:
            pad = block_pad(blk['L'], blk['s'], odd_left=(mutate == 'pad_left'))
            z = dwconv_fwd(a, self._taps(blk, mutate), blk['s'], pad)
            assert z.shape[1] == blk['Lout']
            y = pw_fwd(z, self._p('conv1d_%d/kernel' % blk['bn'])[0])
            if cache is not None:
                cache['a%d' % blk['bn']], cache['z%d' % blk['bn']] = a, z
            a = self._bn(blk['bn'], y, training, cache)
        feat = a.mean(axis=1)
        keep1 = keep2 = None
        fd = feat
        if training:
            keep1 = dropout_mask(dropout_key(seed, step, 1), B * self.C, KEEP1, offset=drop_offset * self.C).reshape(B, self.C)
            fd = feat * keep1 / KEEP1
        hpre = fd @ self._p('dense_1/kernel')
        h = relu6(hpre)
        if training:
            keep2 = dropout_mask(dropout_key(seed, step, 2), B * self.H, KEEP2, offset=drop_offset * self.H).reshape(B, self.H)
            h = h * keep2 / KEEP2
        p = softmax(h @ self._p('dense_2/kernel'))
        if cache is not None:
            cache.update(feat=feat, fd=fd, hpre=hpre, h=h, keep1=keep1, keep2=keep2, p=p)
        return p

    def loss_and_grads(self, x, y_onehot, seed=0, step=0, drop_offset=0, relu_masks=None, mutate=None):
        """Data loss (batch mean) and its gradients (no L2 term)."""
        cache = {}
        p = self.forward(x, training=True, seed=seed, step=step, cache=cache, drop_offset=drop_offset, mutate=mutate)
        loss, per, dp = cce_fwd_bwd(p, y_onehot.astype(np.float64))
        dl = softmax_bwd(dp, p)
        grads = OrderedDict()
        grads['dense_2/kernel'] = cache['h'].T @ dl
        dh = (dl @ self._p('dense_2/kernel').T) * cache['keep2'] / KEEP2
        hmask = relu_masks['hidden'] if relu_masks is not None and 'hidden' in relu_masks else relu6_mask(cache['hpre'])
        dh = dh * hmask
        grads['dense_1/kernel'] = cache['fd'].T @ dh
        dfeat = (dh @ self._p('dense_1/kernel').T) * cache['keep1'] / KEEP1
        da = np.repeat((dfeat / self.T)[:, None, :], self.T, axis=1)

        def bn_bwd(n, da):
            y, st = cache['y%d' % n], cache['st%d' % n]
            ga = self._p('batch_normalization_%d/gamma' % n)
            if relu_masks is not None and n in relu_masks:
                mask = relu_masks[n]
            else:
                mask = relu6_mask(y * (st[2] * ga) + (self._p('batch_normalization_%d/beta' % n) - st[0] * st[2] * ga))
            dy, dga, dbe = bn_train_bwd(da * mask, y, ga, st)
            grads['batch_normalization_%d/gamma' % n] = dga
            grads['batch_normalization_%d/beta' % n] = dbe
            return dy

        for blk in reversed(self.blocks):
            n = blk['bn']
            dy = bn_bwd(n, da)
            dz, dW = pw_bwd(dy, cache['z%d' % n], self._p('conv1d_%d/kernel' % n)[0])
            grads['conv1d_%d/kernel' % n] = dW[None]
            pad = block_pad(blk['L'], blk['s'], odd_left=(mutate == 'pad_left'))
            da, dw = dwconv_bwd(dz, cache['a%d' % n], self._taps(blk, mutate), blk['s'], pad)
            if mutate == 'reversed_taps':
                dw = dw[::-1]
            grads['depthwise_conv2d_%d/depthwise_kernel' % blk['dw']] = dw[None, :, :, None]
        dy = bn_bwd(1, da)
        _, dW1 = conv1d_bwd(dy, cache['cols1'], self._p('conv1d_1/kernel'), cache['frames_shape'], stride=STRIDE, need_dx=False)
        grads['conv1d_1/kernel'] = dW1
        ordered = OrderedDict((k, grads[k]) for k in self.params)
        return loss, p, ordered, cache
