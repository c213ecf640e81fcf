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
import numpy as np

from oracle.layers import conv1d_bwd, conv1d_fwd, frame_same, pw_bwd, pw_fwd, same_pad
from oracle_blocks import OracleNet, act_fwd, act_mask, dw_bwd, dw_fwd, same_geometry

# (stride, filters / filter_mult) of the thirteen blocks; the expected lengths behind the first convolution and each block
SPEC = [(1, 64), (2, 128), (1, 128), (2, 192), (1, 192), (2, 256), (1, 256), (2, 320), (1, 320), (2, 384), (1, 384), (2, 512),
        (1, 512)]
LENGTHS = {16000: [399, 397, 199, 197, 99, 97, 49, 47, 24, 22, 11, 9, 5, 3], 12000: [299, 297, 149, 147, 74, 72, 36, 34, 17, 15, 8, 6, 3, 1]}
FRAME, HOP, TAPS, STRIDE = 40, 20, 3, 2
KEEP1, KEEP2 = 0.6, 0.7   # Dropout(0.4), Dropout(0.3)


def block_pad(L, stride, odd_left=False):
    """(pad_l, pad_r) of a 3-tap depthwise layer: stride 2 SAME, stride 1 VALID"""
    return (0, 0) if stride == 1 else same_geometry(L, 3, 2, odd_left=odd_left)[1:]


class TimeSlicedNet(OracleNet):
    """conv_1d_time_sliced; input [B, input_size] raw samples."""

    def __init__(self, num_classes=12, filter_mult=1, input_size=16000, seed=1234):
        super(TimeSlicedNet, self).__init__(num_classes, seed)
        fm = filter_mult
        self.fm, self.input_size = fm, input_size
        self.C1 = 32 * fm
        self.add_kernel('conv1d', (TAPS, FRAME, self.C1), TAPS * FRAME, TAPS * self.C1, l2=True)
        self.add_bn(self.C1)
        frames = same_pad(input_size, FRAME, HOP)[0]
        L, C = (frames - TAPS) // STRIDE + 1, self.C1
        self.L1 = L
        self.blocks = []
        for i, (s, F) in enumerate(SPEC):
            F *= fm
            self.add_kernel('depthwise_conv2d', (1, 3, C, 1), 3 * C, 3, l2=True, suffix='depthwise_kernel')
            self.add_kernel('conv1d', (1, C, F), C, F, l2=True)
            self.add_bn(F)
            pl, pr = block_pad(L, s)
            Lout = (L + pl + pr - 3) // s + 1
            assert Lout >= 1, "input_size %d: block %d keeps no row" % (input_size, i)
            self.blocks.append({'dw': i + 1, 'bn': i + 2, 's': s, 'C': C, 'F': F, 'L': L, 'Lout': Lout})
            L, C = Lout, F
        self.T, self.C, self.H = L, C, 256 * fm
        self.add_kernel('dense', (C, self.H), C, self.H)
        self.add_kernel('dense', (self.H, num_classes), self.H, num_classes, l2=True)

    def lengths(self):
        return [self.L1] + [b['Lout'] for b in self.blocks]

    def _taps(self, blk, mutate):
        w = self._p('depthwise_conv2d_%d/depthwise_kernel' % blk['dw'])[0, :, :, 0]
        return w[::-1] if mutate == 'reversed_taps' else w

    def _bn_act(self, n, y, training, cache):
        if cache is not None:
            cache['y%d' % n] = y
        return self.bn_act_fwd(n, y, training, cache)

    def forward(self, x, training=False, seed=0, step=0, cache=None, drop_offset=0, mutate=None):
        B = x.shape[0]
        if cache is not None:
            cache['batch_stats'] = {}
        F = frame_same(x.astype(np.float64), FRAME, HOP)
        y, cols = conv1d_fwd(F, self._p('conv1d_1/kernel'), stride=STRIDE)
        if cache is not None:
            cache['cols1'], cache['frames_shape'] = cols, F.shape
        a = self._bn_act(1, y, training, cache)
        for blk in self.blocks:
            pad_l = block_pad(blk['L'], blk['s'], odd_left=(mutate == 'pad_left'))[0]
            z = dw_fwd(a, self._taps(blk, mutate), blk['s'], pad_l, blk['Lout'])
            y = pw_fwd(z, self._p('conv1d_%d/kernel' % blk['bn'])[0])
            if cache is not None:
                cache['a%d' % blk['bn']], cache['z%d' % blk['bn']] = a, z
            a = self._bn_act(blk['bn'], y, training, cache)
        feat = a.mean(axis=1)
        keep1 = keep2 = None
        fd = feat
        if training:
            keep1 = self.dropout(seed, step, 1, B, self.C, KEEP1, drop_offset)
            fd = feat * keep1 / KEEP1
        hpre = self.dense_fwd(fd, 'dense_1/kernel')
        h = act_fwd(hpre)
        if training:
            keep2 = self.dropout(seed, step, 2, B, self.H, KEEP2, drop_offset)
            h = h * keep2 / KEEP2
        p = self.head_fwd(h, 'dense_2/kernel')
        if cache is not None:
            cache.update(feat=feat, fd=fd, hpre=hpre, h=h, keep1=keep1, keep2=keep2, p=p)
        return p

    def loss_and_grads(self, x, y_onehot, seed=0, step=0, drop_offset=0, relu_masks=None, mutate=None):
        """Data loss (batch mean) and its gradients (no L2 term)."""
        cache, grads = {}, {}
        p = self.forward(x, training=True, seed=seed, step=step, cache=cache, drop_offset=drop_offset, mutate=mutate)
        loss, dh = self.head_bwd(p, y_onehot, cache['h'], 'dense_2/kernel', None, grads)
        hmask = relu_masks['hidden'] if relu_masks is not None and 'hidden' in relu_masks else act_mask(cache['hpre'])
        dh = dh * cache['keep2'] / KEEP2 * hmask
        dfeat = self.dense_bwd(dh, cache['fd'], 'dense_1/kernel', None, grads) * cache['keep1'] / KEEP1
        da = np.repeat((dfeat / self.T)[:, None, :], self.T, axis=1)
        for blk in reversed(self.blocks):
            n = blk['bn']
            dy = self.bn_act_bwd(n, da, cache, grads, relu_masks)
            dz, dW = pw_bwd(dy, cache['z%d' % n], self._p('conv1d_%d/kernel' % n)[0])
            grads['conv1d_%d/kernel' % n] = dW[None]
            pad_l = block_pad(blk['L'], blk['s'], odd_left=(mutate == 'pad_left'))[0]
            da, dw = dw_bwd(dz, cache['a%d' % n], self._taps(blk, mutate), blk['s'], pad_l)
            if mutate == 'reversed_taps':
                dw = dw[::-1]
            grads['depthwise_conv2d_%d/depthwise_kernel' % blk['dw']] = dw[None, :, :, None]
        dy = self.bn_act_bwd(1, da, cache, grads, relu_masks)
        _, grads['conv1d_1/kernel'] = conv1d_bwd(dy, cache['cols1'], self._p('conv1d_1/kernel'), cache['frames_shape'], stride=STRIDE,
                                                 need_dx=False)
        return loss, p, self.ordered(grads), cache
