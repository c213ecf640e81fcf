"""Float64 NumPy oracle of the general depthwise ladder conv_1d_gru (reference model.py:470-512; no recurrent layer): forward,
loss and every gradient, restated layer by layer for the GPU parity tests (the depthwise convolution is oracle_blocks.dw_fwd /
dw_bwd, which the kernel tests compare kws_dwconvk_* with).

TEST INFRASTRUCTURE ONLY.  A block is DepthwiseConv2D((1, k), strides=s, SAME or VALID, no bias) -> Conv1D(F, 1, no bias) ->
BatchNormalization -> relu6; SAME padding is TensorFlow's (the odd sample on the right) and pads the ACTIVATED input.  The head
is Flatten -> Dropout(.3) -> Dense(256) -> relu6 -> Dropout(.3) -> Dense -> softmax with oracle/layers.py's counter-based
dropout masks (layer ids 1 and 2), as on the device.

`relu_masks` hands the device's own ReLU6 decisions to the backward pass ({block number 1..6: mask, 'hidden': mask}); `mutate`
names a deliberately wrong variant for the negative controls:
  'pad_left'       SAME padding with the odd sample on the LEFT (pad_l one too large where the total padding is odd)
  'reversed_taps'  the depthwise kernels applied back to front
"""
import numpy as np

from oracle_blocks import DwPwNet, act_fwd, act_mask, same_geometry

# (filters, taps, stride, padding) of the six blocks; the expected (L_in, pad_l, L_out) ladder for 16000 samples
SPEC = [(128, 63, 16, 'same'), (256, 31, 4, 'same'), (384, 15, 4, 'same'), (448, 7, 4, 'same'), (512, 5, 2, 'same'),
        (512, 8, 1, 'valid')]
LADDER = [(16000, 23, 1000), (1000, 13, 250), (250, 6, 63), (63, 2, 16), (16, 1, 8), (8, 0, 1)]
HIDDEN = 256
KEEP = 0.7   # both Dropout(0.3)


class DwkNet(DwPwNet):
    """conv_1d_gru; input [B, 16000] raw samples."""

    def __init__(self, num_classes=12, seed=1234, input_size=16000):
        super(DwkNet, self).__init__(num_classes, seed)
        self.blocks = []
        L, C = input_size, 1
        for F, k, s, pad in SPEC:
            n = self.add_block(k, C, F)
            Lout, pad_l = same_geometry(L, k, s)[:2] if pad == 'same' else ((L - k) // s + 1, 0)
            self.blocks.append({'idx': n, 'k': k, 's': s, 'same': pad == 'same', 'C': C, 'F': F, 'L': L, 'Lout': Lout, 'pad_l': pad_l})
            L, C = Lout, F
        assert L == 1
        self.D = C
        self.add_kernel('dense', (C, HIDDEN), C, HIDDEN, bias=HIDDEN)
        self.add_kernel('dense', (HIDDEN, num_classes), HIDDEN, num_classes, bias=num_classes)

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
            a = self.block_fwd(blk['idx'], a, blk['s'], self._pad_l(blk, mutate), blk['Lout'], training, cache, mutate == 'reversed_taps')
        flat = a.reshape(B, self.D)
        keep1 = keep2 = None
        if training:
            keep1 = self.dropout(seed, step, 1, B, self.D, KEEP, drop_offset)
            flat = flat * keep1 / KEEP
        hpre = self.dense_fwd(flat, 'dense_1/kernel', 'dense_1/bias')
        h = act_fwd(hpre)
        if training:
            keep2 = self.dropout(seed, step, 2, B, HIDDEN, KEEP, drop_offset)
            h = h * keep2 / KEEP
        p = self.head_fwd(h, 'dense_2/kernel', 'dense_2/bias')
        if cache is not None:
            cache.update(flat=flat, hpre=hpre, h=h, keep1=keep1, keep2=keep2, p=p)
        return p

    def loss_and_grads(self, x, y_onehot, seed=0, step=0, drop_offset=0, relu_masks=None, mutate=None):
        """Data loss (batch mean) and its gradients (no L2 term)."""
        cache, grads = {}, {}
        B = x.shape[0]
        p = self.forward(x, training=True, seed=seed, step=step, cache=cache, drop_offset=drop_offset, mutate=mutate)
        loss, dh = self.head_bwd(p, y_onehot, cache['h'], 'dense_2/kernel', 'dense_2/bias', grads)
        hmask = relu_masks['hidden'] if relu_masks is not None and 'hidden' in relu_masks else act_mask(cache['hpre'])
        dh = dh * cache['keep2'] / KEEP * hmask
        da = (self.dense_bwd(dh, cache['flat'], 'dense_1/kernel', 'dense_1/bias', grads) * cache['keep1'] / KEEP).reshape(B, 1, self.D)
        for blk in reversed(self.blocks):
            da = self.block_bwd(blk['idx'], da, blk['s'], self._pad_l(blk, mutate), cache, grads, relu_masks, mutate == 'reversed_taps')
        return loss, p, self.ordered(grads), cache
