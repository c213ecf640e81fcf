"""Float64 NumPy oracle of conv_1d_learned_spec (reference model.py:1159-1246): forward, loss and every gradient, restated layer
by layer for the CPU cross-check against torch autograd and the GPU parity tests.  The interface and the grouped ladder are
grouped_oracle.GroupedConvNet's (GroupedBlocksNet).

TEST INFRASTRUCTURE ONLY.  The front end is six Conv1D(40, k, strides=160, 'same', no bias) layers on the waveform, concatenated:
TensorFlow's SAME rule gives ceil(L / 160) rows and, per layer, pad_l = max((rows - 1) * 160 + k - L, 0) // 2 zeros in front of the
clip.  A grouped block is g Conv1D(F / g, 3, VALID, no bias) layers over the slices x[:, :, q * gs:(q + 1) * gs] CLIPPED at the
channel count (gs = num_channels / g from the block's argument), each followed by its own BatchNormalization and relu6,
concatenated in group order: the second block asks for 2 x 180 of 300 channels, so its groups read 180 and 120.  Dropout masks are
oracle/layers.py's counter-based ones (layer_id 1), as on the device.
"""
import numpy as np

from grouped_oracle import KEEP, GroupedBlocksNet  # noqa: F401 (KEEP: this model's Dropout(0.3) too)
from oracle_blocks import gconv_bwd, gconv_fwd, same_geometry

FRONT_K = (479, 383, 319, 255, 191, 161)
FRONT_N, FRONT_STRIDE = 40, 160
# (filters, k, groups, num_channels, stride) per grouped block
BLOCKS = [(300, 3, 3, 240, 2), (300, 3, 2, 360, 1), (360, 3, 3, 300, 2), (360, 3, 2, 360, 1),
          (420, 3, 3, 240, 2), (420, 3, 2, 420, 1), (480, 3, 3, 420, 2), (480, 3, 2, 480, 1)]
MUTATIONS = ('front_pad', 'ragged_split')


def same_pads(L, stride=FRONT_STRIDE, ks=FRONT_K):
    """(rows, [pad_l]) of the front layers: TensorFlow's SAME rule"""
    return -(-L // stride), [same_geometry(L, k, stride)[1] for k in ks]


def padded(x, pad_l, length):
    """x [B, L] with pad_l zeros in front, cut or zero filled to `length` samples"""
    out = np.zeros((x.shape[0], length), x.dtype)
    n = min(x.shape[1], length - pad_l)
    out[:, pad_l:pad_l + n] = x[:, :n]
    return out


class LearnedSpecNet(GroupedBlocksNet):
    def __init__(self, num_classes=12, input_size=16000, seed=1234):
        super(LearnedSpecNet, self).__init__(num_classes, seed)
        self.input_size = input_size
        self.rows, self.pads = same_pads(input_size)
        self.front = [self.add_kernel('conv1d', (k, 1, FRONT_N), k, k * FRONT_N, l2=True) for k in FRONT_K]
        self.add_blocks(BLOCKS, self.rows, FRONT_N * len(FRONT_K))

    def _front_inputs(self, x, mutate):
        """per bank: the clip padded so that a VALID convolution at stride 160 gives exactly `rows` rows"""
        out = []
        for q, k in enumerate(FRONT_K):
            pad = self.pads[q] + (1 if mutate == 'front_pad' and q == 2 else 0)
            out.append(padded(x, pad, (self.rows - 1) * FRONT_STRIDE + k)[:, :, None])
        return out

    def _slices(self, i, mutate):
        sl = self.blocks[i]['slices']
        if mutate == 'ragged_split' and i == 1:      # the second window starts where an even 150 | 150 split would
            (a0, b0), (a1, b1) = sl
            return [(a0, b0), (150, 150 + b1 - a1)]
        return sl

    def forward(self, x, training=False, seed=0, step=0, cache=None, drop_offset=0, mutate=None):
        xs = self._front_inputs(x.astype(np.float64).reshape(x.shape[0], self.input_size), mutate)
        h = np.concatenate([gconv_fwd(xq, [self._p(n)], k, FRONT_STRIDE, 1) for xq, n, k in zip(xs, self.front, FRONT_K)], axis=2)
        if cache is not None:
            cache['front_inputs'] = xs
        return self.blocks_fwd(h, training, seed, step, cache, drop_offset, mutate)

    def loss_and_grads(self, x, y_onehot, seed=0, step=0, drop_offset=0, relu_masks=None, mutate=None):
        """Data loss (batch mean) and its gradients (no L2 term).  relu_masks: {bn index: [B, Lout, Ng]} decisions to use in
        place of the oracle's own (the device's, read back, so that values at the ReLU6 kinks cannot flip).  cache['da%d' % i]:
        the gradient wrt block i's activated input."""
        cache, grads = {}, {}
        p = self.forward(x, training=True, seed=seed, step=step, cache=cache, drop_offset=drop_offset, mutate=mutate)
        loss, da = self.blocks_bwd(p, y_onehot, cache, grads, relu_masks, mutate, need_dx=True)
        for q, (name, k) in enumerate(zip(self.front, FRONT_K)):
            _, (grads[name],) = gconv_bwd(da[:, :, q * FRONT_N:(q + 1) * FRONT_N], cache['front_inputs'][q], [self._p(name)], k,
                                          FRONT_STRIDE, 1, need_dx=False)
        return loss, p, self.ordered(grads), cache
