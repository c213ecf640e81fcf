"""Float64 NumPy oracle of conv_1d_learned_spec (reference model.py:1159-1246): forward, loss and every gradient, restated layer
by layer for the CPU cross-check against torch autograd and the GPU parity tests.  The interface is grouped_oracle.GroupedConvNet's.

TEST INFRASTRUCTURE ONLY.  The front end is six Conv1D(40, k, strides=160, 'same', no bias) layers on the waveform, concatenated:
TensorFlow's SAME rule gives ceil(L / 160) rows and, per layer, pad_l = max((rows - 1) * 160 + k - L, 0) // 2 zeros in front of the
clip.  A grouped block is g Conv1D(F / g, 3, VALID, no bias) layers over the slices x[:, :, q * gs:(q + 1) * gs] CLIPPED at the
channel count (gs = num_channels / g from the block's argument), each followed by its own BatchNormalization and relu6,
concatenated in group order: the second block asks for 2 x 180 of 300 channels, so its groups read 180 and 120.  Dropout masks are
oracle/layers.py's counter-based ones (layer_id 1), as on the device.
"""
from collections import OrderedDict

import numpy as np

from grouped_oracle import KEEP, gconv_bwd, gconv_fwd, glorot
from oracle.layers import (bn_infer_fwd, bn_train_bwd, bn_train_fwd, cce_fwd_bwd, dropout_key, dropout_mask, relu6, relu6_mask,
                           softmax, softmax_bwd)

FRONT_K = (479, 383, 319, 255, 191, 161)
FRONT_N, FRONT_STRIDE = 40, 160
# (filters, k, groups, num_channels, stride) per grouped block
BLOCKS = [(300, 3, 3, 240, 2), (300, 3, 2, 360, 1), (360, 3, 3, 300, 2), (360, 3, 2, 360, 1),
          (420, 3, 3, 240, 2), (420, 3, 2, 420, 1), (480, 3, 3, 420, 2), (480, 3, 2, 480, 1)]
MUTATIONS = ('front_pad', 'ragged_split')


def same_pads(L, stride=FRONT_STRIDE, ks=FRONT_K):
    """(rows, [pad_l]) of the front layers: TensorFlow's SAME rule"""
    rows = -(-L // stride)
    return rows, [max((rows - 1) * stride + k - L, 0) // 2 for k in ks]


def padded(x, pad_l, length):
    """x [B, L] with pad_l zeros in front, cut or zero filled to `length` samples"""
    out = np.zeros((x.shape[0], length), x.dtype)
    n = min(x.shape[1], length - pad_l)
    out[:, pad_l:pad_l + n] = x[:, :n]
    return out


class LearnedSpecNet(object):
    def __init__(self, num_classes=12, input_size=16000, seed=1234):
        rng = np.random.RandomState(seed)
        self.nc, self.input_size = num_classes, input_size
        P, S = OrderedDict(), OrderedDict()
        self.rows, self.pads = same_pads(input_size)
        self.front = ['conv1d_%d/kernel' % (i + 1) for i in range(len(FRONT_K))]
        for name, k in zip(self.front, FRONT_K):
            P[name] = glorot(rng, (k, 1, FRONT_N), k, k * FRONT_N)
        conv, bn = len(FRONT_K) + 1, 1
        L, C = self.rows, FRONT_N * len(FRONT_K)
        self.blocks = []
        for F, k, g, nch, s in BLOCKS:
            gs, Ng = nch // g, F // g
            slices = [(min(q * gs, C), min((q + 1) * gs, C)) for q in range(g)]
            blk = {'F': F, 'k': k, 'g': g, 'gs': gs, 'Ng': Ng, 'stride': s, 'L': L, 'C': C, 'Lout': (L - k) // s + 1,
                   'slices': slices, 'convs': [], 'bns': []}
            for a, b in slices:
                name = 'conv1d_%d/kernel' % conv
                P[name] = glorot(rng, (k, b - a, Ng), k * (b - a), k * Ng)
                conv += 1
                base = 'batch_normalization_%d/' % bn
                P[base + 'gamma'] = np.ones(Ng, np.float32)
                P[base + 'beta'] = np.zeros(Ng, np.float32)
                S[base + 'moving_mean'] = np.zeros(Ng, np.float32)
                S[base + 'moving_variance'] = np.ones(Ng, np.float32)
                blk['convs'].append(name)
                blk['bns'].append(bn)
                bn += 1
            self.blocks.append(blk)
            L, C = blk['Lout'], F
        self.D = L * C
        P['dense_1/kernel'] = glorot(rng, (self.D, num_classes), self.D, num_classes)
        P['dense_1/bias'] = np.zeros(num_classes, np.float32)
        self.params, self.state = P, S
        self.l2_names = list(self.front)

    def count_params(self):
        return sum(v.size for v in self.params.values()) + sum(v.size for v in self.state.values())

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
        B = x.shape[0]
        x = x.astype(np.float64).reshape(B, self.input_size)
        xs = self._front_inputs(x, mutate)
        h = np.concatenate([gconv_fwd(xq, [self.params[n].astype(np.float64)], k, FRONT_STRIDE, 1)
                            for xq, n, k in zip(xs, self.front, FRONT_K)], axis=2)
        if cache is not None:
            cache['x0'] = h
            cache['front_inputs'] = xs
            cache['batch_stats'] = {}
        for i, blk in enumerate(self.blocks):
            Ng = blk['Ng']
            ys, outs = [], []
            for (a, b), name, idx in zip(self._slices(i, mutate), blk['convs'], blk['bns']):
                yq = gconv_fwd(h[:, :, a:b], [self.params[name].astype(np.float64)], blk['k'], blk['stride'], b - a)
                ga = self.params['batch_normalization_%d/gamma' % idx].astype(np.float64)
                be = self.params['batch_normalization_%d/beta' % idx].astype(np.float64)
                if training:
                    z, st = bn_train_fwd(yq, ga, be)
                    if cache is not None:
                        cache['bn%d' % idx] = (st, z)
                        cache['batch_stats'][idx] = (st[0], st[1])
                else:
                    z = bn_infer_fwd(yq, ga, be, self.state['batch_normalization_%d/moving_mean' % idx].astype(np.float64),
                                     self.state['batch_normalization_%d/moving_variance' % idx].astype(np.float64))
                ys.append(yq)
                outs.append(relu6(z))
            if cache is not None:
                cache['y%d' % i] = np.concatenate(ys, axis=2)
                cache['in%d' % i] = h
            h = np.concatenate(outs, axis=2)
            assert h.shape[1:] == (blk['Lout'], blk['F']) and len(outs) * Ng == blk['F']
        flat = h.reshape(B, -1)
        if training:
            keep = dropout_mask(dropout_key(seed, step, 1), B * self.D, KEEP, offset=drop_offset * self.D).reshape(B, self.D)
            f = flat * keep / KEEP
        else:
            keep = None
            f = flat
        logits = f @ self.params['dense_1/kernel'].astype(np.float64) + self.params['dense_1/bias'].astype(np.float64)
        p = softmax(logits)
        if cache is not None:
            cache.update(a_last=h, f=f, keep=keep, p=p)
        return p

    def loss_and_grads(self, x, y_onehot, seed=0, step=0, drop_offset=0, relu_masks=None, mutate=None):
        """Data loss (batch mean) and its gradients (no L2 term).  relu_masks: {bn index: [B, Lout, Ng]} decisions to use in
        place of the oracle's own (the device's, read back, so that values at the ReLU6 kinks cannot flip).  cache['da%d' % i]:
        the gradient wrt block i's activated input."""
        cache = {}
        p = self.forward(x, training=True, seed=seed, step=step, cache=cache, drop_offset=drop_offset, mutate=mutate)
        loss, per, dp = cce_fwd_bwd(p, y_onehot.astype(np.float64))
        dl = softmax_bwd(dp, p)
        grads = OrderedDict()
        Wd = self.params['dense_1/kernel'].astype(np.float64)
        grads['dense_1/kernel'] = cache['f'].T @ dl
        grads['dense_1/bias'] = dl.sum(axis=0)
        da = ((dl @ Wd.T) * cache['keep'] / KEEP).reshape(cache['a_last'].shape)
        for i in range(len(self.blocks) - 1, -1, -1):
            blk = self.blocks[i]
            Ng = blk['Ng']
            h = cache['in%d' % i]
            dh = np.zeros_like(h)
            for q, ((a, b), name, idx) in enumerate(zip(self._slices(i, mutate), blk['convs'], blk['bns'])):
                st, z = cache['bn%d' % idx]
                mask = relu_masks[idx] if relu_masks is not None and idx in relu_masks else relu6_mask(z)
                yq = cache['y%d' % i][:, :, q * Ng:(q + 1) * Ng]
                ga = self.params['batch_normalization_%d/gamma' % idx].astype(np.float64)
                dyq, dga, dbe = bn_train_bwd(da[:, :, q * Ng:(q + 1) * Ng] * mask, yq, ga, st)
                grads['batch_normalization_%d/gamma' % idx] = dga
                grads['batch_normalization_%d/beta' % idx] = dbe
                dxq, (dW,) = gconv_bwd(dyq, h[:, :, a:b], [self.params[name].astype(np.float64)], blk['k'], blk['stride'], b - a)
                dh[:, :, a:b] += dxq
                grads[name] = dW
            cache['da%d' % i] = dh
            da = dh
        for q, (name, k) in enumerate(zip(self.front, FRONT_K)):
            _, (dW,) = gconv_bwd(da[:, :, q * FRONT_N:(q + 1) * FRONT_N], cache['front_inputs'][q],
                                 [self.params[name].astype(np.float64)], k, FRONT_STRIDE, 1, need_dx=False)
            grads[name] = dW
        ordered = OrderedDict((k, grads[k]) for k in self.params)
        return loss, p, ordered, cache
