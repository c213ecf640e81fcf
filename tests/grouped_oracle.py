"""Float64 NumPy oracle of the grouped-Conv1D models conv_1d_fast (reference model.py:642-713) and conv_1d_spec
(model.py:1249-1323): forward, loss and every gradient, restated layer by layer for the GPU parity tests.

TEST INFRASTRUCTURE ONLY.  A grouped block is g separate Conv1D(F/g, k, VALID, no bias) layers over the slices
x[:, :, q*gs:(q+1)*gs] (gs = num_channels / g from the block's argument), each followed by its own BatchNormalization and
relu6, concatenated in group order.  Dropout masks are oracle/layers.py's counter-based ones (layer_id 1), as on the device.
"""
from collections import OrderedDict

import numpy as np

from oracle.layers import (bn_infer_fwd, bn_train_bwd, bn_train_fwd, cce_fwd_bwd, dropout_key, dropout_mask, relu6,
                           relu6_mask, softmax, softmax_bwd)

# (filters, k, groups, num_channels, stride) per grouped block
FAST_BLOCKS = [(300, 15, 6, 252, 2), (360, 7, 5, 300, 2)]
SPEC_BLOCKS = [(300, 3, 4, 252, 2), (300, 3, 3, 300, 1), (360, 3, 4, 300, 2), (360, 3, 3, 360, 1),
               (420, 3, 4, 360, 2), (420, 3, 3, 360, 1), (480, 3, 4, 420, 2), (480, 3, 3, 480, 1)]
KEEP = 0.7   # Dropout(0.3)


def gconv_fwd(x, Ws, k, stride, gs, reverse=False):
    """x [B, L, C], Ws: g kernels [k, gs, Ng] -> [B, Lout, g * Ng] (reverse: groups concatenated in reverse - a mutation)."""
    L = x.shape[1]
    Lout = (L - k) // stride + 1
    idx = stride * np.arange(Lout)[:, None] + np.arange(k)[None, :]
    B = x.shape[0]
    outs = [(x[:, :, q * gs:(q + 1) * gs][:, idx, :].reshape(B * Lout, -1) @ W.reshape(-1, W.shape[2])).reshape(B, Lout, -1)
            for q, W in enumerate(Ws)]
    return np.concatenate(outs[::-1] if reverse else outs, axis=2)


def gconv_bwd(dy, x, Ws, k, stride, gs, need_dx=True, swap_phase=False):
    """-> (dx [B, L, C] (zeros outside the groups), [dW_q]).  swap_phase: rows tau and tau ^ 1 of dx trade places (a
    mutation of the data gradient's phase split)."""
    L = x.shape[1]
    Lout = dy.shape[1]
    Ng = Ws[0].shape[2]
    idx = stride * np.arange(Lout)[:, None] + np.arange(k)[None, :]
    dx = np.zeros_like(x) if need_dx else None
    dWs = []
    for q, W in enumerate(Ws):
        B = x.shape[0]
        cols = x[:, :, q * gs:(q + 1) * gs][:, idx, :].reshape(B * Lout, -1)
        dyq = dy[:, :, q * Ng:(q + 1) * Ng].reshape(B * Lout, Ng)
        dWs.append((cols.T @ dyq).reshape(W.shape))
        if need_dx:
            dcols = (dyq @ W.reshape(-1, Ng).T).reshape(B, Lout, k, gs)
            for j in range(k):
                dx[:, stride * np.arange(Lout) + j, q * gs:(q + 1) * gs] += dcols[:, :, j, :]
    if need_dx and swap_phase:
        n = L - L % 2
        dx[:, :n] = dx[:, :n].reshape(dx.shape[0], n // 2, 2, -1)[:, :, ::-1].reshape(dx.shape[0], n, -1)
    return dx, dWs


def glorot(rng, shape, fan_in, fan_out):
    lim = np.sqrt(6.0 / (fan_in + fan_out))
    return rng.uniform(-lim, lim, size=shape).astype(np.float32)


class GroupedConvNet(object):
    """kind 'fast' (raw [16000]) or 'spec' ([98 * 257] = the generator's 'spec' output)."""

    def __init__(self, kind, num_classes=12, input_size=16000, seed=1234):
        rng = np.random.RandomState(seed)
        self.kind, self.nc = kind, num_classes
        P, S = OrderedDict(), OrderedDict()
        conv, bn = 1, 1
        self.front = None
        if kind == 'fast':
            self.front = 'conv1d_%d/kernel' % conv
            P[self.front] = glorot(rng, (479, 1, 252), 479, 479 * 252)
            conv += 1
            L, C = (input_size - 479) // 160 + 1, 252
            spec = FAST_BLOCKS
            self.in_shape = (input_size, 1)
        else:
            L, C = 98, 257
            spec = SPEC_BLOCKS
            self.in_shape = (98, 257)
        self.blocks = []
        for F, k, g, nch, s in spec:
            gs, Ng = nch // g, F // g
            blk = {'F': F, 'k': k, 'g': g, 'gs': gs, 'Ng': Ng, 'stride': s, 'L': L, 'C': C, 'Lout': (L - k) // s + 1,
                   'convs': [], 'bns': []}
            for q in range(g):
                name = 'conv1d_%d/kernel' % conv
                P[name] = glorot(rng, (k, gs, Ng), k * gs, k * Ng)
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
        self.l2_names = [self.front] if self.front else []

    def count_params(self):
        return sum(v.size for v in self.params.values()) + sum(v.size for v in self.state.values())

    def _W(self, blk):
        return [self.params[n].astype(np.float64) for n in blk['convs']]

    def forward(self, x, training=False, seed=0, step=0, cache=None, drop_offset=0, mutate=None):
        B = x.shape[0]
        h = x.astype(np.float64).reshape((B,) + self.in_shape)
        if self.front:
            W0 = self.params[self.front].astype(np.float64)
            h = gconv_fwd(h, [W0], 479, 160, 1)
        if cache is not None:
            cache['x0'] = h
            cache['batch_stats'] = {}
        for i, blk in enumerate(self.blocks):
            y = gconv_fwd(h, self._W(blk), blk['k'], blk['stride'], blk['gs'], reverse=(mutate == 'reverse_groups'))
            outs = []
            Ng = blk['Ng']
            for q, idx in enumerate(blk['bns']):
                yq = y[:, :, q * Ng:(q + 1) * Ng]
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
                outs.append(relu6(z))
            if cache is not None:
                cache['y%d' % i] = y
                cache['in%d' % i] = h
            h = np.concatenate(outs, axis=2)
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
        """Data loss (batch mean) and its gradients (no L2 term).  relu_masks: {bn index: [B, Lout, Ng]} decisions to use
        in place of the oracle's own (the device's, read back, so that values at the ReLU6 kinks cannot flip)."""
        cache = {}
        B = x.shape[0]
        p = self.forward(x, training=True, seed=seed, step=step, cache=cache, drop_offset=drop_offset, mutate=mutate)
        loss, per, dp = cce_fwd_bwd(p, y_onehot.astype(np.float64))
        dl = softmax_bwd(dp, p)
        grads = OrderedDict()
        Wd = self.params['dense_1/kernel'].astype(np.float64)
        dWd = cache['f'].T @ dl
        dbd = dl.sum(axis=0)
        da = ((dl @ Wd.T) * cache['keep'] / KEEP).reshape(cache['a_last'].shape)
        for i in range(len(self.blocks) - 1, -1, -1):
            blk = self.blocks[i]
            Ng = blk['Ng']
            dy = np.zeros_like(cache['y%d' % i])
            for q, idx in enumerate(blk['bns']):
                st, z = cache['bn%d' % idx]
                mask = relu_masks[idx] if relu_masks is not None and idx in relu_masks else relu6_mask(z)
                yq = cache['y%d' % i][:, :, q * Ng:(q + 1) * Ng]
                ga = self.params['batch_normalization_%d/gamma' % idx].astype(np.float64)
                dyq, dga, dbe = bn_train_bwd(da[:, :, q * Ng:(q + 1) * Ng] * mask, yq, ga, st)
                dy[:, :, q * Ng:(q + 1) * Ng] = dyq
                grads['batch_normalization_%d/gamma' % idx] = dga
                grads['batch_normalization_%d/beta' % idx] = dbe
            if mutate == 'reverse_groups':
                g = blk['g']
                dy = np.concatenate([dy[:, :, q * Ng:(q + 1) * Ng] for q in range(g)][::-1], axis=2)
            need_dx = i > 0 or self.front is not None
            da, dWs = gconv_bwd(dy, cache['in%d' % i], self._W(blk), blk['k'], blk['stride'], blk['gs'], need_dx=need_dx,
                                swap_phase=(mutate == 'swap_phase'))
            for name, dW in zip(blk['convs'], dWs):
                grads[name] = dW
        if self.front:
            _, (dW0,) = gconv_bwd(da, x.astype(np.float64).reshape((B,) + self.in_shape),
                                  [self.params[self.front].astype(np.float64)], 479, 160, 1, need_dx=False)
            grads[self.front] = dW0
        grads['dense_1/kernel'] = dWd
        grads['dense_1/bias'] = dbd
        ordered = OrderedDict((k, grads[k]) for k in self.params)
        return loss, p, ordered, cache
