"""Float64 NumPy oracle of the dense-Conv1D ladders conv_1d_time_stacked (reference model.py:257-309) and conv_1d_heavy
(model.py:409-467): forward, loss and every gradient, restated layer by layer for the GPU parity tests.

TEST INFRASTRUCTURE ONLY.  A ladder layer is Conv1D(F, k, VALID, stride 1, no bias) -> BatchNormalization -> relu6, every
second one followed by MaxPool1D(3, strides=2, 'valid') whose gradient goes to the FIRST maximum of a window (TF MaxPoolGrad).
Dropout masks are oracle/layers.py's counter-based ones (layer ids in Keras creation order), as on the device.

`relu_masks` / `pool_ind` hand the device's own ReLU6 and arg-max decisions to the backward pass (values at a kink or a tie
cannot flip then); `mutate` names a deliberately wrong variant for the negative controls:
  'last_max'         the LAST maximum of a window wins
  'pool_before_act'  the pool picks its winner on the raw convolution output (= pooling y and normalising afterwards)
  'no_gate'          the ReLU6 gate of the pooled layers is dropped
"""
from collections import OrderedDict

import numpy as np

import pool_oracle
from oracle.layers import (bn_infer_fwd, bn_train_bwd, bn_train_fwd, cce_fwd_bwd, dropout_key, dropout_mask, relu6, relu6_mask,
                           softmax, softmax_bwd)

# input view [L, C] and the widths of the reduce / context pairs
NETS = {'time_stacked': ((800, 20), (48, 96, 128, 160, 192, 256)),
        'heavy': ((1600, 10), (48, 96, 128, 160, 192, 256, 320))}
KEEP1, KEEP2 = 0.7, 0.9   # Dropout(0.3), Dropout(0.1)
HEAD_WIDTH = 128          # conv_1d_heavy's Conv1D(128, 5)


def conv_fwd(x, W):
    """x [B, L, Cin], W [k, Cin, F] -> [B, L - k + 1, F] (VALID, stride 1), one matrix product per tap."""
    k = W.shape[0]
    Lout = x.shape[1] - k + 1
    y = x[:, 0:Lout, :] @ W[0]
    for j in range(1, k):
        y += x[:, j:j + Lout, :] @ W[j]
    return y


def conv_bwd(dy, x, W, need_dx=True):
    k = W.shape[0]
    Lout = dy.shape[1]
    dy2 = dy.reshape(-1, dy.shape[2])
    dW = np.stack([x[:, j:j + Lout, :].reshape(-1, x.shape[2]).T @ dy2 for j in range(k)])
    dx = None
    if need_dx:
        dx = np.zeros_like(x)
        for j in range(k):
            dx[:, j:j + Lout, :] += dy @ W[j].T
    return dx, dW


def pool_len(L):
    return (L - 3) // 2 + 1


def pool_windows(a):
    """[B, L, C] -> [B, Lp, 3, C] windows of MaxPool1D(3, strides=2, 'valid')."""
    return pool_oracle.windows(a, pool_len(a.shape[1]), 0)


def pool_argmax(a, last=False):
    return pool_oracle.argmax(a, pool_len(a.shape[1]), 0, last)


def pool_fwd(a, ind):
    return pool_oracle.fwd(a, ind, 0)


def pool_bwd(dz, ind, L):
    return pool_oracle.bwd(dz, ind, L, 0)


def glorot(rng, shape, fan_in, fan_out):
    lim = np.sqrt(6.0 / (fan_in + fan_out))
    return rng.uniform(-lim, lim, size=shape).astype(np.float32)


class StackedConvNet(object):
    """kind 'time_stacked' or 'heavy'; input [B, 16000] raw samples."""

    def __init__(self, kind, num_classes=12, seed=1234):
        rng = np.random.RandomState(seed)
        self.kind, self.nc = kind, num_classes
        self.in_shape, widths = NETS[kind]
        P, S = OrderedDict(), OrderedDict()
        self.layers = []
        L, C = self.in_shape

        def add(F, k, pool, bn=True):
            n = len(self.layers) + 1
            name = 'conv1d_%d/kernel' % n
            P[name] = glorot(rng, (k, C, F), k * C, k * F)
            if bn:
                base = 'batch_normalization_%d/' % n
                P[base + 'gamma'] = np.ones(F, np.float32)
                P[base + 'beta'] = np.zeros(F, np.float32)
                S[base + 'moving_mean'] = np.zeros(F, np.float32)
                S[base + 'moving_variance'] = np.ones(F, np.float32)
            Lout = L - k + 1
            lay = {'idx': n, 'conv': name, 'k': k, 'C': C, 'F': F, 'pool': pool, 'L': L, 'Lout': Lout,
                   'Lp': pool_len(Lout) if pool else Lout}
            self.layers.append(lay)
            return lay['Lp'], F

        L, C = add(32, 1, False)
        for F in widths:
            L, C = add(F, 3, True)
            L, C = add(F, 3, False)
        self.ladder = len(self.layers)
        self.l2_names = [l['conv'] for l in self.layers]
        self.Dd = L * C                       # width of dropout_1
        assert L == 5
        if kind == 'heavy':
            add(HEAD_WIDTH, 5, False)
            self.out_kernel = 'conv1d_%d/kernel' % (len(self.layers) + 1)
            P[self.out_kernel] = glorot(rng, (1, HEAD_WIDTH, num_classes), HEAD_WIDTH, num_classes)
            self.out_bias = None
        else:
            self.out_kernel = 'conv1d_%d/kernel' % (len(self.layers) + 1)
            self.out_bias = 'conv1d_%d/bias' % (len(self.layers) + 1)
            P[self.out_kernel] = glorot(rng, (5, C, num_classes), 5 * C, 5 * num_classes)
            P[self.out_bias] = np.zeros(num_classes, np.float32)
        self.params, self.state = P, S

    def count_params(self):
        return sum(v.size for v in self.params.values()) + sum(v.size for v in self.state.values())

    def _p(self, name):
        return self.params[name].astype(np.float64)

    def _layer(self, lay, h, training, cache, mutate, pool_ind):
        idx = lay['idx']
        y = conv_fwd(h, self._p(lay['conv']))
        ga, be = self._p('batch_normalization_%d/gamma' % idx), self._p('batch_normalization_%d/beta' % idx)
        if training:
            pre, st = bn_train_fwd(y, ga, be)
        else:
            st = None
            pre = bn_infer_fwd(y, ga, be, self.state['batch_normalization_%d/moving_mean' % idx].astype(np.float64),
                               self.state['batch_normalization_%d/moving_variance' % idx].astype(np.float64))
        a = relu6(pre)
        ind = None
        if lay['pool']:
            if mutate == 'last_max':
                ind = pool_argmax(a, last=True)
            elif mutate == 'pool_before_act':
                ind = pool_argmax(y)
            elif pool_ind is not None and idx in pool_ind:
                ind = pool_ind[idx]
            else:
                ind = pool_argmax(a)
            out = pool_fwd(a, ind)
        else:
            out = a
        if cache is not None:
            cache['in%d' % idx], cache['y%d' % idx], cache['st%d' % idx], cache['ind%d' % idx] = h, y, st, ind
            if training:
                cache['batch_stats'][idx] = (st[0], st[1])
        return out

    def forward(self, x, training=False, seed=0, step=0, cache=None, drop_offset=0, mutate=None, pool_ind=None):
        B = x.shape[0]
        h = x.astype(np.float64).reshape((B,) + self.in_shape)
        if cache is not None:
            cache['batch_stats'] = {}
        for lay in self.layers[:self.ladder]:
            h = self._layer(lay, h, training, cache, mutate, pool_ind)
        flat = h.reshape(B, self.Dd)
        keep1 = keep2 = None
        if training:
            keep1 = dropout_mask(dropout_key(seed, step, 1), B * self.Dd, KEEP1, offset=drop_offset * self.Dd).reshape(B, self.Dd)
            flat = flat * keep1 / KEEP1
        if self.kind == 'heavy':
            f1 = flat.reshape(B, 5, -1)
            a = self._layer(self.layers[-1], f1, training, cache, mutate, pool_ind).reshape(B, HEAD_WIDTH)
            if training:
                keep2 = dropout_mask(dropout_key(seed, step, 2), B * HEAD_WIDTH, KEEP2,
                                     offset=drop_offset * HEAD_WIDTH).reshape(B, HEAD_WIDTH)
                a = a * keep2 / KEEP2
            f = a
            logits = f @ self._p(self.out_kernel)[0]
        else:
            f = flat
            logits = f @ self._p(self.out_kernel).reshape(self.Dd, self.nc) + self._p(self.out_bias)
        p = softmax(logits)
        if cache is not None:
            cache.update(f=f, keep1=keep1, keep2=keep2, p=p)
        return p

    def _layer_bwd(self, lay, dout, cache, grads, relu_masks, mutate, need_dx):
        """dout: gradient wrt the layer's output (pooled if the layer pools) -> gradient wrt its input."""
        idx = lay['idx']
        y, st = cache['y%d' % idx], cache['st%d' % idx]
        ga = self._p('batch_normalization_%d/gamma' % idx)
        if relu_masks is not None and idx in relu_masks:
            mask = relu_masks[idx]
        else:
            mask = relu6_mask(y * (st[2] * ga) + (self._p('batch_normalization_%d/beta' % idx) - st[0] * st[2] * ga))
        if lay['pool']:
            dout = pool_bwd(dout, cache['ind%d' % idx], lay['Lout'])
            if mutate == 'no_gate':
                mask = 1.0
        dy, dga, dbe = bn_train_bwd(dout * mask, y, ga, st)
        grads['batch_normalization_%d/gamma' % idx] = dga
        grads['batch_normalization_%d/beta' % idx] = dbe
        dx, dW = conv_bwd(dy, cache['in%d' % idx], self._p(lay['conv']), need_dx=need_dx)
        grads[lay['conv']] = dW
        return dx

    def loss_and_grads(self, x, y_onehot, seed=0, step=0, drop_offset=0, relu_masks=None, pool_ind=None, mutate=None):
        """Data loss (batch mean) and its gradients (no L2 term)."""
        cache = {}
        B = x.shape[0]
        p = self.forward(x, training=True, seed=seed, step=step, cache=cache, drop_offset=drop_offset, mutate=mutate,
                         pool_ind=pool_ind)
        loss, per, dp = cce_fwd_bwd(p, y_onehot.astype(np.float64))
        dl = softmax_bwd(dp, p)
        grads = OrderedDict()
        if self.kind == 'heavy':
            Wo = self._p(self.out_kernel)[0]
            grads[self.out_kernel] = (cache['f'].T @ dl)[None]
            da = (dl @ Wo.T) * cache['keep2'] / KEEP2
            dflat = self._layer_bwd(self.layers[-1], da.reshape(B, 1, HEAD_WIDTH), cache, grads, relu_masks, mutate, True)
            dflat = dflat.reshape(B, self.Dd)
        else:
            Wo = self._p(self.out_kernel).reshape(self.Dd, self.nc)
            grads[self.out_kernel] = (cache['f'].T @ dl).reshape(self.params[self.out_kernel].shape)
            grads[self.out_bias] = dl.sum(axis=0)
            dflat = dl @ Wo.T
        top = self.layers[self.ladder - 1]
        da = (dflat * cache['keep1'] / KEEP1).reshape(B, top['Lp'], top['F'])
        for i in range(self.ladder - 1, -1, -1):
            da = self._layer_bwd(self.layers[i], da, cache, grads, relu_masks, mutate, need_dx=i > 0)
        ordered = OrderedDict((k, grads[k]) for k in self.params)
        return loss, p, ordered, cache
