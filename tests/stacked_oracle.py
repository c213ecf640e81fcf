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
import numpy as np

import pool_oracle
from oracle_blocks import OracleNet, conv_bwd, conv_fwd
from pool_oracle import pool_len

# input view [L, C] and the widths of the reduce / context pairs
NETS = {'time_stacked': ((800, 20), (48, 96, 128, 160, 192, 256)),
        'heavy': ((1600, 10), (48, 96, 128, 160, 192, 256, 320))}
KEEP1, KEEP2 = 0.7, 0.9   # Dropout(0.3), Dropout(0.1)
HEAD_WIDTH = 128          # conv_1d_heavy's Conv1D(128, 5)


class StackedConvNet(OracleNet):
    """kind 'time_stacked' or 'heavy'; input [B, 16000] raw samples."""

    def __init__(self, kind, num_classes=12, seed=1234):
        super(StackedConvNet, self).__init__(num_classes, seed)
        self.kind = kind
        self.in_shape, widths = NETS[kind]
        self.layers = []
        L, C = self.in_shape

        def add(F, k, pool, l2=True):
            name = self.add_kernel('conv1d', (k, C, F), k * C, k * F, l2=l2)
            Lout = L - k + 1
            lay = {'idx': self.add_bn(F), 'conv': name, 'k': k, 'C': C, 'F': F, 'pool': pool, 'L': L, 'Lout': Lout,
                   'Lp': pool_len(Lout) if pool else Lout}
            self.layers.append(lay)
            return lay['Lp'], F

        L, C = add(32, 1, False)
        for F in widths:
            L, C = add(F, 3, True)
            L, C = add(F, 3, False)
        self.ladder = len(self.layers)
        self.Dd = L * C                       # width of dropout_1
        assert L == 5
        if kind == 'heavy':
            add(HEAD_WIDTH, 5, False, l2=False)
            self.out_kernel, self.out_bias = self.add_kernel('conv1d', (1, HEAD_WIDTH, num_classes), HEAD_WIDTH, num_classes), None
        else:
            self.out_kernel = self.add_kernel('conv1d', (5, C, num_classes), 5 * C, 5 * num_classes, bias=num_classes)
            self.out_bias = self.out_kernel.replace('kernel', 'bias')

    def _layer(self, lay, h, training, cache, mutate, pool_ind):
        idx = lay['idx']
        y, _ = conv_fwd(h, self._p(lay['conv']))
        a = self.bn_act_fwd(idx, y, training, cache)
        ind = None
        if lay['pool']:
            if mutate == 'last_max':
                ind = pool_oracle.argmax(a, lay['Lp'], 0, last=True)
            elif mutate == 'pool_before_act':
                ind = pool_oracle.argmax(y, lay['Lp'], 0)
            elif pool_ind is not None and idx in pool_ind:
                ind = pool_ind[idx]
            else:
                ind = pool_oracle.argmax(a, lay['Lp'], 0)
            a = pool_oracle.fwd(a, ind, 0)
        if cache is not None:
            cache['in%d' % idx], cache['ind%d' % idx] = h, ind
        return a

    def forward(self, x, training=False, seed=0, step=0, cache=None, drop_offset=0, mutate=None, pool_ind=None):
        B = x.shape[0]
        h = x.astype(np.float64).reshape((B,) + self.in_shape)
        if cache is not None:
            cache['batch_stats'] = {}
        for lay in self.layers[:self.ladder]:
            h = self._layer(lay, h, training, cache, mutate, pool_ind)
        f = h.reshape(B, self.Dd)
        keep1 = keep2 = None
        if training:
            keep1 = self.dropout(seed, step, 1, B, self.Dd, KEEP1, drop_offset)
            f = f * keep1 / KEEP1
        if self.kind == 'heavy':
            f = self._layer(self.layers[-1], f.reshape(B, 5, -1), training, cache, mutate, pool_ind).reshape(B, HEAD_WIDTH)
            if training:
                keep2 = self.dropout(seed, step, 2, B, HEAD_WIDTH, KEEP2, drop_offset)
                f = f * keep2 / KEEP2
        p = self.head_fwd(f, self.out_kernel, self.out_bias)
        if cache is not None:
            cache.update(f=f, keep1=keep1, keep2=keep2, p=p)
        return p

    def _layer_bwd(self, lay, dout, cache, grads, relu_masks, mutate, need_dx):
        """dout: gradient wrt the layer's output (pooled if the layer pools) -> gradient wrt its input."""
        idx = lay['idx']
        if lay['pool']:
            dout = pool_oracle.bwd(dout, cache['ind%d' % idx], lay['Lout'], 0)
        dy = self.bn_act_bwd(idx, dout, cache, grads, relu_masks, gate=not (lay['pool'] and mutate == 'no_gate'))
        dx, grads[lay['conv']] = conv_bwd(dy, cache['in%d' % idx], self._p(lay['conv']), lay['L'], need_dx=need_dx)
        return dx

    def loss_and_grads(self, x, y_onehot, seed=0, step=0, drop_offset=0, relu_masks=None, pool_ind=None, mutate=None):
        """Data loss (batch mean) and its gradients (no L2 term)."""
        cache, grads = {}, {}
        B = x.shape[0]
        p = self.forward(x, training=True, seed=seed, step=step, cache=cache, drop_offset=drop_offset, mutate=mutate,
                         pool_ind=pool_ind)
        loss, df = self.head_bwd(p, y_onehot, cache['f'], self.out_kernel, self.out_bias, grads)
        if self.kind == 'heavy':
            da = (df * cache['keep2'] / KEEP2).reshape(B, 1, HEAD_WIDTH)
            df = self._layer_bwd(self.layers[-1], da, cache, grads, relu_masks, mutate, True).reshape(B, self.Dd)
        top = self.layers[self.ladder - 1]
        da = (df * cache['keep1'] / KEEP1).reshape(B, top['Lp'], top['F'])
        for i in range(self.ladder - 1, -1, -1):
            da = self._layer_bwd(self.layers[i], da, cache, grads, relu_masks, mutate, need_dx=i > 0)
        return loss, p, self.ordered(grads), cache
