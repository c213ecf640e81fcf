"""NumPy oracle of inception_d1 (reference model.py:312-406, conv_inception_d1_model): forward, loss and every gradient, restated
layer by layer for the CPU cross-checks and the GPU parity tests, plus float64 references of the two new operations
(dense Conv1D with padding / dilation / channel windows, AveragePooling1D(3, 1, 'same')).

TEST INFRASTRUCTURE ONLY.  Every convolution is Conv1D(F, k, stride 1, no bias) -> BatchNormalization -> relu6; a _reduce_conv
adds MaxPool1D(3, strides=2) whose gradient goes to the FIRST maximum of a window (TF MaxPoolGrad).  The net runs in float64 by
default; `dtype=np.float32` runs the same arithmetic in float32 (the float32-against-float64 figures of the GPU test's docstring).

`relu_masks` (Conv1D number -> gate) / `pool_ind` (Conv1D number of a pooled convolution, or 'mixed<block>' for the pool branch
of a reduce block -> winners) hand the device's own decisions to the backward pass; `mutate` names a deliberately wrong variant:
  'avg_count_include_pad'  the average pool divides by 3 at the two ends of a clip as well
  'ignore_dilation'        every convolution has dilation 1
  'pad_before_act'         SAME convolutions pad the RAW tensor: a padded tap contributes relu6(shift) of its producer
  'concat_order'           an inception block joins [branch5x5, branch1x1, branch3x3dbl, branch_pool]
"""
from collections import OrderedDict

import numpy as np

from mts_oracle import pool_same_argmax, pool_same_bwd, pool_same_fwd
from oracle.layers import (BN_EPS, bn_infer_fwd, cce_fwd_bwd, dropout_key, dropout_mask, relu6, relu6_mask,
                           softmax, softmax_bwd)
from stacked_oracle import glorot, pool_argmax, pool_bwd, pool_fwd, pool_len

IN_SHAPE = (800, 20)
STEM = (64, 128, 256)
BASE = 32
# (kind, dilation) in model order: blocks 1 .. 12
BLOCKS = (('inc', 2), ('inc', 2), ('red', 0), ('inc', 2), ('inc', 1), ('red', 0), ('inc', 1), ('inc', 1), ('red', 0), ('inc', 1),
          ('inc', 1), ('red', 0))
KEEP = 0.8          # Dropout(0.2)
HEAD_TAPS = 6


# ---- the two operations -----------------------------------------------------------------------------------------------------
def same_pad_l(k, dil):
    """TF SAME at stride 1: dil * (k - 1) zeros in all, the smaller half in front."""
    return dil * (k - 1) // 2


def conv_fwd(a, W, dil=1, pad_l=0, Lout=None, pad_value=None):
    """a [B, L, Cin] (ACTIVATED), W [k, Cin, F] -> [B, Lout, F]: y[b,t] = sum_j a[b, t - pad_l + dil*j] W[j], 0 outside [0, L)
    (pad_value [Cin]: the mutated padding).  Without Lout: L if there is padding in front, else VALID.  -> (y, the padded input)"""
    k, L = W.shape[0], a.shape[1]
    span = dil * (k - 1)
    if Lout is None:
        Lout = L if pad_l else L - span
    pad_r = Lout - L - pad_l + span
    assert pad_r >= 0
    ap = np.zeros((a.shape[0], L + pad_l + pad_r, a.shape[2]), a.dtype)
    if pad_value is not None:
        ap[:] = pad_value
    ap[:, pad_l:pad_l + L] = a
    y = ap[:, 0:Lout] @ W[0]
    for j in range(1, k):
        y += ap[:, dil * j:dil * j + Lout] @ W[j]
    return y, ap


def conv_bwd(dy, ap, W, dil, pad_l, L, need_dx=True):
    """-> (gradient wrt the activated input [B, L, Cin], dW)"""
    k, Lout = W.shape[0], dy.shape[1]
    dy2 = dy.reshape(-1, dy.shape[2])
    dW = np.stack([ap[:, dil * j:dil * j + Lout].reshape(-1, ap.shape[2]).T @ dy2 for j in range(k)])
    dx = None
    if need_dx:
        dap = np.zeros_like(ap)
        for j in range(k):
            dap[:, dil * j:dil * j + Lout] += dy @ W[j].T
        dx = dap[:, pad_l:pad_l + L]
    return dx, dW


def avgpool_counts(L, include_pad=False):
    n = np.full(L, 3.0)
    if not include_pad:
        n[0] -= 1
        n[-1] -= 1       # (L = 1: the one row loses both neighbours)
    return n


def avgpool_fwd(a, include_pad=False):
    """AveragePooling1D(3, 1, 'same') of a [B, L, C]: TF divides by the rows that exist."""
    ap = np.pad(a, ((0, 0), (1, 1), (0, 0)))
    L = a.shape[1]
    n = avgpool_counts(L, include_pad).astype(a.dtype)
    return (ap[:, 0:L] + ap[:, 1:L + 1] + ap[:, 2:L + 2]) / n[None, :, None]


def avgpool_bwd(dz, include_pad=False):
    L = dz.shape[1]
    g = dz / avgpool_counts(L, include_pad).astype(dz.dtype)[None, :, None]
    gp = np.pad(g, ((0, 0), (1, 1), (0, 0)))
    return gp[:, 0:L] + gp[:, 1:L + 1] + gp[:, 2:L + 2]


def bn_train_fwd(y, gamma, beta, eps=BN_EPS):
    """oracle.layers.bn_train_fwd with the column sums taken in float64 whatever y's type is (in float64 the same function): the
    device adds its float32 tile sums in double, so a float32 run that summed thousands of rows in float32 would charge the
    number format with an error the kernels do not make."""
    t = y.dtype.type
    mean = y.mean(axis=(0, 1), dtype=np.float64)
    var = ((y - mean) ** 2).mean(axis=(0, 1), dtype=np.float64)
    rstd = (1.0 / np.sqrt(var + eps)).astype(t)
    mean, var = mean.astype(t), var.astype(t)
    inv = rstd * gamma
    return y * inv + (beta - mean * inv), (mean, var, rstd)


def bn_train_bwd(dout, y, gamma, stats):
    """oracle.layers.bn_train_bwd, its two column sums in float64 as well."""
    mean, var, rstd = stats
    t = y.dtype.type
    n = y.shape[0] * y.shape[1]
    xhat = (y - mean) * rstd
    dbeta = dout.sum(axis=(0, 1), dtype=np.float64)
    dgamma = (dout * xhat).sum(axis=(0, 1), dtype=np.float64)
    dy = (gamma * rstd) * (dout - (dbeta / n).astype(t) - xhat * (dgamma / n).astype(t))
    return dy, dgamma.astype(t), dbeta.astype(t)


def same_pool_pad_l(L):
    return L & 1          # MaxPool1D(3, 2, 'same'): (1, 1) at an odd L, (0, 1) at an even one


# ---- the net -------------------------------------------------------------------------------------------------------------------
class InceptionD1Net(object):
    """input [B, 16000] raw samples."""

    def __init__(self, num_classes=12, seed=1234, dtype=np.float64):
        self.nc, self.dtype = num_classes, dtype
        self.rng = np.random.RandomState(seed)
        self.params, self.state = OrderedDict(), OrderedDict()
        self.convs = []          # records of Conv1D 1 .. 79 in creation order
        self.plan = []           # the stem: ('conv', record) in model order
        L, C = IN_SHAPE
        c = self._add(C, 32, 1, 1, 'same', L)
        self.plan.append(('conv', c))
        L, C = c['Lout'], 32
        for F in STEM:
            c = self._add(C, F, 3, 1, 'valid', L, pool='valid')
            self.plan.append(('conv', c))
            L, C = c['Lp'], F
            c = self._add(C, F, 3, 1, 'valid', L)
            self.plan.append(('conv', c))
            L = c['Lout']
        self.blocks = []
        for bid, (kind, d) in enumerate(BLOCKS, 1):
            b = BASE
            if kind == 'inc':
                rec = {'id': bid, 'kind': 'inc', 'L': L, 'Cin': C, 'convs': [
                    self._add(C, 2 * b, 1, 1, 'same', L),
                    self._add(C, 3 * b // 2, 1, 1, 'same', L), self._add(3 * b // 2, 2 * b, 3, 2, 'same', L),
                    self._add(C, 2 * b, 1, 1, 'same', L), self._add(2 * b, 3 * b, 3, d, 'same', L), self._add(3 * b, 3 * b, 3, d, 'same', L),
                    self._add(C, b, 1, 1, 'same', L)]}
                C = 2 * b + 2 * b + 3 * b + b
            else:
                rec = {'id': bid, 'kind': 'red', 'L': L, 'Cin': C, 'convs': [
                    self._add(C, 6 * b, 3, 1, 'same', L, pool='same'),
                    self._add(C, b, 1, 1, 'same', L), self._add(b, 3 * b // 2, 3, 1, 'same', L),
                    self._add(3 * b // 2, 3 * b // 2, 3, 1, 'same', L, pool='same')]}
                L, C = (L + 1) // 2, 6 * b + 3 * b // 2 + C
            rec['Lout'], rec['Cout'] = L, C
            self.blocks.append(rec)
        assert (L, C) == (HEAD_TAPS, 496)
        self.D = L * C
        self.l2_names = [c['conv'] for c in self.convs]
        n = len(self.convs) + 1
        self.out_kernel, self.out_bias = 'conv1d_%d/kernel' % n, 'conv1d_%d/bias' % n
        self.params[self.out_kernel] = glorot(self.rng, (HEAD_TAPS, C, num_classes), HEAD_TAPS * C, HEAD_TAPS * num_classes)
        self.params[self.out_bias] = np.zeros(num_classes, np.float32)

    def _add(self, C, F, k, dil, padding, L, pool=None):
        n = len(self.convs) + 1
        name, base = 'conv1d_%d/kernel' % n, 'batch_normalization_%d/' % n
        self.params[name] = glorot(self.rng, (k, C, F), k * C, k * F)
        self.params[base + 'gamma'] = np.ones(F, np.float32)
        self.params[base + 'beta'] = np.zeros(F, np.float32)
        self.state[base + 'moving_mean'] = np.zeros(F, np.float32)
        self.state[base + 'moving_variance'] = np.ones(F, np.float32)
        Lout = L if padding == 'same' else L - dil * (k - 1)
        c = {'idx': n, 'conv': name, 'k': k, 'dil': dil, 'padding': padding, 'C': C, 'F': F, 'L': L, 'Lout': Lout, 'pool': pool,
             'Lp': Lout if pool is None else pool_len(Lout) if pool == 'valid' else (Lout + 1) // 2}
        self.convs.append(c)
        return c

    def count_params(self):
        return sum(v.size for v in self.params.values()) + sum(v.size for v in self.state.values())

    def _p(self, name):
        return self.params[name].astype(self.dtype)

    # -- forward ------------------------------------------------------------------------------------------------------------
    def _conv(self, c, h, ctx):
        """Conv1D + BatchNormalization + relu6 (+ its max pool) of the activated tensor h = (values, pad_value)."""
        a_in, padv = h
        idx, mutate = c['idx'], ctx['mutate']
        dil = 1 if mutate == 'ignore_dilation' else c['dil']
        pad_l = same_pad_l(c['k'], dil) if c['padding'] == 'same' else 0
        y, ap = conv_fwd(a_in, self._p(c['conv']), dil, pad_l, c['Lout'],
                         pad_value=padv if (mutate == 'pad_before_act' and c['padding'] == 'same') else None)
        ga, be = self._p('batch_normalization_%d/gamma' % idx), self._p('batch_normalization_%d/beta' % idx)
        if ctx['training']:
            pre, st = bn_train_fwd(y, ga, be)
            shift = be - st[0] * st[2] * ga
        else:
            st = None
            mm = self.state['batch_normalization_%d/moving_mean' % idx].astype(self.dtype)
            mv = self.state['batch_normalization_%d/moving_variance' % idx].astype(self.dtype)
            pre = bn_infer_fwd(y, ga, be, mm, mv)
            shift = be - mm * (ga / np.sqrt(mv + BN_EPS))
        a = relu6(pre)
        ind = None
        if c['pool']:
            pind = ctx['pool_ind']
            if c['pool'] == 'valid':
                ind = pind[idx] if pind is not None and idx in pind else pool_argmax(a)
                a = pool_fwd(a, ind)
            else:
                pl = same_pool_pad_l(c['Lout'])
                ind = pind[idx] if pind is not None and idx in pind else pool_same_argmax(a, pl)
                a = pool_same_fwd(a, ind, pl)
        cache = ctx['cache']
        if cache is not None:
            cache[idx] = {'ap': ap, 'y': y, 'st': st, 'ind': ind, 'dil': dil, 'pad_l': pad_l, 'pre': pre}
            if ctx['training']:
                cache['batch_stats'][idx] = (st[0], st[1])
        return a, (np.zeros(c['F'], self.dtype) if c['pool'] else relu6(shift))

    def _order(self, ctx):
        return (1, 0, 2, 3) if ctx['mutate'] == 'concat_order' else (0, 1, 2, 3)

    def _inception(self, rec, h, ctx):
        cs = rec['convs']
        b1 = self._conv(cs[0], h, ctx)
        b5 = self._conv(cs[2], self._conv(cs[1], h, ctx), ctx)
        b3 = self._conv(cs[5], self._conv(cs[4], self._conv(cs[3], h, ctx), ctx), ctx)
        z = avgpool_fwd(h[0], include_pad=ctx['mutate'] == 'avg_count_include_pad')
        bp = self._conv(cs[6], (z, np.zeros(z.shape[2], self.dtype)), ctx)
        br = [b1, b5, b3, bp]
        order = self._order(ctx)
        return (np.concatenate([br[i][0] for i in order], axis=2), np.concatenate([br[i][1] for i in order]))

    def _reduce(self, rec, h, ctx):
        cs = rec['convs']
        b3 = self._conv(cs[0], h, ctx)
        bd = self._conv(cs[3], self._conv(cs[2], self._conv(cs[1], h, ctx), ctx), ctx)
        key, pl = 'mixed%d' % rec['id'], same_pool_pad_l(rec['L'])
        pind = ctx['pool_ind']
        ind = pind[key] if pind is not None and key in pind else pool_same_argmax(h[0], pl)
        if ctx['cache'] is not None:
            ctx['cache'][key] = ind
        bp = pool_same_fwd(h[0], ind, pl)
        out = np.concatenate([b3[0], bd[0], bp], axis=2)
        return out, np.zeros(out.shape[2], self.dtype)

    def forward(self, x, training=False, seed=0, step=0, cache=None, drop_offset=0, mutate=None, pool_ind=None):
        B = x.shape[0]
        ctx = {'training': training, 'cache': cache, 'mutate': mutate, 'pool_ind': pool_ind}
        if cache is not None:
            cache['batch_stats'] = {}
        h = (x.astype(self.dtype).reshape((B,) + IN_SHAPE), np.zeros(IN_SHAPE[1], self.dtype))
        for _, c in self.plan:
            h = self._conv(c, h, ctx)
        for rec in self.blocks:
            h = self._inception(rec, h, ctx) if rec['kind'] == 'inc' else self._reduce(rec, h, ctx)
        flat = h[0].reshape(B, self.D)
        keep = None
        if training:
            keep = dropout_mask(dropout_key(seed, step, 1), B * self.D, KEEP, offset=drop_offset * self.D).reshape(B, self.D)
            flat = flat * keep.astype(self.dtype) / self.dtype(KEEP)
        logits = flat @ self._p(self.out_kernel).reshape(self.D, self.nc) + self._p(self.out_bias)
        p = softmax(logits)
        if cache is not None:
            cache.update(f=flat, keep=keep, p=p)
        return p

    # -- backward -----------------------------------------------------------------------------------------------------------
    def _conv_bwd(self, c, dout, cache, grads, relu_masks, need_dx=True):
        """dout: gradient wrt the layer's (pooled) activated output -> gradient wrt its activated input."""
        idx = c['idx']
        cc = cache[idx]
        ga = self._p('batch_normalization_%d/gamma' % idx)
        mask = relu_masks[idx].astype(self.dtype) if relu_masks is not None and idx in relu_masks else relu6_mask(cc['pre'])
        if c['pool'] == 'valid':
            dout = pool_bwd(dout, cc['ind'], c['Lout'])
        elif c['pool'] == 'same':
            dout = pool_same_bwd(dout, cc['ind'], c['Lout'], same_pool_pad_l(c['Lout']))
        dy, dga, dbe = bn_train_bwd(dout * mask, cc['y'], ga, cc['st'])
        grads['batch_normalization_%d/gamma' % idx] = dga
        grads['batch_normalization_%d/beta' % idx] = dbe
        dx, dW = conv_bwd(dy, cc['ap'], self._p(c['conv']), cc['dil'], cc['pad_l'], c['L'], need_dx=need_dx)
        grads[c['conv']] = dW
        return dx

    def _inception_bwd(self, rec, dJ, cache, grads, relu_masks, mutate):
        cs = rec['convs']
        widths = [cs[0]['F'], cs[2]['F'], cs[5]['F'], cs[6]['F']]
        order = (1, 0, 2, 3) if mutate == 'concat_order' else (0, 1, 2, 3)
        d, off = [None] * 4, 0
        for i in order:
            d[i] = dJ[:, :, off:off + widths[i]]
            off += widths[i]
        bw = lambda c, g: self._conv_bwd(c, g, cache, grads, relu_masks)
        # the four contributions to the block input's gradient, in the device's order (the last branch first)
        dx = avgpool_bwd(bw(cs[6], d[3]), include_pad=mutate == 'avg_count_include_pad')
        dx = dx + bw(cs[3], bw(cs[4], bw(cs[5], d[2])))
        dx = dx + bw(cs[1], bw(cs[2], d[1]))
        dx = dx + bw(cs[0], d[0])
        return dx

    def _reduce_bwd(self, rec, dJ, cache, grads, relu_masks):
        cs = rec['convs']
        w0, w1 = cs[0]['F'], cs[3]['F']
        bw = lambda c, g: self._conv_bwd(c, g, cache, grads, relu_masks)
        dx = pool_same_bwd(dJ[:, :, w0 + w1:], cache['mixed%d' % rec['id']], rec['L'], same_pool_pad_l(rec['L']))
        dx = dx + bw(cs[1], bw(cs[2], bw(cs[3], dJ[:, :, w0:w0 + w1])))
        dx = dx + bw(cs[0], dJ[:, :, :w0])
        return dx

    def loss_and_grads(self, x, y_onehot, seed=0, step=0, drop_offset=0, relu_masks=None, pool_ind=None, mutate=None):
        """Data loss (batch mean) and its gradients (no L2 term)."""
        cache = {}
        B = x.shape[0]
        p = self.forward(x, training=True, seed=seed, step=step, cache=cache, drop_offset=drop_offset, mutate=mutate, pool_ind=pool_ind)
        loss, per, dp = cce_fwd_bwd(p, y_onehot.astype(self.dtype))
        dl = softmax_bwd(dp, p)
        grads = OrderedDict()
        Wo = self._p(self.out_kernel).reshape(self.D, self.nc)
        grads[self.out_kernel] = (cache['f'].T @ dl).reshape(self.params[self.out_kernel].shape)
        grads[self.out_bias] = dl.sum(axis=0)
        top = self.blocks[-1]
        da = ((dl @ Wo.T) * cache['keep'].astype(self.dtype) / self.dtype(KEEP)).reshape(B, top['Lout'], top['Cout'])
        for rec in reversed(self.blocks):
            da = self._inception_bwd(rec, da, cache, grads, relu_masks, mutate) if rec['kind'] == 'inc' else \
                self._reduce_bwd(rec, da, cache, grads, relu_masks)
        for i in range(len(self.plan) - 1, -1, -1):
            da = self._conv_bwd(self.plan[i][1], da, cache, grads, relu_masks, need_dx=i > 0)
        return loss, p, OrderedDict((k, grads[k]) for k in self.params), cache
