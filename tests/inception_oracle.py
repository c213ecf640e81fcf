"""NumPy oracle of inception_d1 (reference model.py:312-406, conv_inception_d1_model): forward, loss and every gradient, restated
layer by layer for the CPU cross-checks and the GPU parity tests, plus the float64 reference of AveragePooling1D(3, 1, 'same')
(the dense Conv1D with padding and dilation is oracle_blocks.conv_fwd / conv_bwd).

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
import numpy as np

import pool_oracle
from oracle.layers import relu6
from oracle_blocks import OracleNet, conv_bwd, conv_fwd, same_geometry
from pool_oracle import pool_len

IN_SHAPE = (800, 20)
STEM = (64, 128, 256)
BASE = 32
# (kind, dilation) in model order: blocks 1 .. 12
BLOCKS = (('inc', 2), ('inc', 2), ('red', 0), ('inc', 2), ('inc', 1), ('red', 0), ('inc', 1), ('inc', 1), ('red', 0), ('inc', 1),
          ('inc', 1), ('red', 0))
KEEP = 0.8          # Dropout(0.2)
HEAD_TAPS = 6


# ---- the average pool --------------------------------------------------------------------------------------------------------
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


def same_pool_pad_l(L):
    return pool_oracle.same_geometry(L)[1]          # MaxPool1D(3, 2, 'same'): (1, 1) at an odd L, (0, 1) at an even one


# ---- the net -------------------------------------------------------------------------------------------------------------------
class InceptionD1Net(OracleNet):
    """input [B, 16000] raw samples."""

    def __init__(self, num_classes=12, seed=1234, dtype=np.float64):
        super(InceptionD1Net, self).__init__(num_classes, seed, dtype)
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
        self.out_kernel = self.add_kernel('conv1d', (HEAD_TAPS, C, num_classes), HEAD_TAPS * C, HEAD_TAPS * num_classes, bias=num_classes)
        self.out_bias = self.out_kernel.replace('kernel', 'bias')

    def _add(self, C, F, k, dil, padding, L, pool=None):
        name = self.add_kernel('conv1d', (k, C, F), k * C, k * F, l2=True)
        Lout = L if padding == 'same' else L - dil * (k - 1)
        c = {'idx': self.add_bn(F), 'conv': name, 'k': k, 'dil': dil, 'padding': padding, 'C': C, 'F': F, 'L': L, 'Lout': Lout,
             'pool': pool, 'Lp': Lout if pool is None else pool_len(Lout) if pool == 'valid' else (Lout + 1) // 2}
        self.convs.append(c)
        return c

    # -- forward ------------------------------------------------------------------------------------------------------------
    def _conv(self, c, h, ctx):
        """Conv1D + BatchNormalization + relu6 (+ its max pool) of the activated tensor h = (values, pad_value)."""
        a_in, padv = h
        idx, mutate, cache = c['idx'], ctx['mutate'], ctx['cache']
        dil = 1 if mutate == 'ignore_dilation' else c['dil']
        pad_l = same_geometry(c['L'], c['k'], 1, dil)[1] if c['padding'] == 'same' else 0
        y, ap = conv_fwd(a_in, self._p(c['conv']), 1, dil, pad_l, c['Lout'],
                         pad_value=padv if (mutate == 'pad_before_act' and c['padding'] == 'same') else None)
        a = self.bn_act_fwd(idx, y, ctx['training'], cache)
        rec = cache['bn%d' % idx]
        ind = None
        if c['pool']:
            pind = ctx['pool_ind']
            pl = 0 if c['pool'] == 'valid' else same_pool_pad_l(c['Lout'])
            ind = pind[idx] if pind is not None and idx in pind else pool_oracle.argmax(a, c['Lp'], pl)
            a = pool_oracle.fwd(a, ind, pl)
        cache[idx] = dict(rec, ap=ap, ind=ind, dil=dil, pad_l=pad_l)
        return a, (np.zeros(c['F'], self.dtype) if c['pool'] else relu6(rec['shift']))

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
        ind = pind[key] if pind is not None and key in pind else pool_oracle.argmax(h[0], rec['Lout'], pl)
        ctx['cache'][key] = ind
        bp = pool_oracle.fwd(h[0], ind, pl)
        out = np.concatenate([b3[0], bd[0], bp], axis=2)
        return out, np.zeros(out.shape[2], self.dtype)

    def forward(self, x, training=False, seed=0, step=0, cache=None, drop_offset=0, mutate=None, pool_ind=None):
        B = x.shape[0]
        cache = {} if cache is None else cache
        cache['batch_stats'] = {}
        ctx = {'training': training, 'cache': cache, 'mutate': mutate, 'pool_ind': pool_ind}
        h = (x.astype(self.dtype).reshape((B,) + IN_SHAPE), np.zeros(IN_SHAPE[1], self.dtype))
        for _, c in self.plan:
            h = self._conv(c, h, ctx)
        for rec in self.blocks:
            h = self._inception(rec, h, ctx) if rec['kind'] == 'inc' else self._reduce(rec, h, ctx)
        flat = h[0].reshape(B, self.D)
        keep = None
        if training:
            keep = self.dropout(seed, step, 1, B, self.D, KEEP, drop_offset)
            flat = flat * keep.astype(self.dtype) / self.dtype(KEEP)
        p = self.head_fwd(flat, self.out_kernel, self.out_bias)
        cache.update(f=flat, keep=keep, p=p)
        return p

    # -- backward -----------------------------------------------------------------------------------------------------------
    def _conv_bwd(self, c, dout, cache, grads, relu_masks, need_dx=True):
        """dout: gradient wrt the layer's (pooled) activated output -> gradient wrt its activated input."""
        idx = c['idx']
        cc = cache[idx]
        if c['pool']:
            dout = pool_oracle.bwd(dout, cc['ind'], c['Lout'], 0 if c['pool'] == 'valid' else same_pool_pad_l(c['Lout']))
        dy = self.bn_act_bwd(idx, dout, cache, grads, relu_masks)
        dx, grads[c['conv']] = conv_bwd(dy, cc['ap'], self._p(c['conv']), c['L'], 1, cc['dil'], cc['pad_l'], need_dx=need_dx)
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
        dx = pool_oracle.bwd(dJ[:, :, w0 + w1:], cache['mixed%d' % rec['id']], rec['L'], same_pool_pad_l(rec['L']))
        dx = dx + bw(cs[1], bw(cs[2], bw(cs[3], dJ[:, :, w0:w0 + w1])))
        dx = dx + bw(cs[0], dJ[:, :, :w0])
        return dx

    def loss_and_grads(self, x, y_onehot, seed=0, step=0, drop_offset=0, relu_masks=None, pool_ind=None, mutate=None):
        """Data loss (batch mean) and its gradients (no L2 term)."""
        cache, grads = {}, {}
        B = x.shape[0]
        p = self.forward(x, training=True, seed=seed, step=step, cache=cache, drop_offset=drop_offset, mutate=mutate, pool_ind=pool_ind)
        loss, df = self.head_bwd(p, y_onehot, cache['f'], self.out_kernel, self.out_bias, grads)
        top = self.blocks[-1]
        da = (df * cache['keep'].astype(self.dtype) / self.dtype(KEEP)).reshape(B, top['Lout'], top['Cout'])
        for rec in reversed(self.blocks):
            da = self._inception_bwd(rec, da, cache, grads, relu_masks, mutate) if rec['kind'] == 'inc' else \
                self._reduce_bwd(rec, da, cache, grads, relu_masks)
        for i in range(len(self.plan) - 1, -1, -1):
            da = self._conv_bwd(self.plan[i][1], da, cache, grads, relu_masks, need_dx=i > 0)
        return loss, p, self.ordered(grads), cache
