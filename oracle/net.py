"""Oracle: the Depthwise1D networks, forward + backward (+ step for the headline model).

TEST INFRASTRUCTURE ONLY (see oracle/__init__.py).

  * TimeSlicedAttentionNet - reference model.py:775-838
    (`conv_1d_time_sliced_with_attention_model`, the model train.py:50-54 builds);
    layer table SURVEY.md Appendix B.1, variable shapes pinned by fixture K1.
  * The residual family, stated once in ResidualFamilyNet (table builder _add_block / _add_plain / _add_dense over a
    KerasNames allocator, one block / plain-layer / dense-tail forward and backward, one loss_and_grads walker) - the
    Python twin of the block planner in csrc/net_logmfcc.hip.  Its four members keep their table, stem and pooling head:
      - LogMfccNet - model.py:1400-1479 (`conv_1d_log_mfcc_model`), Appendix B.2; at 257 features and 12 classes it is
        `conv_1d_spectrogram_model` (model.py:1482-1561)
      - SteffeNet - model.py:1663-1726 (`steffeNet`)
      - Conv1dResidualNet - model.py:841-908 (`conv_1d_residual_model`)
      - MfccAndRawNet - model.py:1563-1660 (`conv_1d_mfcc_and_raw_model`)

Parameters are kept in an ordered dict under their Keras variable names so the
HIP implementation's flat parameter buffer can be compared tensor by tensor.
"""
from collections import OrderedDict

import numpy as np

from . import layers as L

# (stride, padding, Cout) of the 11 depthwise blocks of model.py:812-817:
# _context_conv(128) then 5 x _reduce_block(n) = [_reduce_conv(n, s2 same), _context_conv(n, s1 valid)]
TS_BLOCKS = [(1, 'valid', 128),
             (2, 'same', 192), (1, 'valid', 192),
             (2, 'same', 256), (1, 'valid', 256),
             (2, 'same', 320), (1, 'valid', 320),
             (2, 'same', 384), (1, 'valid', 384),
             (2, 'same', 512), (1, 'valid', 512)]


def glorot_uniform(rng, shape, fan_in, fan_out):
    """Keras glorot_uniform: U(-l, l), l = sqrt(6/(fan_in+fan_out))."""
    limit = np.sqrt(6.0 / (fan_in + fan_out))
    return rng.uniform(-limit, limit, size=shape).astype(np.float32)


class TimeSlicedAttentionNet(object):
    def __init__(self, num_classes=12, filter_mult=1, input_size=16000, seed=87654321,
                 dtype=np.float64):
        self.dtype = dtype
        self.num_classes = num_classes
        self.input_size = input_size
        rng = np.random.RandomState(seed)
        P = OrderedDict()
        S = OrderedDict()
        c0 = 128 * filter_mult
        P['conv1d_1/kernel'] = glorot_uniform(rng, (3, 40, c0), 3 * 40, 3 * c0)
        self._add_bn(P, S, 1, c0)
        self.blocks = []
        cin = c0
        Lcur = L.valid_len(-(-input_size // 20), 3, 2)
        for i, (stride, padding, cout) in enumerate(TS_BLOCKS):
            cout *= filter_mult
            # DepthwiseConv2D kernel [1,3,C,1]: fan_in = 3*C, fan_out = 3*1
            P['depthwise_conv2d_%d/depthwise_kernel' % (i + 1)] = glorot_uniform(
                rng, (1, 3, cin, 1), 3 * cin, 3)
            P['conv1d_%d/kernel' % (i + 2)] = glorot_uniform(rng, (1, cin, cout), cin, cout)
            self._add_bn(P, S, i + 2, cout)
            if padding == 'same':
                Lout, pl, pr = L.same_pad(Lcur, 3, stride)
            else:
                Lout, pl, pr = L.valid_len(Lcur, 3, stride), 0, 0
            self.blocks.append(dict(stride=stride, pad=(pl, pr), cin=cin, cout=cout, Lin=Lcur, Lout=Lout))
            cin, Lcur = cout, Lout
        self.T, self.C = Lcur, cin
        P['dense_1/kernel'] = glorot_uniform(rng, (self.T * cin, self.T), self.T * cin, self.T)
        P['dense_1/bias'] = np.zeros((self.T,), np.float32)
        P['dense_2/kernel'] = glorot_uniform(rng, (2 * cin, num_classes), 2 * cin, num_classes)
        self.params = P
        self.state = S
        self.l2_names = [k for k in P if k.endswith('kernel')]
        self.drop_keep = 0.6       # Dropout(0.4), model.py:819,828
        self.label_smoothing = 0.1  # model.py:835-836

    @staticmethod
    def _add_bn(P, S, idx, c):
        P['batch_normalization_%d/gamma' % idx] = np.ones((c,), np.float32)
        P['batch_normalization_%d/beta' % idx] = np.zeros((c,), np.float32)
        S['batch_normalization_%d/moving_mean' % idx] = np.zeros((c,), np.float32)
        S['batch_normalization_%d/moving_variance' % idx] = np.ones((c,), np.float32)

    def count_params(self):
        return sum(v.size for v in self.params.values()) + sum(v.size for v in self.state.values())

    # -- helpers ---------------------------------------------------------------
    def _p(self, name):
        return self.params[name].astype(self.dtype)

    def _bn_fwd(self, idx, y, training, cache):
        g = self._p('batch_normalization_%d/gamma' % idx)
        b = self._p('batch_normalization_%d/beta' % idx)
        if training:
            pre, stats = L.bn_train_fwd(y, g, b)
            cache['bn%d' % idx] = (y, g, stats, pre)
            cache.setdefault('batch_stats', OrderedDict())[idx] = (stats[0], stats[1])
        else:
            pre = L.bn_infer_fwd(y, g, b,
                                 self.state['batch_normalization_%d/moving_mean' % idx].astype(self.dtype),
                                 self.state['batch_normalization_%d/moving_variance' % idx].astype(self.dtype))
        return L.relu6(pre)

    def _bn_bwd(self, idx, da, cache, grads):
        y, g, stats, pre = cache['bn%d' % idx]
        mask = L.relu6_mask(pre)
        override = cache.get('relu_masks')
        if override is not None and idx in override:
            # decision-aligned parity: use the mask another implementation actually took (a
            # pre-activation within rounding of a ReLU6 kink may fall on either side in f32 vs f64)
            mask = np.asarray(override[idx], dtype=self.dtype).reshape(pre.shape)
        dpre = da * mask
        dy, dg, db = L.bn_train_bwd(dpre, y, g, stats)
        grads['batch_normalization_%d/gamma' % idx] = dg
        grads['batch_normalization_%d/beta' % idx] = db
        return dy

    # -- forward ---------------------------------------------------------------
    def forward(self, x, training=False, seed=0, step=0, cache=None, drop_offset=0):
        """x [B, input_size] -> softmax probabilities [B, num_classes].
        drop_offset = global index of row 0 (for data-parallel shards)."""
        dt = self.dtype
        cache = {} if cache is None else cache
        x = np.asarray(x, dtype=dt)
        B = x.shape[0]
        frames = L.frame_same(x, 40, 20)                                   # model.py:805
        y, cols = L.conv1d_fwd(frames, self._p('conv1d_1/kernel'), stride=2)   # model.py:807
        cache['conv1_cols'] = cols
        a = self._bn_fwd(1, y, training, cache)
        for i, blk in enumerate(self.blocks):                              # model.py:812-817
            w = self._p('depthwise_conv2d_%d/depthwise_kernel' % (i + 1)).reshape(3, blk['cin'])
            z = L.dwconv_fwd(a, w, blk['stride'], blk['pad'])
            cache['dw%d' % (i + 1)] = (a, w)
            W = self._p('conv1d_%d/kernel' % (i + 2)).reshape(blk['cin'], blk['cout'])
            y = L.pw_fwd(z, W)
            cache['pw%d' % (i + 2)] = (z, W)
            a = self._bn_fwd(i + 2, y, training, cache)
        T, C = self.T, self.C
        flat = a.reshape(B, T * C)                                         # Flatten: index t*C + c
        if training:
            m1 = L.dropout_mask(L.dropout_key(seed, step, 1), B * T * C, self.drop_keep,
                                drop_offset * T * C).reshape(B, T * C)
            fd = flat * m1 / dt(self.drop_keep)
        else:
            m1 = None
            fd = flat
        W1, b1 = self._p('dense_1/kernel'), self._p('dense_1/bias')
        att = L.softmax(fd @ W1 + b1, axis=1)                              # model.py:820-821  [B, T]
        xa = a * att[:, :, None]                                           # model.py:824
        xmax = xa.max(axis=1)                                              # model.py:825
        xavg = a.mean(axis=1)                                              # model.py:826 (unweighted x)
        feat = np.concatenate([xmax, xavg], axis=1)                        # model.py:827
        if training:
            m2 = L.dropout_mask(L.dropout_key(seed, step, 2), B * 2 * C, self.drop_keep,
                                drop_offset * 2 * C).reshape(B, 2 * C)
            featd = feat * m2 / dt(self.drop_keep)
        else:
            m2 = None
            featd = feat
        W2 = self._p('dense_2/kernel')
        p = L.softmax(featd @ W2, axis=1)                                  # model.py:829-830
        cache['tail'] = (a, m1, fd, W1, att, xa, xmax, m2, featd, W2, p)
        return p

    def reg_loss(self):
        return sum(L.L2_COEF * float((self._p(k) ** 2).sum()) for k in self.l2_names)

    # -- backward --------------------------------------------------------------
    def loss_and_grads(self, x, y_onehot, seed=0, step=0, drop_offset=0, loss_scale_B=None,
                       relu_masks=None, pool_ind=None):
        """Returns (data_loss, probs, grads incl. L2 terms, cache).  loss_scale_B: divide the
        data-loss gradient by this batch size instead of the local one (data-parallel mean).
        relu_masks {bn index: 0/1 array} / pool_ind [B,T,C] override the discrete decisions of the
        backward pass (ReLU6 masks, max-pool winners) with those another implementation took."""
        dt = self.dtype
        cache = {'relu_masks': relu_masks}
        p = self.forward(x, training=True, seed=seed, step=step, cache=cache, drop_offset=drop_offset)
        y_onehot = np.asarray(y_onehot, dtype=dt)
        loss, per, dp = L.smooth_cce_fwd_bwd(p, y_onehot, self.label_smoothing)
        B = x.shape[0]
        if loss_scale_B is not None:
            dp = dp * dt(B) / dt(loss_scale_B)
        grads = OrderedDict()
        a, m1, fd, W1, att, xa, xmax, m2, featd, W2, p = cache['tail']
        T, C = self.T, self.C
        dl2 = L.softmax_bwd(dp, p, axis=1)
        grads['dense_2/kernel'] = featd.T @ dl2
        dfeat = (dl2 @ W2.T) * m2 / dt(self.drop_keep)
        dxmax, dxavg = dfeat[:, :C], dfeat[:, C:]
        # reduce_max gradient: split equally among ties (_MinOrMaxGrad)
        ind = (xa == xmax[:, None, :]).astype(dt)
        if pool_ind is not None:
            ind = np.asarray(pool_ind, dtype=dt).reshape(xa.shape)
        ind = ind / ind.sum(axis=1, keepdims=True)
        dxa = ind * dxmax[:, None, :]
        da = dxa * att[:, :, None] + dxavg[:, None, :] / dt(T)
        datt = (dxa * a).sum(axis=2)
        dl1 = L.softmax_bwd(datt, att, axis=1)
        grads['dense_1/kernel'] = fd.T @ dl1
        grads['dense_1/bias'] = dl1.sum(axis=0)
        da = da + ((dl1 @ W1.T) * m1 / dt(self.drop_keep)).reshape(B, T, C)
        for i in reversed(range(len(self.blocks))):
            blk = self.blocks[i]
            dy = self._bn_bwd(i + 2, da, cache, grads)
            z, W = cache['pw%d' % (i + 2)]
            dz, dW = L.pw_bwd(dy, z, W)
            grads['conv1d_%d/kernel' % (i + 2)] = dW.reshape(1, blk['cin'], blk['cout'])
            a_in, w = cache['dw%d' % (i + 1)]
            da, dw = L.dwconv_bwd(dz, a_in, w, blk['stride'], blk['pad'])
            grads['depthwise_conv2d_%d/depthwise_kernel' % (i + 1)] = dw.reshape(1, 3, blk['cin'], 1)
        dy = self._bn_bwd(1, da, cache, grads)
        Wc = self._p('conv1d_1/kernel')
        B2, Lo, Co = dy.shape
        grads['conv1d_1/kernel'] = (cache['conv1_cols'].T @ dy.reshape(B2 * Lo, Co)).reshape(Wc.shape)
        for k in self.l2_names:                                            # kernel_regularizer=l2(1e-5)
            grads[k] = grads[k] + dt(2.0 * L.L2_COEF) * self._p(k)
        ordered = OrderedDict((k, grads[k]) for k in self.params)
        return loss, p, ordered, cache

    # -- training step ---------------------------------------------------------
    def init_optimizer(self, kind='rmsprop'):
        self.opt_kind = kind
        self.slots = OrderedDict((k, np.zeros(v.shape, self.dtype)) for k, v in self.params.items())
        self.master = OrderedDict((k, v.astype(self.dtype)) for k, v in self.params.items())

    def train_step(self, x, y_onehot, lr, seed=0, step=0):
        """One Keras train_on_batch: forward, loss (+L2), backward, optimizer update, BN
        moving-average update.  Returns (total_loss, categorical_accuracy)."""
        loss, p, grads, cache = self.loss_and_grads(x, y_onehot, seed, step)
        total = loss + self.reg_loss()
        for k in self.params:
            if self.opt_kind == 'rmsprop':
                self.master[k], self.slots[k] = L.rmsprop_step(self.master[k], grads[k].reshape(self.master[k].shape),
                                                               self.slots[k], lr)
            else:
                self.master[k], self.slots[k] = L.sgd_momentum_step(self.master[k], grads[k].reshape(self.master[k].shape),
                                                                    self.slots[k], lr)
            self.params[k] = self.master[k].astype(np.float32) if self.dtype == np.float32 else self.master[k]
        for idx, (mean, var) in cache['batch_stats'].items():
            for nm, val in (('moving_mean', mean), ('moving_variance', var)):
                key = 'batch_normalization_%d/%s' % (idx, nm)
                self.state[key] = L.bn_moving_update(self.state[key].astype(self.dtype), val)
        acc = float((p.argmax(axis=1) == np.asarray(y_onehot).argmax(axis=1)).mean())
        return float(total), acc


# ================================================================================================
# The residual family: conv_1d_log_mfcc / conv_1d_spectrogram, steffeNet,
# conv_1d_residual, conv_1d_mfcc_and_raw.  One table builder and one forward / backward walker (ResidualFamilyNet); the four
# classes below it hold their layer table, their stem and their pooling head.
# ================================================================================================
def maxpool_same_fwd(a, pool):
    """MaxPool1D(pool_size=pool, strides=pool, padding='same') (model.py:1440): ceil(L / pool) windows; TF pads the END
    of a length that is not a multiple of the pool (with -inf for max pooling), so the last window is short."""
    if pool == 1:
        return a, None
    B, L, C = a.shape
    Lo = -(-L // pool)
    if Lo * pool != L:
        a = np.concatenate([a, np.full((B, Lo * pool - L, C), -np.inf, dtype=a.dtype)], axis=1)
    w = a.reshape(B, Lo, pool, C)
    return w.max(axis=2), w.argmax(axis=2)     # first maximum wins (MaxPoolGrad semantics)


def maxpool_same_bwd(do, arg, pool, L):
    if pool == 1:
        return do
    B, Lo, C = do.shape
    d = np.zeros((B, Lo, pool, C), dtype=do.dtype)
    for j in range(pool):
        d[:, :, j, :] = do * (arg == j)
    return d.reshape(B, Lo * pool, C)[:, :L, :]   # the padded positions never win


def maxpool3_same_fwd(a, stride):
    """MaxPool1D(pool_size=3, strides=stride, padding='same') on [B, L, C]: -inf padding (TF pads max-pool windows
    with the lowest value), the FIRST maximum of a window wins (MaxPoolGrad's strict '>').  Returns (out, arg)
    with arg in {0, 1, 2} = winner's offset inside its window."""
    B, Lin, C = a.shape
    Lout, pl, pr = L.same_pad(Lin, 3, stride)
    ap = np.pad(a, [[0, 0], [pl, pr], [0, 0]], constant_values=-np.inf)
    win = np.stack([ap[:, j:j + stride * Lout:stride, :] for j in range(3)], axis=2)     # [B, Lout, 3, C]
    return win.max(axis=2), win.argmax(axis=2)


def maxpool3_same_bwd(do, arg, stride, Lin):
    B, Lout, C = do.shape
    _, pl, pr = L.same_pad(Lin, 3, stride)
    dp = np.zeros((B, Lin + pl + pr, C), dtype=do.dtype)
    for j in range(3):
        dp[:, j:j + stride * Lout:stride, :] += do * (arg == j)
    return dp[:, pl:pl + Lin, :]


class KerasNames(object):
    """Keras names a layer by its class and a per-class counter in creation order; the glorot draws come from one
    RandomState in that same order.  One per net: the Python twin of KerasNames in csrc/net_internal.h."""

    def __init__(self, seed):
        self.rng = np.random.RandomState(seed)
        self.P, self.S = OrderedDict(), OrderedDict()
        self.cnt = dict(conv=0, bn=0, dw=0)
        self.l2_names = []

    def conv(self, k, cin, cout, l2):
        self.cnt['conv'] += 1
        name = 'conv1d_%d/kernel' % self.cnt['conv']
        self.P[name] = glorot_uniform(self.rng, (k, cin, cout), k * cin, k * cout)
        if l2:
            self.l2_names.append(name)
        return name

    def bn(self, c):
        self.cnt['bn'] += 1
        TimeSlicedAttentionNet._add_bn(self.P, self.S, self.cnt['bn'], c)
        return self.cnt['bn']

    def dw(self, c):
        self.cnt['dw'] += 1
        name = 'depthwise_conv2d_%d/depthwise_kernel' % self.cnt['dw']
        self.P[name] = glorot_uniform(self.rng, (1, 3, c, 1), 3 * c, 3)
        self.l2_names.append(name)
        return name


# Where a residual block's stride sits: the twin of LmStridePlace in csrc/net_logmfcc.hip
POOL_AFTER = 'pool_after'     # MaxPool1D(stride, stride, 'same') after the second pointwise convolution (conv_1d_log_mfcc)
STRIDED_DW = 'strided_dw'     # the block's first depthwise convolution is strided, 'same'; no pool (steffeNet)
POOL3_SAME = 'pool3_same'     # MaxPool1D(3, stride, 'same') after the second pointwise (conv_1d_residual, _mfcc_and_raw)


class ResidualFamilyNet(object):
    """What the four residual-family oracles share.  A net is: stem -> residual blocks -> plain depthwise layers (`red`)
    -> pooling head [B, F] -> Dropout -> Dense + softmax.  A subclass builds its table in __init__ (stem through self.kn,
    then _add_block / _add_plain on the running activation [self.T, self.C], then _add_dense) and states _stem_fwd /
    _stem_bwd and, unless its head is a global average, _head_fwd / _head_bwd.  The walker asks a block only where its
    stride sits, never which net it belongs to.
    Parameter names follow Keras' per-class auto-numbering in layer CREATION order (shortcut Conv1D + BN of a strided block
    are created before the block's depthwise layers, model.py:1429-1441)."""

    def __init__(self, num_classes, seed, dtype):
        self.dtype = dtype
        self.num_classes = num_classes
        self.kn = KerasNames(seed)
        self.params, self.state, self.l2_names = self.kn.P, self.kn.S, self.kn.l2_names
        self.blocks = []
        self.red = []

    # -- table -----------------------------------------------------------------
    def _add_block(self, nf, stride, place):
        """Appends one residual block of nf filters over the running activation [self.T, self.C] and moves that on to the
        block's output: the twin of lm_add_block.  Keras' 'same' gives ceil(L / stride) whichever layer carries the stride:
        conv_1d_log_mfcc's own default spectrogram_length = 65 runs 63 -> 32 -> 16 -> 8 (model.py:1410)."""
        kn, cin, Lin = self.kn, self.C, self.T
        blk = dict(nf=nf, stride=stride, cin=cin, Lin=Lin, Lout=-(-Lin // stride), place=place, s1=1, pad1=(1, 1))
        if place == STRIDED_DW:
            blk['s1'], blk['pad1'] = stride, L.same_pad(Lin, 3, stride)[1:]
        if stride != 1:
            blk['short'] = (kn.conv(1, cin, nf, False), kn.bn(nf))    # no kernel_regularizer (model.py:1431-1432)
        blk['dw1'], blk['pw1'], blk['bn1'] = kn.dw(cin), kn.conv(1, cin, nf, True), kn.bn(nf)
        blk['dw2'], blk['pw2'], blk['bn2'] = kn.dw(nf), kn.conv(1, nf, nf, True), kn.bn(nf)
        self.blocks.append(blk)
        self.T, self.C = blk['Lout'], nf

    def _add_plain(self, cout, stride, padding):
        """One depthwise k3 -> pointwise -> BN -> ReLU6 layer without a residual over [self.T, self.C] (_context_conv /
        _reduce_conv): the twin of lm_add_plain.  Returns its table entry; the running activation stays where it is."""
        kn, cin, Lin = self.kn, self.C, self.T
        if padding == 'same':
            Lout, pl, pr = L.same_pad(Lin, 3, stride)
        else:
            Lout, pl, pr = L.valid_len(Lin, 3, stride), 0, 0
        return dict(dw=kn.dw(cin), pw=kn.conv(1, cin, cout, True), bn=kn.bn(cout), cin=cin, cout=cout, stride=stride,
                    pad=(pl, pr), Lin=Lin, Lout=Lout)

    def _add_dense(self, fin, bias=True):
        """Dense(num_classes) over the pooled features; closes the table (twin of LmHead::add_dense)."""
        self.params['dense_1/kernel'] = glorot_uniform(self.kn.rng, (fin, self.num_classes), fin, self.num_classes)
        if bias:
            self.params['dense_1/bias'] = np.zeros((self.num_classes,), np.float32)
        self.l2_names.append('dense_1/kernel')

    def count_params(self):
        return sum(v.size for v in self.params.values()) + sum(v.size for v in self.state.values())

    def reg_loss(self):
        return sum(L.L2_COEF * float((self._p(k) ** 2).sum()) for k in self.l2_names)

    # -- layers ----------------------------------------------------------------
    def _p(self, name):
        return self.params[name].astype(self.dtype)

    def _bn(self, idx, y, training, cache, relu=True):
        g = self._p('batch_normalization_%d/gamma' % idx)
        b = self._p('batch_normalization_%d/beta' % idx)
        if training:
            pre, stats = L.bn_train_fwd(y, g, b)
            cache['bn%d' % idx] = (y, g, stats, pre)
            cache.setdefault('batch_stats', OrderedDict())[idx] = (stats[0], stats[1])
        else:
            pre = L.bn_infer_fwd(y, g, b,
                                 self.state['batch_normalization_%d/moving_mean' % idx].astype(self.dtype),
                                 self.state['batch_normalization_%d/moving_variance' % idx].astype(self.dtype))
        return L.relu6(pre) if relu else pre

    def _bn_bwd(self, idx, dout, cache, grads, relu=True):
        y, g, stats, pre = cache['bn%d' % idx]
        if relu:
            mask = L.relu6_mask(pre)
            ov = cache.get('relu_masks')
            if ov is not None and idx in ov:
                mask = np.asarray(ov[idx], dtype=self.dtype).reshape(pre.shape)
            dout = dout * mask
        dy, dg, db = L.bn_train_bwd(dout, y, g, stats)
        grads['batch_normalization_%d/gamma' % idx] = dg
        grads['batch_normalization_%d/beta' % idx] = db
        return dy

    def _first_fwd(self, first, h, training, cache, stride=1, pad=(0, 0)):
        """A stem's Conv1D + BN + ReLU6; first = (kernel name, BN index)."""
        y, cols = L.conv1d_fwd(h, self._p(first[0]), stride=stride, pad=pad)
        cache['cols%d' % first[1]] = cols
        return self._bn(first[1], y, training, cache)

    def _first_bwd(self, first, dh, cache, grads):
        dy = self._bn_bwd(first[1], dh, cache, grads)
        W0 = self._p(first[0])
        B2, Lo, Co = dy.shape
        grads[first[0]] = (cache['cols%d' % first[1]].T @ dy.reshape(B2 * Lo, Co)).reshape(W0.shape)

    def _plain_fwd(self, q, h, training, cache):
        w = self._p(q['dw']).reshape(3, q['cin'])
        z = L.dwconv_fwd(h, w, q['stride'], q['pad'])
        W = self._p(q['pw']).reshape(q['cin'], q['cout'])
        cache['plain%d' % q['bn']] = (h, w, z, W)
        return self._bn(q['bn'], L.pw_fwd(z, W), training, cache)

    def _plain_bwd(self, q, dout, cache, grads):
        hin, w, z, W = cache['plain%d' % q['bn']]
        dy = self._bn_bwd(q['bn'], dout, cache, grads)
        dz, dW = L.pw_bwd(dy, z, W)
        grads[q['pw']] = dW.reshape(1, q['cin'], q['cout'])
        dh, dwk = L.dwconv_bwd(dz, hin, w, q['stride'], q['pad'])
        grads[q['dw']] = dwk.reshape(1, 3, q['cin'], 1)
        return dh

    def _block_fwd(self, i, h, training, cache):
        """Shortcut (Conv1D(nf, 1, strides, same) + BN on a strided block, else the input), 2 x [depthwise k3 -> pointwise ->
        BN -> ReLU6], the join the block's stride placement names, Add (model.py:1429-1443, 1690-1701, 864-878)."""
        blk = self.blocks[i]
        c = {'x': h}
        if 'short' in blk:
            xs = h[:, ::blk['stride'], :]
            Ws = self._p(blk['short'][0]).reshape(blk['cin'], blk['nf'])
            c['xs'], c['Ws'] = xs, Ws
            res = self._bn(blk['short'][1], L.pw_fwd(xs, Ws), training, cache, relu=False)
        else:
            res = h
        w1 = self._p(blk['dw1']).reshape(3, blk['cin'])
        z1 = L.dwconv_fwd(h, w1, blk['s1'], blk['pad1'])
        W1 = self._p(blk['pw1']).reshape(blk['cin'], blk['nf'])
        a1 = self._bn(blk['bn1'], L.pw_fwd(z1, W1), training, cache)
        w2 = self._p(blk['dw2']).reshape(3, blk['nf'])
        z2 = L.dwconv_fwd(a1, w2, 1, (1, 1))
        W2 = self._p(blk['pw2']).reshape(blk['nf'], blk['nf'])
        a2 = self._bn(blk['bn2'], L.pw_fwd(z2, W2), training, cache)
        c.update(w1=w1, z1=z1, W1=W1, a1=a1, w2=w2, z2=z2, W2=W2)
        cache['blk%d' % i] = c
        if blk['place'] == POOL_AFTER:
            pooled, c['arg'] = maxpool_same_fwd(a2, blk['stride'])
        elif blk['place'] == POOL3_SAME:
            pooled, c['arg'] = maxpool3_same_fwd(a2, blk['stride'])
        else:
            pooled = a2                                                               # no pool: the stride was taken by dw1
        return pooled + res                                                           # Add, no activation

    def _block_bwd(self, i, dh, cache, grads):
        blk, c = self.blocks[i], cache['blk%d' % i]
        if blk['place'] == STRIDED_DW:
            da2 = dh
        else:
            pool_args = cache.get('pool_args')
            arg = c['arg'] if pool_args is None or i not in pool_args else pool_args[i]
            if blk['place'] == POOL_AFTER:
                da2 = maxpool_same_bwd(dh, arg, blk['stride'], blk['Lin'])
            else:
                da2 = maxpool3_same_bwd(dh, arg, blk['stride'], blk['Lin'])
        dy2 = self._bn_bwd(blk['bn2'], da2, cache, grads)
        dz2, dW2 = L.pw_bwd(dy2, c['z2'], c['W2'])
        grads[blk['pw2']] = dW2.reshape(1, blk['nf'], blk['nf'])
        da1, dw2 = L.dwconv_bwd(dz2, c['a1'], c['w2'], 1, (1, 1))
        grads[blk['dw2']] = dw2.reshape(1, 3, blk['nf'], 1)
        dy1 = self._bn_bwd(blk['bn1'], da1, cache, grads)
        dz1, dW1 = L.pw_bwd(dy1, c['z1'], c['W1'])
        grads[blk['pw1']] = dW1.reshape(1, blk['cin'], blk['nf'])
        dx, dw1 = L.dwconv_bwd(dz1, c['x'], c['w1'], blk['s1'], blk['pad1'])
        grads[blk['dw1']] = dw1.reshape(1, 3, blk['cin'], 1)
        if 'short' in blk:
            dys = self._bn_bwd(blk['short'][1], dh, cache, grads, relu=False)
            dxs, dWs = L.pw_bwd(dys, c['xs'], c['Ws'])
            grads[blk['short'][0]] = dWs.reshape(1, blk['cin'], blk['nf'])
            dx = dx.copy()
            dx[:, ::blk['stride'], :] += dxs
        else:
            dx = dx + dh
        return dx

    def _head_fwd(self, h, training, cache):
        return h.mean(axis=1)                                                         # GlobalAveragePooling1D

    def _head_bwd(self, dfeat, cache, grads):
        return np.repeat(dfeat[:, None, :], self.T, axis=1) / self.dtype(self.T)

    def _dense_fwd(self, feat, training, seed, step, cache, drop_offset):
        """features [B, F] -> Dropout(1 - drop_keep) -> Dense(num_classes) (+ bias where the net has one) -> softmax."""
        dt = self.dtype
        B, F = feat.shape
        if training:
            m = L.dropout_mask(L.dropout_key(seed, step, 1), B * F, self.drop_keep, drop_offset * F).reshape(B, F)
            fd = feat * m / dt(self.drop_keep)
        else:
            m, fd = None, feat
        Wd = self._p('dense_1/kernel')
        logits = fd @ Wd
        if 'dense_1/bias' in self.params:
            logits = logits + self._p('dense_1/bias')
        p = L.softmax(logits, axis=1)
        cache['dense'] = (m, fd, Wd, p)
        return p

    def _dense_bwd(self, dp, cache, grads):
        m, fd, Wd, p = cache['dense']
        dl = L.softmax_bwd(dp, p, axis=1)
        grads['dense_1/kernel'] = fd.T @ dl
        if 'dense_1/bias' in self.params:
            grads['dense_1/bias'] = dl.sum(axis=0)
        return (dl @ Wd.T) * m / self.dtype(self.drop_keep)

    def _loss(self, p, y_onehot):
        return L.cce_fwd_bwd(p, y_onehot)                                             # categorical_crossentropy

    # -- the walker ------------------------------------------------------------
    def forward(self, x, training=False, seed=0, step=0, cache=None, drop_offset=0):
        """x -> softmax probabilities [B, num_classes].  drop_offset = global index of row 0 (for data-parallel shards)."""
        cache = {} if cache is None else cache
        h = self._stem_fwd(x, training, cache)
        for i in range(len(self.blocks)):
            h = self._block_fwd(i, h, training, cache)
        for q in self.red:
            h = self._plain_fwd(q, h, training, cache)
        feat = self._head_fwd(h, training, cache)
        return self._dense_fwd(feat, training, seed, step, cache, drop_offset)

    def loss_and_grads(self, x, y_onehot, seed=0, step=0, drop_offset=0, loss_scale_B=None, relu_masks=None,
                       pool_args=None):
        """Returns (data_loss, probs, grads incl. L2 terms, cache).  loss_scale_B: divide the data-loss gradient by this
        batch size instead of the local one (data-parallel mean).  relu_masks {bn index: 0/1 array} / pool_args {block
        index: winner offsets} override the discrete decisions of the backward pass (ReLU6 masks, max-pool winners of the
        joins) with those another implementation took."""
        return self._loss_and_grads(x, y_onehot, seed, step, drop_offset, loss_scale_B,
                                    {'relu_masks': relu_masks, 'pool_args': pool_args})

    def _loss_and_grads(self, x, y_onehot, seed, step, drop_offset, loss_scale_B, cache):
        """cache arrives holding the decision overrides, which the backward pass of the layer they belong to reads."""
        dt = self.dtype
        p = self.forward(x, training=True, seed=seed, step=step, cache=cache, drop_offset=drop_offset)
        y_onehot = np.asarray(y_onehot, dtype=dt)
        loss, per, dp = self._loss(p, y_onehot)
        B = p.shape[0]
        if loss_scale_B is not None:
            dp = dp * dt(B) / dt(loss_scale_B)
        grads = OrderedDict()
        dfeat = self._dense_bwd(dp, cache, grads)
        dh = self._head_bwd(dfeat, cache, grads)
        for q in reversed(self.red):
            dh = self._plain_bwd(q, dh, cache, grads)
        for i in reversed(range(len(self.blocks))):
            dh = self._block_bwd(i, dh, cache, grads)
        self._stem_bwd(dh, cache, grads)
        for k in self.l2_names:                                                       # kernel_regularizer=l2(1e-5)
            grads[k] = grads[k] + dt(2.0 * L.L2_COEF) * self._p(k)
        return loss, p, OrderedDict((k, grads[k]) for k in self.params), cache


# ----------------------------------------------------------------------------------------------------------
# a19: conv_1d_log_mfcc_model (reference model.py:1400-1479); with num_features = 257 and 12 classes
# the same table is conv_1d_spectrogram_model (model.py:1482-1561)
# ----------------------------------------------------------------------------------------------------------
LM_BLOCKS = [(64, 1), (64, 1), (128, 2), (128, 1), (192, 2), (192, 1), (192, 1), (256, 2), (256, 1), (256, 1)]


class LogMfccNet(ResidualFamilyNet):
    """Residual depthwise/pointwise 1-D CNN on [spectrogram_length, num_log_mel_features] features (blocks joined by
    MaxPool1D(stride, stride, 'same'), model.py:1440) with a softmax-over-time attention and global average pooling,
    Dropout(.2), Dense + softmax, categorical CE (model.py:1477)."""

    def __init__(self, num_classes=32, spectrogram_length=98, num_features=40, seed=87654321, dtype=np.float64):
        super(LogMfccNet, self).__init__(num_classes, seed, dtype)
        self.T0, self.F = spectrogram_length, num_features
        self.first = (self.kn.conv(3, num_features, 64, True), self.kn.bn(64))
        self.T, self.C = spectrogram_length - 2, 64
        if self.T < 1:
            raise ValueError("LogMfccNet: spectrogram_length %d is too short" % spectrogram_length)
        for nf, stride in LM_BLOCKS:                                                  # model.py:1453-1462
            self._add_block(nf, stride, POOL_AFTER)
        self._att = self._add_plain(1, 1, 'same')                  # _context_conv(x, 1, 3, 'same'), model.py:1464
        self.att = (self._att['dw'], self._att['pw'], self._att['bn'])
        self._add_dense(self.C)
        self.drop_keep = 0.8                                       # Dropout(0.2), model.py:1471

    def _stem_fwd(self, x, training, cache):
        h = np.asarray(x, dtype=self.dtype).reshape(x.shape[0], self.T0, self.F)      # Reshape, model.py:1446
        return self._first_fwd(self.first, h, training, cache)                        # Conv1D(64,3) valid

    def _stem_bwd(self, dh, cache, grads):
        self._first_bwd(self.first, dh, cache, grads)

    def _head_fwd(self, h, training, cache):
        u = self._plain_fwd(self._att, h, training, cache)                            # [B, T, 1]
        att = L.softmax(u, axis=1)                                                    # softmax over time
        cache['head'] = (h, att)
        return (h * att).mean(axis=1)                                                 # Multiply + GAP

    def _head_bwd(self, dfeat, cache, grads):
        h, att = cache['head']
        dprod = np.repeat(dfeat[:, None, :], self.T, axis=1) / self.dtype(self.T)     # GAP backward
        dh = dprod * att
        datt = (dprod * h).sum(axis=2, keepdims=True)
        du = L.softmax_bwd(datt, att, axis=1)
        dh2 = self._plain_bwd(self._att, du, cache, grads)
        return dh + dh2


# ----------------------------------------------------------------------------------------------------------
# steffeNet (reference model.py:1663-1726)
# ----------------------------------------------------------------------------------------------------------
STEFFE_WIDTHS = [320, 384, 512, 768, 1024, 1536]                   # model.py:1709


class SteffeNet(ResidualFamilyNet):
    """Raw waveform -> Conv1D(256, 75, strides=50, same, no bias, no regulariser) + BN + ReLU6 ->
    _context_conv(256, 3, same) -> 6 x [residual block stride 2, residual block stride 1] ->
    GlobalMaxPooling1D ++ GlobalAveragePooling1D -> Dropout(.5) -> Dense(num_classes, no bias) + softmax,
    label-smoothed CE (0.1), RMSprop(1e-3).

    A residual block (model.py:1690-1701) differs from conv_1d_log_mfcc's in where the stride sits: the FIRST
    depthwise convolution is strided (SAME), there is no max-pool, and the sum is not activated."""

    def __init__(self, num_classes=12, input_size=16000, filter_widths=STEFFE_WIDTHS, c0=256, seed=87654321,
                 dtype=np.float64):
        super(SteffeNet, self).__init__(num_classes, seed, dtype)
        self.L_in = input_size
        self.K0, self.S0, self.C0 = 75, 50, c0
        self.L0, self.pl0, self.pr0 = L.same_pad(input_size, self.K0, self.S0)
        self.first = (self.kn.conv(self.K0, 1, c0, False), self.kn.bn(c0))     # model.py:1705-1707
        self.T, self.C = self.L0, c0
        self._ctx = self._add_plain(c0, 1, 'same')                             # _context_conv(x, 256, 3, 'same')
        self.ctx = (self._ctx['dw'], self._ctx['pw'], self._ctx['bn'])
        for nh in filter_widths:
            for stride in (2, 1):
                self._add_block(nh, stride, STRIDED_DW)
        self._add_dense(2 * self.C, bias=False)
        self.drop_keep = 0.5                                                   # Dropout(0.5), model.py:1716
        self.label_smoothing = 0.1                                             # model.py:1722-1724

    def _stem_fwd(self, x, training, cache):
        h = np.asarray(x, dtype=self.dtype).reshape(x.shape[0], self.L_in, 1)  # Reshape([-1, 1])
        h = self._first_fwd(self.first, h, training, cache, stride=self.S0, pad=(self.pl0, self.pr0))
        return self._plain_fwd(self._ctx, h, training, cache)

    def _stem_bwd(self, dh, cache, grads):
        dh0 = self._plain_bwd(self._ctx, dh, cache, grads)
        self._first_bwd(self.first, dh0, cache, grads)

    def _head_fwd(self, h, training, cache):
        xmax, xavg = h.max(axis=1), h.mean(axis=1)
        cache['head'] = (h, xmax)
        return np.concatenate([xmax, xavg], axis=1)                            # Concatenate()([x_max, x_avg])

    def _head_bwd(self, dfeat, cache, grads):
        dt = self.dtype
        h, xmax = cache['head']
        dxmax, dxavg = dfeat[:, :self.C], dfeat[:, self.C:]
        ind = (h == xmax[:, None, :]).astype(dt)                               # reduce_max: ties share the gradient
        if cache.get('pool_ind') is not None:
            ind = np.asarray(cache['pool_ind'], dtype=dt).reshape(h.shape)
        ind = ind / ind.sum(axis=1, keepdims=True)
        return ind * dxmax[:, None, :] + dxavg[:, None, :] / dt(self.T)

    def _loss(self, p, y_onehot):
        return L.smooth_cce_fwd_bwd(p, y_onehot, self.label_smoothing)

    def loss_and_grads(self, x, y_onehot, seed=0, step=0, drop_offset=0, loss_scale_B=None, relu_masks=None,
                       pool_ind=None):
        """As ResidualFamilyNet.loss_and_grads; the one max-pool decision of this net is the global one: pool_ind
        [B, T, C] = 0/1 indicator of the positions that take GlobalMaxPooling1D's gradient."""
        return self._loss_and_grads(x, y_onehot, seed, step, drop_offset, loss_scale_B,
                                    {'relu_masks': relu_masks, 'pool_ind': pool_ind})


# ----------------------------------------------------------------------------------------------------------
# conv_1d_residual_model (reference model.py:841-908)
# ----------------------------------------------------------------------------------------------------------
RES_BLOCKS = [(128, 2), (256, 2)] + [(256, 1)] * 8 + [(512, 2), (728, 2), (728, 2)]    # model.py:888-894


class Conv1dResidualNet(ResidualFamilyNet):
    """Raw waveform -> overlapping_time_slice_stack(40, 20) -> Conv1D(64, 3, strides=2) + BN + ReLU6 -> 13 residual
    blocks of 2 x [depthwise k3 SAME -> pointwise -> BN -> ReLU6] + MaxPool1D(3, strides, 'same') + Add (1x1 strided
    Conv1D + BN shortcut on the strided blocks) -> _reduce_block(1024) = strided SAME block + VALID block ->
    GlobalAveragePooling1D -> Dropout(.5) -> Dense(num_classes) + softmax, categorical CE (model.py:905), RMSprop(1e-4)."""

    def __init__(self, num_classes=12, input_size=16000, blocks=RES_BLOCKS, c0=64, c_reduce=1024, seed=87654321,
                 dtype=np.float64):
        super(Conv1dResidualNet, self).__init__(num_classes, seed, dtype)
        self.L_in = input_size
        self.C0 = c0
        Lf = L.same_pad(input_size, 40, 20)[0]
        self.L0 = L.valid_len(Lf, 3, 2)
        self.first = (self.kn.conv(3, 40, c0, True), self.kn.bn(c0))           # model.py:883-886
        self.T, self.C = self.L0, c0
        for nf, stride in blocks:
            self._add_block(nf, stride, POOL3_SAME)
        # _reduce_block(x, 1024, 3): _reduce_conv (strides 2, 'same') then _context_conv ('valid')
        for stride, padding in ((2, 'same'), (1, 'valid')):
            self.red.append(self._add_plain(c_reduce, stride, padding))
            self.T, self.C = self.red[-1]['Lout'], c_reduce
        self._add_dense(self.C)
        self.drop_keep = 0.5                                                   # Dropout(0.5), model.py:899

    def _stem_fwd(self, x, training, cache):
        frames = L.frame_same(np.asarray(x, dtype=self.dtype), 40, 20)         # model.py:881
        return self._first_fwd(self.first, frames, training, cache, stride=2)

    def _stem_bwd(self, dh, cache, grads):
        self._first_bwd(self.first, dh, cache, grads)


# ----------------------------------------------------------------------------------------------------------
# conv_1d_mfcc_and_raw_model (reference model.py:1563-1660)
# ----------------------------------------------------------------------------------------------------------
MR_BLOCKS = [(160, 1), (160, 1), (192, 2), (192, 1), (256, 2), (256, 1), (320, 2), (320, 1), (384, 2), (384, 1)]


class MfccAndRawNet(ResidualFamilyNet):
    """Two inputs (the generator's 'mfcc_and_raw' output): log-mel features [T, F] -> Conv1D(64, 3) + BN + ReLU6 and raw
    waveform -> overlapping_time_slice_stack(frame_length, frame_step, 'VALID') -> Conv1D(96, 3) + BN + ReLU6,
    concatenated to 160 channels -> 10 residual blocks with MaxPool1D(3, strides, 'same') joins ->
    GlobalAveragePooling1D -> Dropout(.3) -> Dense + softmax, categorical CE (model.py:1657), RMSprop(5e-4).
    Keras creation order: mfcc Conv1D + BN, raw Conv1D + BN, then the blocks (model.py:1611-1639)."""

    def __init__(self, num_classes=12, spectrogram_length=98, num_features=60, raw_size=16000, frame_length=480,
                 frame_step=160, blocks=MR_BLOCKS, c_mfcc=64, c_raw=96, seed=87654321, dtype=np.float64):
        super(MfccAndRawNet, self).__init__(num_classes, seed, dtype)
        self.T0, self.F, self.L_in = spectrogram_length, num_features, raw_size
        self.frame_length, self.frame_step = frame_length, frame_step
        n_frames = 1 + (raw_size - frame_length) // frame_step            # extract_image_patches VALID
        assert n_frames == spectrogram_length, "both branches must have the same number of time steps"
        self.L0 = spectrogram_length - 2
        self.Cm, self.Cr = c_mfcc, c_raw
        self.first_m = (self.kn.conv(3, num_features, c_mfcc, True), self.kn.bn(c_mfcc))  # model.py:1615-1618
        self.first_r = (self.kn.conv(3, frame_length, c_raw, True), self.kn.bn(c_raw))    # model.py:1625-1628
        self.T, self.C = self.L0, c_mfcc + c_raw
        for nf, stride in blocks:
            self._add_block(nf, stride, POOL3_SAME)
        self._add_dense(self.C)
        self.drop_keep = 0.7                                              # Dropout(0.3), model.py:1648

    def _stem_fwd(self, x, training, cache):
        """x = [mfcc [B, T*F], raw [B, L]] -> concatenated, activated [B, T-2, 160]."""
        dt = self.dtype
        xm, xr = x
        B = np.asarray(xm).shape[0]
        hm = np.asarray(xm, dtype=dt).reshape(B, self.T0, self.F)
        xr = np.asarray(xr, dtype=dt)
        idx = self.frame_step * np.arange(self.T0)[:, None] + np.arange(self.frame_length)[None, :]
        frames = xr[:, idx]                                               # [B, T, frame_length], VALID
        am = self._first_fwd(self.first_m, hm, training, cache)
        ar = self._first_fwd(self.first_r, frames, training, cache)
        return np.concatenate([am, ar], axis=2)                           # Concatenate()([x_mfcc, x_raw])

    def _stem_bwd(self, dh, cache, grads):
        self._first_bwd(self.first_m, dh[:, :, :self.Cm], cache, grads)
        self._first_bwd(self.first_r, dh[:, :, self.Cm:self.Cm + self.Cr], cache, grads)
