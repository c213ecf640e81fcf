"""NumPy oracle of the 2-D family: the dense NHWC Conv2D (kws_conv2d_*), MaxPool2D((2, 2), strides 2, 'valid') over an activated
tensor (kws_pool2x2_*), and the two networks built from them - conv_2d_mobile (reference model.py:547-594) and conv_2d_fast
(model.py:597-639): forward, loss and every gradient, restated layer by layer for the GPU parity tests.  float64 by default;
`dtype=np.float32` runs the same arithmetic in float32 (the float32-against-float64 figures of the GPU tests' docstrings).

TEST INFRASTRUCTURE ONLY.  A ladder layer is Conv2D(F, (kh, kw), SAME, bias) -> BatchNormalization -> relu6 (mobile) or relu (fast);
the bias is added HONESTLY in front of the BatchNorm (the device leaves it out of its GEMM and accounts for it where it matters).
Dropout masks are oracle/layers.py's counter-based ones: layer id 1 for the tail's Dropout(.1), ids 2 .. 5 for the four Dropout(.05)
in model order, element counter (row + drop_offset) * H*W*F + i over the NHWC tensor, as on the device.

`relu_masks` / `pool_ind` hand the device's own gate and arg-max decisions to the backward pass (values at a kink or a tie cannot
flip then); `mutate` names a deliberately wrong variant for the negative controls:
  'pad_front'    the odd SAME padding goes in front instead of behind
(Which maximum of a tied pool window wins, and relu against relu6, are kernel-level matters: behind a relu the only ties of a float64
run are zeros, whose gates are shut, and a normalised activation does not reach 6.  tests/test_conv2d_kernels_gpu.py constructs both.)
"""
import numpy as np

from oracle_blocks import OracleNet, same_geometry

H0, W0 = 98, 40
# F, (kh, kw), stride, (dh, dw), pooled, dropout behind the activation
LADDERS = {
    'mobile': [(32, (3, 3), 2, (1, 1), False, False), (32, (3, 3), 1, (1, 1), False, True),
               (64, (3, 3), 2, (1, 1), False, False), (64, (3, 3), 1, (1, 1), False, True),
               (128, (3, 3), 2, (1, 1), False, False), (128, (3, 3), 1, (1, 1), False, True),
               (256, (3, 3), 2, (1, 1), False, False), (256, (3, 3), 1, (1, 1), False, True)],
    'fast': [(16, (11, 5), 1, (2, 1), True, False), (32, (5, 3), 1, (2, 1), True, False), (64, (3, 3), 1, (1, 1), True, False),
             (128, (3, 3), 1, (1, 1), True, False)],
}
ACT = {'mobile': 'relu6', 'fast': 'relu'}
SGD = {'mobile': (1e-3, 0.95), 'fast': (1e-3, 0.9)}
KEEP_LADDER, KEEP_TAIL = 0.95, 0.9     # Dropout(0.05), Dropout(0.1): conv_2d_mobile only
TAIL_DROP_ID, LADDER_DROP_ID0 = 1, 2


def axis_geom(n, k, s=1, d=1, padding='same', front_heavy=False):
    """-> output length, (pad in front, pad behind) of one axis: TensorFlow SAME (the smaller half in front) or VALID"""
    if padding == 'valid':
        return (n - d * (k - 1) - 1) // s + 1, (0, 0)
    out, front, behind = same_geometry(n, k, s, d, odd_left=front_heavy)
    return out, (front, behind)


def conv2d_fwd(a, W, strides=(1, 1), dil=(1, 1), pads=((0, 0), (0, 0)), out_hw=None):
    """a [B, H, W, Cin] (already activated), W [kh, kw, Cin, F] -> y [B, Ho, Wo, F] and the zero-padded input: one matrix product
    per tap"""
    kh, kw = W.shape[:2]
    (sh, sw), (dh, dw) = strides, dil
    ap = np.pad(a, [(0, 0), tuple(pads[0]), tuple(pads[1]), (0, 0)])
    Ho = (ap.shape[1] - dh * (kh - 1) - 1) // sh + 1
    Wo = (ap.shape[2] - dw * (kw - 1) - 1) // sw + 1
    if out_hw is not None:
        assert (Ho, Wo) == tuple(out_hw), ((Ho, Wo), out_hw)
    y = np.zeros((a.shape[0], Ho, Wo, W.shape[3]), a.dtype)
    for i in range(kh):
        for j in range(kw):
            y += ap[:, dh * i:dh * i + sh * (Ho - 1) + 1:sh, dw * j:dw * j + sw * (Wo - 1) + 1:sw, :] @ W[i, j]
    return y, ap


def conv2d_bwd(dy, ap, W, strides, dil, pads, in_hw, need_dx=True):
    """-> dx [B, H, W, Cin] (the gradient wrt the activated input, padding cropped) and dW"""
    kh, kw = W.shape[:2]
    (sh, sw), (dh, dw) = strides, dil
    B, Ho, Wo, F = dy.shape
    dy2 = dy.reshape(-1, F)
    dW = np.zeros(W.shape, dy.dtype)
    dap = np.zeros(ap.shape, dy.dtype) if need_dx else None
    for i in range(kh):
        for j in range(kw):
            sl = (slice(None), slice(dh * i, dh * i + sh * (Ho - 1) + 1, sh), slice(dw * j, dw * j + sw * (Wo - 1) + 1, sw))
            dW[i, j] = ap[sl].reshape(-1, ap.shape[3]).T @ dy2
            if need_dx:
                dap[sl] += dy @ W[i, j].T
    dx = dap[:, pads[0][0]:pads[0][0] + in_hw[0], pads[1][0]:pads[1][0] + in_hw[1], :] if need_dx else None
    return dx, dW


def pool2_windows(a):
    """[B, H, W, C] -> [B, H // 2, W // 2, 4, C]: the windows of MaxPool2D((2, 2), strides 2, 'valid') in row-major order"""
    B, H, W, C = a.shape
    Ho, Wo = H // 2, W // 2
    w = a[:, :2 * Ho, :2 * Wo, :].reshape(B, Ho, 2, Wo, 2, C)
    return w.transpose(0, 1, 3, 2, 4, 5).reshape(B, Ho, Wo, 4, C)


def pool2_argmax(a, last=False):
    """index (0 .. 3, row-major) of the first (last: the last) maximum of every window"""
    w = pool2_windows(a)
    return 3 - np.argmax(w[:, :, :, ::-1, :], axis=3) if last else np.argmax(w, axis=3)


def pool2_fwd(a, ind):
    return np.take_along_axis(pool2_windows(a), ind[:, :, :, None, :], axis=3)[:, :, :, 0, :]


def pool2_bwd(dz, ind, H, W):
    """dz, ind [B, Ho, Wo, C] -> da [B, H, W, C]: every window's gradient goes to the element it names; a last odd row / column
    stays zero"""
    B, Ho, Wo, C = dz.shape
    da = np.zeros((B, H, W, C), dz.dtype)
    for e in range(4):
        da[:, (e >> 1):2 * Ho:2, (e & 1):2 * Wo:2, :] = dz * (ind == e)
    return da


def preprocess(x):
    """model.py:13-16"""
    t = x.dtype.type
    return np.clip((x + t(0.8)) / t(7.0), -5, 5)


class Conv2dNet(OracleNet):
    """kind 'mobile' or 'fast'; input [B, 3920] mfcc features."""

    def __init__(self, kind, num_classes=12, seed=1234, dtype=np.float64):
        super(Conv2dNet, self).__init__(num_classes, seed, dtype)
        self.kind, self.act = kind, ACT[kind]
        self.layers = []
        H, W, C = H0, W0, 1
        drop_id = LADDER_DROP_ID0
        for F, (kh, kw), s, (dh, dw), pool, drop in LADDERS[kind]:
            Ho, ph = axis_geom(H, kh, s, dh)
            Wo, pw = axis_geom(W, kw, s, dw)
            self.add_kernel('conv2d', (kh, kw, C, F), kh * kw * C, kh * kw * F, bias=F)
            lay = dict(idx=self.add_bn(F), k=(kh, kw), strides=(s, s), dil=(dh, dw), C=C, F=F, H=H, W=W, Hout=Ho, Wout=Wo, pads=(ph, pw),
                       pool=pool, drop_id=drop_id if drop else 0, Ho=Ho // 2 if pool else Ho, Wo=Wo // 2 if pool else Wo)
            drop_id += 1 if drop else 0
            self.layers.append(lay)
            H, W, C = lay['Ho'], lay['Wo'], F
        self.T, self.C = H * W, C
        self.add_kernel('dense', (C, num_classes), C, num_classes, bias=num_classes)
        self.keep_tail = KEEP_TAIL if kind == 'mobile' else 1.0

    def _geom(self, lay, mutate):
        if mutate != 'pad_front':
            return lay['pads']
        return tuple(axis_geom(n, k, s, d, front_heavy=True)[1]
                     for n, k, s, d in zip((lay['H'], lay['W']), lay['k'], lay['strides'], lay['dil']))

    def forward(self, x, training=False, seed=0, step=0, cache=None, drop_offset=0, mutate=None, pool_ind=None):
        t = self.dtype
        B = x.shape[0]
        cache = {} if cache is None else cache
        cache['batch_stats'] = {}
        h = preprocess(x.astype(t)).reshape(B, H0, W0, 1)
        for lay in self.layers:
            n = lay['idx']
            pads = self._geom(lay, mutate)
            y, ap = conv2d_fwd(h, self._p('conv2d_%d/kernel' % n), lay['strides'], lay['dil'], pads, (lay['Hout'], lay['Wout']))
            y = y + self._p('conv2d_%d/bias' % n)
            a = self.bn_act_fwd(n, y, training, cache, self.act)
            ind = keep = None
            if lay['pool']:
                ind = pool_ind[n] if pool_ind is not None and n in pool_ind else pool2_argmax(a)
                a = pool2_fwd(a, ind)
            if training and lay['drop_id']:
                keep = self.dropout(seed, step, lay['drop_id'], B, lay['Hout'] * lay['Wout'] * lay['F'], KEEP_LADDER, drop_offset)
                keep = keep.reshape(y.shape).astype(t)
                a = a * keep / t(KEEP_LADDER)
            cache[n] = dict(cache['bn%d' % n], ap=ap, ind=ind, keep=keep, pads=pads)
            h = a
        f = h.reshape(B, self.T, self.C).mean(axis=1)
        keep = None
        if training and self.keep_tail < 1.0:
            keep = self.dropout(seed, step, TAIL_DROP_ID, B, self.C, self.keep_tail, drop_offset).astype(t)
            f = f * keep / t(self.keep_tail)
        p = self.head_fwd(f, 'dense_1/kernel', 'dense_1/bias')
        cache.update(f=f, keep_tail=keep, p=p)
        return p

    def loss_and_grads(self, x, y_onehot, seed=0, step=0, drop_offset=0, relu_masks=None, pool_ind=None, mutate=None):
        """Data loss (batch mean) and its gradients."""
        t = self.dtype
        cache, grads = {}, {}
        B = x.shape[0]
        p = self.forward(x, training=True, seed=seed, step=step, cache=cache, drop_offset=drop_offset, mutate=mutate, pool_ind=pool_ind)
        loss, df = self.head_bwd(p, y_onehot, cache['f'], 'dense_1/kernel', 'dense_1/bias', grads)
        if cache['keep_tail'] is not None:
            df = df * cache['keep_tail'] / t(self.keep_tail)
        top = self.layers[-1]
        da = np.broadcast_to((df / t(self.T))[:, None, None, :], (B, top['Ho'], top['Wo'], self.C)).astype(t)
        for lay in reversed(self.layers):
            n = lay['idx']
            cc = cache[n]
            if cc['keep'] is not None:
                da = da * cc['keep'] / t(KEEP_LADDER)
            if lay['pool']:
                da = pool2_bwd(da, cc['ind'], lay['Hout'], lay['Wout'])
            F = lay['F']
            dy = self.bn_act_bwd(n, da, cache, grads, relu_masks)
            dga, dbe = grads['batch_normalization_%d/gamma' % n], grads['batch_normalization_%d/beta' % n]
            grads['conv2d_%d/bias' % n] = dy.sum(axis=(0, 1, 2))       # zero up to rounding: the BatchNorm backward removes the mean
            # what the terms of that sum are made of, per channel: dy = gamma rstd (g - dbeta / n - xhat dgamma / n), summed over the rows
            g3 = (da * self.gate(n, cache, relu_masks)).reshape(-1, F).astype(np.float64)
            y3 = cc['y'].reshape(-1, F).astype(np.float64)
            xhat = (y3 - cc['st'][0]) * cc['st'][2]
            ga = self._p('batch_normalization_%d/gamma' % n)
            cc['bias_terms'] = np.abs(ga * cc['st'][2]) * (np.abs(g3).sum(0) + np.abs(dbe) + np.abs(xhat).sum(0) * np.abs(dga) / g3.shape[0])
            da, grads['conv2d_%d/kernel' % n] = conv2d_bwd(dy, cc['ap'], self._p('conv2d_%d/kernel' % n), lay['strides'], lay['dil'],
                                                           cc['pads'], (lay['H'], lay['W']), need_dx=n > 1)
        return loss, p, self.ordered(grads), cache
