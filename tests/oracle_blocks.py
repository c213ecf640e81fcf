"""What the family oracles (tests/*_oracle.py) share: the generic layer math on top of oracle/layers.py, stated once, and the
OracleNet base their nets are built on.  TEST INFRASTRUCTURE ONLY; a plain module: no fixtures.

Channels-last [B, L, C]; convolutions are cross-correlations and read an ACTIVATED input, so padding is zeros of the activation.
The device parity bars are measured against these functions; tests/test_oracle_blocks_cpu.py checks each against torch autograd.
"""
from collections import OrderedDict

import numpy as np

from oracle import layers as OL
from oracle.layers import (BN_EPS, bn_infer_fwd, cce_fwd_bwd, conv1d_bwd, conv1d_fwd, dropout_key, dropout_mask, dwconv_bwd,
                           dwconv_fwd, softmax, softmax_bwd)


def glorot(rng, shape, fan_in, fan_out):
    """Keras glorot_uniform: U(-l, l), l = sqrt(6 / (fan_in + fan_out)), drawn in float64 and cast to float32."""
    lim = np.sqrt(6.0 / (fan_in + fan_out))
    return rng.uniform(-lim, lim, size=shape).astype(np.float32)


def same_geometry(L, k, s=1, dil=1, odd_left=False):
    """TensorFlow SAME -> (output length, pad in front, pad behind): ceil(L / s) outputs, the odd sample of the total padding
    behind (odd_left: in front - a mutation)."""
    Lout, pl, pr = OL.same_pad(L, dil * (k - 1) + 1, s)
    return (Lout, pr, pl) if odd_left else (Lout, pl, pr)


# ---- dense Conv1D, one matrix product per tap ----------------------------------------------------------------------------------
def conv_fwd(a, W, stride=1, dil=1, pad_l=0, Lout=None, pad_value=None):
    """a [B, L, Cin], W [k, Cin, F] -> (y [B, Lout, F], the padded input): y[b, t] = sum_j a[b, stride t - pad_l + dil j] W[j], 0
    outside [0, L) (pad_value [Cin]: a mutated padding).  Without Lout: every window that fits behind the pad_l rows (VALID)."""
    k, L = W.shape[0], a.shape[1]
    span = dil * (k - 1)
    if Lout is None:
        Lout = (L + pad_l - span - 1) // stride + 1
    reach = stride * (Lout - 1) + 1                      # rows from a tap's first to one past its last
    pad_r = max(reach + span - pad_l - L, 0)
    ap = np.zeros((a.shape[0], pad_l + L + pad_r, a.shape[2]), a.dtype)
    if pad_value is not None:
        ap[:] = pad_value
    ap[:, pad_l:pad_l + L] = a
    y = ap[:, 0:reach:stride] @ W[0]
    for j in range(1, k):
        y += ap[:, dil * j:dil * j + reach:stride] @ W[j]
    return y, ap


def conv_bwd(dy, ap, W, L, stride=1, dil=1, pad_l=0, need_dx=True):
    """-> (gradient wrt the activated input [B, L, Cin], dW) from conv_fwd's padded input ap"""
    k, Lout = W.shape[0], dy.shape[1]
    reach = stride * (Lout - 1) + 1
    dy2 = dy.reshape(-1, dy.shape[2])
    dW = np.stack([ap[:, dil * j:dil * j + reach:stride].reshape(-1, ap.shape[2]).T @ dy2 for j in range(k)])
    dx = None
    if need_dx:
        dap = np.zeros_like(ap)
        for j in range(k):
            dap[:, dil * j:dil * j + reach:stride] += dy @ W[j].T
        dx = dap[:, pad_l:pad_l + L]
    return dx, dW


# ---- grouped Conv1D: oracle.layers' im2col convolution over channel slices -------------------------------------------------------
def gconv_fwd(x, Ws, k, stride, gs, reverse=False):
    """x [B, L, C], Ws: g kernels [k, gs, Ng] -> [B, Lout, g * Ng] (VALID; reverse: groups concatenated in reverse - a mutation)"""
    outs = [conv1d_fwd(x[:, :, q * gs:(q + 1) * gs], W, stride)[0] for q, W in enumerate(Ws)]
    return np.concatenate(outs[::-1] if reverse else outs, axis=2)


def gconv_bwd(dy, x, Ws, k, stride, gs, need_dx=True, swap_phase=False):
    """-> (dx [B, L, C] (zeros outside the groups), [dW_q]).  swap_phase: rows tau and tau ^ 1 of dx trade places (a mutation of
    the data gradient's phase split)."""
    L, Ng = x.shape[1], Ws[0].shape[2]
    dx = np.zeros_like(x) if need_dx else None
    dWs = []
    for q, W in enumerate(Ws):
        xq = x[:, :, q * gs:(q + 1) * gs]
        cols = conv1d_fwd(xq, W[:, :, :0], stride)[1]                     # the im2col matrix alone: no output column asked for
        dxq, dW = conv1d_bwd(dy[:, :, q * Ng:(q + 1) * Ng], cols, W, xq.shape, stride, need_dx=need_dx)
        dWs.append(dW)
        if need_dx:
            dx[:, :, q * gs:(q + 1) * gs] += dxq
    if need_dx and swap_phase:
        n = L - L % 2
        dx[:, :n] = dx[:, :n].reshape(dx.shape[0], n // 2, 2, -1)[:, :, ::-1].reshape(dx.shape[0], n, -1)
    return dx, dWs


# ---- depthwise Conv1D: oracle.layers' with the padding behind worked out from the output length ----------------------------------
def _dw_pad(L, k, s, pad_l, Lout):
    return pad_l, max(s * (Lout - 1) + k - pad_l - L, 0)


def dw_fwd(a, w, s, pad_l, Lout):
    """a [B, L, C] (already activated), w [k, C] -> z [B, Lout, C]; zeros outside [0, L)."""
    t = np.result_type(a, w)
    return dwconv_fwd(a.astype(t, copy=False), w.astype(t, copy=False), s, _dw_pad(a.shape[1], w.shape[0], s, pad_l, Lout))[:, :Lout]


def dw_bwd(dz, a, w, s, pad_l):
    """-> (gradient wrt a [B, L, C], gradient wrt w [k, C])."""
    t = np.result_type(dz, a, w)
    return dwconv_bwd(dz.astype(t, copy=False), a.astype(t, copy=False), w.astype(t, copy=False), s,
                      _dw_pad(a.shape[1], w.shape[0], s, pad_l, dz.shape[1]))


# ---- training BatchNorm, its column sums in float64 ------------------------------------------------------------------------------
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


def act_fwd(pre, act='relu6'):
    return OL.relu6(pre) if act == 'relu6' else np.maximum(pre, 0)


def act_mask(pre, act='relu6'):
    """The gradient gate of relu6 (oracle.layers.relu6_mask: pre > 0 && pre <= 6) or of relu"""
    return OL.relu6_mask(pre) if act == 'relu6' else (pre > 0).astype(pre.dtype)


# ---- the base of the family nets ---------------------------------------------------------------------------------------------------
class OracleNet(object):
    """Parameters and BatchNorm state under their Keras names in creation order, and the steps every family spells the same way:
    BatchNorm + activation forward / backward, dropout masks, the Dense + softmax + categorical-CE head, the gradient ordering.
    A family class adds its specification table, its wiring and its named mutations."""

    def __init__(self, num_classes, seed, dtype=np.float64):
        self.nc, self.dtype = num_classes, dtype
        self.rng = np.random.RandomState(seed)
        self.params, self.state = OrderedDict(), OrderedDict()
        self.l2_names = []
        self.made = {}            # Keras layer class -> how many exist

    def add_kernel(self, layer, shape, fan_in, fan_out, l2=False, bias=None, suffix='kernel'):
        """The next `layer`_<n> with a glorot kernel (and a zero bias of `bias` entries behind it) -> the kernel's name"""
        self.made[layer] = n = self.made.get(layer, 0) + 1
        name = '%s_%d/%s' % (layer, n, suffix)
        self.params[name] = glorot(self.rng, shape, fan_in, fan_out)
        if bias:
            self.params['%s_%d/bias' % (layer, n)] = np.zeros(bias, np.float32)
        if l2:
            self.l2_names.append(name)
        return name

    def add_bn(self, C):
        """The next BatchNormalization over C channels -> its number"""
        self.made['bn'] = n = self.made.get('bn', 0) + 1
        base = 'batch_normalization_%d/' % n
        self.params[base + 'gamma'] = np.ones(C, np.float32)
        self.params[base + 'beta'] = np.zeros(C, np.float32)
        self.state[base + 'moving_mean'] = np.zeros(C, np.float32)
        self.state[base + 'moving_variance'] = np.ones(C, np.float32)
        return n

    def count_params(self):
        return sum(v.size for v in self.params.values()) + sum(v.size for v in self.state.values())

    def _p(self, name):
        return self.params[name].astype(self.dtype)

    def _bn(self, idx, what):
        name = 'batch_normalization_%d/%s' % (idx, what)
        return (self.state if what.startswith('moving') else self.params)[name].astype(self.dtype)

    def bn_act_fwd(self, idx, y, training, cache, act='relu6'):
        """BatchNormalization `idx` of y [B, ..., C] over all but the channel axis (batch statistics when training, the moving
        ones otherwise) and the activation.  Leaves cache['bn<idx>'] = {y, st = (mean, var, rstd) | None, pre, shift, act} and the
        batch statistics in cache['batch_stats'][idx].  -> the activated tensor"""
        ga, be = self._bn(idx, 'gamma'), self._bn(idx, 'beta')
        y3 = y.reshape(y.shape[0], -1, y.shape[-1])
        if training:
            pre, st = bn_train_fwd(y3, ga, be)
            shift = be - st[0] * st[2] * ga
        else:
            st = None
            mm, mv = self._bn(idx, 'moving_mean'), self._bn(idx, 'moving_variance')
            pre = bn_infer_fwd(y3, ga, be, mm, mv)
            shift = be - mm * (ga / np.sqrt(mv + BN_EPS))
        pre = pre.reshape(y.shape)
        if cache is not None:
            cache['bn%d' % idx] = {'y': y, 'st': st, 'pre': pre, 'shift': shift, 'act': act}
            if training:
                cache['batch_stats'][idx] = (st[0], st[1])
        return act_fwd(pre, act)

    def gate(self, idx, cache, relu_masks=None):
        """The activation's gradient gate: relu_masks[idx] where another implementation's decision is handed in (values at a kink
        cannot flip then), the forward pass's own pre-activation otherwise"""
        c = cache['bn%d' % idx]
        mask = relu_masks[idx] if relu_masks is not None and idx in relu_masks else act_mask(c['pre'], c['act'])
        return np.asarray(mask).astype(self.dtype).reshape(c['pre'].shape)

    def bn_act_bwd(self, idx, dout, cache, grads, relu_masks=None, gate=True):
        """dout: gradient wrt the activated output -> gradient wrt y (gate=False: the activation's gate left out - a mutation);
        stores dgamma and dbeta."""
        c = cache['bn%d' % idx]
        y = c['y']
        if gate:
            dout = dout * self.gate(idx, cache, relu_masks)
        C = y.shape[-1]
        dy, dga, dbe = bn_train_bwd(dout.reshape(y.shape[0], -1, C), y.reshape(y.shape[0], -1, C), self._bn(idx, 'gamma'), c['st'])
        grads['batch_normalization_%d/gamma' % idx] = dga
        grads['batch_normalization_%d/beta' % idx] = dbe
        return dy.reshape(y.shape)

    @staticmethod
    def dropout(seed, step, layer_id, B, D, keep, drop_offset=0):
        """The keep decisions [B, D] of dropout layer `layer_id`: element counter (drop_offset + row) * D + i, as on the device"""
        return dropout_mask(dropout_key(seed, step, layer_id), B * D, keep, offset=drop_offset * D).reshape(B, D)

    def dense_fwd(self, f, kernel, bias=None):
        """f [B, D] @ the kernel seen as [D, -1] (+ bias)"""
        z = f @ self._p(kernel).reshape(f.shape[1], -1)
        return z if bias is None else z + self._p(bias)

    def dense_bwd(self, dz, f, kernel, bias, grads):
        """stores the kernel's and the bias's gradients -> gradient wrt f"""
        grads[kernel] = (f.T @ dz).reshape(self.params[kernel].shape)
        if bias is not None:
            grads[bias] = dz.sum(axis=0)
        return dz @ self._p(kernel).reshape(f.shape[1], -1).T

    def head_fwd(self, f, kernel, bias=None):
        """Dense + softmax over f [B, D]"""
        return softmax(self.dense_fwd(f, kernel, bias))

    def head_bwd(self, p, y_onehot, f, kernel, bias, grads):
        """keras categorical_crossentropy on the head's probabilities -> (mean loss, gradient wrt f)"""
        loss, _, dp = cce_fwd_bwd(p, y_onehot.astype(self.dtype))
        return loss, self.dense_bwd(softmax_bwd(dp, p), f, kernel, bias, grads)

    def ordered(self, grads):
        return OrderedDict((k, grads[k]) for k in self.params)


class DwPwNet(OracleNet):
    """The block DepthwiseConv2D((1, k), strides=s, no bias) -> Conv1D(F, 1, no bias) -> BatchNormalization -> relu6 of the
    depthwise ladders (dwk_oracle.DwkNet, gru_oracle.SimpleNet, mts_oracle.MtsNet), numbered alike in its three Keras layers."""

    def add_block(self, k, C, F):
        self.add_kernel('depthwise_conv2d', (1, k, C, 1), k * C, k, l2=True, suffix='depthwise_kernel')
        self.add_kernel('conv1d', (1, C, F), C, F, l2=True)
        return self.add_bn(F)

    def _taps(self, n, reverse=False):
        w = self._p('depthwise_conv2d_%d/depthwise_kernel' % n)[0, :, :, 0]
        return w[::-1] if reverse else w

    def block_fwd(self, n, a, s, pad_l, Lout, training, cache, reverse=False):
        """-> the activated output; cache['a<n>'] the input, cache['z<n>'] the depthwise output"""
        z = dw_fwd(a, self._taps(n, reverse), s, pad_l, Lout)
        if cache is not None:
            cache['a%d' % n], cache['z%d' % n] = a, z
        return self.bn_act_fwd(n, z @ self._p('conv1d_%d/kernel' % n)[0], training, cache)

    def block_bwd(self, n, da, s, pad_l, cache, grads, relu_masks, reverse=False):
        """da: gradient wrt the activated output -> gradient wrt the block's input"""
        dy = self.bn_act_bwd(n, da, cache, grads, relu_masks)
        z = cache['z%d' % n]
        grads['conv1d_%d/kernel' % n] = (z.reshape(-1, z.shape[2]).T @ dy.reshape(-1, dy.shape[2]))[None]
        da, dw = dw_bwd(dy @ self._p('conv1d_%d/kernel' % n)[0].T, cache['a%d' % n], self._taps(n, reverse), s, pad_l)
        grads['depthwise_conv2d_%d/depthwise_kernel' % n] = (dw[::-1] if reverse else dw)[None, :, :, None]
        return da
