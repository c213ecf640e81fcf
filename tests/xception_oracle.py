"""Float64 NumPy oracle of the attention gate (kws_attn_gate_*) and of xception_with_attention (reference model.py:911-983).
TEST INFRASTRUCTURE ONLY.

The net is composed from three parts: the residual-family walker of oracle/net.py (stem, residual blocks with 3-wide SAME max-pool
joins, their backward), the gate stated here, and gru_oracle.bigru_fwd / bigru_bwd.  Its structure is checked against
tests/golden/xception_models.json (recorded from the reference's own builder) by tests/test_xception_cpu.py.

The gate on x [B, T, C] with the depthwise kernel wa [k, C], the pointwise kernel Wa [C] and a one-channel BatchNorm:
  u = (dw_k 'same' (x)) Wa;  pre = scale u + shift (batch statistics over all B T values when training, eps 1e-3, biased variance);
  att = softmax over TIME of relu6(pre);  y = x att.
`mutate` names a deliberately wrong variant for the negative controls:
  'softmax_channels'  softmax over the channel axis of the [B, T, 1] logits (all ones) instead of time
  'no_direct_term'    the dy att term dropped from dx
"""
import json
import os
from collections import OrderedDict

import numpy as np

from oracle import layers as L
from oracle.net import POOL3_SAME, ResidualFamilyNet, glorot_uniform
from gru_oracle import KEEP, bigru_bwd, bigru_fwd, draw_masks, orthogonal
from net_parity import perturb, waveform_batch

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden', 'xception_models.json')
XC_BLOCKS = [(128, 2), (256, 2)] + [(256, 1)] * 8 + [(384, 2)]     # model.py:964-968
GATE_K = 5
GRU_UNITS = 192

# (B, T, C, k) of the stand-alone op's GPU tests
GATE_CASES = [(1, 1, 4, 5), (3, 2, 8, 5), (37, 7, 132, 3), (5, 50, 384, 5), (2, 128, 64, 5)]


def golden(key='xception_with_attention'):
    with open(GOLDEN) as f:
        return json.load(f)[key]


def gate_fwd(x, wa, Wa, gamma, beta, mm, mv, training, mutate=None):
    """-> (y [B, T, C], cache); cache holds u, att, the table (scale, shift, mean, rstd), the batch variance and pre."""
    dt = x.dtype.type
    k = wa.shape[0]
    pl = (k - 1) // 2
    z = L.dwconv_fwd(x, wa, 1, (pl, k - 1 - pl))
    u = z @ Wa
    if training:
        mean = u.mean()
        var = ((u - mean) ** 2).mean()
    else:
        mean, var = dt(mm), dt(mv)
    rstd = dt(1.0) / np.sqrt(var + dt(L.BN_EPS))
    scale = dt(gamma) * rstd
    shift = dt(beta) - mean * scale
    pre = u * scale + shift
    a = L.relu6(pre)
    att = np.ones_like(a) if mutate == 'softmax_channels' else L.softmax(a, axis=1)
    y = x * att[:, :, None]
    return y, dict(x=x, wa=wa, Wa=Wa, z=z, u=u, att=att, pre=pre, gamma=dt(gamma), mean=mean, var=var, rstd=rstd, scale=scale, shift=shift,
                   training=training)


def gate_bwd(dy, c, mask=None, mutate=None):
    """-> (dx, dwa, dWa, dgamma, dbeta).  mask [B, T]: the ReLU6 decisions of another implementation."""
    x, att, u = c['x'], c['att'], c['u']
    da = (dy * x).sum(axis=2)
    dA = np.zeros_like(da) if mutate == 'softmax_channels' else L.softmax_bwd(da, att, axis=1)
    m = L.relu6_mask(c['pre']) if mask is None else np.asarray(mask, dtype=x.dtype).reshape(da.shape)
    g = dA * m
    xhat = (u - c['mean']) * c['rstd']
    dbeta = g.sum()
    dgamma = (g * xhat).sum()
    if c['training']:
        n = x.dtype.type(g.size)
        du = c['gamma'] * c['rstd'] * (g - dbeta / n - xhat * (dgamma / n))
    else:
        du = c['scale'] * g
    dWa = (du[:, :, None] * c['z']).sum(axis=(0, 1))
    k = c['wa'].shape[0]
    pl = (k - 1) // 2
    dxc, dwa = L.dwconv_bwd(du[:, :, None] * c['Wa'][None, None, :], x, c['wa'], 1, (pl, k - 1 - pl))
    dx = dxc if mutate == 'no_direct_term' else dy * att[:, :, None] + dxc
    return dx, dwa, dWa, dgamma, dbeta


def gate_inputs(B, T, C, k, negative_gamma=False):
    """Inputs of one stand-alone gate case (float32): x like a join's output (a ReLU6 term plus a signed residual), dy like the
    GRU's input gradient, kernels at twice the glorot width so that the softmax is far from flat and some logits leave (0, 6)."""
    rng = np.random.RandomState(1000 * B + 10 * T + C + k)
    x = (np.clip(rng.randn(B, T, C) * 1.5 + 0.5, 0, 6) + 0.3 * rng.randn(B, T, C)).astype(np.float32)
    dy = (rng.randn(B, T, C) * 0.1).astype(np.float32)
    lim = 2.0 * np.sqrt(6.0 / (k * C + k))
    wa = rng.uniform(-lim, lim, (k, C)).astype(np.float32)
    Wa = rng.uniform(-1.0, 1.0, C).astype(np.float32) * np.float32(2.0 * np.sqrt(6.0 / (C + 1)))
    gamma = np.float32(-1.7 if negative_gamma else 1.6)
    beta = np.float32(2.2)
    mm, mv = np.float32(0.05 * rng.randn()), np.float32(0.4 + 0.2 * rng.rand())
    return x, dy, wa, Wa, gamma, beta, mm, mv


class XceptionNet(ResidualFamilyNet):
    """Raw waveform -> overlapping_time_slice_stack(40, 20) -> Conv1D(64, 3, strides=2) + BN + ReLU6 -> eleven residual blocks with
    MaxPool1D(3, strides, 'same') joins -> attention gate (k 5) -> Bidirectional(GRU(192, dropout=.2, recurrent_dropout=.2)) -> Dense
    + softmax, categorical CE, RMSprop(5e-4).  l2 1e-5 on every convolution kernel but the shortcuts', on the GRU's two `kernel`
    tensors and on dense_1/kernel."""

    def __init__(self, num_classes=12, input_size=16000, filter_mult=1, seed=87654321, dtype=np.float64):
        super(XceptionNet, self).__init__(num_classes, seed, dtype)
        kn = self.kn
        self.L_in = input_size
        self.C0 = 64 * filter_mult
        Lf = L.same_pad(input_size, 40, 20)[0]
        self.L0 = L.valid_len(Lf, 3, 2)
        self.first = (kn.conv(3, 40, self.C0, True), kn.bn(self.C0))
        self.T, self.C = self.L0, self.C0
        for nf, stride in XC_BLOCKS:
            self._add_block(nf * filter_mult, stride, POOL3_SAME)
        C = self.C
        kn.cnt['dw'] += 1
        self.att_dw = 'depthwise_conv2d_%d/depthwise_kernel' % kn.cnt['dw']
        self.params[self.att_dw] = glorot_uniform(kn.rng, (1, GATE_K, C, 1), GATE_K * C, GATE_K)
        self.l2_names.append(self.att_dw)
        self.att_pw = kn.conv(1, C, 1, True)
        self.att_bn = kn.bn(1)
        self.I, self.H, self.keep = C, GRU_UNITS, KEEP
        self.gru_names = []
        for d in ('forward', 'backward'):
            base = 'bidirectional_1/%s_gru_1/' % d
            self.params[base + 'kernel'] = glorot_uniform(kn.rng, (C, 3 * self.H), C, 3 * self.H)
            self.params[base + 'recurrent_kernel'] = orthogonal(kn.rng, (self.H, 3 * self.H))
            self.params[base + 'bias'] = np.zeros(3 * self.H, np.float32)
            self.l2_names.append(base + 'kernel')
            self.gru_names.append(base)
        self._add_dense(2 * self.H)

    def _stem_fwd(self, x, training, cache):
        frames = L.frame_same(np.asarray(x, dtype=self.dtype), 40, 20)
        return self._first_fwd(self.first, frames, training, cache, stride=2)

    def _stem_bwd(self, dh, cache, grads):
        self._first_bwd(self.first, dh, cache, grads)

    def _gru_weights(self):
        return [tuple(self._p(b + w) for w in ('kernel', 'recurrent_kernel', 'bias')) for b in self.gru_names]

    def _bn_name(self, w):
        return 'batch_normalization_%d/%s' % (self.att_bn, w)

    def forward(self, x, training=False, seed=0, step=0, cache=None, drop_offset=0, mutate=None):
        cache = {} if cache is None else cache
        h = self._stem_fwd(x, training, cache)
        for i in range(len(self.blocks)):
            h = self._block_fwd(i, h, training, cache)
        B = h.shape[0]
        y, gc = gate_fwd(h, self._p(self.att_dw)[0, :, :, 0], self._p(self.att_pw)[0, :, 0], self._p(self._bn_name('gamma'))[0],
                         self._p(self._bn_name('beta'))[0], self.state[self._bn_name('moving_mean')].astype(self.dtype)[0],
                         self.state[self._bn_name('moving_variance')].astype(self.dtype)[0], training, mutate)
        if training:
            cache.setdefault('batch_stats', OrderedDict())[self.att_bn] = (np.array([gc['mean']]), np.array([gc['var']]))
        mx = mh = None
        if training:
            mx, mh = draw_masks(seed, step, B, self.I, self.H, self.keep, drop_offset, self.T)
            if self.dtype != np.float64:
                mx = [[m.astype(self.dtype) for m in d] for d in mx]
                mh = [[m.astype(self.dtype) for m in d] for d in mh]
        out, caches = bigru_fwd(y, self._gru_weights(), mx, mh)
        p = L.softmax(out @ self._p('dense_1/kernel') + self._p('dense_1/bias'), axis=1)
        cache.update(gate=gc, gate_out=y, gru_out=out, gru=caches, p=p)
        return p

    def moving_after(self, cache):
        """The moving statistics of every BatchNorm after the training step that filled `cache` (momentum 0.99, biased variance)."""
        out = OrderedDict()
        for idx, (mean, var) in cache['batch_stats'].items():
            for nm, batch in (('moving_mean', mean), ('moving_variance', var)):
                name = 'batch_normalization_%d/%s' % (idx, nm)
                out[name] = L.bn_moving_update(self.state[name].astype(np.float64), np.asarray(batch, dtype=np.float64))
        return out

    def loss_and_grads(self, x, y_onehot, seed=0, step=0, drop_offset=0, relu_masks=None, pool_args=None, decisions=None, mutate=None):
        """Data loss (batch mean) and its gradients (no L2 term).  relu_masks {bn index: 0/1 array} (the attention BatchNorm's
        [B, T] included), pool_args {block: winner offsets} and decisions {(d, 'z' | 'r'): bool [B, T, H]} hand in the discrete
        decisions another implementation took."""
        cache = {'relu_masks': relu_masks, 'pool_args': pool_args}
        p = self.forward(x, training=True, seed=seed, step=step, cache=cache, drop_offset=drop_offset, mutate=mutate)
        loss, per, dp = L.cce_fwd_bwd(p, np.asarray(y_onehot, dtype=self.dtype))
        dl = L.softmax_bwd(dp, p, axis=1)
        grads = OrderedDict()
        grads['dense_1/kernel'] = cache['gru_out'].T @ dl
        grads['dense_1/bias'] = dl.sum(axis=0)
        dout = dl @ self._p('dense_1/kernel').T
        dgy, gg = bigru_bwd(dout, cache['gate_out'], self._gru_weights(), cache['gru'], decisions)
        for base, (dW, dU, db) in zip(self.gru_names, gg):
            grads[base + 'kernel'], grads[base + 'recurrent_kernel'], grads[base + 'bias'] = dW, dU, db
        mask = None if relu_masks is None else relu_masks.get(self.att_bn)
        dh, dwa, dWa, dgamma, dbeta = gate_bwd(dgy, cache['gate'], mask, mutate)
        grads[self.att_dw] = dwa[None, :, :, None]
        grads[self.att_pw] = dWa[None, :, None]
        grads[self._bn_name('gamma')] = np.array([dgamma])
        grads[self._bn_name('beta')] = np.array([dbeta])
        for i in reversed(range(len(self.blocks))):
            dh = self._block_bwd(i, dh, cache, grads)
        self._stem_bwd(dh, cache, grads)
        return loss, p, OrderedDict((k, grads[k]) for k in self.params), cache


def gate_reference(B, T, C, k, training, negative_gamma=False, dtype=np.float64, mask=None):
    """The stand-alone gate op on gate_inputs(...) in `dtype`: every output the device op has, under the device's names.  mask: the
    ReLU6 decisions to take in the backward pass (None: the run's own)."""
    x, dy, wa, Wa, gamma, beta, mm, mv = [np.asarray(a, dtype=dtype) for a in gate_inputs(B, T, C, k, negative_gamma)]
    y, c = gate_fwd(x, wa, Wa, gamma, beta, mm, mv, training)
    dx, dwa, dWa, dgamma, dbeta = gate_bwd(dy, c, mask)
    one = dtype(1.0 - L.BN_MOMENTUM)
    out = dict(u=c['u'], table=np.array([c['scale'], c['shift'], c['mean'], c['rstd']]), att=c['att'], y=y, dx=dx, dwa=dwa, dWa=dWa,
               dgamma=np.array([dgamma]), dbeta=np.array([dbeta]), pre=c['pre'],
               mm=np.array([mm - (mm - c['mean']) * one if training else mm]), mv=np.array([mv - (mv - c['var']) * one if training else mv]))
    # what a sum of the masked softmax gradients is measured against: the sum of their magnitudes (the terms cancel; without a
    # mask they cancel exactly)
    da = (dy * x).sum(axis=2)
    g = L.softmax_bwd(da, c['att'], axis=1) * (L.relu6_mask(c['pre']) if mask is None else mask)
    out['g_abs_sum'] = np.abs(g).sum()
    out['gx_abs_sum'] = np.abs(g * (c['u'] - c['mean']) * c['rstd']).sum()
    return out


GATE_FWD_KEYS = ('u', 'table', 'att', 'y', 'mm', 'mv')
GATE_BWD_KEYS = ('dx', 'dwa', 'dWa', 'dgamma', 'dbeta')


def gate_errors(got, ref, near=None):
    """max |got - ref| of every output relative to the reference's largest magnitude (dgamma / dbeta: to the sum of magnitudes of
    their terms).  near [B, T]: elements of att left out of the comparison."""
    errs = {}
    for k in GATE_FWD_KEYS + GATE_BWD_KEYS:
        g, r = np.asarray(got[k], dtype=np.float64).reshape(-1), np.asarray(ref[k], dtype=np.float64).reshape(-1)
        if k == 'att' and near is not None:
            keep = ~np.asarray(near).reshape(-1)
            g, r = g[keep], r[keep]
        scale = {'dgamma': ref['gx_abs_sum'], 'dbeta': ref['g_abs_sum']}.get(k, np.abs(r).max() if r.size else 0.0)
        errs[k] = np.abs(g - r).max() / max(float(scale), 1e-7) if r.size else 0.0
    return errs


def perturbed_net(input_size=16000, dtype=np.float64, num_classes=12, seed=5, att_gamma=1.5):
    """The net the parity tests run: scales, shifts, biases and moving statistics moved off their initial values (net_parity.perturb),
    about a third of the BatchNorm scales negative, the attention BatchNorm wide enough that some logits leave (0, 6)."""
    ora = XceptionNet(num_classes=num_classes, input_size=input_size, dtype=dtype)
    perturb(ora, seed)
    rng = np.random.RandomState(seed + 1)
    for k in ora.params:
        if k.endswith('gamma') and ora.params[k].size > 1:
            ora.params[k] = (ora.params[k] * np.where(rng.rand(*ora.params[k].shape) < 0.33, -1.0, 1.0)).astype(np.float32)
    ora.params[ora._bn_name('gamma')] = np.array([att_gamma], np.float32)
    ora.params[ora._bn_name('beta')] = np.array([2.0], np.float32)
    return ora


def net_float32_figures(B, input_size, seed=77, step=2):
    """The net in float32 against itself in float64, on the batch and weights of the GPU parity test and on the float64 run's ReLU6,
    pool and hard-sigmoid decisions.  gru_oracle's recurrence keeps its state in float64, so from the GRU on the float32 run is
    float64: the figures for probabilities and loss are lower bounds.  -> dict of figures."""
    x, y = waveform_batch(B, 12, B, L=input_size)
    o64 = perturbed_net(input_size)
    loss, p, g, c = o64.loss_and_grads(x.astype(np.float64), y.astype(np.float64), seed=seed, step=step)
    masks = {int(k[2:]): L.relu6_mask(v[3]) for k, v in c.items() if k.startswith('bn') and k[2:].isdigit()}
    masks[o64.att_bn] = L.relu6_mask(c['gate']['pre'])
    args = {i: c['blk%d' % i]['arg'] for i in range(len(o64.blocks))}
    dec = {(d, k): np.abs(c['gru'][d]['p' + k]) < 2.5 for d in range(2) for k in 'zr'}
    o32 = perturbed_net(input_size, dtype=np.float32)
    loss2, p2, g2, c2 = o32.loss_and_grads(x, y, seed=seed, step=step, relu_masks=masks, pool_args=args, decisions=dec)
    errs = {k: np.abs(g2[k].astype(np.float64) - g[k]).max() / max(np.abs(g[k]).max(), 1e-7) for k in g}
    worst = max(errs, key=errs.get)
    m64, m32 = o64.moving_after(c), o32.moving_after(c2)
    return {'probs': float(np.abs(p2 - p).max()), 'loss': float(abs(loss2 - loss)), 'worst_gradient': worst, 'gradient': float(errs[worst]),
            'moving': float(max(np.abs(m32[k] - m64[k]).max() for k in m64))}
