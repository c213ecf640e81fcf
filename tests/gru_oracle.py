"""Float64 NumPy oracle of Keras 2.1.2's Bidirectional(GRU(H, dropout, recurrent_dropout)) (GRUCell.call, implementation=1,
return_sequences=False, merge_mode='concat') and of conv_1d_simple (reference model.py:116-156), built from the structure recorded
in tests/golden/gru_models.json.  TEST INFRASTRUCTURE ONLY.

Per direction d (0: t = 0 .. T-1, 1: t = T-1 .. 0; h = 0 before the first step), gates (z, r, h) = column blocks of kernel [I, 3H]:
  a_g = (x_t * mx_g) W_g + bias_g;  z = hs(a_z + (h * mh_z) U_z);  r = hs(a_r + (h * mh_r) U_r);  hs(v) = clip(0.2 v + 0.5, 0, 1)
  c = tanh(a_h + (r * h * mh_h) U_h);  h' = z h + (1 - z) c;  output [h_fwd(T-1) | h_bwd(0)]
The six masks of a direction are drawn once per batch row from oracle/layers.py's counter RNG (layer id 16 + 6 d + g for mx_g,
16 + 6 d + 3 + g for mh_g; element counter (row_offset + b) * n + i) and hold 0 or 1 / keep.

`decisions` hands hard-sigmoid decisions in from outside: {(d, 'z' | 'r'): bool [B, T, H]}, True where the gate is in its linear
region.  `mutate` names a deliberately wrong variant for the negative controls:
  'reset_after'            r applied AFTER the product: c = tanh(a_h + r * ((h mh_h) U_h))
  'gate_order'             the z and r column blocks swapped
  'backward_not_reversed'  direction 1 walks forward in time as well
  'mask_per_step'          a fresh mask at every time step (layer id + 100 (t + 1))
"""
import json
import os

import numpy as np

from oracle.layers import dropout_key, dropout_mask
from oracle_blocks import DwPwNet, glorot

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden', 'gru_models.json')
KEEP = 0.8


def hsig(v):
    return np.clip(0.2 * v + 0.5, 0.0, 1.0)


def draw_masks(seed, step, B, I, H, keep=KEEP, row_offset=0, T=None, per_step=False):
    """-> (mx [2][3][B, T, I], mh [2][3][B, T, H]) float64, the same mask at every step unless per_step."""
    def one(layer_id, n):
        if not per_step:
            m = dropout_mask(dropout_key(seed, step, layer_id), B * n, keep, offset=row_offset * n).reshape(B, 1, n)
            return np.repeat(m, T, axis=1) / keep
        return np.stack([dropout_mask(dropout_key(seed, step, layer_id + 100 * (t + 1)), B * n, keep, offset=row_offset * n).reshape(B, n)
                         for t in range(T)], axis=1) / keep
    mx = [[one(16 + 6 * d + g, I) for g in range(3)] for d in range(2)]
    mh = [[one(16 + 6 * d + 3 + g, H) for g in range(3)] for d in range(2)]
    return mx, mh


def _blocks(M, H, mutate):
    order = (1, 0, 2) if mutate == 'gate_order' else (0, 1, 2)
    return [M[..., g * H:(g + 1) * H] for g in order], order


def gru_dir_fwd(x, W, U, b, mx, mh, reverse, mutate=None):
    """One direction.  x [B, T, I]; mx [3][B, T, I] / mh [3][B, T, H] or None.  -> (h_last [B, H], cache)."""
    B, T, I = x.shape
    H = U.shape[0]
    ones_x, ones_h = np.ones((B, T, I)), np.ones((B, T, H))
    mx = [ones_x] * 3 if mx is None else mx
    mh = [ones_h] * 3 if mh is None else mh
    (Wz, Wr, Wh), order = _blocks(W, H, mutate)
    (Uz, Ur, Uh), _ = _blocks(U, H, mutate)
    (bz, br, bh), _ = _blocks(b, H, mutate)
    steps = list(range(T - 1, -1, -1)) if reverse else list(range(T))
    h = np.zeros((B, H))
    c = {k: np.zeros((B, T, H)) for k in ('z', 'r', 'c', 'h', 'hp', 'pz', 'pr', 'q')}
    for t in steps:
        pz = (x[:, t] * mx[0][:, t]) @ Wz + bz + (h * mh[0][:, t]) @ Uz
        pr = (x[:, t] * mx[1][:, t]) @ Wr + br + (h * mh[1][:, t]) @ Ur
        z, r = hsig(pz), hsig(pr)
        hh = h * mh[2][:, t]
        q = hh @ Uh                                  # reset_after only
        rec = r * q if mutate == 'reset_after' else (r * hh) @ Uh
        cand = np.tanh((x[:, t] * mx[2][:, t]) @ Wh + bh + rec)
        c['hp'][:, t], c['pz'][:, t], c['pr'][:, t], c['z'][:, t], c['r'][:, t], c['c'][:, t], c['q'][:, t] = h, pz, pr, z, r, cand, q
        h = z * h + (1 - z) * cand
        c['h'][:, t] = h
    c.update(steps=steps, mx=mx, mh=mh, order=order)
    return h, c


def gru_dir_bwd(dh, x, W, U, c, zlin=None, rlin=None, mutate=None):
    """-> (dx [B, T, I], dW, dU, db) of one direction from the gradient wrt its final state."""
    B, T, I = x.shape
    H = U.shape[0]
    (Wz, Wr, Wh), order = _blocks(W, H, mutate)
    (Uz, Ur, Uh), _ = _blocks(U, H, mutate)
    mx, mh = c['mx'], c['mh']
    zlin = (np.abs(c['pz']) < 2.5) if zlin is None else zlin
    rlin = (np.abs(c['pr']) < 2.5) if rlin is None else rlin
    dx = np.zeros_like(x)
    dWg = [np.zeros((I, H)) for _ in range(3)]
    dUg = [np.zeros((H, H)) for _ in range(3)]
    dbg = [np.zeros(H) for _ in range(3)]
    for t in reversed(c['steps']):
        z, r, cand, hp = c['z'][:, t], c['r'][:, t], c['c'][:, t], c['hp'][:, t]
        hh = hp * mh[2][:, t]
        dpc = dh * (1 - z) * (1 - cand * cand)
        dz = dh * (hp - cand)
        dhp = dh * z
        if mutate == 'reset_after':
            dr = dpc * c['q'][:, t]
            dhh = (dpc * r) @ Uh.T
            dUg[2] += hh.T @ (dpc * r)
        else:
            drh = dpc @ Uh.T
            dr = drh * hh
            dhh = drh * r
            dUg[2] += (r * hh).T @ dpc
        dhp = dhp + dhh * mh[2][:, t]
        dpz = dz * 0.2 * zlin[:, t]
        dpr = dr * 0.2 * rlin[:, t]
        dhp = dhp + (dpz @ Uz.T) * mh[0][:, t] + (dpr @ Ur.T) * mh[1][:, t]
        dUg[0] += (hp * mh[0][:, t]).T @ dpz
        dUg[1] += (hp * mh[1][:, t]).T @ dpr
        for g, (dp, Wg) in enumerate(((dpz, Wz), (dpr, Wr), (dpc, Wh))):
            dWg[g] += (x[:, t] * mx[g][:, t]).T @ dp
            dbg[g] += dp.sum(axis=0)
            dx[:, t] += (dp @ Wg.T) * mx[g][:, t]
        dh = dhp
    dW, dU, db = np.zeros_like(W), np.zeros_like(U), np.zeros(3 * H)
    for g, pos in enumerate(order):
        dW[:, pos * H:(pos + 1) * H], dU[:, pos * H:(pos + 1) * H], db[pos * H:(pos + 1) * H] = dWg[g], dUg[g], dbg[g]
    return dx, dW, dU, db


def bigru_fwd(x, weights, mx=None, mh=None, mutate=None):
    """weights: [(W, U, b) forward, (W, U, b) backward] -> (out [B, 2H], caches)."""
    outs, caches = [], []
    for d in range(2):
        rev = d == 1 and mutate != 'backward_not_reversed'
        h, c = gru_dir_fwd(x, weights[d][0], weights[d][1], weights[d][2], None if mx is None else mx[d], None if mh is None else mh[d],
                           rev, mutate)
        outs.append(h)
        caches.append(c)
    return np.concatenate(outs, axis=1), caches


def bigru_bwd(dout, x, weights, caches, decisions=None, mutate=None):
    """-> (dx, [(dW, dU, db) forward, (dW, dU, db) backward])."""
    H = weights[0][1].shape[0]
    dx = np.zeros_like(x)
    grads = []
    for d in range(2):
        zl = None if decisions is None else decisions.get((d, 'z'))
        rl = None if decisions is None else decisions.get((d, 'r'))
        dxd, dW, dU, db = gru_dir_bwd(dout[:, d * H:(d + 1) * H], x, weights[d][0], weights[d][1], caches[d], zl, rl, mutate)
        dx += dxd
        grads.append((dW, dU, db))
    return dx, grads


def orthogonal(rng, shape):
    """Keras 2.1.2 Orthogonal(gain=1): SVD of a normal [rows, cols] matrix, the factor of that shape."""
    a = rng.normal(0.0, 1.0, shape)
    u, _, v = np.linalg.svd(a, full_matrices=False)
    return (u if u.shape == shape else v).astype(np.float32)


# (B, T, I, H) of the stand-alone op's GPU tests and their inputs (test_gru_cpu.py measures how close these come to +-2.5)
KERNEL_CASES = [(1, 1, 8, 16), (5, 2, 8, 16), (37, 10, 8, 16), (5, 1, 224, 128), (37, 2, 224, 128), (37, 10, 224, 128), (1, 2, 384, 192),
                (5, 10, 384, 192), (37, 10, 384, 192)]


def kernel_inputs(B, T, I, H):
    """-> (x [B, T, I], [(W, U, b)] * 2, dout [B, 2H]) float32; wide enough that a few per cent of the gates saturate."""
    rng = np.random.RandomState(B * 1000 + T * 100 + H)
    x = (0.5 * rng.randn(B, T, I)).astype(np.float32)
    ws = []
    for d in range(2):
        lim = np.sqrt(6.0 / (I + 3 * H)) * 2.0
        W = rng.uniform(-lim, lim, (I, 3 * H)).astype(np.float32)
        U = (1.5 * orthogonal(rng, (H, 3 * H))).astype(np.float32)
        b = (0.3 * rng.randn(3 * H)).astype(np.float32)
        ws.append((W, U, b))
    dout = rng.randn(B, 2 * H).astype(np.float32)
    return x, ws, dout


def golden():
    with open(GOLDEN) as f:
        return json.load(f)['conv_1d_simple']


class SimpleNet(DwPwNet):
    """conv_1d_simple from the recorded structure; input [B, 16000] raw samples."""

    def __init__(self, num_classes=12, seed=1234):
        super(SimpleNet, self).__init__(num_classes, seed)
        gold = golden()
        self.blocks = []
        dws = [l for l in gold['layers'] if l['class'] == 'DepthwiseConv2D']
        convs = [l for l in gold['layers'] if l['class'] == 'Conv1D']
        for dwl, cv in zip(dws, convs):
            assert dwl['padding'] == 'valid'
            _, k, C, _ = dwl['kernel']
            F = cv['kernel'][2]
            self.blocks.append({'idx': self.add_block(k, C, F), 'k': k, 's': dwl['strides'], 'C': C, 'F': F, 'L': dwl['input_length'],
                                'Lout': dwl['output'][0]})
        bi = [l for l in gold['layers'] if l['class'] == 'Bidirectional'][0]
        self.T, self.I = bi['input']
        self.H = bi['units']
        self.keep = 1.0 - bi['dropout']
        assert abs(bi['dropout'] - bi['recurrent_dropout']) < 1e-12 and abs(self.keep - KEEP) < 1e-12
        assert (self.blocks[-1]['Lout'], self.blocks[-1]['F']) == (self.T, self.I)
        self.gru_names = []
        for d in ('forward', 'backward'):
            base = '%s/%s_%s/' % (bi['name'], d, bi['layer'])
            self.params[base + 'kernel'] = glorot(self.rng, (self.I, 3 * self.H), self.I, 3 * self.H)
            self.params[base + 'recurrent_kernel'] = orthogonal(self.rng, (self.H, 3 * self.H))
            self.params[base + 'bias'] = np.zeros(3 * self.H, np.float32)
            self.gru_names.append(base)
        self.add_kernel('dense', (2 * self.H, num_classes), 2 * self.H, num_classes, bias=num_classes)

    def _gru_weights(self):
        return [tuple(self._p(b + w) for w in ('kernel', 'recurrent_kernel', 'bias')) for b in self.gru_names]

    def forward(self, x, training=False, seed=0, step=0, cache=None, drop_offset=0, mutate=None):
        B = x.shape[0]
        a = x.astype(self.dtype)[:, :, None]
        if cache is not None:
            cache['batch_stats'] = {}
        for blk in self.blocks:
            a = self.block_fwd(blk['idx'], a, blk['s'], 0, blk['Lout'], training, cache)
        mx = mh = None
        if training:
            mx, mh = draw_masks(seed, step, B, self.I, self.H, self.keep, drop_offset, self.T, per_step=mutate == 'mask_per_step')
            if self.dtype != np.float64:
                mx = [[m.astype(self.dtype) for m in d] for d in mx]
                mh = [[m.astype(self.dtype) for m in d] for d in mh]
        out, caches = bigru_fwd(a, self._gru_weights(), mx, mh, mutate)
        p = self.head_fwd(out, 'dense_1/kernel', 'dense_1/bias')
        if cache is not None:
            cache.update(gru_in=a, gru_out=out, gru=caches, p=p)
        return p

    def loss_and_grads(self, x, y_onehot, seed=0, step=0, drop_offset=0, relu_masks=None, decisions=None, mutate=None):
        """Data loss (batch mean) and its gradients (no L2 term)."""
        cache, grads = {}, {}
        p = self.forward(x, training=True, seed=seed, step=step, cache=cache, drop_offset=drop_offset, mutate=mutate)
        loss, dout = self.head_bwd(p, y_onehot, cache['gru_out'], 'dense_1/kernel', 'dense_1/bias', grads)
        da, gg = bigru_bwd(dout, cache['gru_in'], self._gru_weights(), cache['gru'], decisions, mutate)
        for base, (dW, dU, db) in zip(self.gru_names, gg):
            grads[base + 'kernel'], grads[base + 'recurrent_kernel'], grads[base + 'bias'] = dW, dU, db
        for blk in reversed(self.blocks):
            da = self.block_bwd(blk['idx'], da, blk['s'], 0, cache, grads, relu_masks)
        return loss, p, self.ordered(grads), cache
