"""Float64 NumPy oracle of conv_1d_top_down (reference model.py:1326-1397): forward, loss and every gradient, restated layer by
layer for the CPU cross-check against torch autograd and the GPU parity tests, on oracle_blocks (dw_fwd / dw_bwd, OracleNet).

TEST INFRASTRUCTURE ONLY.  The front end is Conv1D(480, 479, strides=160, VALID) WITH bias and nothing behind it.  A block is g
groups, each DepthwiseConv2D((1, 3), VALID, strides=s) -> Conv1D(F / g, 1) -> BatchNormalization -> relu6 (no bias, l2 1e-5 on both
kernels), concatenated in group order.  The groups of a reduce block (stride 2) read the slices [q * gs, (q + 1) * gs), gs =
num_channels / g from the block's argument - the third block asks for 300 of 420 channels, so 120 are never read.  The groups of a
context block (stride 1) EACH read the whole input: the reference cuts the slice and then hands x to the group, so the depthwise
kernels are [3, C].  Dropout masks are oracle/layers.py's counter-based ones (layer_id 1), as on the device.

Mutations (what the device must NOT agree with): 'context_sliced' - the context groups read the slice the reference cuts and drops
(the kernels' other columns unused); 'reduce_full_width' - the third block's windows start at multiples of 420 / 3 = 140, not 100.
"""
import numpy as np

from oracle_blocks import OracleNet, dw_bwd, dw_fwd, gconv_bwd, gconv_fwd

FRONT_K, FRONT_N, FRONT_STRIDE = 479, 480, 160
# (filters, groups, num_channels, stride, shared) per block
BLOCKS = [(420, 3, 480, 2, False), (420, 2, 420, 1, True), (360, 3, 300, 2, False), (360, 2, 360, 1, True),
          (300, 3, 360, 2, False), (300, 2, 300, 1, True), (240, 3, 300, 2, False), (240, 2, 240, 1, True)]
KEEP = 0.95   # Dropout(0.05)
K = 3
MUTATIONS = ('context_sliced', 'reduce_full_width')


def front_rows(L):
    return (L - FRONT_K) // FRONT_STRIDE + 1


class TopDownNet(OracleNet):
    def __init__(self, num_classes=12, input_size=16000, seed=1234):
        super(TopDownNet, self).__init__(num_classes, seed)
        self.input_size = input_size
        self.rows = front_rows(input_size)
        self.front = self.add_kernel('conv1d', (FRONT_K, 1, FRONT_N), FRONT_K, FRONT_K * FRONT_N, bias=FRONT_N)
        self.front_bias = 'conv1d_1/bias'
        self.blocks = []
        L, C = self.rows, FRONT_N
        for F, g, nch, s, shared in BLOCKS:
            assert nch % g == 0 and F % g == 0 and nch <= C
            gs, Ng = (C if shared else nch // g), F // g
            blk = {'F': F, 'g': g, 'gs': gs, 'Ng': Ng, 'stride': s, 'shared': shared, 'L': L, 'C': C, 'nch': nch,
                   'Lout': (L - K) // s + 1, 'dws': [], 'pws': [], 'bns': []}
            for q in range(g):
                blk['dws'].append(self.add_kernel('depthwise_conv2d', (1, K, gs, 1), K * gs, K, l2=True, suffix='depthwise_kernel'))
                blk['pws'].append(self.add_kernel('conv1d', (1, gs, Ng), gs, Ng, l2=True))
                blk['bns'].append(self.add_bn(Ng))
            self.blocks.append(blk)
            L, C = blk['Lout'], F
        self.D = L * C
        self.add_kernel('dense', (self.D, self.nc), self.D, self.nc, bias=self.nc)

    def windows(self, i, mutate=None):
        """per group: (first channel, channels read, the kernel columns that meet them)"""
        blk = self.blocks[i]
        g, gs, C = blk['g'], blk['gs'], blk['C']
        if blk['shared']:
            if mutate == 'context_sliced':
                w = blk['nch'] // g
                return [(q * w, w, slice(q * w, (q + 1) * w)) for q in range(g)]
            return [(0, C, slice(None))] * g
        if mutate == 'reduce_full_width' and i == 2:
            return [(q * (C // g), gs, slice(None)) for q in range(g)]
        return [(q * gs, gs, slice(None)) for q in range(g)]

    def forward(self, x, training=False, seed=0, step=0, cache=None, drop_offset=0, mutate=None):
        B = x.shape[0]
        x3 = x.astype(np.float64).reshape(B, self.input_size, 1)
        front = gconv_fwd(x3, [self._p(self.front)], FRONT_K, FRONT_STRIDE, 1)
        h = front + self._p(self.front_bias)
        if cache is not None:
            cache.update(front=front, x0=h, batch_stats={})
        for i, blk in enumerate(self.blocks):
            outs = []
            for q, (c0, width, cols) in enumerate(self.windows(i, mutate)):
                a = h[:, :, c0:c0 + width]
                w = self._p(blk['dws'][q])[0, :, cols, 0]
                z = dw_fwd(a, w, blk['stride'], 0, blk['Lout'])
                if cache is not None:
                    cache['z%d_%d' % (i, q)] = z
                outs.append(self.bn_act_fwd(blk['bns'][q], z @ self._p(blk['pws'][q])[0, cols], training, cache))
            if cache is not None:
                cache['in%d' % i] = h
            h = np.concatenate(outs, axis=2)
            assert h.shape[1:] == (blk['Lout'], blk['F'])
        f, keep = h.reshape(B, -1), None
        if training:
            keep = self.dropout(seed, step, 1, B, self.D, KEEP, drop_offset)
            f = f * keep / KEEP
        p = self.head_fwd(f, 'dense_1/kernel', 'dense_1/bias')
        if cache is not None:
            cache.update(a_last=h, f=f, keep=keep, p=p)
        return p

    def loss_and_grads(self, x, y_onehot, seed=0, step=0, drop_offset=0, relu_masks=None, mutate=None):
        """Data loss (batch mean) and its gradients (no L2 term).  relu_masks: {bn index: [B, Lout, Ng]} decisions to use in place
        of the oracle's own (the device's, read back, so that values at the ReLU6 kinks cannot flip).  cache['da%d' % i]: the
        gradient wrt block i's activated input (i = 0: wrt the front convolution's output + bias)."""
        cache, grads = {}, {}
        p = self.forward(x, training=True, seed=seed, step=step, cache=cache, drop_offset=drop_offset, mutate=mutate)
        loss, df = self.head_bwd(p, y_onehot, cache['f'], 'dense_1/kernel', 'dense_1/bias', grads)
        da = (df * cache['keep'] / KEEP).reshape(cache['a_last'].shape)
        for i in range(len(self.blocks) - 1, -1, -1):
            blk = self.blocks[i]
            Ng, h = blk['Ng'], cache['in%d' % i]
            dh = np.zeros_like(h)
            for q, (c0, width, cols) in enumerate(self.windows(i, mutate)):
                dy = self.bn_act_bwd(blk['bns'][q], da[:, :, q * Ng:(q + 1) * Ng], cache, grads, relu_masks)
                z = cache['z%d_%d' % (i, q)]
                pw = self._p(blk['pws'][q])[0]
                dpw = np.zeros_like(pw)
                dpw[cols] = z.reshape(-1, z.shape[2]).T @ dy.reshape(-1, Ng)
                grads[blk['pws'][q]] = dpw[None]
                taps = self._p(blk['dws'][q])[0, :, :, 0]
                dxq, dw = dw_bwd(dy @ pw[cols].T, h[:, :, c0:c0 + width], taps[:, cols], blk['stride'], 0)
                dtaps = np.zeros_like(taps)
                dtaps[:, cols] = dw
                grads[blk['dws'][q]] = dtaps[None, :, :, None]
                dh[:, :, c0:c0 + width] += dxq
            cache['da%d' % i] = da = dh
        grads[self.front_bias] = da.sum(axis=(0, 1))
        x3 = x.astype(np.float64).reshape(x.shape[0], self.input_size, 1)
        _, (grads[self.front],) = gconv_bwd(da, x3, [self._p(self.front)], FRONT_K, FRONT_STRIDE, 1, need_dx=False)
        return loss, p, self.ordered(grads), cache
