"""Float64 NumPy oracle of the grouped-Conv1D models conv_1d_fast (reference model.py:642-713) and conv_1d_spec
(model.py:1249-1323): forward, loss and every gradient, restated layer by layer for the GPU parity tests.

TEST INFRASTRUCTURE ONLY.  A grouped block is g separate Conv1D(F/g, k, VALID, no bias) layers over the slices
x[:, :, q*gs:(q+1)*gs] (gs = num_channels / g from the block's argument), each followed by its own BatchNormalization and
relu6, concatenated in group order.  Dropout masks are oracle/layers.py's counter-based ones (layer_id 1), as on the device.
"""
import numpy as np

from oracle_blocks import OracleNet, gconv_bwd, gconv_fwd

# (filters, k, groups, num_channels, stride) per grouped block
FAST_BLOCKS = [(300, 15, 6, 252, 2), (360, 7, 5, 300, 2)]
SPEC_BLOCKS = [(300, 3, 4, 252, 2), (300, 3, 3, 300, 1), (360, 3, 4, 300, 2), (360, 3, 3, 360, 1),
               (420, 3, 4, 360, 2), (420, 3, 3, 360, 1), (480, 3, 4, 420, 2), (480, 3, 3, 480, 1)]
KEEP = 0.7   # Dropout(0.3)


class GroupedBlocksNet(OracleNet):
    """A ladder of grouped blocks behind a front end, Flatten -> Dropout(.3) -> Dense -> softmax on top: what GroupedConvNet and
    learned_spec_oracle.LearnedSpecNet share.  A block's groups read the channel windows blk['slices'] (clipped at the channel
    count) of its input."""

    def add_blocks(self, spec, L, C):
        self.blocks = []
        for F, k, g, nch, s in spec:
            gs, Ng = nch // g, F // g
            slices = [(min(q * gs, C), min((q + 1) * gs, C)) for q in range(g)]
            blk = {'F': F, 'k': k, 'g': g, 'gs': gs, 'Ng': Ng, 'stride': s, 'L': L, 'C': C, 'Lout': (L - k) // s + 1,
                   'slices': slices, 'convs': [], 'bns': []}
            for a, b in slices:
                blk['convs'].append(self.add_kernel('conv1d', (k, b - a, Ng), k * (b - a), k * Ng))
                blk['bns'].append(self.add_bn(Ng))
            self.blocks.append(blk)
            L, C = blk['Lout'], F
        self.D = L * C
        self.add_kernel('dense', (self.D, self.nc), self.D, self.nc, bias=self.nc)

    def _slices(self, i, mutate):
        return self.blocks[i]['slices']

    def blocks_fwd(self, h, training, seed, step, cache, drop_offset, mutate):
        """h: the front end's output -> probabilities"""
        B = h.shape[0]
        if cache is not None:
            cache['x0'] = h
            cache['batch_stats'] = {}
        for i, blk in enumerate(self.blocks):
            ys = [gconv_fwd(h[:, :, a:b], [self._p(name)], blk['k'], blk['stride'], b - a)
                  for (a, b), name in zip(self._slices(i, mutate), blk['convs'])]
            if mutate == 'reverse_groups':
                ys = ys[::-1]
            if cache is not None:
                cache['in%d' % i] = h
            h = np.concatenate([self.bn_act_fwd(idx, yq, training, cache) for idx, yq in zip(blk['bns'], ys)], axis=2)
            assert h.shape[1:] == (blk['Lout'], blk['F'])
        f, keep = h.reshape(B, -1), None
        if training:
            keep = self.dropout(seed, step, 1, B, self.D, KEEP, drop_offset)
            f = f * keep / KEEP
        p = self.head_fwd(f, 'dense_1/kernel', 'dense_1/bias')
        if cache is not None:
            cache.update(a_last=h, f=f, keep=keep, p=p)
        return p

    def blocks_bwd(self, p, y_onehot, cache, grads, relu_masks, mutate, need_dx):
        """-> (mean loss, gradient wrt the front end's output or None); cache['da<i>']: the gradient wrt block i's input"""
        loss, df = self.head_bwd(p, y_onehot, cache['f'], 'dense_1/kernel', 'dense_1/bias', grads)
        da = (df * cache['keep'] / KEEP).reshape(cache['a_last'].shape)
        for i in range(len(self.blocks) - 1, -1, -1):
            blk = self.blocks[i]
            Ng = blk['Ng']
            h = cache['in%d' % i]
            dys = [self.bn_act_bwd(idx, da[:, :, q * Ng:(q + 1) * Ng], cache, grads, relu_masks) for q, idx in enumerate(blk['bns'])]
            if mutate == 'reverse_groups':
                dys = dys[::-1]
            dh = np.zeros_like(h) if i > 0 or need_dx else None
            for (a, b), name, dyq in zip(self._slices(i, mutate), blk['convs'], dys):
                dxq, (grads[name],) = gconv_bwd(dyq, h[:, :, a:b], [self._p(name)], blk['k'], blk['stride'], b - a,
                                                need_dx=dh is not None, swap_phase=(mutate == 'swap_phase'))
                if dh is not None:
                    dh[:, :, a:b] += dxq
            cache['da%d' % i] = da = dh
        return loss, da


class GroupedConvNet(GroupedBlocksNet):
    """kind 'fast' (raw [16000]) or 'spec' ([98 * 257] = the generator's 'spec' output)."""

    def __init__(self, kind, num_classes=12, input_size=16000, seed=1234):
        super(GroupedConvNet, self).__init__(num_classes, seed)
        self.kind, self.front = kind, None
        if kind == 'fast':
            self.front = self.add_kernel('conv1d', (479, 1, 252), 479, 479 * 252, l2=True)
            self.in_shape = (input_size, 1)
            self.add_blocks(FAST_BLOCKS, (input_size - 479) // 160 + 1, 252)
        else:
            self.in_shape = (98, 257)
            self.add_blocks(SPEC_BLOCKS, 98, 257)

    def forward(self, x, training=False, seed=0, step=0, cache=None, drop_offset=0, mutate=None):
        h = x.astype(np.float64).reshape((x.shape[0],) + self.in_shape)
        if self.front:
            h = gconv_fwd(h, [self._p(self.front)], 479, 160, 1)
        return self.blocks_fwd(h, training, seed, step, cache, drop_offset, mutate)

    def loss_and_grads(self, x, y_onehot, seed=0, step=0, drop_offset=0, relu_masks=None, mutate=None):
        """Data loss (batch mean) and its gradients (no L2 term).  relu_masks: {bn index: [B, Lout, Ng]} decisions to use
        in place of the oracle's own (the device's, read back, so that values at the ReLU6 kinks cannot flip)."""
        cache, grads = {}, {}
        p = self.forward(x, training=True, seed=seed, step=step, cache=cache, drop_offset=drop_offset, mutate=mutate)
        loss, da = self.blocks_bwd(p, y_onehot, cache, grads, relu_masks, mutate, need_dx=self.front is not None)
        if self.front:
            _, (grads[self.front],) = gconv_bwd(da, x.astype(np.float64).reshape((x.shape[0],) + self.in_shape), [self._p(self.front)],
                                                479, 160, 1, need_dx=False)
        return loss, p, self.ordered(grads), cache
