"""Float64 NumPy oracle of the three-branch raw-waveform net conv_1d_multi_time_sliced (reference model.py:1080-1156): forward,
loss and every gradient, restated layer by layer for the GPU parity tests.

TEST INFRASTRUCTURE ONLY.  The structure - names, order, shapes, l2, which tensor feeds which block, the pools and their left
padding, the concatenation - is read from tests/golden/mts_models.json (recorded from the reference by
tests/golden/make_golden_mts.py); nothing about it is restated here.  A block is DepthwiseConv2D((1, k), VALID, no bias) ->
Conv1D(F, 1, no bias) -> BatchNormalization -> relu6 (oracle_blocks.DwPwNet); a reduce block is followed by
MaxPool1D(3, strides=2, 'same'): TensorFlow's SAME geometry (ceil(L / 2) windows, pad_left = pad_total // 2, the padding never
wins), the gradient to the FIRST maximum of a window.  Dropout masks are oracle/layers.py's counter-based ones (layer ids 1 and 2).

`relu_masks` / `pool_ind` hand the device's own ReLU6 and arg-max decisions to the backward pass ({block number 1..32: array});
`mutate` names a deliberately wrong variant for the negative controls:
  'drop_fork'      at a tensor with two consumers the tap's gradient (the branch end's) is dropped instead of added
  'pool_pad_side'  the pool's odd padding sample on the LEFT (even input lengths: pad_left 1 instead of 0)
  'last_max'       the LAST maximum of a window wins
"""
import json
import os

import numpy as np

import pool_oracle
from oracle_blocks import DwPwNet, glorot

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden', 'mts_models.json')
MODEL = 'conv_1d_multi_time_sliced'


# ---- the net -------------------------------------------------------------------------------------------------------------------
def load_structure(num_classes=None):
    """The fixture as block records, in creation order.  A block: idx (Keras number), k, C, F, L, Lout, src = ('raw', L, C) |
    ('pool', block) | ('act', block) | ('concat',), pool = None | {'pad_l', 'pad_total', 'Lp'}.  -> (blocks, ends, gold)"""
    with open(GOLDEN) as f:
        gold = json.load(f)[MODEL]
    layers = gold['layers']
    by_name = {l['name']: l for l in layers}
    blocks, pools = [], {}
    for l in layers:
        if l['class'] == 'MaxPool1D':
            assert l['input_from'].startswith('activation_') and (l['pool_size'], l['strides'], l['padding']) == (3, 2, 'same')
            pools[l['name']] = int(l['input_from'].split('_')[1])
    for l in layers:
        if l['class'] != 'DepthwiseConv2D':
            continue
        idx = int(l['name'].split('_')[-1])
        conv = by_name['conv1d_%d' % idx]
        src = l['input_from']
        if src.startswith('reshape_'):
            s = ('raw',) + tuple(by_name[src]['output'])
        elif src.startswith('max_pool1d_'):
            s = ('pool', pools[src])
        elif src.startswith('activation_'):
            s = ('act', int(src.split('_')[1]))
        else:
            assert src.startswith('dropout_') and by_name[src]['input_from'].startswith('concatenate_')
            s = ('concat',)
        assert (l['strides'], l['padding'], conv['kernel'][0], conv['kernel'][1]) == (1, 'valid', 1, l['kernel'][2])
        blocks.append({'idx': idx, 'k': l['kernel'][1], 'C': l['kernel'][2], 'F': conv['kernel'][2], 'L': l['input_length'],
                       'Lout': l['output'][0], 'src': s, 'pool': None})
    for name, idx in pools.items():
        l = by_name[name]
        blocks[idx - 1]['pool'] = {'pad_l': l['pad_left'], 'pad_total': l['pad_total'], 'Lp': l['output'][0]}
    assert [b['idx'] for b in blocks] == list(range(1, len(blocks) + 1))
    cat = [l for l in layers if l['class'] == 'Concatenate']
    assert len(cat) == 1
    ends = [int(s.split('_')[1]) for s in cat[0]['inputs_from']]
    return blocks, ends, gold


class MtsNet(DwPwNet):
    """conv_1d_multi_time_sliced; input [B, 16000] raw samples."""

    def __init__(self, num_classes=12, seed=1234):
        super(MtsNet, self).__init__(num_classes, seed)
        self.blocks, self.ends, gold = load_structure()
        self.keep = [1.0 - l['rate'] for l in gold['layers'] if l['class'] == 'Dropout']
        assert len(self.keep) == 2
        self.l2 = {}
        for w in gold['weights']:
            shape = list(w['shape'])
            name = w['name']
            if name.startswith('conv1d_%d/' % (len(self.blocks) + 1)):
                shape[-1] = num_classes          # the fixture was recorded at 12 classes
            if name.endswith('depthwise_kernel'):
                v = glorot(self.rng, shape, shape[1] * shape[2], shape[1])
            elif name.endswith('/kernel'):
                v = glorot(self.rng, shape, shape[0] * shape[1], shape[0] * shape[2])
            elif name.endswith('gamma') or name.endswith('moving_variance'):
                v = np.ones(shape, np.float32)
            else:
                v = np.zeros(shape, np.float32)
            (self.state if w.get('state') else self.params)[name] = v
            if not w.get('state'):
                self.l2[name] = w['l2']
        self.l2_names = [k for k, v in self.l2.items() if v > 0]
        self.out_kernel = 'conv1d_%d/kernel' % (len(self.blocks) + 1)
        self.out_bias = 'conv1d_%d/bias' % (len(self.blocks) + 1)
        self.head = self.blocks[-1]
        assert self.head['src'] == ('concat',)
        self.D = self.head['C']
        self.consumers = {}
        for b in self.blocks:
            if b['src'][0] == 'act':
                self.consumers.setdefault(b['src'][1], []).append(b['idx'])
        self.forks = sorted(k for k, v in self.consumers.items() if len(v) > 1)

    def _pad_l(self, blk, mutate):
        if mutate == 'pool_pad_side':
            return blk['pool']['pad_total'] - blk['pool']['pad_l']
        return blk['pool']['pad_l']

    def _block(self, blk, a, training, cache, mutate, pool_ind):
        n = blk['idx']
        act = self.block_fwd(n, a, 1, 0, blk['Lout'], training, cache)
        ind = pooled = None
        if blk['pool'] is not None:
            pad_l, Lp = self._pad_l(blk, mutate), blk['pool']['Lp']
            if mutate == 'last_max':
                ind = pool_oracle.argmax(act, Lp, pad_l, last=True)
            elif pool_ind is not None and n in pool_ind and mutate != 'pool_pad_side':
                ind = pool_ind[n]
            else:
                ind = pool_oracle.argmax(act, Lp, pad_l)
            pooled = pool_oracle.fwd(act, ind, pad_l)
        if cache is not None:
            cache['ind%d' % n] = ind
        return act, pooled

    def forward(self, x, training=False, seed=0, step=0, cache=None, drop_offset=0, mutate=None, pool_ind=None):
        B = x.shape[0]
        x = x.astype(np.float64)
        if cache is not None:
            cache['batch_stats'] = {}
        act, pooled = {}, {}
        for blk in self.blocks[:-1]:
            s = blk['src']
            a = x.reshape(B, s[1], s[2]) if s[0] == 'raw' else (pooled[s[1]] if s[0] == 'pool' else act[s[1]])
            act[blk['idx']], pooled[blk['idx']] = self._block(blk, a, training, cache, mutate, pool_ind)
        feat = np.concatenate([act[e] for e in self.ends], axis=2)       # [B, 1, 320]
        assert feat.shape == (B, 1, self.D)
        keep1 = keep2 = None
        if training:
            keep1 = self.dropout(seed, step, 1, B, self.D, self.keep[0], drop_offset).reshape(B, 1, self.D)
            feat = feat * keep1 / self.keep[0]
        h, _ = self._block(self.head, feat, training, cache, mutate, pool_ind)
        H = self.head['F']
        h = h.reshape(B, H)
        if training:
            keep2 = self.dropout(seed, step, 2, B, H, self.keep[1], drop_offset)
            h = h * keep2 / self.keep[1]
        p = self.head_fwd(h, self.out_kernel, self.out_bias)
        if cache is not None:
            cache.update(h=h, keep1=keep1, keep2=keep2, p=p)
        return p

    def loss_and_grads(self, x, y_onehot, seed=0, step=0, drop_offset=0, relu_masks=None, pool_ind=None, mutate=None):
        """Data loss (batch mean) and its gradients (no L2 term)."""
        cache, grads = {}, {}
        B = x.shape[0]
        p = self.forward(x, training=True, seed=seed, step=step, cache=cache, drop_offset=drop_offset, mutate=mutate,
                         pool_ind=pool_ind)
        loss, dh = self.head_bwd(p, y_onehot, cache['h'], self.out_kernel, self.out_bias, grads)
        dh = (dh * cache['keep2'] / self.keep[1]).reshape(B, 1, self.head['F'])
        dfeat = self.block_bwd(self.head['idx'], dh, 1, 0, cache, grads, relu_masks) * cache['keep1'] / self.keep[0]
        dact, dpool = {}, {}                       # gradients wrt activated / pooled outputs, by producing block
        col = 0
        for e in self.ends:
            F = self.blocks[e - 1]['F']
            dact[e] = dfeat[:, :, col:col + F]
            col += F
        for blk in reversed(self.blocks[:-1]):
            n = blk['idx']
            if blk['pool'] is not None:
                d = pool_oracle.bwd(dpool[n], cache['ind%d' % n], blk['Lout'], self._pad_l(blk, mutate))
                dact[n] = dact[n] + d if n in dact else d
            da = self.block_bwd(n, dact[n], 1, 0, cache, grads, relu_masks)
            s = blk['src']
            if s[0] == 'pool':
                dpool[s[1]] = da
            elif s[0] == 'act':
                if mutate == 'drop_fork' and s[1] in self.forks and n in self.ends:
                    continue
                dact[s[1]] = dact[s[1]] + da if s[1] in dact else da
        return loss, p, self.ordered(grads), cache
