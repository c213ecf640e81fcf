"""The conv_1d_multi_time_sliced oracle net (tests/mts_oracle.py) restated on torch autograd, CPU only: float64 to check the oracle's
hand-written backward, float32 to measure what single precision alone costs against the float64 oracle (the source of the GPU
parity bars).  TEST INFRASTRUCTURE ONLY.  F.conv1d with groups = C is the depthwise layer, F.max_pool1d over explicit -inf padding
the SAME pool, F.batch_norm in training mode the BatchNormalization; the dropout masks are the oracle's."""
import numpy as np
import torch
import torch.nn.functional as Fn

from oracle.layers import dropout_key, dropout_mask


def same_pool(h, pad_l):
    """h [B, C, L] -> MaxPool1D(3, 2, 'same') with TensorFlow's padding, as -inf rows."""
    L = h.shape[2]
    Lp = -(-L // 2)
    return Fn.max_pool1d(Fn.pad(h, (pad_l, 2 * Lp + 1 - pad_l - L), value=float('-inf')), 3, 2)


def torch_step(ora, x, y, seed, step, dtype=torch.float64):
    """-> (loss, probabilities, {name: gradient}, {block: pre-activation [B, L, C]}) of one training step."""
    P = {k: torch.tensor(v.astype(np.float64), dtype=dtype, requires_grad=True) for k, v in ora.params.items()}
    B = x.shape[0]
    xt = torch.tensor(x.astype(np.float64), dtype=dtype)
    pres = {}

    def block(blk, h):   # h [B, C, L]
        n = blk['idx']
        w = P['depthwise_conv2d_%d/depthwise_kernel' % n][0, :, :, 0]          # [k, C]
        h = Fn.conv1d(h, w.t()[:, None, :], groups=blk['C'])
        h = Fn.conv1d(h, P['conv1d_%d/kernel' % n].permute(2, 1, 0))
        pre = Fn.batch_norm(h, None, None, P['batch_normalization_%d/gamma' % n], P['batch_normalization_%d/beta' % n],
                            training=True, eps=1e-3)
        pres[n] = pre.detach().permute(0, 2, 1).numpy()
        return pre.clamp(0, 6)

    act, pooled = {}, {}
    for blk in ora.blocks[:-1]:
        s = blk['src']
        h = xt.reshape(B, s[1], s[2]).permute(0, 2, 1) if s[0] == 'raw' else (pooled[s[1]] if s[0] == 'pool' else act[s[1]])
        a = block(blk, h)
        act[blk['idx']] = a
        if blk['pool'] is not None:
            pooled[blk['idx']] = same_pool(a, blk['pool']['pad_l'])
    feat = torch.cat([act[e] for e in ora.ends], dim=1)                        # [B, 320, 1]
    keep1 = dropout_mask(dropout_key(seed, step, 1), B * ora.D, ora.keep[0]).reshape(B, ora.D, 1)
    feat = feat * torch.tensor(keep1.astype(np.float64), dtype=dtype) / ora.keep[0]
    H = ora.head['F']
    h = block(ora.head, feat).reshape(B, H)
    keep2 = dropout_mask(dropout_key(seed, step, 2), B * H, ora.keep[1]).reshape(B, H)
    h = h * torch.tensor(keep2.astype(np.float64), dtype=dtype) / ora.keep[1]
    p = torch.softmax(h @ P[ora.out_kernel][0] + P[ora.out_bias], dim=1)
    loss = -(torch.tensor(y.astype(np.float64), dtype=dtype) * torch.log(p.clamp(1e-7, 1 - 1e-7))).sum(1).mean()
    loss.backward()
    return float(loss.detach()), p.detach().numpy(), {k: v.grad.numpy() for k, v in P.items()}, pres


def decisions_from_pres(ora, pres):
    """ReLU6 masks and pool winners of a run, from its pre-activations (what the GPU tests read back from the device)."""
    import pool_oracle
    masks, inds = {}, {}
    for blk in ora.blocks:
        pre = pres[blk['idx']]
        masks[blk['idx']] = ((pre > 0) & (pre <= 6)).astype(np.float64)
        if blk['pool'] is not None:
            inds[blk['idx']] = pool_oracle.argmax(np.clip(pre, 0, 6), blk['pool']['Lp'], blk['pool']['pad_l'])
    return masks, inds
