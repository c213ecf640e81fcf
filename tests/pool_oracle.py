"""Float64-capable NumPy oracle of MaxPool1D(3, strides=2) in either padding: Lp windows over the input padded with -inf, window t
covering the rows 2t - pad_l + j, j < 3.  TEST INFRASTRUCTURE ONLY.
  'valid'  Lp = (L - 3) // 2 + 1, pad_l = 0 (no window reaches a padded row)      pool_len
  'same'   Lp = ceil(L / 2),      pad_l = pad_total // 2 (TensorFlow)             same_geometry
The gradient of a window goes to the FIRST maximum (TF MaxPoolGrad); the padding never wins."""
import numpy as np

import oracle_blocks


def pool_len(L):
    return (L - 3) // 2 + 1


def same_geometry(L, odd_left=False):
    """-> (windows, pad_left): TensorFlow SAME for pool 3, stride 2 (odd_left: the odd padding sample on the left)."""
    return oracle_blocks.same_geometry(L, 3, 2, odd_left=odd_left)[:2]


def windows(a, Lp, pad_l):
    """[B, L, C] -> [B, Lp, 3, C]."""
    ap = np.pad(a, ((0, 0), (pad_l, max(2 * Lp + 1 - pad_l - a.shape[1], 0)), (0, 0)), constant_values=-np.inf)
    return ap[:, 2 * np.arange(Lp)[:, None] + np.arange(3)[None, :], :]


def argmax(a, Lp, pad_l, last=False):
    """Offset (0..2) of the first (last: the last) maximum of every window."""
    w = windows(a, Lp, pad_l)
    return 2 - np.argmax(w[:, :, ::-1, :], axis=2) if last else np.argmax(w, axis=2)


def fwd(a, ind, pad_l):
    return np.take_along_axis(windows(a, ind.shape[1], pad_l), ind[:, :, None, :], axis=2)[:, :, 0, :]


def bwd(dz, ind, L, pad_l):
    """dz [B, Lp, C], ind [B, Lp, C] -> da [B, L, C]: every window's gradient goes to the row it names."""
    B, Lp, C = dz.shape
    dap = np.zeros((B, max(2 * Lp + 1, pad_l + L), C), dz.dtype)
    for j in range(3):
        dap[:, j:j + 2 * Lp:2, :] += dz * (ind == j)
    return dap[:, pad_l:pad_l + L, :]
