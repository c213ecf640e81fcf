"""Cases, inputs and float64 references of the kws_pool3s2_same_* / kws_stem_* kernel tests (tests/test_mts_kernels_gpu.py), kept
in a plain module so that tests/test_mts_cpu.py can check on the CPU what those tests assume about their own inputs.  TEST
INFRASTRUCTURE ONLY."""
import numpy as np

import pool_oracle

# (B, L, C): both parities, the smallest L, the thread-run boundaries of forward (4 outputs) and backward (8 rows), the widest and
# narrowest C of the ladders
POOL_CASES = [(2, 2, 4), (2, 3, 8), (3, 20, 192), (2, 37, 128), (2, 59, 160), (2, 122, 128), (1, 1997, 32), (2, 3998, 16),
              (2, 5, 1024), (2, 8, 1024)]   # C = 1024: one run per workgroup (R = 1)
# (B, L, C, N)
STEM_CASES = [(2, 6, 3, 8), (2, 37, 4, 16), (2, 41, 5, 16), (3, 19, 25, 32), (1, 4000, 4, 16), (2, 3200, 5, 16), (2, 640, 25, 32),
              (2, 300, 32, 64), (2, 50, 1, 4)]
KINK_EPS, TIE_EPS = 1e-5, 1e-6


def pool_inputs(B, L, C, seed=None):
    """-> y [B, L, C], table [4 C] (scale | shift | mean | rstd, about 35 % of the scales negative), dz [B, Lp, C]; float32."""
    rng = np.random.RandomState(1000 * L + C if seed is None else seed)
    y = rng.randn(B, L, C).astype(np.float32)
    scale = (1.0 + 0.1 * rng.randn(C)) * np.where(rng.rand(C) < 0.35, -1.0, 1.0)
    scale[0] = -abs(scale[0])
    tab = np.concatenate([scale, 0.5 + 0.3 * rng.randn(C), 0.3 * rng.randn(C), 0.5 + rng.rand(C)]).astype(np.float32)
    dz = rng.randn(B, pool_oracle.same_geometry(L)[0], C).astype(np.float32)
    return y, tab, dz


def pool_pre(y, tab):
    """float64 pre-activation and its float32 rounding (the device's one fused multiply-add)."""
    C = y.shape[2]
    pre = y.astype(np.float64) * tab[:C].astype(np.float64) + tab[C:2 * C].astype(np.float64)
    return pre, pre.astype(np.float32)


def pool_compared(y, tab, dz=None):
    """Mask [B, L, C] of the elements of g the backward test compares: the float64 pre-activation farther than KINK_EPS from 0 and
    6, and no window the row belongs to whose two largest activations are closer than TIE_EPS while its maximum lies strictly
    inside (0, 6).  (A tie of saturated values needs no exclusion: whichever row wins, its gate is shut and g is 0, except at
    pre = 6 exactly, which the kink margin covers.)"""
    B, L, C = y.shape
    Lp, pad_l = pool_oracle.same_geometry(L)
    pre, _ = pool_pre(y, tab)
    far = (np.abs(pre) > KINK_EPS) & (np.abs(pre - 6) > KINK_EPS)
    w = np.sort(pool_oracle.windows(np.clip(pre, 0, 6), Lp, pad_l), axis=2)          # ascending; -inf = padding
    tie = (w[:, :, 2] - w[:, :, 1] <= TIE_EPS) & (w[:, :, 2] > 0) & (w[:, :, 2] < 6)   # [B, Lp, C]
    bad = np.zeros((B, 2 * Lp + 1, C), bool)
    for j in range(3):
        bad[:, j:j + 2 * Lp:2, :] |= tie
    return far & ~bad[:, pad_l:pad_l + L, :]


def pool_excluded_share(y, tab, dz=None):
    return 1.0 - pool_compared(y, tab).mean()


def stem_inputs(B, L, C, N):
    rng = np.random.RandomState(100 * L + 10 * C + N)
    x = rng.randn(B, L, C).astype(np.float32)
    w = (rng.randn(3, C) / np.sqrt(3)).astype(np.float32)
    p = (rng.randn(C, N) / np.sqrt(C)).astype(np.float32)
    dy = rng.randn(B, L - 2, N).astype(np.float32)
    return x, w, p, dy


def stem_reference(x, w, p, dy):
    """float64 (y, |terms| of y, dp, |terms| of dp, dw, |terms| of dw): the sums the device forms and the sums of the magnitudes of
    their terms, which scale the rounding bars."""
    x, w, p, dy = (v.astype(np.float64) for v in (x, w, p, dy))
    Lout = x.shape[1] - 2
    taps = np.stack([x[:, j:j + Lout, :] for j in range(3)])                   # [3, B, Lout, C]
    z = np.einsum('jc,jblc->blc', w, taps)
    za = np.einsum('jc,jblc->blc', np.abs(w), np.abs(taps))
    y, ya = z @ p, za @ np.abs(p)
    dp = np.einsum('blc,bln->cn', z, dy)
    dpa = np.einsum('blc,bln->cn', za, np.abs(dy))
    dz = dy @ p.T
    dza = np.abs(dy) @ np.abs(p).T
    dw = np.einsum('jblc,blc->jc', taps, dz)
    dwa = np.einsum('jblc,blc->jc', np.abs(taps), dza)
    return y, ya, dp, dpa, dw, dwa
