"""Cases, seeded inputs, references, error bounds and mutant references of the edge-shape tests of the oldest entry points
(test_edge_kernel_cases_cpu.py checks the premises, test_edge_kernels_gpu.py runs the kernels): kws_rmsprop_step,
kws_sgd_momentum_step, kws_l2_loss (csrc/optim.hip), kws_augment_f32/_i16, kws_tta_transform, kws_tta_combine, kws_head32to12
(csrc/augment.hip), kws_transpose_f32 (csrc/gemm.hip) and kws_time_stretch_* (csrc/stretch.hip).  NumPy only.

Every bound below is derived from the roundings of the operation or taken from the project's existing bar, none is measured."""
import numpy as np

from oracle import layers as OL
from oracle import stretch as OS

U = 2.0 ** -24          # unit roundoff of float32


def f64(a):
    return np.asarray(a, dtype=np.float64)


def ratio(got, ref, bound):
    """largest |got - ref| / bound; an element whose bound is 0 must be met exactly (inf otherwise)"""
    err = np.abs(f64(got) - ref)
    with np.errstate(divide='ignore', invalid='ignore'):
        r = np.where(bound > 0, err / np.where(bound > 0, bound, 1.0), np.where(err == 0, 0.0, np.inf))
    return float(r.max())


def outside(got, ref, bound):
    """elements of got that lie outside ref +- bound (NaN counts as outside)"""
    return ~(np.abs(f64(got) - ref) <= bound)


# ------------------------------------------------------------------------------------------------------------------------------
# 1. RMSprop / SGD with momentum: one-step comparisons on the update
# ------------------------------------------------------------------------------------------------------------------------------
OPT_N = [1, 2, 3, 4, 5, 8, 1023, 1024, 1025, 100003]        # float4 body only, tail only, both; one workgroup and many
GRAD_SCALES = [1.0, 0.125]
OPT_STEPS = 5
MUTANT_N, MUTANT_MIN = 100003, 1000
# the kernels' constants are float32: the float64 rule is given their float32 values (tests/test_adam_gpu.py does so with its betas)
LR_RMS, RHO, EPS = float(np.float32(1e-3)), float(np.float32(0.9)), float(np.float32(1e-8))
LR_SGD, MOM = float(np.float32(1e-2)), float(np.float32(0.9))
ORDINARY, TINY, DEAD, SMALL = 0, 1, 2, 3
RMS_MUTANTS = ['eps_in_root', 'no_one_minus_rho', 'no_l2', 'l2_factor_1', 'no_grad_scale']
SGD_MUTANTS = ['plus_lr_g', 'nesterov', 'no_l2', 'l2_factor_1', 'no_grad_scale']


def opt_inputs(n):
    """p, state (RMSprop accumulator / SGD velocity), l2 and OPT_STEPS gradients of n elements in four regimes, drawn per element:
    ORDINARY g ~ 1e-2 randn, acc ~ 1e-4 rand, l2 in {0, 1e-5};  TINY g ~ 1e-7 randn on a zero state (sqrt(a') ~ 3e-8, beside
    eps = 1e-8);  DEAD g = 0 on a zero state (0 / (0 + eps): p' == p, state stays 0);  SMALL p ~ 5e-4 randn.  l2 = 0 outside
    ORDINARY, so the L2 term never cancels the gradient.  The first elements are DEAD, TINY, ORDINARY, SMALL: n = 1 is the dead
    element, n = 3 has no float4 body, n = 4 is one float4 holding all four regimes."""
    rng = np.random.RandomState(7000 + n)
    regime = rng.randint(0, 4, n)
    head = [DEAD, TINY, ORDINARY, SMALL]
    regime[:min(n, 4)] = head[:min(n, 4)]
    zero_state = (regime == TINY) | (regime == DEAD)
    p = rng.randn(n)
    p = np.where(regime == SMALL, 5e-4 * rng.randn(n), p)
    acc = np.where(zero_state, 0.0, 1e-4 * rng.rand(n))
    vel = np.where(zero_state, 0.0, 1e-3 * rng.randn(n))
    l2 = np.where((rng.rand(n) < 0.5) & (regime == ORDINARY), 1e-5, 0.0)
    grads = []
    for _ in range(OPT_STEPS):
        g = 1e-2 * rng.randn(n)
        g = np.where(regime == TINY, 1e-7 * rng.randn(n), g)
        grads.append(np.where(regime == DEAD, 0.0, g).astype(np.float32))
    return dict(regime=regime, p=p.astype(np.float32), acc=acc.astype(np.float32), vel=vel.astype(np.float32),
                l2=l2.astype(np.float32), grads=grads)


def g_eff(p, grad, l2, gs, mutant=None):
    factor = {'no_l2': 0.0, 'l2_factor_1': 1.0}.get(mutant, 2.0)
    return f64(grad) * (1.0 if mutant == 'no_grad_scale' else gs) + factor * f64(l2) * f64(p)


def rmsprop_ref(p, grad, acc, l2, gs, mutant=None):
    """(p', a') of the float64 Keras rule (oracle.layers.rmsprop_step) from the float32 state it is handed"""
    p, acc = f64(p), f64(acc)
    g = g_eff(p, grad, l2, gs, mutant)
    p2, a2 = OL.rmsprop_step(p, g, acc, LR_RMS, RHO, EPS)
    if mutant == 'no_one_minus_rho':
        a2 = RHO * acc + g * g
        p2 = p - LR_RMS * g / (np.sqrt(a2) + EPS)
    elif mutant == 'eps_in_root':
        p2 = p - LR_RMS * g / np.sqrt(a2 + EPS)
    return p2, a2


def rmsprop_bounds(p, p2, a2):
    """At most 8 float32 roundings lie on the update lr g / (sqrt(a') + eps) (g: 1 with the fused multiply-add, counted twice in
    g^2; two products and a sum in a', halved by the root; root, sum, product, quotient): below 2e-6 of it; the final subtraction
    rounds p' once.  a': the roundings of g (twice), two products, rho a and the sum: 4 on either term (+ the smallest denormal)."""
    return U * np.abs(p2) + 2e-6 * np.abs(p2 - f64(p)), 4 * U * a2 + 1.5e-45


def sgd_ref(p, grad, vel, l2, gs, mutant=None):
    """(p', v', g_eff) of the float64 Keras rule (oracle.layers.sgd_momentum_step)"""
    p, vel = f64(p), f64(vel)
    g = g_eff(p, grad, l2, gs, mutant)
    p2, v2 = OL.sgd_momentum_step(p, g, vel, LR_SGD, MOM)
    if mutant == 'plus_lr_g':
        v2 = MOM * vel + LR_SGD * g
        p2 = p + v2
    elif mutant == 'nesterov':
        p2 = p + MOM * v2 - LR_SGD * g
    return p2, v2, g


def sgd_bounds(p2, vel, g):
    """v' = mom v - lr g: g rounds once (grad * gs is exact for gs a power of two, the multiply-add fused), lr g once more, mom v
    once, the difference once: 3 x 2^-24 on the two terms' magnitudes covers them.  p' = p + v' rounds once."""
    bv = 3 * U * (np.abs(MOM * f64(vel)) + np.abs(LR_SGD * g))
    return U * np.abs(p2) + bv, bv


def rmsprop_f32(p, grad, acc, l2, gs):
    """the rule in float32 NumPy, operation for operation as csrc/optim.hip writes it (without the fused multiply-add)"""
    f = np.float32
    g = f(2.0) * l2 * p + grad * f(gs)
    a = f(RHO) * acc + (f(1.0) - f(RHO)) * g * g
    return p - f(LR_RMS) * g / (np.sqrt(np.maximum(a, f(0.0))) + f(EPS)), a


def sgd_f32(p, grad, vel, l2, gs):
    f = np.float32
    g = f(2.0) * l2 * p + grad * f(gs)
    v = f(MOM) * vel - f(LR_SGD) * g
    return p + v, v


def judge_step(kind, before, after, grad, l2, gs, mutant=None):
    """One step of `kind` ('rmsprop' | 'sgd') judged against the float64 rule applied to the float32 state `before` = (p, s):
    returns (largest error/bound ratio of p', of the state, elements outside either bound)."""
    p, s = before
    if kind == 'rmsprop':
        p2, s2 = rmsprop_ref(p, grad, s, l2, gs, mutant)
        bp, bs = rmsprop_bounds(p, p2, s2)
    else:
        p2, s2, g = sgd_ref(p, grad, s, l2, gs, mutant)
        bp, bs = sgd_bounds(p2, s, g)
    bad = outside(after[0], p2, bp) | outside(after[1], s2, bs)
    return ratio(after[0], p2, bp), ratio(after[1], s2, bs), int(bad.sum())


def mutants_of(kind, gs):
    names = RMS_MUTANTS if kind == 'rmsprop' else SGD_MUTANTS
    return [m for m in names if not (m == 'no_grad_scale' and gs == 1.0)]       # (ignoring a scale of 1 is no mutation)


# ------------------------------------------------------------------------------------------------------------------------------
# 2. kws_l2_loss
# ------------------------------------------------------------------------------------------------------------------------------
L2_N = [1, 3, 4, 5, 4095, 4096, 4097, 100003]     # remainder loop only, float4 loop only, both; 4096 = one float4 per thread


def l2_inputs(n):
    rng = np.random.RandomState(8000 + n)
    p = rng.randn(n).astype(np.float32)
    l2 = np.where(rng.rand(n) < 0.5, 1e-5, 0.0).astype(np.float32)
    p[-1], l2[-1] = 1.5, 1e-5                       # the last element counts: the control drops it
    return p, l2


def l2_ref(p, l2):
    return float(np.sum(f64(l2) * f64(p) ** 2))


def l2_bound(ref):
    """double accumulation (relative error about n x 2^-53 = 1e-11 here): only the final cast to float32 rounds"""
    return U * abs(ref) * (1 + 1e-3)


# ------------------------------------------------------------------------------------------------------------------------------
# 3. kws_augment_f32 / _i16
# ------------------------------------------------------------------------------------------------------------------------------
AUG_L = [1, 3, 4, 5, 7, 8, 1021, 1024, 4099]
AUG_VARIANTS = ['noise', 'no_noise', 'short_noise']
AUG_BIG_B = 65538                                   # rows 65535.. go out in a second launch


def augment_ref(bank_f, idx, fg, shift, noise, noise_len, off, bgv, reverse_roll=False):
    """out[b,t] = f32(noise[off_b + t] * bgv_b) + f32(bank[idx_b][(t - shift_b) mod L] * fg_b) in float32, the operation order
    of oracle/features.py:augment (multiply, roll, multiply, add), whole batch at once.  A noise sample outside [0, noise_len)
    is 0, which oracle.features.augment_batch (a slice of the recording) cannot express.  reverse_roll: the control."""
    B, L = len(idx), bank_f.shape[1]
    t = np.arange(L, dtype=np.int64)[None, :]
    s = np.asarray(shift, dtype=np.int64)[:, None]
    src = (t + s) % L if reverse_roll else (t - s) % L
    f = bank_f[np.asarray(idx, dtype=np.int64)[:, None], src] * np.asarray(fg, np.float32)[:, None]
    if noise is None:
        return np.float32(0.0) + f
    o = np.asarray(off, dtype=np.int64)[:, None] + t
    valid = (o >= 0) & (o < noise_len)
    seg = np.where(valid, noise[np.clip(o, 0, noise_len - 1)], np.float32(0.0))
    out = seg * np.asarray(bgv, np.float32)[:, None] + f
    assert out.dtype == np.float32 and out.shape == (B, L)
    return out


def bank_as_f32(bank):
    """DecodeWav: int16 / 32768, exact in float32"""
    return bank if bank.dtype == np.float32 else bank.astype(np.float32) / np.float32(32768.0)


def _bank(rng, n_clips, L, bank_dtype):
    if bank_dtype == 'f32':
        return (rng.randn(n_clips, L) * 0.08).astype(np.float32)
    bank = rng.randint(-32768, 32768, size=(n_clips, L)).astype(np.int16)
    bank[0, 0], bank[1, L - 1] = -32768, 32767
    return bank


def augment_case(L, bank_dtype, variant):
    """11 rows: every shift of {0, 1, -1, 2, 3, L-1, L, L+1, -L, -(2L+3), 5L+2}; noise offsets 0, an interior odd one, the exact
    fit noise_len - L, two past it (runs off the end), noise_len - 1, noise_len + 5 (wholly outside), -3, -L-1; fg 0, negative,
    1; bg_vol 0 and positive.  'no_noise': noise NULL, every bg_vol 0.  'short_noise': noise_len < L (None at L = 1)."""
    if variant == 'short_noise' and L < 3:
        return None
    rng = np.random.RandomState(9000 + 7 * L + (bank_dtype == 'i16') + 3 * AUG_VARIANTS.index(variant))
    n_clips, B = 5, 11
    bank = _bank(rng, n_clips, L, bank_dtype)
    idx = (np.arange(B) % n_clips).astype(np.int32)
    shift = np.array([0, 1, -1, 2, 3, L - 1, L, L + 1, -L, -(2 * L + 3), 5 * L + 2], dtype=np.int32)
    fg = (1 + rng.uniform(-0.15, 0.15, B)).astype(np.float32)
    fg[1], fg[2], fg[3] = 0.0, -fg[2], 1.0
    bgv = rng.uniform(0.01, 0.15, B).astype(np.float32)
    if variant == 'noise':
        nl = 2 * L + 37
        off = np.array([0, 3, nl - L, nl - L + 2, nl - 1, nl + 5, -3, -L - 1, 3, nl - L, -3], dtype=np.int64)
        bgv[8], bgv[10] = 0.0, 0.0
    elif variant == 'short_noise':
        nl = L // 2
        off = np.array([0, 1, -1, -3, nl - 1, nl, L, -L, 0, 2, -2], dtype=np.int64)
        bgv[8] = 0.0
    else:
        nl, off = 0, None
        bgv[:] = 0.0
    noise = (rng.randn(nl) * 0.3).astype(np.float32) if nl else None
    return dict(bank=bank, n_clips=n_clips, L=L, B=B, idx=idx, fg=fg, shift=shift, noise=noise, noise_len=nl, off=off, bgv=bgv)


def augment_big_case(bank_dtype):
    """B = 65538 rows of L = 8: the second launch of the grid.y loop, with its offset pointers"""
    rng = np.random.RandomState(9900 + (bank_dtype == 'i16'))
    n_clips, L, B, nl = 7, 8, AUG_BIG_B, 1000
    bank = _bank(rng, n_clips, L, bank_dtype)
    r = np.arange(B)
    idx = ((r * 3) % n_clips).astype(np.int32)
    shift = (r % 19 - 9).astype(np.int32)
    off = ((r * 7) % (nl + 20) - 10).astype(np.int64)
    fg = (1 + rng.uniform(-0.15, 0.15, B)).astype(np.float32)
    bgv = np.where(r % 5 == 0, 0.0, rng.uniform(0.01, 0.15, B)).astype(np.float32)
    noise = (rng.randn(nl) * 0.3).astype(np.float32)
    return dict(bank=bank, n_clips=n_clips, L=L, B=B, idx=idx, fg=fg, shift=shift, noise=noise, noise_len=nl, off=off, bgv=bgv)


def augment_case_ref(c, reverse_roll=False):
    return augment_ref(bank_as_f32(c['bank']), c['idx'], c['fg'], c['shift'], c['noise'], c['noise_len'], c['off'], c['bgv'],
                       reverse_roll)


# ------------------------------------------------------------------------------------------------------------------------------
# 4. kws_tta_transform, kws_tta_combine, kws_head32to12
# ------------------------------------------------------------------------------------------------------------------------------
TTA_L = [1, 2, 255, 256, 257, 1499, 1500, 1501, 16000]       # the roll of 1500 wraps more than once, exactly once, not at all
TTA_KINDS = [0, 1, 2, 3, 4]
TTA_BIG = (65538, 8, [1, 3])


def tta_specials():
    """+-1/1.1 (where kind 3's clip sets in) with the floats either side of it, +-1, +-2, +-0"""
    c = np.float32(1.0 / 1.1)
    lo, hi = np.nextafter(c, np.float32(0)), np.nextafter(c, np.float32(2))
    return np.array([c, lo, hi, -c, -lo, -hi, 1, -1, 2, -2, 0.0, -0.0], dtype=np.float32)


def tta_input(B, L):
    rng = np.random.RandomState(10000 + L)
    x = rng.randn(B, L).astype(np.float32)
    sp = np.roll(tta_specials(), -L)                  # (the shortest inputs hold a few of them each: a different few)
    k = min(x.size, len(sp))
    x.reshape(-1)[:k] = sp[:k]
    return x


COMBINE_TERMS = [(1, 1.0), (2, 2.0), (3, 3.0), (6, 10.0), (8, 8.0)]     # (6, 10): make_submission.py:137-140
COMBINE_B = [1, 256, 257]
COMBINE_C = [1, 12, 32]


def combine_case(n_terms, B, C):
    """terms [n_terms][B, C]; with C >= 2 row 0 holds its largest value twice (columns j0 < j1, j0 > 0 where C allows), so the
    argmax is the first of a tie; the last row is negative throughout (B = 1: row 0 is both).  Returns (terms, tie or None)."""
    rng = np.random.RandomState(11000 + 100 * n_terms + 10 * B + C)
    terms = [(rng.rand(B, C) / C).astype(np.float32) for _ in range(n_terms)]
    for t in terms:
        t[B - 1] = -(t[B - 1] + np.float32(0.5))
    tie = None
    if C >= 2:
        j0, j1 = (1, C - 1) if C >= 3 else (0, 1)
        top = np.float32(-0.125) if B == 1 else np.float32(2.0)
        for t in terms:
            t[0, j0] = t[0, j1] = top
        tie = (j0, j1)
    return terms, tie


def combine_ref(terms, divisor):
    """((p0 + p1) + p2) + ... in float32, then one float32 division"""
    s = terms[0].copy()
    for t in terms[1:]:
        s = s + t
    s = s / np.float32(divisor)
    assert s.dtype == np.float32
    return s, np.argmax(s, axis=1).astype(np.int32)


ALL_CLASSES = ('sheila nine stop bed four six down bird marvin cat off right seven eight up three happy go zero on wow dog yes '
               'five one tree house two left no').split()
WANTED = 'stop down off right up go on yes left no'.split()


def real_head_map():
    """freeze_graph_32_classes.py:55-69: silence, unknown (the maximum over every unwanted word), the wanted words in order"""
    mp = np.zeros(32, np.int32)
    mp[0], mp[1] = 0, 1
    slot = 2
    for i, c in enumerate(ALL_CLASSES):
        if c in WANTED:
            mp[i + 2] = slot
            slot += 1
        else:
            mp[i + 2] = 1
    return mp


# name -> (C_in, C_out, map): the real head; the widest output the kernel takes; a map that leaves slot 3 without an input
# (probability exactly 0) and carries the entries -1 and C_out, which are ignored
HEAD_CASES = {
    'real': (32, 12, real_head_map()),
    'identity64': (64, 64, np.arange(64, dtype=np.int32)),
    'unmapped': (10, 6, np.array([0, 1, 2, 4, 5, 1, 2, -1, 6, 0], dtype=np.int32)),
}
HEAD_B = [1, 257]
HEAD_RTOL = 1e-5            # the project's bar for this kernel (tests/test_kernels_gpu.py)


def head_input(name, B):
    C_in = HEAD_CASES[name][0]
    rng = np.random.RandomState(12000 + C_in + B)
    return OL.softmax(rng.randn(B, C_in) * 2).astype(np.float32)


def head_ref(p_in, mp, C_out, reduce='max'):
    """softmax over the slots' maxima in float64; a slot no input maps to holds -inf (probability 0).  reduce='sum': control."""
    p = f64(p_in)
    z = np.full((p.shape[0], C_out), -np.inf)
    for i, s in enumerate(mp):
        if 0 <= s < C_out:
            if reduce == 'max':
                z[:, s] = np.maximum(z[:, s], p[:, i])
            else:
                z[:, s] = np.where(np.isinf(z[:, s]), p[:, i], z[:, s] + p[:, i])
    return OL.softmax(z, axis=1)


# ------------------------------------------------------------------------------------------------------------------------------
# 5. kws_transpose_f32
# ------------------------------------------------------------------------------------------------------------------------------
TRANSPOSE_SHAPES = [(1, 1), (1, 33), (33, 1), (31, 65), (32, 32), (100, 40), (257, 3)]


# ------------------------------------------------------------------------------------------------------------------------------
# 6. kws_time_stretch_* at short clips
# ------------------------------------------------------------------------------------------------------------------------------
STRETCH_L = [1025, 1536, 2047, 2500]               # 1025: the shortest clip the reflect padding takes; 1025, 2047: odd
STRETCH_RATES = [0.5, 0.9, 1.0, 2.5, 7.0]
STRETCH_ATOL = 2e-5                                # the project's bar (tests/test_stretch_gpu.py)
LSB = 1.0 / 32768


def stretch_steps(L, rate):
    """T = number of vocoder steps = output frames"""
    return len(np.arange(0, 1 + L // OS.HOP, rate))


def stretch_pcm(L):
    """int16 [3, L]: white noise at 0.0774 clipped to +-1, the same behind 600 leading zeros, silence (no pure tone:
    tests/test_stretch_gpu.py says why)"""
    rng = np.random.RandomState(13000 + L)
    x = np.zeros((3, L))
    x[0] = (rng.randn(L) * 0.0774).clip(-1, 1)
    x[1] = x[0]
    x[1, :600] = 0.0
    return np.int16(x * 32767)


def stretch_float(pcm):
    """create_tta_set.py:18: np.float32(data) / 32767 - the floats the f32 entry point is fed (in_scale 1)"""
    return np.float32(pcm) / np.float32(32767)


def stretch_keeps(Ltrim):
    return [Ltrim, Ltrim + 37, max(1, Ltrim - 100)] if Ltrim > 0 else [64]


_STRETCH_REF = {}


def stretch_ref(L, rate):
    """float64 oracle.stretch.time_stretch of the three rows (computed once)"""
    if (L, rate) not in _STRETCH_REF:
        x = stretch_float(stretch_pcm(L))
        _STRETCH_REF[(L, rate)] = [OS.time_stretch(f64(x[b]), rate) for b in range(3)]
    return _STRETCH_REF[(L, rate)]


def stretch_want(ref, keep):
    """the last `keep` samples, zero padded at the end"""
    want = np.zeros(keep)
    tail = ref[len(ref) - min(keep, len(ref)):]
    want[:len(tail)] = tail
    return want


def stretch_want_quantized(want):
    """np.int16(data * 32767) (truncation) read back through DecodeWav's / 32768"""
    return np.int16(np.float32(want) * np.float32(32767)).astype(np.float32) / np.float32(32768.0)
