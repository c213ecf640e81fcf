"""Shared by tests/test_bn_cols_kernels_gpu.py and tests/test_bn_cols_cpu.py: layouts, inputs and float64 references for the
BatchNorm bookkeeping of csrc/bncols.hip (kws_gbn_finalize / _infer / _bwd / _bwd_finish).

Everything here is in the WINDOW's own shape - data [M, F], table [4, F] (scale | shift | mean | rstd), parameters [F] - and the
index helpers say where element (m, c) / table entry (r, c) / parameter c sits in the buffers the launchers see, for the two
layouts of kws_gbn_cols: g groups of Ng dense columns with tables bn[g][4][Ng], or the column window [c0, c0 + F) of a tensor of
row pitch `pitch` with the table bn[4][pitch].

The backward's inputs make its sums exact.  dA, y and add are integers in [-4, 4]; per column the table holds an integer mean in
[-2, 2], rstd in {0.5, 1, 2}, scale in {+-0.5, +-1, +-2} and an integer shift.  Then pre = fma(y, scale, shift) is a small multiple
of 0.5 (exactly 0 and exactly 6 occur), the gated gradient g is an integer, xhat = (y - mean) rstd and g xhat are multiples of
0.5 with |g xhat| <= 96, every 64-row float32 chunk sum stays far below 2^23 and the double sums over the chunks are exact: the
partial rows, dgamma, dbeta and coef = (float)(sum * (1.0 / M)) are the float64 reference cast to float32, bit for bit
(premise_bwd asserts the conditions from the reference; they are conditions of the test, not tolerances)."""
import numpy as np

U = 2.0 ** -24           # float32 unit roundoff
CHUNK = 64               # GBWD_ROWS of bncols.hip
BN_EPS = np.float32(1e-3)
BN_MOMENTUM = np.float32(0.99)
SENT = 0x7FC0DEAD        # the poison of test_resblock_kernels_gpu.Guarded

LAYOUTS = {
    # F = 60 is no multiple of the reduction's 16 columns; M = 17 chunks + 5 rows: more chunks than its 16 row groups, short last one
    "grouped": dict(g=3, Ng=20, pitch=60, c0=0, M=1093),
    "window": dict(g=1, Ng=20, pitch=72, c0=8, M=1093),
    # F > 256: a second blockIdx.y in pass 1; 64 + 6 rows
    "wide_window": dict(g=1, Ng=260, pitch=272, c0=8, M=70),
    # g = 1 dense = the window (pitch 20, first column 0): fed "window"'s own columns, it must give "window"'s bits
    "plain": dict(g=1, Ng=20, pitch=20, c0=0, M=1093),
}
FIN_ROWS = [1, 16, 17, 40]     # statistics rows: one, exactly the 16 row groups, one more, several rounds
MUTATIONS = ["add_before_gate", "gate_open_at_zero", "short_chunk_dropped"]


def f64(a):
    return np.asarray(a, dtype=np.float64)


def width(lay):
    return lay["g"] * lay["Ng"]


def is_window(lay):
    return lay["pitch"] != width(lay) or lay["c0"] != 0


def data_idx(lay):
    """[M, F]: float index of element (m, c) in a data buffer of M * pitch floats"""
    return np.arange(lay["M"])[:, None] * lay["pitch"] + lay["c0"] + np.arange(width(lay))[None, :]


def table_size(lay):
    return 4 * lay["pitch"]


def table_idx(lay):
    """[4, F]: float index of table row r (scale | shift | mean | rstd) of column c"""
    c = np.arange(width(lay))
    grp, n = c // lay["Ng"], c % lay["Ng"]
    stride = lay["pitch"] if is_window(lay) else lay["Ng"]
    return grp[None, :] * 4 * lay["Ng"] + lay["c0"] + n[None, :] + np.arange(4)[:, None] * stride


def refs_layout(lay):
    """Where the per-column parameters sit in a flat buffer (gamma | beta of the parameters and gradients, moving mean | variance
    of the state): dict(size, base, pstride, boff, first[F], second[F]).  Grouped: group q at q * pstride with pstride > 2 Ng and
    the second tensor boff > Ng behind the first, so that both gaps exist; one layer: neighbours in front, between and behind."""
    F, Ng = width(lay), lay["Ng"]
    c = np.arange(F)
    if lay["g"] > 1:
        base, pstride, boff = 0, 2 * Ng + 7, Ng + 3
        size = lay["g"] * pstride
    else:
        base, pstride, boff = 5, 0, F + 6
        size = 5 + F + 6 + F + 5
    first = base + (c // Ng) * pstride + c % Ng
    return dict(size=size, base=base, pstride=pstride, boff=boff, first=first, second=first + boff)


# ---------------------------------------------------------------------------------------------------------------------------
# backward
# ---------------------------------------------------------------------------------------------------------------------------
def bwd_inputs(name):
    """dA, y, add [M, F] and table [4, F], float32"""
    if name == "plain":
        return bwd_inputs("window")
    lay = LAYOUTS[name]
    M, F = lay["M"], width(lay)
    rng = np.random.RandomState(100 + M + F)
    ints = lambda *shape: rng.randint(-4, 5, size=shape).astype(np.float32)   # noqa: E731
    scale = rng.choice([0.5, 1.0, 2.0], size=F) * np.where(np.arange(F) % 3 == 1, -1.0, 1.0)
    table = np.stack([scale, rng.randint(-1, 5, size=F), rng.randint(-2, 3, size=F), rng.choice([0.5, 1.0, 2.0], size=F)])
    return dict(dA=ints(M, F), y=ints(M, F), add=ints(M, F), table=table.astype(np.float32))


def bwd_ref(inp, with_add, mutate=None):
    """float64 reference of the three passes: g (gated, + add behind the gate), part [rows, 2, F], dgamma, dbeta, coef [2, F],
    dy and its bar.  mutate: one of MUTATIONS, a reference that is wrong on purpose."""
    dA, y, add = f64(inp["dA"]), f64(inp["y"]), f64(inp["add"])
    sc, sh, mean, rstd = f64(inp["table"])
    M, F = dA.shape
    pre = y * sc + sh
    gate = (pre >= 0) & (pre <= 6) if mutate == "gate_open_at_zero" else (pre > 0) & (pre <= 6)
    if with_add and mutate == "add_before_gate":
        g = np.where(gate, dA + add, 0.0)
    else:
        g = np.where(gate, dA, 0.0) + (add if with_add else 0.0)
    xhat = (y - mean) * rstd
    rows = -(-M // CHUNK)
    part = np.zeros((rows, 2, F))
    for t in range(rows):
        sl = slice(t * CHUNK, min((t + 1) * CHUNK, M))
        part[t, 0] = g[sl].sum(axis=0)
        part[t, 1] = (g * xhat)[sl].sum(axis=0)
    if mutate == "short_chunk_dropped" and M % CHUNK:
        part[-1] = 0.0
    s, sx = part[:, 0].sum(axis=0), part[:, 1].sum(axis=0)
    inv = 1.0 / M                                                  # the device's double steps: s * (1.0 / M), then the cast
    coef = np.stack([s * inv, sx * inv]).astype(np.float32).astype(np.float64)
    # pass 3 in float32: a = g - c1 rounds once (U |a|); (y - mean) rstd is exact here; its product with c2 and the subtraction
    # from a round once each, or once together when the compiler fuses them; the product with scale rounds once.  To first order
    # the error is below |scale| (U |a| + U |p| + U |a - p|) + U |dy| <= 3 U |scale| (|g| + |c1| + |p|); 4 U covers the rest
    p = xhat * coef[1]
    dy = sc * (g - coef[0] - p)
    dy_bar = 4 * U * np.abs(sc) * (np.abs(g) + np.abs(coef[0]) + np.abs(p))
    return dict(pre=pre, g=g, xhat=xhat, part=part, dgamma=sx, dbeta=s, coef=coef, dy=dy, dy_bar=dy_bar)


def premise_bwd(inp, ref):
    """The conditions under which the float32 device sums equal the float64 reference: every term a multiple of 0.5, every chunk's
    sum of magnitudes below 2^22 (then every partial sum in any order is a float32 value), pre exact; and the gate's two edges are
    both met by elements whose gradient is not 0.  Returns (elements at pre == 0, at pre == 6)."""
    terms = ref["g"] * ref["xhat"]
    assert np.array_equal(ref["g"], np.rint(ref["g"])) and np.array_equal(2 * terms, np.rint(2 * terms))
    assert np.array_equal(2 * ref["pre"], np.rint(2 * ref["pre"])) and np.abs(ref["pre"]).max() < 64
    M = terms.shape[0]
    for t in range(-(-M // CHUNK)):
        sl = slice(t * CHUNK, (t + 1) * CHUNK)
        assert np.abs(terms[sl]).sum(axis=0).max() < 2 ** 22 and np.abs(ref["g"][sl]).sum(axis=0).max() < 2 ** 22
    for k in ("part", "dgamma", "dbeta"):
        assert np.array_equal(ref[k], ref[k].astype(np.float32).astype(np.float64)), k
    live = f64(inp["dA"]) != 0
    return int(((ref["pre"] == 0) & live).sum()), int(((ref["pre"] == 6) & live).sum())


EXACT_OUTPUTS = ("part", "dgamma", "dbeta", "coef")


def differs_exactly(a, b):
    """two references differ in at least one of the outputs the device is held to bit for bit"""
    return any(not np.array_equal(a[k].astype(np.float32), b[k].astype(np.float32)) for k in EXACT_OUTPUTS)


# ---------------------------------------------------------------------------------------------------------------------------
# forward tables
# ---------------------------------------------------------------------------------------------------------------------------
def params_inputs(F, seed):
    """gamma (both signs), beta, moving mean, moving variance [F], float32"""
    rng = np.random.RandomState(seed)
    gamma = (1.0 + 0.1 * rng.randn(F)) * np.where(rng.rand(F) < 0.3, -1.0, 1.0)
    return dict(gamma=gamma.astype(np.float32), beta=(0.1 * rng.randn(F)).astype(np.float32),
                mm=(0.05 * rng.randn(F)).astype(np.float32), mv=(1.0 + 0.2 * rng.rand(F)).astype(np.float32))


ROWS_PER_STAT = 5


def fin_inputs(name, rows):
    """statistics rows part [rows, 2, F] = (sum x, sum x^2) over ROWS_PER_STAT rows each of an integer matrix in [-4, 4] (so that
    every sum is a small integer: exact in float32 and in the double reduction), the count, and the layer's parameters / state"""
    lay = LAYOUTS[name]
    F = width(lay)
    rng = np.random.RandomState(7 * rows + F)
    x = rng.randint(-4, 5, size=(rows, ROWS_PER_STAT, F)).astype(np.float64)
    part = np.stack([x.sum(axis=1), (x * x).sum(axis=1)], axis=1)
    out = params_inputs(F, 11 * rows + F)
    out.update(part=part.astype(np.float32), count=rows * ROWS_PER_STAT)
    return out


def fin_ref(inp):
    """float64 reference of gbn_finalize_kernel doing its double steps (mean = s * (1.0 / count), var = ss * inv - mean^2 clamped
    at 0, rstd = 1 / sqrt(var + (double)eps)), then its float32 steps in float64.  Returns (values, bars), each a dict over
    scale | shift | mean | rstd | mm | mv.  The double steps differ from the device's at most in a fused multiply-add: 2^-52 ss / n
    of var, absolutely, which eps = 1e-3 keeps at 1e-11 of rstd (tests/test_bn_cols_cpu.py asserts it); besides that a cast to
    float32 may land one ulp = 2 U |x| apart; the float32 steps are bounded operation by operation."""
    s, ss = f64(inp["part"])[:, 0].sum(axis=0), f64(inp["part"])[:, 1].sum(axis=0)
    inv = 1.0 / inp["count"]
    mean = s * inv
    var = np.maximum(ss * inv - mean * mean, 0.0)
    rstd = 1.0 / np.sqrt(var + float(BN_EPS))
    gamma, beta, mm, mv = (f64(inp[k]) for k in ("gamma", "beta", "mm", "mv"))
    omm = float(np.float32(1.0 - float(BN_MOMENTUM)))
    scale = gamma * rstd
    val = dict(mean=mean, rstd=rstd, scale=scale, shift=beta - mean * scale, mm=mm - (mm - mean) * omm, mv=mv - (mv - var) * omm)
    bar = dict(
        mean=2 * U * np.abs(mean),                                    # one cast
        rstd=2 * U * np.abs(rstd),                                    # one cast
        scale=4 * U * np.abs(scale),                                  # rstd's ulp (2 U) and the product's rounding (U); 4 U with margin
        # beta - meanf * scale: the final rounding (U |shift|) and, relative to |mean scale|, mean's ulp (2 U), scale's error
        # (3 U) and the product's rounding (U, none when fused)
        shift=U * np.abs(val["shift"]) + 8 * U * np.abs(mean * scale),
        # x - (x - m) * omm with omm = 0.01: the difference rounds (U (|x| + |m|)) and carries m's ulp (2 U |m|), both times 0.01;
        # the product and the final subtraction round once each (U |x| (1 + ...)): below 2 U (|x| + |m|), 3 U with margin
        mm=3 * U * (np.abs(mm) + np.abs(mean)),
        mv=3 * U * (np.abs(mv) + np.abs(var)))
    return val, bar


def infer_ref(inp):
    """float64 reference of gbn_infer_kernel, all float32 steps: rstd = 1.0f / sqrtf(mv + eps) - the sum rounds (U, halved by the
    root), the correctly rounded root and quotient round once each: 2.5 U |rstd|, 3 U with margin; scale = gamma * rstd one more
    (4 U); shift = beta - mm * scale: the final rounding and, relative to |mm scale|, scale's 4 U and the product's U (6 U with
    margin); the mean entry is the moving mean itself."""
    gamma, beta, mm, mv = (f64(inp[k]) for k in ("gamma", "beta", "mm", "mv"))
    rstd = 1.0 / np.sqrt(mv + float(BN_EPS))
    scale = gamma * rstd
    val = dict(mean=mm, rstd=rstd, scale=scale, shift=beta - mm * scale)
    bar = dict(mean=np.zeros_like(mm), rstd=3 * U * np.abs(rstd), scale=4 * U * np.abs(scale),
               shift=U * np.abs(val["shift"]) + 6 * U * np.abs(mm * scale))
    return val, bar
