"""Cases, exact inputs and float64 references of the direct tests of the 3-tap depthwise chain (csrc/dwconv.hip,
csrc/dw_bwd_body.h) and of the folds of csrc/bn.hip (kws_dw_bwd_finalize, kws_bn_stats_finalize, kws_dw_grad_finalize_batch,
kws_bn_infer_prepare[_batch]); tests/test_dw3_cpu.py checks this module without a GPU, tests/test_dw3_kernels_gpu.py runs the
kernels against it.

The method is that of tests/gemm_exact.py: inputs chosen so that float32 cannot round.  y is integers in [-4, 4], w in [-2, 2],
dz in [-3, 3]; per channel the BatchNorm table has scale in {1, 2, -1}, an integer shift in [-2, 3], mean in {-1, 0, 1} and rstd in
{0.5, 1, 2} (gamma = scale / rstd, so kws_bn_bwd_apply's gamma * rstd is pass 2's scale); the pass-2 coefficients are multiples of
1/4 in [-2, 2].  The activation, g, xhat, the five column sums and dy are then short dyadic numbers: every product and every
partial sum is a float32 value whatever the order of the additions and whether or not a product and a sum were contracted to an
fma, so each output must EQUAL the float64 reference built from oracle/layers.py (gemm_exact.same_bits: as numbers - the sign of
a zero, which depends on which operand of an exact cancellation was negative, is the one thing not compared with the reference;
it is compared between the kernels, whose outputs must agree bit for bit).  premise() asserts what the argument needs: the sum of
magnitudes of every reduced column is below 2^22 (the terms are multiples of 1/2).

The BatchNorm pre-activation y * scale + shift is an integer in [-10, 11] that equals 0 for 9.3 % and 6 for 4.3 % of the elements
(counted over the draws above: 1/9, 1/9, 1/18 and 1/27, 1/27, 1/18 for the three scales), which is where the kernels' ReLU6
gradient rule - pre > 0 && pre <= 6, oracle.layers.relu6_mask - differs from its neighbours; mask="exclusive" is the wrong rule
(pre < 6) of the host-side control.

bwd_geom / fwd_threads / pre_reduce_plan restate the launch geometry of the sources; every case is tagged with the corners of it
that it is in the table for, and corners_of() says which a case reaches."""
import functools

import numpy as np

from oracle import layers as OL

# csrc/dw_bwd_body.h, csrc/dwconv.hip, csrc/bn.hip, include/kws_hip.h
TT = 8                    # KWS_DW_TT: positions per thread (and DW_BWD_HT: positions per batch of loads)
BWD_THREADS = 512         # DW_BWD_THREADS = DW_BWD2_THREADS
BWD_PARTS = 256           # DW_BWD_PARTS: workgroups (= partial rows) of the row-writing modes at most
BWD2_GRID = 1024          # pass 2's cap
FWD_GRID = 4096           # DW_FWD_GRID workgroups of 256 threads
REDUCE_SLICES = 32        # KWS_REDUCE_SLICES
PRE_REDUCE_MIN = 256      # KWS_PRE_REDUCE_MIN: more partial rows than this, and a scratch buffer, take slice_reduce_kernel
FIN_BATCH = 16            # KWS_DW_FIN_BATCH = KWS_BN_INFER_BATCH
ABSMAX_SLOTS, ABSMAX_STRIDE = 16, 16
LIMIT = 2.0 ** 22


def cdiv(a, b):
    return -(-a // b)


def bwd_geom(B, Lin, C, parts=True):
    """kws_dw::bwd_geom: channel slices ny of Cb channels, R (clip, chunk) units per workgroup of `block` threads, `grid`
    workgroups in x, `groups` unit groups for them to stride over"""
    ny = cdiv(C // 4, 256)
    Cb = C // ny
    C4 = Cb // 4
    nchunks = cdiv(Lin, TT)
    R = max(BWD_THREADS // C4, 1)
    groups = cdiv(B * nchunks, R)
    return dict(ny=ny, Cb=Cb, nchunks=nchunks, R=R, block=R * C4, groups=groups,
                grid=min(groups, BWD_PARTS if parts else BWD2_GRID))


def bwd_geom_ok(C):
    return C > 0 and C % 4 == 0 and (C // 4) % cdiv(C // 4, 256) == 0


def part_floats(B, Lin, C):
    """kws_dwconv_bwd_part_floats"""
    return bwd_geom(B, Lin, C)["grid"] * 5 * C


def fwd_threads(B, Lout, C):
    """dwconv_fwd_kernel: one thread per (clip, chunk of TT outputs, channel quad); the grid it is given"""
    n = B * cdiv(Lout, TT) * (C // 4)
    return n, min(cdiv(n, 256), FWD_GRID)


def pre_reduce_plan(n, scratch):
    """bn.hip pre_reduce: None = the finalise kernel sums the n rows itself; else (rows_per, S) of slice_reduce_kernel"""
    if not scratch or n <= PRE_REDUCE_MIN:
        return None
    rows_per = cdiv(n, REDUCE_SLICES)
    return rows_per, cdiv(n, rows_per)


# (B, L_in, C, stride, pad_l, L_out, forward only, the corners the case is in the table for)
CASES = [
    (2, 1, 4, 1, 1, 1, False, {"one_position", "idle_units", "R512"}),
    (2, 1, 4, 2, 1, 1, False, {"one_position", "idle_units", "stride2"}),
    (3, 7, 64, 1, 1, 7, False, {"below_load_batch", "same_s1"}),
    (3, 8, 320, 2, 0, 4, False, {"exact_load_batch", "s2_pad0", "block480"}),
    (2, 9, 64, 2, 1, 5, False, {"above_load_batch", "s2_pad1"}),
    (3, 17, 1000, 1, 0, 15, False, {"partial_wave", "valid_s1"}),
    (2, 11, 1536, 2, 1, 6, False, {"two_slices", "Cb768"}),
    (2, 10, 2048, 1, 1, 10, False, {"two_slices", "Cb1024"}),
    (3, 12, 128, 2, 0, 5, False, {"uncovered_rows"}),
    (820, 33, 512, 2, 1, 17, False, {"rows_stride", "pass2_stride"}),
    (1040, 3, 4096, 1, 1, 3, True, {"fwd_stride"}),
    (1040, 3, 4096, 2, 1, 2, True, {"fwd_stride", "stride2"}),
]
CORNERS = {"one_position", "idle_units", "R512", "stride2", "below_load_batch", "exact_load_batch", "above_load_batch", "same_s1",
           "valid_s1", "s2_pad0", "s2_pad1", "block480", "partial_wave", "two_slices", "Cb768", "Cb1024", "uncovered_rows",
           "rows_stride", "pass2_stride", "fwd_stride"}
CASES = [c[:7] + (frozenset(c[7]),) for c in CASES]      # (hashable: inputs() and the references are cached per case)
BWD_CASES = [c for c in CASES if not c[6]]


def case_id(c):
    return "B%d-L%d-C%d-s%d-p%d-Lo%d" % c[:6]


def pad_of(c):
    """(pad_l, pad_r) that give the case's L_out windows; L_out itself is an argument of the kernels, not derived by them"""
    B, Lin, C, stride, pad_l, Lout = c[:6]
    pad_r = max(0, stride * (Lout - 1) + 3 - pad_l - Lin)
    assert OL.valid_len(Lin + pad_l + pad_r, 3, stride) == Lout
    return pad_l, pad_r


def corners_of(c):
    B, Lin, C, stride, pad_l, Lout, fwd_only = c[:7]
    got = set()
    g, g2 = bwd_geom(B, Lin, C), bwd_geom(B, Lin, C, parts=False)
    if Lin == 1 and Lout == 1:
        got.add("one_position")
    if g["groups"] * g["R"] > B * g["nchunks"]:
        got.add("idle_units")                                   # threads whose unit lies past the last clip (b >= B)
    if g["R"] == 512:
        got.add("R512")
    if stride == 2:
        got.add("stride2")
        got.add("s2_pad%d" % (pad_l & 1))
    got.add({7: "below_load_batch", 0: "exact_load_batch", 1: "above_load_batch"}.get(Lin % TT, "mid_load_batch"))
    if stride == 1:
        got.add("same_s1" if pad_l == 1 and Lout == Lin else "valid_s1" if pad_l == 0 and Lout == Lin - 2 else "other_s1")
    if g["block"] == 480:
        got.add("block480")
    if g["block"] % 64:
        got.add("partial_wave")
    if g["ny"] == 2:
        got |= {"two_slices", "Cb%d" % g["Cb"]}
    if stride * (Lout - 1) + 2 - pad_l < Lin - 1:
        got.add("uncovered_rows")                                # input rows at the end that no window covers
    if not fwd_only and g["groups"] > BWD_PARTS:
        got.add("rows_stride")
    if not fwd_only and g2["groups"] > BWD2_GRID:
        got.add("pass2_stride")
    n, grid = fwd_threads(B, Lout, C)
    if n > grid * 256:
        got.add("fwd_stride")
    return got


# ---------------------------------------------------------------------------------------------------------------------------
# inputs and references of the depthwise chain
# ---------------------------------------------------------------------------------------------------------------------------
def f64(a):
    return np.asarray(a, dtype=np.float64)


@functools.lru_cache(maxsize=2)
def inputs(c):
    """float32: y [B, L_in, C], w [3, C], dz [B, L_out, C], the table bn [4, C] = scale | shift | mean | rstd, gamma [C] and the
    hand-made pass-2 coefficients coef [2, C]"""
    B, Lin, C, stride, pad_l, Lout = c[:6]
    rng = np.random.RandomState(B * 7919 + Lin * 131 + C + stride)
    y = rng.randint(-4, 5, size=(B, Lin, C)).astype(np.float32)
    w = rng.randint(-2, 3, size=(3, C)).astype(np.float32)
    dz = rng.randint(-3, 4, size=(B, Lout, C)).astype(np.float32)
    bn = np.stack([np.array([1.0, 2.0, -1.0])[rng.randint(0, 3, size=C)], rng.randint(-2, 4, size=C),
                   rng.randint(-1, 2, size=C), np.array([0.5, 1.0, 2.0])[rng.randint(0, 3, size=C)]]).astype(np.float32)
    gamma = (bn[0] / bn[3]).astype(np.float32)
    coef = (rng.randint(-8, 9, size=(2, C)) / 4.0).astype(np.float32)
    for a in (y, w, dz, bn, gamma, coef):
        a.setflags(write=False)
    return dict(y=y, w=w, dz=dz, bn=bn, gamma=gamma, coef=coef)


def activation(inp, with_bn):
    """(pre, a) in float64; without a table the kernels read y itself (pre = None: no mask, xhat = 0)"""
    y = f64(inp["y"])
    if not with_bn:
        return None, y
    pre = y * f64(inp["bn"][0]) + f64(inp["bn"][1])
    return pre, OL.relu6(pre)


def fwd_ref(c, with_bn):
    """z in float64 (oracle.layers.dwconv_fwd over the activation) and the pre-activation"""
    inp = inputs(c)
    pre, a = activation(inp, with_bn)
    return OL.dwconv_fwd(a, f64(inp["w"]), c[3], pad_of(c)), pre


def fwd_ref_int(c, with_bn):
    """z of the two forward-only cases in int32 (every quantity is an integer): a tenth of the float64 reference's memory"""
    inp = inputs(c)
    stride, (pad_l, pad_r), Lout = c[3], pad_of(c), c[5]
    a = inp["y"].astype(np.int32)
    if with_bn:
        a = np.clip(a * inp["bn"][0].astype(np.int32) + inp["bn"][1].astype(np.int32), 0, 6)
    ap = np.pad(a, [[0, 0], [pad_l, pad_r], [0, 0]])
    w = inp["w"].astype(np.int32)
    z = np.zeros((c[0], Lout, c[2]), np.int32)
    for j in range(3):
        z += ap[:, j:j + stride * Lout:stride] * w[j]
    return z


def mask_of(pre, mask):
    if mask == "exclusive":                                      # the wrong rule of the control: pre == 6 loses its gradient
        return ((pre > 0) & (pre < 6)).astype(pre.dtype)
    return OL.relu6_mask(pre)


@functools.lru_cache(maxsize=2)
def _bwd_ref(c, with_bn, mask):
    inp = inputs(c)
    B, Lin, C, stride = c[:4]
    pre, a = activation(inp, with_bn)
    da, dw = OL.dwconv_bwd(f64(inp["dz"]), a, f64(inp["w"]), stride, pad_of(c))
    ref = dict(pre=pre)
    if with_bn:
        g = da * mask_of(pre, mask)
        xhat = (f64(inp["y"]) - f64(inp["bn"][2])) * f64(inp["bn"][3])
        gx = g * xhat
        co = f64(inp["coef"])
        ref["dy"] = f64(inp["bn"][0]) * (g - co[0] - xhat * co[1])   # oracle.layers.bn_train_bwd with the hand-made means
        ref["xhat"] = xhat
    else:
        g, gx = da, np.zeros_like(da)
    ref["g"] = g
    ref["sums"] = np.stack([g.sum((0, 1)), gx.sum((0, 1)), dw[0], dw[1], dw[2]])
    # magnitudes of the five reduced columns (premise); the rows' own contributions to the sums (controls)
    ap = np.pad(a, [[0, 0], list(pad_of(c)), [0, 0]])
    Lout = c[5]
    taps = [np.abs(f64(inp["dz"]) * ap[:, j:j + stride * Lout:stride]).sum((0, 1)) for j in range(3)]
    ref["mags"] = np.stack([np.abs(g).sum((0, 1)), np.abs(gx).sum((0, 1))] + taps)
    ref["count"] = B * Lin
    return ref


def bwd_ref(c, with_bn, mask="project"):
    """float64: g [B, L_in, C], the five column sums [5, C] = sum g | sum g xhat | dw[3] in the order of a partial row, dy (with
    the table) from the hand-made coefficients, and what premise() and the controls need"""
    return _bwd_ref(c, bool(with_bn), mask)


def premise(ref):
    """every reduced column: sum of magnitudes below 2^22, and every term a multiple of 1/2 - so each partial sum, in any order,
    fits float32's 24 bits"""
    assert ref["mags"].max() < LIMIT, "shape too large for the exact method: a column reaches %g" % ref["mags"].max()
    for k in ("g", "dy"):
        if k in ref:
            assert np.array_equal(np.rint(ref[k] * 8), ref[k] * 8) and np.abs(ref[k]).max() < 2 ** 10
            assert np.array_equal(f64(ref[k].astype(np.float32)), ref[k])
    assert np.array_equal(np.rint(ref["sums"] * 2), ref["sums"] * 2)
    return float(ref["mags"].max())


def edge_shares(pre):
    return float((pre == 0).mean()), float((pre == 6).mean())


def coef_of(sums, count):
    """dw_bwd_finalize_kernel: coef = float32(double sum * (1.0 / count)) - the reciprocal in double, then one product"""
    inv = 1.0 / float(count)
    return np.stack([(f64(sums[0]) * inv).astype(np.float32), (f64(sums[1]) * inv).astype(np.float32)])


def row_terms(c, with_bn, b, u):
    """[5, C]: what unit row (clip b, input position u) adds to the five column sums - tap j's product belongs to the row whose
    activation it reads"""
    inp = inputs(c)
    ref = bwd_ref(c, with_bn)
    B, Lin, C, stride, pad_l, Lout = c[:6]
    _, a = activation(inp, with_bn)
    out = np.zeros((5, C))
    out[0] = ref["g"][b, u]
    if with_bn:
        out[1] = ref["g"][b, u] * ref["xhat"][b, u]
    for j in range(3):
        t, r = divmod(u + pad_l - j, stride)
        if r == 0 and 0 <= t < Lout:
            out[2 + j] = f64(inp["dz"][b, t]) * a[b, u]
    return out


def control_row(c, with_bn):
    """the (b, u) row the dropped-row / doubled-row controls use: the one with the largest gradient"""
    g = bwd_ref(c, with_bn)["g"]
    b, u = np.unravel_index(int(np.argmax(np.abs(g).sum(-1))), g.shape[:2])
    return int(b), int(u)


def control_sums(c, with_bn):
    """(sums of a reference that lost the control row, sums of one that counted it twice)"""
    ref = bwd_ref(c, with_bn)
    t = row_terms(c, with_bn, *control_row(c, with_bn))
    return ref["sums"] - t, ref["sums"] + t


# ---------------------------------------------------------------------------------------------------------------------------
# the folds on their own: synthetic integer partial rows
# ---------------------------------------------------------------------------------------------------------------------------
FOLD_N = [1, 255, 256, 257, 1000, 1024, 3001]
FOLD_C = [4, 20, 64]                    # 20: a partial 16-channel workgroup of the finalise kernels
FOLD_CASES = [(n, C) for n in FOLD_N for C in FOLD_C]


def scratch_floats(n, W, scratch):
    """floats of the scratch buffer a fold of n rows of width W writes"""
    plan = pre_reduce_plan(n, scratch)
    return 0 if plan is None else plan[1] * W


def dw_fold_inputs(n, C):
    """part [n, 5, C] of integers in [-8, 8]; count"""
    rng = np.random.RandomState(n * 31 + C)
    return rng.randint(-8, 9, size=(n, 5, C)).astype(np.float32), 4 * n + 3


def stats_fold_inputs(n, C):
    """part [n, 2, C] = (sum y, sum y^2) of four rows per tile: integers in [-8, 8] and in [40, 80], so that the batch mean lies in
    [-2, 2] and the variance in [6, 20]; gamma, beta, moving mean, moving variance"""
    rng = np.random.RandomState(n * 17 + C)
    part = np.stack([rng.randint(-8, 9, size=(n, C)), rng.randint(40, 81, size=(n, C))], axis=1).astype(np.float32)
    gamma = (1 + 0.1 * rng.randn(C)).astype(np.float32)
    beta = (0.1 * rng.randn(C)).astype(np.float32)
    mm = rng.randn(C).astype(np.float32)
    mv = (1 + rng.rand(C)).astype(np.float32)
    return dict(part=part, count=4 * n, gamma=gamma, beta=beta, mm=mm, mv=mv)


def premise_fold(part):
    assert np.array_equal(part, np.rint(part)) and np.abs(f64(part)).sum(0).max() < LIMIT


BATCH_LAYERS = [(4, 1), (20, 17), (512, 256)]      # (C, rows) of the three layers of the kws_dw_grad_finalize_batch test
INFER_C = [4, 257, 1024]
BN_EPS = 1e-3
U = 2.0 ** -24


def infer_inputs(C):
    rng = np.random.RandomState(C)
    return dict(gamma=(1 + 0.1 * rng.randn(C)).astype(np.float32), beta=(0.5 * rng.randn(C)).astype(np.float32),
                mm=rng.randn(C).astype(np.float32), mv=(0.5 + 1.5 * rng.rand(C)).astype(np.float32))


def infer_ref(inp):
    """float64 table [4, C] of bn_infer_prepare_kernel and its bars [4, C]: rstd = 1 / sqrt(mv + eps) is three float32 roundings
    (3 U relative), scale = gamma * rstd one more (4 U), shift = beta - mm * scale gets 4 U (|beta| + |mm scale|), the moving mean
    is copied (0)"""
    eps = float(np.float32(BN_EPS))
    rstd = 1.0 / np.sqrt(f64(inp["mv"]) + eps)
    scale = f64(inp["gamma"]) * rstd
    ms = f64(inp["mm"]) * scale
    table = np.stack([scale, f64(inp["beta"]) - ms, f64(inp["mm"]), rstd])
    bars = np.stack([4 * U * np.abs(scale), 4 * U * (np.abs(f64(inp["beta"])) + np.abs(ms)), np.zeros_like(rstd), 3 * U * rstd])
    return table, bars
