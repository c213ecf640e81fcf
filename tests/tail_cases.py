"""Shared by tests/test_tail_kernels_gpu.py and tests/test_tail_cpu.py: case tables, input builders, float64 references and a
restatement of the slice planner for the classifier tails - csrc/tail.hip (kws_ts_tail_launch, kws_small_wgrad_launch,
kws_tail_post_launch, kws_metrics_launch) and csrc/gconv.hip kws_flat_tail_launch.  Imports without a GPU.

Exact inputs (small_wgrad / colsum / metrics): X ternary, D small integers, so that every partial sum is an integer below 2^24
and the device must give the float64 result bit for bit whatever the slicing (tests/gemm_exact.py's method).

Grid inputs (the fused tails): y in steps of 1/32, BN scale k/16, shift k/32 (test_resblock_kernels_gpu.py join_inputs), so that
bn(y) = fma(y, scale, shift) is exact in float32: the float64 reference sees the device's very activations, the ReLU6 gate has
no knife-edge, and a share of the pre-activations sits exactly on 0 and on 6.

The pool-winner premise (ts_tail).  The kernel finds the winners of max_t x[t, c] att[t] by comparing float32 products with ITS
attention weights; the reference compares float64 products with its own.  Both name the same winners when, for every (b, c),
the runner-up is either an exact STRUCTURAL tie or below the maximum by a relative gap of

    POOL_GAP = 2^-17 = 128 x 2^-24,

128 roundings of one float32 product: one for each of the two products compared, the rest for the relative error of the
device's attention weights (measured at most 8.8e-7 = 15 x 2^-24: profiles/tail_direct_error_vs_f64.txt, column att_rel).  A structural tie is an
all-zero channel (every product is 0 x att = 0) or time rows 0 and 1 holding the same activation under bit-equal attention
weights: W1 columns 0 and 1 and b1[0:2] are made equal, so logits 0 and 1 are the same chain of operations on the same values
on the device and in the reference.  The seeds of the case table are ones for which the premise holds; no element is ever left
out of a comparison."""
import numpy as np

import gemm_exact as GE
from oracle import layers as OL

U = 2.0 ** -24
SLICES = 32              # KWS_SMALL_WGRAD_SLICES (csrc/internal.h)
ROWS = 64                # KWS_SMALL_WGRAD_ROWS (csrc/tail.hip): rows of D a slice of the rows kernel may hold
MAXT, MAXNC = 16, 64     # csrc/tail.hip
FT_MAXD, FT_MAXNC = 8192, 64     # csrc/gconv.hip
POOL_GAP = 2.0 ** -17
KEEP = 0.6               # Dropout(0.4) of the headline model (csrc/net.hip DROP_KEEP); np.float32(0.6) on the device
SMOOTH = 0.1             # label smoothing; np.float32(0.1) on the device
# the loss clips p at float32 constants on the device (and in the float32 graph it restates): eps and 1 - eps as float32
LO32 = float(np.float32(1e-7))
HI32 = float(np.float32(1.0) - np.float32(1e-7))
# T = the attention width the headline planner gives for 12000 / 16000 / 20000 samples (tests/test_tail_cpu.py reads it back)
TS_T = {12000: 6, 16000: 9, 20000: 12}


def f64(a):
    return np.asarray(a, dtype=np.float64)


# ---------------------------------------------------------------------------------------------------------------------------
# the slice planner of kws_small_wgrad_launch / kws_tail_post_launch, restated
# ---------------------------------------------------------------------------------------------------------------------------
def small_wgrad_plan(B, K, N, scratch):
    """dict(S, rows_per, kernel 'rows' | 'generic', slab 'none' | 'reduce_slabs' | 'slab_sum', colsum (KP, NT))"""
    S = min(SLICES if scratch else 1, B)
    rows_per = GE.ceil_div(B, S)
    S = GE.ceil_div(B, rows_per)
    kernel = "rows" if (N <= 16 and rows_per <= ROWS) else "generic"
    slab = "none" if S == 1 else ("reduce_slabs" if (K * N) % 4 == 0 else "slab_sum")
    colsum = (16, 256) if N <= 16 else ((32, 1024) if N <= 32 else (64, 1024))
    return dict(S=S, rows_per=rows_per, kernel=kernel, slab=slab, colsum=colsum)


def tail_post_eligible(B, K1, N1, K2, N2):
    if B <= 0:
        return False
    S = min(SLICES, B)
    rows_per = GE.ceil_div(B, S)
    S = GE.ceil_div(B, rows_per)
    return not (S <= 1 or N1 > 16 or N2 > 16 or rows_per > ROWS or (K1 * N1) % 4 != 0 or (K2 * N2) % 4 != 0)


def wgrad_corners(B, K, N, scratch, bias=True):
    """the corners of the launcher and its kernels that a case reaches"""
    pl = small_wgrad_plan(B, K, N, scratch)
    out = {pl["kernel"], "slab:" + pl["slab"]}
    if bias:
        out.add("colsum<%d,%d>" % pl["colsum"])
    else:
        out.add("no_bias")
    out.add("scratch" if scratch else "scratch_null")
    if pl["S"] == 1 and scratch:
        out.add("S=1_with_scratch")
    out.add("rows_per=%d" % pl["rows_per"] if pl["rows_per"] in (1, 2, ROWS, ROWS + 1) else "rows_per_other")
    last = B - (pl["S"] - 1) * pl["rows_per"]
    if pl["S"] > 1 and last < pl["rows_per"]:
        out.add("ragged_last_slice")
        if last == 1:
            out.add("last_slice_one_row")
    if pl["kernel"] == "rows" and pl["rows_per"] % 8:
        out.add("unroll8_tail")
    if K % 256:
        out.add("K_ends_inside_block")
    if N > 16:
        out.add("N>16")
    return out


# (B, K, N, scratch given, out_bias given, corners the case is in the table for)
WGRAD_CASES = [
    (1, 260, 12, True, True, {"S=1_with_scratch", "slab:none", "rows"}),
    (31, 260, 12, True, True, {"rows_per=1", "rows", "slab:reduce_slabs"}),
    (33, 260, 12, True, True, {"rows_per=2", "last_slice_one_row"}),
    (100, 1024, 12, True, True, {"rows", "unroll8_tail"}),                        # rows_per 4: the 8-row unroll's tail
    (1000, 516, 9, True, True, {"ragged_last_slice", "K_ends_inside_block", "rows"}),      # last slice of 8; N = T
    (2048, 64, 16, True, True, {"rows_per=64", "rows"}),                          # the sD bound
    (2049, 64, 12, True, True, {"rows_per=65", "generic"}),
    (2048, 128, 32, True, True, {"generic", "N>16", "colsum<32,1024>"}),          # C3's head
    (1000, 96, 33, True, True, {"generic", "colsum<64,1024>"}),
    (1000, 96, 64, True, True, {"generic", "colsum<64,1024>"}),
    (70, 37, 11, True, True, {"rows", "slab:slab_sum"}),
    (70, 37, 17, True, True, {"generic", "slab:slab_sum"}),
    (40, 260, 12, False, True, {"rows", "scratch_null", "slab:none"}),
    (70, 260, 12, False, True, {"generic", "scratch_null", "slab:none"}),
    (64, 260, 12, True, False, {"no_bias"}),
]
WGRAD_CORNERS = {"rows", "generic", "slab:none", "slab:reduce_slabs", "slab:slab_sum", "colsum<16,256>", "colsum<32,1024>",
                 "colsum<64,1024>", "no_bias", "scratch_null", "S=1_with_scratch", "rows_per=1", "rows_per=2", "rows_per=64",
                 "rows_per=65", "ragged_last_slice", "last_slice_one_row", "unroll8_tail", "K_ends_inside_block", "N>16"}

# colsum_kernel<KP, NT>: G = NT / KP row groups, four interleaved accumulators each: B around one full round of 4 G rows
COLSUM_FORMS = [((16, 256), 12, 16), ((32, 1024), 32, 32), ((64, 1024), 33, 16)]          # (form, N, G)
COLSUM_CASES = [(B, N, form) for form, N, G in COLSUM_FORMS for B in (1, 4 * G - 1, 4 * G, 4 * G + 1, 1000)]
COLSUM_K = 8

METRICS_B = [1, 255, 256, 257, 1000]

# kws_tail_post_launch: the headline shapes, and shapes it must refuse (B, K1, N1, K2, N2)
TAIL_POST_HEADLINE = dict(K2=1024, N2=12, K1=4608, N1=9)
TAIL_POST_B = [2, 33, 100]
TAIL_POST_REFUSED = [(100, 36, 9, 64, 32, "N2 = 32"), (1, 36, 9, 64, 12, "B = 1"), (2049, 36, 9, 64, 12, "B = 2049"),
                     (100, 37, 9, 64, 12, "K1 N1 % 4 != 0"), (100, 36, 9, 63, 11, "K2 N2 % 4 != 0")]


def wgrad_inputs(B, K, N, seed=None):
    """ternary X [B, K], D [B, N] of integers in -3 .. 3"""
    rng = np.random.RandomState(B + 3 * K + 7 * N if seed is None else seed)
    return GE.ternary(rng, B, K), rng.randint(-3, 4, size=(B, N)).astype(np.float32)


def premise_wgrad(X, D):
    """every partial sum of X^T D and of D's column sums is an integer below 2^24, in any order"""
    assert np.array_equal(f64(X), np.rint(f64(X))) and np.array_equal(f64(D), np.rint(f64(D)))
    assert (np.abs(f64(X)).T @ np.abs(f64(D))).max() < GE.LIMIT and np.abs(f64(D)).sum(axis=0).max() < GE.LIMIT, \
        "shape too large for the exact method"


def metrics_inputs(B):
    """per_loss: multiples of 2^-10 below 8, per_correct 0 / 1: both totals are float32 values (B <= 2048)"""
    rng = np.random.RandomState(900 + B)
    per_loss = rng.randint(0, 8192, size=B).astype(np.float32) / 1024
    per_correct = rng.randint(0, 2, size=B).astype(np.float32)
    per_loss[-1] = max(per_loss[-1], 1.0 / 1024)                              # the last element counts: the controls drop it
    assert B * 8192 < 2 ** 24 and np.array_equal(f64(per_loss) * 1024, np.rint(f64(per_loss) * 1024))
    return per_loss, per_correct


# ---------------------------------------------------------------------------------------------------------------------------
# grid inputs
# ---------------------------------------------------------------------------------------------------------------------------
def grid_bn(rng, C):
    bn = np.zeros((4, C), np.float32)
    bn[0] = rng.randint(8, 40, size=C) / 16.0                                 # scale 0.5 .. 2.44
    bn[1] = rng.randint(-32, 32, size=C) / 32.0                               # shift
    bn[2] = (0.5 * rng.randn(C)).astype(np.float32)                           # mean
    bn[3] = (0.5 + rng.rand(C)).astype(np.float32)                            # rstd
    return bn


def act64(y, scale, shift):
    """(pre, relu6(pre)) in float64; asserts that pre is exact in float32 (scale / shift broadcast over y's last axis)"""
    pre = f64(y) * f64(scale) + f64(shift)
    assert np.array_equal(pre.astype(np.float32).astype(np.float64), pre), "inputs do not make bn(y) exact in float32"
    return pre, np.clip(pre, 0.0, 6.0)


def put_on_edges(rng, y, scale, shift, frac=0.04):
    """moves a share of y so that bn(y) is exactly 0, and another so that it is exactly 6, where a grid value of y does it"""
    for target in (0.0, 6.0):
        want = (target - f64(shift)) / f64(scale) + 0.0 * f64(y)
        on_grid = np.equal(want * 32, np.rint(want * 32))
        m = (rng.rand(*y.shape) < frac) & on_grid
        y[m] = want[m].astype(np.float32)
    return y


# ---------------------------------------------------------------------------------------------------------------------------
# ts_tail
# ---------------------------------------------------------------------------------------------------------------------------
# (name, B, T, C, NC, seed, what it covers)
TS_CASES = [
    ("headline", 5, 9, 512, 12, 11, "ts_tail_kernel<., 9> + the float4 walk of W2 (NC % 4 == 0, NC <= 16)"),
    ("nc32", 3, 9, 512, 32, 12, "the per-class walk of W2 on the fast-9 path"),
    ("nc11", 3, 9, 64, 11, 13, "NC & 3 != 0"),
    ("w1_off", 3, 9, 512, 12, 14, "W1 one float past an aligned base: the host check routes T = 9 to <., 0>"),
    ("t6", 3, TS_T[12000], 512, 12, 15, "T of a 12000-sample input"),
    ("t12", 3, TS_T[20000], 512, 12, 16, "T of a 20000-sample input"),
    ("t1", 2, 1, 64, 12, 17, "T = 1"),
    ("maxt", 2, 16, 320, 16, 18, "T = MAXT; C not a multiple of 256; NC = 16"),
    ("big_lds", 2, 16, 1024, 12, 19, "more than 64 KB of LDS: the hipFuncSetAttribute path"),
    ("saturated", 3, 9, 512, 12, 20, "a dominant W2 column: p at both clip edges, dl2 = 0, the clipped loss"),
    ("shard", 6, 9, 64, 12, 21, "B = 6 for the shard test: two launches of 3 at row offsets 0 and 3"),
]
TS_BY_NAME = dict((c[0], c) for c in TS_CASES)
TS_STEP, TS_SEED = 3, 0x1234567ABCDEF


def ts_lds_bytes(T, C):
    return 4 * (T * C + 4 * C + 4 * MAXNC + 4 * MAXT + 3 * MAXNC + 256 + MAXNC + MAXT)


def ts_inputs(name):
    """dict(y [B, T, C], bn [4, C], W1 [T C, T], b1 [T], W2 [2 C, NC], labels [B, NC]) of case `name`, float32"""
    _, B, T, C, NC, seed, _ = TS_BY_NAME[name]
    rng = np.random.RandomState(seed)
    y = rng.randint(-96, 224, size=(B, T, C)).astype(np.float32) / 32         # [-3, 7) in steps of 1/32
    bn = grid_bn(rng, C)
    y = put_on_edges(rng, y, bn[0], bn[1])
    zero_c = np.nonzero(rng.rand(C) < 0.04)[0]                                # all-zero channels: bn(y) <= 0 at every t
    for c in zero_c:
        y[:, :, c] = -np.abs(y[:, :, c]) - 3.0                                # pre <= -3 scale + shift < 0 (scale >= 0.5, shift < 1)
    if T >= 2:                                                                # rows 0 and 1 equal and dominant: structural ties
        tie_c = np.setdiff1d(np.nonzero(rng.rand(C) < 0.08)[0], zero_c)
        for c in tie_c:
            hi = rng.randint(160, 224, size=B).astype(np.float32) / 32        # y in [5, 7): pre >= 0.5 * 5 - 1 = 1.5
            y[:, 0, c] = hi
            y[:, 1, c] = hi
            y[:, 2:, c] = -np.abs(y[:, 2:, c]) - 1.0                          # the other rows: pre <= shift - scale < 0.5
    W1 = (rng.randn(T * C, T) * (0.2 / np.sqrt(T * C))).astype(np.float32)    # logits of a few tenths
    b1 = (0.1 * rng.randn(T)).astype(np.float32)
    if T >= 2:
        W1[:, 1] = W1[:, 0]
        b1[1] = b1[0]
    W2 = (rng.randn(2 * C, NC) * (1.0 / np.sqrt(2 * C))).astype(np.float32)
    labels = np.eye(NC, dtype=np.float32)[rng.randint(0, NC, size=B)]
    inp = dict(y=y, bn=bn, W1=W1, b1=b1, W2=W2, labels=labels)
    if name == "saturated":
        # column k0 of W2 constant, the others tiny: logit k0 leads by about 21, so p[k0] rounds to 1 in float32 (above the
        # upper clip edge) and every other p is around e^-21 = 8e-10 (below the lower one) yet far from 0
        W2 *= np.float32(0.01)
        k0 = 5
        W2[:, k0] = 1.0
        fd = ts_tail_ref(dict(inp, W2=W2), 0)["fd"]
        W2[:, k0] = np.float32(21.0 / fd.sum(axis=1).mean())
    return inp


def smooth_cce(p, y, smoothing, loss_batch, clip_gate=True):
    """oracle.layers.smooth_cce_fwd_bwd with the clip edges the float32 graph has (LO32, HI32) and the gradient divided by
    loss_batch; tests/test_tail_cpu.py holds it to the oracle's function wherever no probability is outside the edges"""
    NC = p.shape[1]
    ysm = y * (1.0 - smoothing) + smoothing / NC
    pc = np.clip(p, LO32, HI32)
    S = pc.sum(axis=1, keepdims=True)
    per = -(ysm * (np.log(pc) - np.log(S))).sum(axis=1)
    dpc = (-ysm / pc + ysm.sum(axis=1, keepdims=True) / S) / float(loss_batch)
    inside = ((p >= LO32) & (p <= HI32)).astype(np.float64) if clip_gate else 1.0
    return per, dpc * inside


def keras_cce(p, y, loss_batch):
    """oracle.layers.cce_fwd_bwd (the Keras CE of the grouped oracle) with the float32 clip edges, gradient / loss_batch"""
    s = p.sum(axis=1, keepdims=True)
    pn = p / s
    pc = np.clip(pn, LO32, HI32)
    per = -(y * np.log(pc)).sum(axis=1)
    inside = ((pn >= LO32) & (pn <= HI32)).astype(np.float64)
    dpn = (-y / pc) * inside / float(loss_batch)
    return per, dpn / s - (dpn * p).sum(axis=1, keepdims=True) / (s * s)


MUTATIONS = ("first_winner", "no_mask2", "mean_by_C", "no_clip_gate", "no_b1", "row_offset_ignored")


# (mutation, case, the output the device must miss it on)
TS_CONTROLS = [("first_winner", "headline", "g"), ("no_mask2", "headline", "g"), ("mean_by_C", "headline", "g"),
               ("no_clip_gate", "saturated", "dl2"), ("no_b1", "headline", "att"), ("row_offset_ignored", "nc11", "xd")]
FLAT_CONTROLS = [("row_offset_ignored", "offset", "fd")]


def ts_tail_ref(inp, row_offset, loss_batch=None, train=True, mutate=None):
    """float64 reference of ts_tail_kernel: every output, as a dict.  mutate: one of MUTATIONS - a reference that is wrong on
    purpose (negative controls)."""
    assert mutate is None or mutate in MUTATIONS
    y, bn, W1, b1, W2, labels = (f64(inp[k]) for k in ("y", "bn", "W1", "b1", "W2", "labels"))
    B, T, C = y.shape
    NC = W2.shape[1]
    TC = T * C
    keep = float(np.float32(KEEP))
    if mutate == "row_offset_ignored":
        row_offset = 0
    pre, a = act64(y, bn[0], bn[1])
    flat = a.reshape(B, TC)
    out = {}
    if train:
        m1 = OL.dropout_mask(OL.dropout_key(TS_SEED, TS_STEP, 1), B * TC, keep, row_offset * TC).reshape(B, TC)
        m2 = OL.dropout_mask(OL.dropout_key(TS_SEED, TS_STEP, 2), B * 2 * C, keep, row_offset * 2 * C).reshape(B, 2 * C)
        xd = flat * m1 / keep
    else:
        xd = flat
    logits1 = xd @ W1 + (0.0 if mutate == "no_b1" else b1)
    att = OL.softmax(logits1, axis=1)
    xa = a * att[:, :, None]
    xmax = xa.max(axis=1)
    feat = np.concatenate([xmax, a.mean(axis=1)], axis=1)
    fd = feat * m2 / keep if train else feat
    p = OL.softmax(fd @ W2, axis=1)
    out.update(probs=p, att=att, xd=xd, fd=fd, a=a, pre=pre, xa=xa)
    if not train:
        return out
    per, dp = smooth_cce(p, labels, float(np.float32(SMOOTH)), B if loss_batch is None else loss_batch,
                         clip_gate=(mutate != "no_clip_gate"))
    dl2 = OL.softmax_bwd(dp, p, axis=1)
    dfeat = (dl2 @ W2.T) * (1.0 if mutate == "no_mask2" else m2) / keep
    ind = (xa == xmax[:, None, :]).astype(np.float64)                         # reduce_max: ties share equally (oracle/net.py)
    if mutate == "first_winner":
        ind = ind * (np.cumsum(ind, axis=1) == 1)
    nwin = ind.sum(axis=1, keepdims=True)
    dxa = ind / nwin * dfeat[:, None, :C]
    da = dxa * att[:, :, None] + dfeat[:, None, C:] / float(C if mutate == "mean_by_C" else T)
    dl1 = OL.softmax_bwd((dxa * a).sum(axis=2), att, axis=1)
    da = da + ((dl1 @ W1.T) * m1 / keep).reshape(B, T, C)
    g = da * OL.relu6_mask(pre)
    xh = (y - bn[2]) * bn[3]
    out.update(m1=m1, m2=m2, dl1=dl1, dl2=dl2, g=g, xh=xh, part0=g.sum(axis=1), part1=(g * xh).sum(axis=1), per_loss=per,
               per_correct=(p.argmax(axis=1) == labels.argmax(axis=1)).astype(np.float64), nwin=nwin[:, 0, :], dxmax=dfeat[:, :C])
    return out


def premise_ts(inp, ref):
    """the pool-winner premise (module docstring) and the premise of an exact per_correct; returns the number of structural
    ties with a non-zero incoming gradient: (all-zero channels, equal rows 0 / 1)"""
    a, att, xa = ref["a"], ref["att"], ref["xa"]
    B, T, C = a.shape
    m = xa.max(axis=1, keepdims=True)
    win = xa == m
    n = win.sum(axis=1)
    assert (xa[~win] <= (m * (1.0 - POOL_GAP) + 0.0 * xa)[~win]).all(), "a runner-up within POOL_GAP of the maximum: other seed"
    allzero = (a == 0).all(axis=1)
    multi = n > 1
    pair = np.zeros_like(multi)
    if T >= 2:
        assert np.array_equal(att[:, 0], att[:, 1]), "the reference's attention weights 0 and 1 are not bit-equal"
        pair = win[:, 0] & win[:, 1] & (n == 2) & (a[:, 0] == a[:, 1]) & ~allzero
    assert (n[allzero] == T).all()
    assert (multi == ((allzero & (T > 1)) | pair)).all(), "a tie that is not structural: other seed"
    p = np.sort(ref["probs"], axis=1)
    if p.shape[1] > 1:
        assert (p[:, -1] - p[:, -2] > 1e-3).all(), "arg-max of p too close to call: other seed"
    live = ref["dxmax"] != 0
    return int((allzero & live).sum()), int((pair & live).sum())


def premise_saturated(ref):
    p = ref["probs"]
    top = p.max(axis=1)
    rest = np.sort(p, axis=1)[:, :-1]
    assert (top >= 1.0 - 5e-8).all() and (rest < 0.5 * LO32).all() and (rest > 1e-11).all(), "not saturated as designed"


def edge_shares(pre):
    """(share of pre-activations exactly 0, exactly 6)"""
    return float((pre == 0).mean()), float((pre == 6).mean())


# ---------------------------------------------------------------------------------------------------------------------------
# flat_tail
# ---------------------------------------------------------------------------------------------------------------------------
# (name, B, D, F, Ng, NC, bd given, raw, layer_id, row_offset, seed, what it covers)
FLAT_CASES = [
    ("maxd", 5, 8192, 64, 16, 12, True, False, 0, 0, 31, "D = FT_MAXD"),
    ("odd", 3, 300, 60, 20, 32, True, False, 0, 0, 32, "D not a multiple of 256; three groups"),
    ("heavy", 4, 128, 128, 128, 12, False, False, 0, 0, 33, "the heavy head: bd NULL"),
    ("gru", 4, 256, 256, 256, 12, True, True, 0, 0, 34, "the GRU head: raw signed features, no dropout"),
    ("nc1", 2, 4, 4, 4, 1, True, False, 0, 0, 35, "NC = 1"),
    ("maxnc", 2, 64, 64, 64, 64, True, False, 0, 0, 36, "NC = FT_MAXNC"),
    ("layer3", 3, 300, 60, 20, 12, True, False, 3, 0, 37, "a non-default dropout layer_id"),
    ("offset", 3, 300, 60, 20, 12, True, False, 0, 5, 38, "a non-zero row_offset"),
]
FLAT_BY_NAME = dict((c[0], c) for c in FLAT_CASES)
FLAT_KEEP = 0.7            # Dropout(0.3) of the grouped models


def flat_inputs(name):
    _, B, D, F, Ng, NC, has_bd, raw, _, _, seed, _ = FLAT_BY_NAME[name]
    rng = np.random.RandomState(seed)
    groups = F // Ng
    bn = np.stack([grid_bn(rng, Ng) for _ in range(groups)])                  # [groups, 4, Ng]: scale | shift | mean | rstd
    if raw:
        y = rng.randn(B, D).astype(np.float32)
    else:
        y = rng.randint(-96, 224, size=(B, D)).astype(np.float32) / 32
        y = put_on_edges(rng, y.reshape(B, D // F, F), bn[:, 0].reshape(F), bn[:, 1].reshape(F)).reshape(B, D)
    Wd = (rng.randn(D, NC) * (1.0 / np.sqrt(D))).astype(np.float32)
    bd = (0.1 * rng.randn(NC)).astype(np.float32) if has_bd else None
    labels = np.eye(NC, dtype=np.float32)[rng.randint(0, NC, size=B)]
    return dict(y=y, bn=bn, Wd=Wd, bd=bd, labels=labels)


def flat_tail_ref(name, inp, train=True, mutate=None):
    _, B, D, F, Ng, NC, has_bd, raw, layer_id, row_offset, _, _ = FLAT_BY_NAME[name]
    y, Wd, labels = f64(inp["y"]), f64(inp["Wd"]), f64(inp["labels"])
    keep = float(np.float32(FLAT_KEEP))
    if mutate == "row_offset_ignored":
        row_offset = 0
    if raw:
        pre, f = y, y
    else:
        pre, f = act64(y.reshape(B, D // F, F), inp["bn"][:, 0].reshape(F), inp["bn"][:, 1].reshape(F))
        pre, f = pre.reshape(B, D), f.reshape(B, D)
    m = np.ones((B, D))
    if train and not raw:
        m = OL.dropout_mask(OL.dropout_key(TS_SEED, TS_STEP, layer_id if layer_id else 1), B * D, keep,
                            row_offset * D).reshape(B, D) / keep
    fd = f * m
    logits = fd @ Wd + (f64(inp["bd"]) if has_bd else 0.0)
    p = OL.softmax(logits, axis=1)
    out = dict(probs=p, fd=fd, pre=pre)
    if not train:
        return out
    per, dp = keras_cce(p, labels, B)
    dl = OL.softmax_bwd(dp, p, axis=1)
    out.update(dl=dl, dA=(dl @ Wd.T) * m, per_loss=per,
               per_correct=(p.argmax(axis=1) == labels.argmax(axis=1)).astype(np.float64))
    return out


def premise_flat(ref):
    p = np.sort(ref["probs"], axis=1)
    if p.shape[1] > 1:
        assert (p[:, -1] - p[:, -2] > 1e-3).all(), "arg-max of p too close to call: other seed"


# ---------------------------------------------------------------------------------------------------------------------------
# bars
# ---------------------------------------------------------------------------------------------------------------------------
def rel_err(got, ref):
    """max-norm error relative to the reference's max norm"""
    return float(np.abs(f64(got) - f64(ref)).max() / max(float(np.abs(f64(ref)).max()), 1e-300))


CEILING = 5e-5             # the whole-net bar of tests/test_net_gpu.py: no direct bar may be looser
# Chained outputs: 2 x the worst max-norm error against the float64 reference measured on these very inputs on the MI355X
# (profiles/tail_direct_error_vs_f64.txt, row "worst"; regenerate with `python tests/test_tail_kernels_gpu.py`).
TS_BARS = dict(att=2 * 3.37e-7, probs=2 * 5.69e-7, dl1=2 * 4.75e-7, dl2=2 * 4.42e-7, g=2 * 4.44e-7, per_loss=2 * 2.32e-7)
FLAT_BARS = dict(probs=2 * 1.57e-6, dl=2 * 1.2e-6, dA=2 * 1.03e-6, per_loss=2 * 1.77e-7)
