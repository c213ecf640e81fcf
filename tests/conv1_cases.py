"""Shared by tests/test_conv1_cpu.py and tests/test_conv1_kernels_gpu.py: the cases, the float64 references and a Python
restatement of the two host planners of the raw-waveform net's first convolution (csrc/conv1.hip: kws_conv1_fwd,
kws_conv1_wgrad, kws_conv1_wgrad_slabs).

The references are written from the definition of the operation, not from the kernels' tiling:

    A[(b, t), k] = x[b, stride_t t + base_off + k]  for k < 80, 0 where the sample lies outside [0, x_len)       toeplitz()
    Weff[s]      = sum_j W[j][s - hop j]            (the `taps` overlapping taps of `cin` samples, `hop` apart)   fold()
    C            = A Weff
    dWeff        = A^T G,   dW[j][c] = dWeff[hop j + c]                                                           unfold()

The planners (fwd_plan / wgrad_plan restate kws_conv1_stats_rows / wgrad_plan of conv1.hip) are not visible from outside the
library; tests/test_conv1_cpu.py checks the restatement against kwst_conv1_stats_rows / kwst_conv1_wgrad_workspace_floats for
every case and a sweep of M, so the corners the table claims (edges()) cannot drift silently.

The exact runs use gemm_exact.py's method: ternary x, W and G make every product and partial sum an integer; premise_* assert
from the float64 reference that the sums stay below 2^24 (a condition of the test, not a tolerance)."""
import functools

import numpy as np

import gemm_exact as GE

KF = 80            # folded samples per output row
NOUT = 128         # output channels
FM = 64            # forward row tile
UM = 32            # weight-gradient row unit
FWD_WGS = 768      # persistent forward workgroups: three per CU
PER_GROUP = 32     # slabs per group of the two-stage slab sum
SLACK = 1000.0     # what the GPU test writes between x_len and x_batch_stride: a read past x_len changes an integer


def ceil_div(a, b):
    return -(-a // b)


# ---------------------------------------------------------------------------------------------------------------------------
# the planners, restated
# ---------------------------------------------------------------------------------------------------------------------------
def fwd_plan(M):
    """dict(tiles, rows): 64-row tiles; rows = grid = statistics rows the forward kernel writes"""
    tiles = ceil_div(M, FM)
    return dict(tiles=tiles, rows=min(tiles, FWD_WGS))


def wgrad_plan(M):
    """dict(chunk, S, groups): S splits of `chunk` rows (whole 32-row units), summed in groups of 32 slabs"""
    chunk = max(UM, UM * ceil_div(ceil_div(M, FWD_WGS), UM))
    S = ceil_div(M, chunk)
    return dict(chunk=chunk, S=S, groups=ceil_div(S, PER_GROUP))


def workspace_floats(M):
    return wgrad_plan(M)["S"] * KF * NOUT


# ---------------------------------------------------------------------------------------------------------------------------
# cases
# ---------------------------------------------------------------------------------------------------------------------------
def _case(B, L_out, stride_t, base_off, x_len, x_batch_stride, taps, cin, hop, product, corners):
    return dict(B=B, L_out=L_out, stride_t=stride_t, base_off=base_off, x_len=x_len, x_batch_stride=x_batch_stride, taps=taps,
                cin=cin, hop=hop, product=product, corners=set(corners))


_MODEL = (399, 40, -10, 16000, 16000, 3, 40, 20)     # input_size 16000: the headline configuration

# name -> case; `product`: a configuration ts_build can produce (False: a gather kws_conv1_supported accepts but no product
# configuration builds).  `corners`: what the case is in the table for; each must be among edges(case).
CASES = {
    # 7 tiles, the last of 15 rows; 13 splits of one unit, the last of 15 rows; one slab group
    "B1": _case(1, *_MODEL, product=True,
                corners={"fwd_ragged_last_tile", "fwd_one_tile_per_wg", "wg_units_per_split=1", "wg_last_split_ragged",
                         "wg_one_group", "clip_start_overhang"}),
    # exactly 399 tiles: every tile takes the store path without a per-row test; two units per split; 13 groups, the last of 15
    "B64": _case(64, *_MODEL, product=True,
                 corners={"fwd_all_tiles_whole", "wg_units_per_split=2", "wg_last_split_whole", "wg_ragged_last_group"}),
    # 774 tiles on 768 workgroups: six take a second tile through the prefetch buffer and the 4-row last tile is one of them;
    # chunk 96, 516 splits, the last of 36 rows = one whole unit + 4 rows; 17 groups, the last of 4 slabs
    "B124": _case(124, *_MODEL, product=True,
                  corners={"fwd_second_tile_few", "fwd_ragged_tile_is_second", "wg_units_per_split=3",
                           "wg_last_split_unit_plus_ragged", "wg_ragged_last_group"}),
    # 1247 tiles: 479 workgroups run two tiles, 289 run one; chunk 128, 624 splits, 20 groups
    "B200": _case(200, *_MODEL, product=True,
                  corners={"fwd_second_tile_most", "wg_units_per_split=4", "wg_many_groups"}),
    # one clip of 810 samples (input_size must be >= 1600 in the product, but the kernels do not know): below one 32-row unit
    "short": _case(1, 20, 40, -10, 810, 810, 3, 40, 20, product=False,
                   corners={"fwd_one_partial_tile", "wg_below_one_unit", "wg_S=1", "clip_end_overhang"}),
    # input_size = 1604: SAME padding puts 18 zeros in front and row 39 reads samples 1542 .. 1621 of 1604
    "in1604": _case(7, 40, 40, -18, 1604, 1604, 3, 40, 20, product=True,
                    corners={"clip_start_overhang", "clip_end_overhang", "tile_spans_clips"}),
    # odd x_len: the 8-byte load at sample 1532 straddles the clip's end; one float of slack between clips; W already folded
    "odd_folded": _case(5, 37, 42, -6, 1533, 1534, 1, 80, 0, product=False,
                        corners={"float2_straddles_x_len", "batch_stride_slack", "taps=1", "clip_end_overhang"}),
    "two_taps": _case(7, 41, 40, -10, 1611, 1612, 2, 60, 20, product=False,
                      corners={"taps=2", "float2_straddles_x_len", "batch_stride_slack"}),
}
EXACT_CASES = list(CASES)
FLOAT_CASES = ["B1", "B124", "in1604"]
# corners the table as a whole must reach
CORNERS = {
    # forward: tile walk of the persistent grid
    "fwd_one_partial_tile", "fwd_ragged_last_tile", "fwd_all_tiles_whole", "fwd_one_tile_per_wg", "fwd_second_tile_few",
    "fwd_second_tile_most", "fwd_ragged_tile_is_second",
    # weight gradient: splits, units and the two-stage slab sum
    "wg_below_one_unit", "wg_S=1", "wg_S>1", "wg_units_per_split=1", "wg_units_per_split=2", "wg_units_per_split=3",
    "wg_units_per_split=4", "wg_last_split_whole", "wg_last_split_ragged", "wg_last_split_unit_plus_ragged", "wg_one_group",
    "wg_many_groups", "wg_ragged_last_group",
    # the gather
    "clip_start_overhang", "clip_end_overhang", "float2_straddles_x_len", "batch_stride_slack", "tile_spans_clips", "taps=1",
    "taps=2", "taps=3",
}


def rows_of(c):
    return c["B"] * c["L_out"]


def edges(c):
    """the corners of the kernels' walks that case c reaches"""
    M = rows_of(c)
    out = set()
    f = fwd_plan(M)
    tiles = f["tiles"]
    if M % FM:
        out.add("fwd_ragged_last_tile")
        if tiles == 1:
            out.add("fwd_one_partial_tile")
    else:
        out.add("fwd_all_tiles_whole")
    if tiles <= FWD_WGS:
        out.add("fwd_one_tile_per_wg")
    elif tiles < 2 * FWD_WGS:
        out.add("fwd_second_tile_few" if 2 * (tiles - FWD_WGS) < FWD_WGS else "fwd_second_tile_most")
    if M % FM and tiles - 1 >= FWD_WGS:
        out.add("fwd_ragged_tile_is_second")
    w = wgrad_plan(M)
    out.add("wg_S=1" if w["S"] == 1 else "wg_S>1")
    if M < UM:
        out.add("wg_below_one_unit")
    out.add("wg_units_per_split=%d" % (w["chunk"] // UM))
    last = M - (w["S"] - 1) * w["chunk"]
    if last % UM == 0:
        out.add("wg_last_split_whole")
    else:
        out.add("wg_last_split_ragged")
        if last > UM:
            out.add("wg_last_split_unit_plus_ragged")
    if w["groups"] == 1:
        out.add("wg_one_group")
    else:
        out.add("wg_many_groups")
        if w["S"] % PER_GROUP:
            out.add("wg_ragged_last_group")
    last_sample = c["stride_t"] * (c["L_out"] - 1) + c["base_off"] + KF     # one past the last sample the last row reads
    if c["base_off"] < 0:
        out.add("clip_start_overhang")
    if last_sample > c["x_len"]:
        out.add("clip_end_overhang")
        # every staged 8-byte pair starts at an even sample: with an odd x_len the pair at x_len - 1 is half inside
        if c["x_len"] % 2 == 1 and (c["base_off"] + c["stride_t"] * (c["L_out"] - 1)) % 2 == 0:
            out.add("float2_straddles_x_len")
    if c["x_batch_stride"] > c["x_len"]:
        out.add("batch_stride_slack")
    if c["B"] > 1 and c["L_out"] % FM:
        out.add("tile_spans_clips")
    out.add("taps=%d" % c["taps"])
    return out


def folded_desc(c):
    """the folded view: one tap of 80 samples (kws_gather_t members)"""
    return dict(L_out=c["L_out"], cin=KF, taps=1, stride_t=c["stride_t"], stride_j=0, base_off=c["base_off"], x_len=c["x_len"],
                x_batch_stride=c["x_batch_stride"])


def unfolded_desc(c):
    """the reference's view: `taps` taps of `cin` samples, `hop` apart"""
    return dict(folded_desc(c), cin=c["cin"], taps=c["taps"], stride_j=c["hop"])


# ---------------------------------------------------------------------------------------------------------------------------
# references
# ---------------------------------------------------------------------------------------------------------------------------
def toeplitz(x, g):
    """float64 A[B L_out, 80] of clips x[B, x_len] under the folded descriptor g"""
    x = GE.f64(x)
    assert x.ndim == 2 and x.shape[1] == g["x_len"]
    t = np.arange(g["L_out"])[:, None]
    k = np.arange(KF)[None, :]
    pos = g["stride_t"] * t + g["base_off"] + k
    inside = (pos >= 0) & (pos < g["x_len"])
    A = np.where(inside[None], x[:, np.where(inside, pos, 0)], 0.0)
    return A.reshape(x.shape[0] * g["L_out"], KF)


def fold(W, hop):
    """float64 Weff[hop (taps - 1) + cin, N] of W[taps, cin, N]"""
    W = GE.f64(W)
    taps, cin, N = W.shape
    Weff = np.zeros((hop * (taps - 1) + cin, N))
    for j in range(taps):
        Weff[hop * j:hop * j + cin] += W[j]
    return Weff


def unfold(dWeff, taps, cin, hop):
    """dW[taps, cin, N]: every tap row takes the gradient of the sample it multiplies"""
    return np.stack([dWeff[hop * j:hop * j + cin] for j in range(taps)])


def inputs(name, exact):
    """x[B, x_len], W[taps, cin, 128], G[M, 128]: ternary (drawn as gemm_exact.ternary draws) or random floats"""
    c = CASES[name]
    rng = np.random.RandomState(11 + sorted(CASES).index(name) + (0 if exact else 100))
    M = rows_of(c)
    if exact:
        return GE.ternary(rng, c["B"], c["x_len"]), GE.ternary(rng, c["taps"], c["cin"], NOUT), GE.ternary(rng, M, NOUT)
    return ((rng.randn(c["B"], c["x_len"]) * 0.1).astype(np.float32), (rng.randn(c["taps"], c["cin"], NOUT) * 0.1).astype(np.float32),
            (rng.randn(M, NOUT) * 0.1).astype(np.float32))


@functools.lru_cache(maxsize=2)
def reference(name, exact):
    """the inputs of a case and its float64 results, computed once and shared: dict(x, W, G, A, Weff, C, dWeff, dW).  Callers
    must not change the arrays."""
    c = CASES[name]
    x, W, G = inputs(name, exact)
    A = toeplitz(x, folded_desc(c))
    Weff = fold(W, c["hop"])
    assert Weff.shape == (KF, NOUT)
    C = A @ Weff
    dWeff = A.T @ GE.f64(G)
    out = dict(x=x, W=W, G=G, A=A, Weff=Weff, C=C, dWeff=dWeff, dW=unfold(dWeff, c["taps"], c["cin"], c["hop"]))
    for v in out.values():
        v.setflags(write=False)
    return out


def x_with_slack(x, c):
    """[B, x_batch_stride]: the clips as the device sees them, SLACK between x_len and x_batch_stride"""
    out = np.full((c["B"], c["x_batch_stride"]), SLACK, np.float32)
    out[:, :c["x_len"]] = x
    return out


# kws_conv1_supported(folded, unfolded, N): (changes to the folded descriptor, changes to the unfolded one, N) -> accepted
_F0 = folded_desc(CASES["B1"])
_U0 = unfolded_desc(CASES["B1"])
SUPPORTED_TABLE = [
    (dict(), dict(), 128, True),                                       # the net's own pair
    (dict(), dict(taps=1, cin=80, stride_j=0), 128, True),             # an already folded kernel
    (dict(), dict(taps=2, cin=60, stride_j=20), 128, True),
    (dict(), dict(taps=2, cin=40, stride_j=40), 128, True),            # taps that do not overlap
    (dict(), dict(taps=3, cin=80, stride_j=0), 128, True),             # three taps on the same samples
    (dict(x_len=1533, x_batch_stride=1534, base_off=-6, stride_t=42), dict(), 128, True),
    (dict(), dict(), 256, False),                                      # filter_mult 2
    (dict(), dict(), 64, False),
    (dict(stride_t=41), dict(), 128, False),                           # 8-byte staging loads
    (dict(base_off=-9), dict(), 128, False),
    (dict(x_batch_stride=16001), dict(), 128, False),
    (dict(), dict(taps=4, cin=20, stride_j=20), 128, False),           # the fold-on-load prologue has three candidates
    (dict(), dict(taps=0), 128, False),
    (dict(cin=120), dict(), 128, False),                               # folded cin != 80
    (dict(cin=40), dict(), 128, False),
    (dict(taps=3), dict(), 128, False),                                # the first descriptor is not a folded one
    (dict(L_out=0), dict(), 128, False),
    # the unfolded taps must span the 80 folded samples exactly, hop >= 0
    (dict(), dict(taps=3, cin=40, stride_j=25), 128, False),           # 90 samples: weights dropped, slab rows 80 .. 89 read
    (dict(), dict(taps=3, cin=40, stride_j=10), 128, False),           # 60 samples
    (dict(), dict(taps=1, cin=40, stride_j=0), 128, False),
    (dict(), dict(taps=2, cin=120, stride_j=-40), 128, False),         # spans 80 on paper, with a negative hop
    (dict(), dict(taps=1, cin=80, stride_j=-20), 128, False),
]


def supported_args(row):
    return dict(_F0, **row[0]), dict(_U0, **row[1]), row[2], row[3]
