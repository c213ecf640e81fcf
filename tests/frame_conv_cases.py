"""Shared by tests/test_time_sliced_cpu.py and tests/test_frame_conv_kernels_gpu.py: the cases, the float64 references and a
Python restatement of the two host planners of the framed first convolution at narrow widths (csrc/frame_conv.hip:
kws_frame_conv_fwd_f32, kws_frame_conv_wgrad_f32).

The references are written from the definition of the operation - the frames are built, tap by tap, and contracted with the
UNFOLDED kernel - not from the kernels' folded Toeplitz view:

    F[b, t, j, c] = x[b, hop (stride t + j) + c - pad_l]       0 where the sample lies outside [0, L)                  frames()
    y[b, t, n]    = sum_{j, c} F[b, t, j, c] W[j, c, n]
    dW[j, c, n]   = sum_{b, t} F[b, t, j, c] G[b, t, n]

The geometry of a case follows from (L, ksize, hop, taps, stride) as the reference model builds it: overlapping_time_slice_stack
with SAME padding (ceil(L / hop) frames, the odd padding sample behind the clip), then a VALID Conv1D over the frames.

The exact runs use gemm_exact.py's method: ternary x, W and G make every product and partial sum an integer; premise_* assert
from the float64 reference that the sums stay below 2^24 (a condition of the test, not a tolerance)."""
import functools

import numpy as np

import gemm_exact as GE

TM = 64            # rows per tile: a tile never spans two clips
FWD_WGS = 1024     # persistent forward workgroups = statistics rows at most
WG_WGS = 1024      # persistent weight-gradient workgroups = slabs at most
MAX_SPAN = 128
SLACK = 1000.0     # what the GPU test writes between L and x_batch_stride: a read past L changes an integer


def ceil_div(a, b):
    return -(-a // b)


def same_frames(L, ksize, hop):
    """(frames, pad_l) of overlapping_time_slice_stack(x, ksize, hop, 'SAME')"""
    frames = ceil_div(L, hop)
    pad = max((frames - 1) * hop + ksize - L, 0)
    return frames, pad // 2


def _case(B, L, slack, N, ksize=40, hop=20, taps=3, stride=2, corners=()):
    frames, pad_l = same_frames(L, ksize, hop)
    return dict(B=B, L=L, Lout=(frames - taps) // stride + 1, ksize=ksize, hop=hop, pad_l=pad_l, taps=taps, stride=stride, N=N,
                x_batch_stride=L + slack, corners=set(corners))


def span_of(c):
    return c["hop"] * (c["taps"] - 1) + c["ksize"]


def rows_of(c):
    return c["B"] * c["Lout"]


def tiles_of(c):
    return c["B"] * ceil_div(c["Lout"], TM)


# ---------------------------------------------------------------------------------------------------------------------------
# the planners, restated
# ---------------------------------------------------------------------------------------------------------------------------
def stats_rows(c):
    return min(tiles_of(c), FWD_WGS)


def workspace_floats(c):
    return min(tiles_of(c), WG_WGS) * span_of(c) * c["N"]


def in_domain(c):
    span = span_of(c)
    if c["N"] not in (32, 64) or min(c["B"], c["L"], c["Lout"], c["ksize"], c["hop"], c["taps"]) < 1 or c["stride"] not in (1, 2):
        return False
    if span > MAX_SPAN or c["hop"] % 2 or c["pad_l"] % 2 or c["pad_l"] < 0 or c["x_batch_stride"] % 2 or c["x_batch_stride"] < c["L"]:
        return False
    return c["hop"] * (c["stride"] * (c["Lout"] - 1) + c["taps"] - 1) + c["ksize"] - c["pad_l"] <= c["L"] + span


# ---------------------------------------------------------------------------------------------------------------------------
# cases: ksize 40, hop 20, taps 3, stride 2 (the model's front end) unless said otherwise, each at N = 32 and N = 64
# ---------------------------------------------------------------------------------------------------------------------------
def _both(name, *args, **kw):
    return {"%s_n%d" % (name, N): _case(*args, N=N, **kw) for N in (32, 64)}


CASES = {}
# L 1600: 39 rows per clip, pad_l 10.  B 3: M = 117, less than one 128-row tile of the generic kernel; B 4: M = 156, one and a ragged one
CASES.update(_both("L1600_B3", 3, 1600, 0, corners={"clip_below_one_tile", "clip_start_overhang"}))
CASES.update(_both("L1600_B4", 4, 1600, 6, corners={"clip_below_one_tile", "batch_stride_slack"}))
# L 1604: pad_l 18, 40 rows per clip; the last row reads samples 1542 .. 1621 of 1604
CASES.update(_both("L1604_B2", 2, 1604, 6, corners={"clip_start_overhang", "clip_end_overhang", "batch_stride_slack"}))
# one clip of the model's length: 399 rows = six whole tiles and one of 15 rows (odd: the weight gradient's last step is half empty)
CASES.update(_both("L16000_B1", 1, 16000, 0, corners={"whole_tiles", "ragged_odd_tile"}))
# stride 1: 78 rows per clip at a row pitch of 20 samples = one whole tile and one of 14 rows
CASES.update(_both("stride1", 3, 1600, 2, stride=1, corners={"stride=1", "ragged_even_tile"}))
# two taps: span 60, padded to 64 in the kernels (four zero weight rows behind real samples)
CASES.update(_both("two_taps", 3, 1600, 2, taps=2, corners={"taps=2", "span_padded"}))
# the sizes at which the kernels take another path
# rows that do not overlap (row pitch 40 > span 8): staged row by row, not as one segment
CASES.update(_both("no_overlap", 3, 1604, 2, ksize=8, taps=1, corners={"rows_staged_one_by_one", "taps=1"}))
# the widest span: 128 samples (with N = 64 the launch asks for exactly 64 KB of LDS); four k blocks in the weight gradient
CASES.update(_both("span128", 2, 1600, 0, ksize=48, hop=40, stride=1, corners={"span=128"}))
# the staged samples of a tile pass through registers, 8 or 16 pairs per thread: more than 4096 floats take the deeper kernels,
# as one segment (row pitch 80 = span 80: 5120 floats) and row by row (pitch 80 > span 72: 4608 floats); 80 rows per clip
CASES.update(_both("deep_segment", 2, 6400, 0, hop=40, taps=2, corners={"prefetch_16_segment"}))
CASES.update(_both("deep_rows", 1, 6400, 2, ksize=72, hop=80, taps=1, stride=1, corners={"prefetch_16_rows"}))
# 150 clips = 1050 tiles: 26 workgroups of either kernel take a second tile; 32 slab groups
CASES["many_tiles_n32"] = _case(150, 16000, 0, N=32, corners={"fwd_second_tile", "wg_second_tile", "many_slab_groups"})
EXACT_CASES = list(CASES)
FLOAT_CASES = {"float_B1_n%d" % N: _case(1, 16000, 0, N=N) for N in (32, 64)}
FLOAT_CASES.update({"float_B5_n%d" % N: _case(5, 16000, 0, N=N) for N in (32, 64)})
CORNERS = {"clip_below_one_tile", "clip_start_overhang", "clip_end_overhang", "batch_stride_slack", "whole_tiles", "ragged_odd_tile",
           "ragged_even_tile", "stride=1", "taps=1", "taps=2", "span_padded", "rows_staged_one_by_one", "span=128", "fwd_second_tile",
           "wg_second_tile", "many_slab_groups", "prefetch_16_segment", "prefetch_16_rows"}
FEW_FLOATS = 4096  # staged floats of a whole tile up to which the 8-pairs-per-thread kernels run


def edges(c):
    """the corners of the kernels' walks that case c reaches"""
    out = set()
    span, pitch = span_of(c), c["hop"] * c["stride"]
    kp = ceil_div(span, 8) * 8
    if c["Lout"] < TM:
        out.add("clip_below_one_tile")
    if c["Lout"] >= TM:
        out.add("whole_tiles")
    if c["Lout"] % TM:
        out.add("ragged_odd_tile" if (c["Lout"] % TM) % 2 else "ragged_even_tile")
    if c["pad_l"] > 0:
        out.add("clip_start_overhang")
    if pitch * (c["Lout"] - 1) + span - c["pad_l"] > c["L"]:
        out.add("clip_end_overhang")
    if c["x_batch_stride"] > c["L"]:
        out.add("batch_stride_slack")
    out.add("stride=%d" % c["stride"])
    out.add("taps=%d" % c["taps"])
    if kp > span:
        out.add("span_padded")
    if pitch > kp:
        out.add("rows_staged_one_by_one")
    if span == MAX_SPAN:
        out.add("span=128")
    staged = TM * kp if pitch > kp else (TM - 1) * pitch + kp
    if staged > FEW_FLOATS and c["Lout"] >= TM:          # a whole tile: pairs 8 .. 15 of a thread are in use
        out.add("prefetch_16_rows" if pitch > kp else "prefetch_16_segment")
    if tiles_of(c) > FWD_WGS:
        out.add("fwd_second_tile")
    if tiles_of(c) > WG_WGS:
        out.add("wg_second_tile")
    if min(tiles_of(c), WG_WGS) > 32:
        out.add("many_slab_groups")
    return out


def desc_fields(c):
    """the members of kws_frame_conv_t"""
    return {k: c[k] for k in ("B", "L", "Lout", "ksize", "hop", "pad_l", "taps", "stride", "N", "x_batch_stride")}


def folded_gather(c):
    """the same operation as a gather of the generic GEMMs: ONE tap of `span` samples (kws_gather_t members)"""
    return dict(L_out=c["Lout"], cin=span_of(c), taps=1, stride_t=c["hop"] * c["stride"], stride_j=0, base_off=-c["pad_l"],
                x_len=c["L"], x_batch_stride=c["x_batch_stride"])


# ---------------------------------------------------------------------------------------------------------------------------
# references
# ---------------------------------------------------------------------------------------------------------------------------
def frames(x, c):
    """float64 F[B, Lout, taps, ksize] of clips x[B, L]"""
    x = GE.f64(x)
    assert x.shape == (c["B"], c["L"])
    t = np.arange(c["Lout"])[:, None, None]
    j = np.arange(c["taps"])[None, :, None]
    k = np.arange(c["ksize"])[None, None, :]
    pos = c["hop"] * (c["stride"] * t + j) + k - c["pad_l"]
    inside = (pos >= 0) & (pos < c["L"])
    return np.where(inside[None], x[:, np.where(inside, pos, 0)], 0.0)


def fold32(W, c):
    """the folded kernel [span, N] in float32, taps added in ascending order: what the generic path's fold_taps gives"""
    out = np.zeros((span_of(c), c["N"]), np.float32)
    for j in range(c["taps"]):
        out[c["hop"] * j:c["hop"] * j + c["ksize"]] += W[j]
    return out


def unfold(dWeff, c):
    return np.stack([dWeff[c["hop"] * j:c["hop"] * j + c["ksize"]] for j in range(c["taps"])])


def inputs(c, seed, exact):
    """x[B, L], W[taps, ksize, N], G[M, N]: ternary or random normal floats"""
    rng = np.random.RandomState(seed)
    shapes = (c["B"], c["L"]), (c["taps"], c["ksize"], c["N"]), (rows_of(c), c["N"])
    if exact:
        return tuple(GE.ternary(rng, *s) for s in shapes)
    return tuple((rng.randn(*s) * 0.1).astype(np.float32) for s in shapes)


@functools.lru_cache(maxsize=2)
def reference(name, exact):
    """the inputs of a case and its float64 results, computed once and shared: dict(x, W, G, y, dW).  Callers must not change
    the arrays."""
    table = CASES if exact else FLOAT_CASES
    c = table[name]
    x, W, G = inputs(c, 23 + sorted(table).index(name) + (0 if exact else 100), exact)
    F = frames(x, c).reshape(rows_of(c), c["taps"] * c["ksize"])
    y = F @ GE.f64(W).reshape(-1, c["N"])
    dW = (F.T @ GE.f64(G)).reshape(c["taps"], c["ksize"], c["N"])
    out = dict(x=x, W=W, G=G, F=F, y=y, dW=dW)
    for v in out.values():
        v.setflags(write=False)
    return out


def x_with_slack(x, c):
    """[B, x_batch_stride]: the clips as the device sees them, SLACK between L and x_batch_stride"""
    out = np.full((c["B"], c["x_batch_stride"]), SLACK, np.float32)
    out[:, :c["L"]] = x
    return out


# descriptors the library must refuse: changes to the first case -> why
_C0 = _case(3, 1600, 0, N=32)
REFUSED = [
    (dict(N=48), "N is 32 or 64"),
    (dict(N=128), "N is 32 or 64"),
    (dict(pad_l=9), "odd pad_l"),
    (dict(ksize=89), "span 129"),
    (dict(hop=21), "odd hop"),
    (dict(x_batch_stride=1601), "odd x_batch_stride"),
    (dict(x_batch_stride=1598), "x_batch_stride below L"),
    (dict(stride=3), "stride 3"),
    (dict(taps=0), "no taps"),
    (dict(Lout=45), "rows past the padded clip"),
    (dict(B=0), "an empty batch"),
]


def refused(changes):
    return dict(_C0, **changes)
