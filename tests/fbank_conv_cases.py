"""Shared by tests/test_learned_spec_cpu.py and tests/test_fbank_conv_kernels_gpu.py: the cases, the float64 references and a
Python restatement of the host planner of the banked strided first convolution (csrc/fbank_conv.hip: kws_fbank_conv_fwd_f32,
kws_fbank_conv_wgrad_f32, kws_fbank_conv_wgrad_workspace_floats).

The references are written from the definition of the operation, bank by bank - the windows of a bank are built and contracted
with that bank's kernel - not from the kernels' view of one banded product over a staged segment:

    F_q[b, t, c] = x[b, stride t + c - pad_l[q]]        0 where the sample lies outside [0, L)                  windows()
    y[b, t, q N + n] = sum_c F_q[b, t, c] W_q[c, n]
    dW_q[c, n]       = sum_{b, t} F_q[b, t, c] G[b, t, q N + n]

The exact runs use integer x, W and G in [-3, 3]: every product and partial sum is an integer below 512 * 9 (forward) or
M * 9 (weight gradient) < 2^24, so float32 is exact in any order (premise(), from the float64 reference: a condition of the test,
not a tolerance)."""
import functools

import numpy as np

TM = 112           # rows per workgroup tile at most: a tile never spans two clips
TPG = 288          # accumulator tiles of the weight gradient per workgroup (16 waves x 18)
WG_SLABS = 256     # weight-gradient workgroups = slabs at most
PER_GROUP = 16     # slabs per group of the two-stage slab sum
MAX_SPAN = 512
MAX_STRIDE = 4096
SEG_FLOATS = 36 * 1024
LDS_TAB = 128 + TPG
SLACK = 1000.0     # what the GPU test writes between L and x_batch_stride: a read past L changes an integer
MODEL_BANKS = (479, 383, 319, 255, 191, 161)


def ceil_div(a, b):
    return -(-a // b)


def same_geometry(L, stride, ksizes):
    """(Lout, [pad_l]) of Conv1D(k, strides=stride, padding='same') per bank: TensorFlow's rule"""
    Lout = ceil_div(L, stride)
    return Lout, [max((Lout - 1) * stride + k - L, 0) // 2 for k in ksizes]


def _case(B, L, slack, N, ksizes, stride=160, pads=None, Lout=None, corners=()):
    same_Lout, same_pads = same_geometry(L, stride, ksizes)
    return dict(B=B, L=L, Lout=same_Lout if Lout is None else Lout, stride=stride, nbanks=len(ksizes), N=N, ksize=list(ksizes),
                pad_l=list(same_pads if pads is None else pads), x_batch_stride=L + slack, corners=set(corners))


def rows_of(c):
    return c["B"] * c["Lout"]


def F_of(c):
    return c["nbanks"] * c["N"]


def span_of(c):
    return max(k - p for k, p in zip(c["ksize"], c["pad_l"])) + max(c["pad_l"])


# ---------------------------------------------------------------------------------------------------------------------------
# the planner, restated
# ---------------------------------------------------------------------------------------------------------------------------
def in_domain(c):
    if min(c["B"], c["L"], c["Lout"]) < 1 or c["stride"] < 2 or c["stride"] % 2 or c["stride"] > MAX_STRIDE:
        return False
    if not 1 <= c["nbanks"] <= 8 or c["N"] % 4 or not 4 <= c["N"] <= 64:
        return False
    if c["x_batch_stride"] < c["L"] or c["x_batch_stride"] % 2:
        return False
    ks, pads = c["ksize"][:c["nbanks"]], c["pad_l"][:c["nbanks"]]
    if any(k < 1 or k > MAX_SPAN or p < 0 or p >= k for k, p in zip(ks, pads)):
        return False
    if max(k - p for k, p in zip(ks, pads)) + max(pads) > MAX_SPAN:
        return False
    return c["stride"] * (c["Lout"] - 1) < c["L"] + max(pads) and c["B"] * c["Lout"] < 2 ** 31


def plan(c):
    """what fb_fill derives: dict(pade, off, k0, k1, tile0, T, kstage, padw, P, R, tpc, tiles, S, lds_bytes)"""
    N, F = c["N"], F_of(c)
    pade = (max(c["pad_l"]) + 1) & ~1
    off = [pade - p for p in c["pad_l"]]
    k0, k1, tile0, T, kstage = [], [], [], 0, 0
    for ct in range(ceil_div(F, 16)):
        c0, c1 = ct * 16, min(ct * 16 + 16, F)
        banks = [q for q in range(c["nbanks"]) if q * N < c1 and (q + 1) * N > c0]
        lo = min(off[q] for q in banks) & ~3
        hi = (max(off[q] + c["ksize"][q] for q in banks) + 3) & ~3
        nt = ceil_div(hi - lo, 16)
        k0.append(lo), k1.append(hi), tile0.append(T)
        T += nt
        kstage = max(kstage, lo + 16 * nt)
    padw = 4 if c["stride"] % 32 == 0 else 0
    P = c["stride"] + padw
    fit = 1 + (SEG_FLOATS - kstage - (kstage // c["stride"] + 2) * padw - 8) // P
    R = min(TM, c["Lout"], max(fit, 1))
    tpc = ceil_div(c["Lout"], R)
    tiles = c["B"] * tpc
    npos = (R - 1) * c["stride"] + kstage
    return dict(pade=pade, off=off, k0=k0, k1=k1, tile0=tile0, T=T, kstage=kstage, padw=padw, P=P, R=R, tpc=tpc, tiles=tiles,
                S=min(tiles, WG_SLABS), lds_bytes=4 * (LDS_TAB + npos + (npos // c["stride"] + 1) * padw + 8))


def workspace_floats(c):
    if not in_domain(c):
        return 0
    p = plan(c)
    return p["S"] * p["T"] * 256


# ---------------------------------------------------------------------------------------------------------------------------
# cases
# ---------------------------------------------------------------------------------------------------------------------------
CASES = {
    # the model's layer: 100 rows per clip = six whole MFMA row tiles and one of 4 rows; 288 accumulator tiles; LDS above 64 KB
    "model_B2": _case(2, 16000, 0, 40, MODEL_BANKS,
                      corners={"model_banks", "overhang_front", "overhang_back", "ragged_row_tile", "straddling_tile",
                               "lds_padding", "lds_opt_in", "odd_pad"}),
    # a clip shorter than two spans: 4 rows, the widest window overhangs in rows 0 and 3 and ends on the last sample in row 2
    "short_clip": _case(3, 640, 6, 40, MODEL_BANKS,
                        corners={"clip_below_two_spans", "batch_stride_slack", "below_one_row_tile"}),
    # L no multiple of the stride: 7 rows, pads 219, 171, 139, 107, 75, 60 from the TF rule
    "L1000": _case(2, 1000, 2, 40, MODEL_BANKS, corners={"L_not_multiple_of_stride", "even_pad"}),
    # one bank, VALID: a single column tile of 8 columns and the smallest K
    "one_bank": _case(2, 800, 0, 8, (161,), pads=[0], Lout=4, corners={"one_bank", "narrow_column_tile", "no_pad"}),
    # two banks at N 16: column tiles on the bank borders
    "two_banks_n16": _case(2, 800, 0, 16, (319, 161), corners={"tiles_on_bank_borders"}),
    # two banks at N 40, the widest against the narrowest: tile 2 straddles K ranges [0, 480) and [160, 321)
    "two_banks_n40": _case(2, 640, 0, 40, (479, 161), corners={"straddle_widest_narrowest"}),
    # eight banks at N 4: a column tile holds four banks; stride 2, no LDS padding
    "eight_banks": _case(3, 50, 2, 4, (3, 4, 5, 6, 7, 8, 9, 10), stride=2,
                         corners={"eight_banks", "stride=2", "no_lds_padding", "four_banks_per_tile"}),
    # 259 clips of 2 rows: 3 weight-gradient workgroups take a second clip; 16 slab groups
    "batch_wraps": _case(259, 320, 0, 16, (161, 63), corners={"wg_second_tile", "many_slab_groups"}),
    # 130 rows per clip: two row tiles (112 + 18)
    "two_row_tiles": _case(1, 20800, 0, 16, (191, 161), corners={"two_row_tiles"}),
    # 8 banks x 64 filters x 200 taps: 416 accumulator tiles, a second tile part in the weight gradient's grid
    "second_part": _case(1, 640, 0, 64, (200,) * 8, corners={"second_tile_part", "widest_output"}),
    # stride 4096: the LDS budget cuts a tile to 9 rows
    "long_stride": _case(1, 4096 * 12, 0, 4, (33,), stride=4096, corners={"rows_cut_by_lds"}),
    # the widest union window: span 512 from a 512-tap bank with an odd front pad beside a short one
    "span512": _case(2, 640, 0, 8, (512, 5), pads=[255, 2], Lout=4, corners={"span=512"}),
}
FLOAT_CASES = {"float_B1": _case(1, 16000, 0, 40, MODEL_BANKS), "float_B4": _case(4, 16000, 0, 40, MODEL_BANKS),
               "float_L15000": _case(2, 15000, 0, 40, MODEL_BANKS)}
CORNERS = {"model_banks", "overhang_front", "overhang_back", "ragged_row_tile", "straddling_tile", "lds_padding", "lds_opt_in",
           "odd_pad", "even_pad", "no_pad", "clip_below_two_spans", "batch_stride_slack", "below_one_row_tile",
           "L_not_multiple_of_stride", "one_bank", "narrow_column_tile", "tiles_on_bank_borders", "straddle_widest_narrowest",
           "eight_banks", "stride=2", "no_lds_padding", "four_banks_per_tile", "wg_second_tile", "many_slab_groups", "two_row_tiles",
           "second_tile_part", "widest_output", "rows_cut_by_lds", "span=512"}


def edges(c):
    """the corners of the kernels' walks that case c reaches"""
    out, p = set(), plan(c)
    N, F, s = c["N"], F_of(c), c["stride"]
    ks, pads = c["ksize"], c["pad_l"]
    if tuple(ks) == MODEL_BANKS:
        out.add("model_banks")
    if max(pads) > 0:
        out.add("overhang_front")
    if any(s * (c["Lout"] - 1) + k - q > c["L"] for k, q in zip(ks, pads)):
        out.add("overhang_back")
    if min(p["R"], c["Lout"]) % 16:
        out.add("ragged_row_tile")
    if c["Lout"] < 16:
        out.add("below_one_row_tile")
    straddles = [ct for ct in range(ceil_div(F, 16)) if (ct * 16) // N != (min(ct * 16 + 16, F) - 1) // N]
    if straddles:
        out.add("straddling_tile")
    else:
        out.add("tiles_on_bank_borders" if c["nbanks"] > 1 else "one_bank")
    if any((min(ct * 16 + 16, F) - 1) // N - (ct * 16) // N == 3 for ct in straddles):
        out.add("four_banks_per_tile")
    if c["nbanks"] == 2 and straddles and sorted(ks) == [161, 479]:
        out.add("straddle_widest_narrowest")
    out.add("lds_padding" if p["padw"] else "no_lds_padding")
    if p["lds_bytes"] > 64 * 1024:
        out.add("lds_opt_in")
    if any(q % 2 for q in pads):
        out.add("odd_pad")
    if any(q and q % 2 == 0 for q in pads):
        out.add("even_pad")
    if max(pads) == 0:
        out.add("no_pad")
    if c["L"] < 2 * span_of(c):
        out.add("clip_below_two_spans")
    if c["x_batch_stride"] > c["L"]:
        out.add("batch_stride_slack")
    if c["L"] % s:
        out.add("L_not_multiple_of_stride")
    if F < 16:
        out.add("narrow_column_tile")
    if c["nbanks"] == 8:
        out.add("eight_banks")
    if F == 512:
        out.add("widest_output")
    out.add("stride=%d" % s)
    if p["tiles"] > WG_SLABS:
        out.add("wg_second_tile")
    if p["S"] > PER_GROUP:
        out.add("many_slab_groups")
    if p["tpc"] > 1 and p["R"] == TM:
        out.add("two_row_tiles")
    if p["T"] > TPG:
        out.add("second_tile_part")
    if p["R"] < min(TM, c["Lout"]):
        out.add("rows_cut_by_lds")
    out.add("span=%d" % span_of(c))
    return out


def desc_fields(c, w_off=None):
    """the members of kws_fbank_conv_t, in the header's order; w_off defaults to the banks packed back to back"""
    if w_off is None:
        w_off = packed_offsets(c)
    pad8 = lambda v: (list(v) + [0] * 8)[:8]
    return [("B", c["B"]), ("L", c["L"]), ("Lout", c["Lout"]), ("stride", c["stride"]), ("nbanks", c["nbanks"]), ("N", c["N"]),
            ("ksize", pad8(c["ksize"])), ("pad_l", pad8(c["pad_l"])), ("w_off", pad8(w_off)), ("x_batch_stride", c["x_batch_stride"])]


DESC_MEMBERS = ["B", "L", "Lout", "stride", "nbanks", "N", "ksize", "pad_l", "w_off", "x_batch_stride"]


def packed_offsets(c):
    return [int(v) for v in np.cumsum([0] + [k * c["N"] for k in c["ksize"][:-1]])]


def dense_fold_gather(c):
    """the same layer as a gather of the generic GEMMs over a dense zero-padded fold [span8, F]: kws_gather_t members"""
    span8 = ceil_div(span_of(c), 8) * 8
    return dict(L_out=c["Lout"], cin=span8, taps=1, stride_t=c["stride"], stride_j=0, base_off=-max(c["pad_l"]), x_len=c["L"],
                x_batch_stride=c["x_batch_stride"])


# ---------------------------------------------------------------------------------------------------------------------------
# references
# ---------------------------------------------------------------------------------------------------------------------------
def windows(x, c, q):
    """float64 F_q[B * Lout, ksize[q]] of clips x[B, L]"""
    x = np.asarray(x, dtype=np.float64)
    assert x.shape == (c["B"], c["L"])
    pos = c["stride"] * np.arange(c["Lout"])[:, None] + np.arange(c["ksize"][q])[None, :] - c["pad_l"][q]
    inside = (pos >= 0) & (pos < c["L"])
    return np.where(inside[None], x[:, np.where(inside, pos, 0)], 0.0).reshape(rows_of(c), c["ksize"][q])


def inputs(c, seed, exact):
    """x[B, L], [W_q[ksize_q, N]], G[M, F]: integers in [-3, 3] or random normal floats"""
    rng = np.random.RandomState(seed)
    shapes = [(c["B"], c["L"])] + [(k, c["N"]) for k in c["ksize"]] + [(rows_of(c), F_of(c))]
    if exact:
        a = [rng.randint(-3, 4, size=s).astype(np.float32) for s in shapes]
    else:
        a = [(rng.randn(*s) * 0.1).astype(np.float32) for s in shapes]
    return a[0], a[1:-1], a[-1]


@functools.lru_cache(maxsize=2)
def reference(name, exact):
    """the inputs of a case and its float64 results, computed once and shared: dict(x, W, G, y, dW, abs_y, abs_dW); abs_*: the
    same sums over absolute values (the error bounds of the float runs).  Callers must not change the arrays."""
    table = CASES if exact else FLOAT_CASES
    c = table[name]
    x, W, G = inputs(c, 41 + sorted(table).index(name) + (0 if exact else 100), exact)
    N = c["N"]
    G64 = np.asarray(G, dtype=np.float64)
    y, dW, abs_y, abs_dW = [], [], [], []
    for q in range(c["nbanks"]):
        Fq, Wq, Gq = windows(x, c, q), np.asarray(W[q], dtype=np.float64), G64[:, q * N:(q + 1) * N]
        y.append(Fq @ Wq)
        dW.append(Fq.T @ Gq)
        abs_y.append(np.abs(Fq) @ np.abs(Wq))
        abs_dW.append(np.abs(Fq).T @ np.abs(Gq))
    out = dict(x=x, G=G, y=np.concatenate(y, axis=1), abs_y=np.concatenate(abs_y, axis=1))
    for v in list(out.values()) + W + dW + abs_dW:
        v.setflags(write=False)
    out.update(W=tuple(W), dW=tuple(dW), abs_dW=tuple(abs_dW))
    return out


def premise(r):
    """every sum of absolute values stays below 2^24: float32 is exact in any order"""
    assert np.array_equal(r["y"], np.rint(r["y"]))
    assert r["abs_y"].max() < 2 ** 24 and max(a.max() for a in r["abs_dW"]) < 2 ** 24


def x_with_slack(x, c):
    """[B, x_batch_stride]: the clips as the device sees them, SLACK between L and x_batch_stride"""
    out = np.full((c["B"], c["x_batch_stride"]), SLACK, np.float32)
    out[:, :c["L"]] = x
    return out


# descriptors the library must refuse: changes to the model's case -> why
_C0 = _case(2, 16000, 0, 40, MODEL_BANKS)
REFUSED = [
    (dict(nbanks=0), "no banks"),
    (dict(nbanks=9), "nine banks"),
    (dict(ksize=[479, 383, 0, 255, 191, 161]), "a bank without taps"),
    (dict(pad_l=[159, 111, 79, 47, 15, 161]), "pad_l = ksize"),
    (dict(pad_l=[159, 111, 79, 47, -1, 0]), "a negative pad_l"),
    (dict(N=42), "N no multiple of 4"),
    (dict(N=68), "N above 64"),
    (dict(stride=161), "an odd stride"),
    (dict(stride=0), "no stride"),
    (dict(ksize=[479, 383, 319, 255, 191, 400], pad_l=[159, 111, 79, 47, 15, 0]), "span 559"),
    (dict(ksize=[513, 383, 319, 255, 191, 161]), "a bank of 513 taps"),
    (dict(x_batch_stride=15998), "x_batch_stride below L"),
    (dict(x_batch_stride=16001), "an odd x_batch_stride"),
    (dict(Lout=102), "rows past the padded clip"),
    (dict(B=0), "an empty batch"),
]


def refused(changes):
    c = dict(_C0, **changes)
    n = max(c["nbanks"], 0)
    c["ksize"] = (list(c["ksize"]) + [1] * 8)[:max(n, len(c["ksize"]))]
    c["pad_l"] = (list(c["pad_l"]) + [0] * 8)[:max(n, len(c["pad_l"]))]
    return c
