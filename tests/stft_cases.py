"""Shared by tests/test_stft_cases_cpu.py and tests/test_stft_kernels_gpu.py: the plans, clip lengths, batches, inputs,
float64 references and bars of the direct tests of kws_stft_mel_f32 (csrc/stft.hip: the generic kernel in a 4-wave and a
7-wave form; csrc/stft4.hip: the register-FFT kernel in four mel-shape instances, each with 16-byte and 8-byte PCM loads),
and a NumPy restatement of the host arithmetic that chooses between them (kws_stft_plan_create's band tables,
stft4_shape, kws_stft_mel_kernel).  TEST INFRASTRUCTURE ONLY.

Every plan carries the kernel it is in the table for (`shape`: 0 = generic, 1..4 = the stft4 instance).  The CPU test
asserts the restatement lands every plan there; the GPU test asserts the library's own answer (kws_stft_mel_kernel) before
it compares anything, so a change to a table or to the dispatch cannot move a case onto another path unnoticed.

References: oracle.features.features(..., dtype=np.float64, return_all=True), unchanged (checked against a direct O(N^2)
DFT in the CPU test).

Bars (one place; origin beside each):
  MAG_BAR, LOGMEL_BAR   tests/test_kernels_gpu.py::test_stft_mel_features: twice the error measured in round 4 on this
                        input family (0.0774 randn + 0.05 sin 440 Hz), on both kernels and all shipped plan shapes
  logmel_bar()          LOGMEL_BAR per element, plus - at the 0.03 % of the elements where a band is nearly empty in a frame - what
                        half an ulp of the frame's largest bin becomes through d log(s) = ds / s (the float64 argument is there)
  mfcc_bar()            the log-mel bar through the DCT + the rounding of an n_mel-term f32 / split-f16 product chain
                        (9.3e-5 for path B 80 -> 60 and 1.04e-4 for path A 40 -> 40: test_stft_mel_features' 1.1e-4)
  chain_bar()           the generic kernel's DCT is f32 fma chains (four interleaved ones) of n_mel terms in all over the log-mel row
                        it stores at kind 2: at most n_mel roundings of at most 2^-24 of the running sums' bound
The error of a frame does not depend on F, B or the clip's position, so the bars transfer to every geometry below.

Worst measured error per stage and plan beside its bar: see the docstring of tests/test_stft_kernels_gpu.py."""
import functools
import zlib

import numpy as np

from oracle import features as OF

MAG_BAR = 2.3e-6       # |spectrogram - float64|, absolute
LOGMEL_BAR = 5e-6      # |log-mel - float64|, absolute

NBINS = 257
MAGF = 260             # floats of a magnitude row in stft4's LDS (stft.hip MAGF4, stft4.hip MAGF)
LDS_CAP = 160 * 1024
# four-tap blocks per lane group of the four stft4 instances (stft4.hip: stft4_shape / the MCP template argument)
SHAPES = {1: (1, 2, 2, 3, 4), 2: (4, 4, 4, 4, 4), 3: (2, 5, 8), 4: (8, 8, 8)}


# ---------------------------------------------------------------------------------------------------------------------------
# plans
# ---------------------------------------------------------------------------------------------------------------------------
def hand_tables():
    """P7: 40 triangles of 7 bins starting at bin 2 + 6 m; band 20 is 29 bins wide (122 .. 150), band 39 sits on bins
    250 .. 256 (weight on the Nyquist bin), band 5 is all zero.  Path B's window, DCT and log offset."""
    t = OF.tables_path_b(480, 40, 40)
    mel = np.zeros((NBINS, 40), np.float32)
    tri7 = np.array([1, 2, 3, 4, 3, 2, 1], np.float32) / 4
    for m in range(40):
        if m == 5:
            continue
        if m == 20:
            i = np.arange(29)
            mel[122:151, m] = np.minimum(i + 1, 29 - i).astype(np.float32) / 15
            continue
        lo = 250 if m == 39 else 2 + 6 * m
        mel[lo:lo + 7, m] = tri7
    return dict(t, mel=mel)


def _plan(tables, step, n_mel, n_out, shape, why):
    return dict(tables=tables, frame_len=len(tables["window"]), step=step, n_mel=n_mel, n_out=n_out, shape=shape, why=why)


@functools.lru_cache(maxsize=None)
def plan(name):
    """dict(tables, frame_len, step, n_mel, n_out, shape, why).  Callers must not change the tables."""
    B, A = OF.tables_path_b, OF.tables_path_a
    if name == "P1":
        return _plan(B(480, 80, 60), 160, 80, 60, 1, "the shipped form, f16 DCT image")
    if name == "P2":
        return _plan(B(480, 68, 40, lower_hz=300.0, upper_hz=8000.0), 160, 68, 40, 2,
                     "five lane groups at full width; 68 bands are no multiple of 16; the last band reaches bin 255")
    if name == "P3":
        return _plan(A(480, 16000, 40, 40), 160, 40, 40, 3, "log floor, f32 DCT table")
    if name == "P4":
        return _plan(B(480, 36, 36), 160, 36, 36, 4, "three lane groups at full width")
    if name == "P5":
        return _plan(A(480, 16000, 13, 40, lower=300.0, upper=8000.0), 160, 40, 13, 3,
                     "group 2 reads 32 taps where the plan has 28: the table image shifts the weights")
    if name == "P6":
        return _plan(B(400, 80, 60), 240, 80, 60, 1, "step != 160, window shorter than 480")
    if name == "P7":
        return _plan(hand_tables(), 160, 40, 40, 4, "host clamp of the tap window, weight on bin 256, an empty band")
    if name == "G1":
        return _plan(B(480, 80, 80), 160, 80, 80, 0, "n_out > 64")
    if name == "G2":
        return _plan(B(480, 78, 60), 160, 78, 60, 0, "n_mel % 4 != 0")
    if name == "G3":
        return _plan(B(479, 80, 60), 160, 80, 60, 0, "odd frame_len")
    if name == "G4":
        return _plan(B(480, 16, 10), 160, 16, 10, 0, "a 65-bin band: mel_maxw = 0")
    if name == "G5":
        return _plan(B(480, 128, 100), 160, 128, 100, 0, "the largest n_mel: 8 lane groups")
    raise KeyError(name)


PLANS = ["P1", "P2", "P3", "P4", "P5", "P6", "P7", "G1", "G2", "G3", "G4", "G5"]
FULL_GRID = ["P1", "P3", "G1"]               # every L x every B
ISOLATION_PLANS = ["P1", "P3", "P4", "G1"]   # clip isolation at B = 7, L = 1120 and 1122


def tables32(p):
    """the tables as the device holds them (float32), as float64 arrays: window, mel [257, n_mel], dct [n_mel, n_out]"""
    t = p["tables"]
    return tuple(np.asarray(t[k], np.float32).astype(np.float64) for k in ("window", "mel", "dct"))


# ---------------------------------------------------------------------------------------------------------------------------
# clip lengths and batches
# ---------------------------------------------------------------------------------------------------------------------------
# (L for window 480 / step 160, frames): 1122 has L % 4 == 2 (the 8-byte-load form of stft4), 1278 leaves 158 samples unused,
# F = 14 is one workgroup of the generic kernel's 7-wave form, F = 15 a ragged second workgroup of its 4-wave form
L_480 = [(480, 1), (640, 2), (800, 3), (960, 4), (1120, 5), (1122, 5), (1278, 5), (2560, 14), (2720, 15), (4800, 28)]
F_LIST = [f for _, f in L_480]
BATCHES = [1, 3, 7, 13]
# the batch each length gets on the plans outside FULL_GRID: B = 13 at F = 1 (13 one-frame quads), B = 7 at F = 5 (14 quads:
# two workgroups of 7 waves' worth), every batch size at least twice
SPARSE_B = {480: 13, 640: 3, 800: 7, 960: 1, 1120: 7, 1122: 7, 1278: 13, 2560: 3, 2720: 3, 4800: 1}
UNALIGNED_L, UNALIGNED_B = 1120, 3            # clips that start 8 bytes into a 16-byte line
PERSISTENT = ("P1", 1120, 1600)              # 3200 quads > 3072: 256 workgroups of 12.5 quads each (uneven q_lo / q_hi)


def length_for(p, L480):
    """the clip length of plan p that gives the same frame count as L480 does at window 480 / step 160, with the same L % 4
    and the same number of unused trailing samples where the step allows"""
    if (p["frame_len"], p["step"]) == (480, 160):
        return L480
    if p["step"] == 160:                      # G3, window 479: the same lengths give the same frame counts
        L = L480
    else:
        F = 1 + (L480 - 480) // 160
        L = p["frame_len"] + p["step"] * (F - 1) + (L480 - 480) % 160
    assert L % 2 == 0 and num_frames(p, L) == 1 + (L480 - 480) // 160 and L % 4 == L480 % 4
    return L


def num_frames(p, L):
    return 0 if L < p["frame_len"] else 1 + (L - p["frame_len"]) // p["step"]


def _cases():
    out = []
    for name in PLANS:
        p = plan(name)
        for L480, _ in L_480:
            for B in (BATCHES if name in FULL_GRID else [SPARSE_B[L480]]):
                out.append((name, length_for(p, L480), B, 0))
        out.append((name, length_for(p, UNALIGNED_L), UNALIGNED_B, 2))
    return out


# (plan, L, B, off): `off` floats between a 16-byte boundary and the first clip
CASES = _cases()


def case_id(c):
    return "%s-L%d-B%d%s" % (c[0], c[1], c[2], "-off%d" % c[3] if c[3] else "")


# ---------------------------------------------------------------------------------------------------------------------------
# inputs and references
# ---------------------------------------------------------------------------------------------------------------------------
SILENT, HALF_SILENT, SMALL, NEGATED = 1, 2, 3, 4     # the special rows (B >= 5: all four; B = 3: rows 0 .. 2 take the first three)


def special_rows(B):
    """{variant: row}"""
    if B >= 5:
        return {SILENT: 1, HALF_SILENT: 2, SMALL: 3, NEGATED: 4}
    if B == 3:
        return {SILENT: 0, HALF_SILENT: 1, SMALL: 2}
    return {}


def inputs(name, L, B):
    """float32 [B, L]: 0.0774 randn + 0.05 sin(2 pi 440 t), seeded from the case; one silent row, one whose first 60 % is
    digital silence (frames all zero, one partly zero), one scaled by 2^-10 (mel sums near the log offset), one that is
    row 0 times -1"""
    rng = np.random.RandomState(zlib.crc32(("%s/%d/%d" % (name, L, B)).encode()) & 0x7FFFFFFF)
    t = np.arange(L) / 16000.0
    x = (rng.randn(B, L) * 0.0774 + 0.05 * np.sin(2 * np.pi * 440 * t)[None]).astype(np.float32)
    rows = special_rows(B)
    if SILENT in rows:
        x[rows[SILENT]] = 0.0
    if HALF_SILENT in rows:
        x[rows[HALF_SILENT], :(6 * L) // 10] = 0.0
    if SMALL in rows:
        x[rows[SMALL]] *= np.float32(2.0 ** -10)
    if NEGATED in rows:
        x[rows[NEGATED]] = -x[0]
    return x


@functools.lru_cache(maxsize=4)
def reference(name, L, B):
    """dict(x, mag, logmel, mfcc): the inputs of a case and its float64 results.  Callers must not change the arrays."""
    p = plan(name)
    x = inputs(name, L, B)
    mag, logmel, mfcc = OF.features(x.astype(np.float64), p["tables"], p["step"], dtype=np.float64, return_all=True)
    out = dict(x=x, mag=mag, logmel=logmel, mfcc=mfcc)
    for v in out.values():
        v.setflags(write=False)
    return out


# ---------------------------------------------------------------------------------------------------------------------------
# bars
# ---------------------------------------------------------------------------------------------------------------------------
def logmel_bar(p, ref):
    """[B, F, n_mel] bar of |log-mel - float64|: LOGMEL_BAR, except at the elements where float32 cannot deliver it.

    The float64 argument.  Every butterfly of a float32 FFT adds numbers of the size of the frame's largest bin, so no output
    bin is known more exactly than one rounding of that peak, up to u_f = 2^-24 max_k |X_ref[f, k]| (a property of the number format,
    not of a kernel: scipy's complex64 rfft is no closer).  d log(s) = ds / s carries such an error of the band's bins to
        t[f, m] = u_f sum_k W[k, m] / (mel_ref[f, m] + offset)
    of log-mel error.  Where t <= LOGMEL_BAR the bar stands as it was set - that is 99.97 % of the elements of the case table
    and at least 99 % of every case, tests/test_stft_cases_cpu.py asserts both; where a band is so nearly empty in a frame that t alone exceeds it
    (mel sum below about 0.07 x the band's weight for a peak of 6), the bar is LOGMEL_BAR + t.  The mel / log stage itself is
    held to the flat LOGMEL_BAR everywhere by the replay from the device's magnitudes (logmel_of_mag), and the magnitudes to
    MAG_BAR, so nothing hides behind the wider elements but the conditioning of the logarithm."""
    u = 2.0 ** -24 * np.asarray(ref["mag"], np.float64).max(-1)                     # [B, F]
    t = u[..., None] * tables32(p)[1].sum(0) / np.exp(np.asarray(ref["logmel"], np.float64))
    return np.where(t <= LOGMEL_BAR, LOGMEL_BAR, LOGMEL_BAR + t)


def _weighted(logmel, dct):
    """max over frames and q of sum_m |logmel[m] D[m, q]|"""
    lm = np.abs(np.asarray(logmel, np.float64)).reshape(-1, dct.shape[0])
    return float((lm @ np.abs(dct)).max())


def mfcc_bar(tables, logmel_ref):
    """|MFCC - float64| of one case: the log-mel bar through the DCT, plus the rounding of the n_mel-term product chain"""
    D = np.asarray(tables["dct"], np.float64)
    return LOGMEL_BAR * float(np.abs(D).sum(0).max()) + 2.0 ** -22 * _weighted(logmel_ref, D)


def chain_bar(p, logmel_dev):
    """|generic kind 0 - float64(device log-mel) @ D|: f32 fma chains of n_mel terms in all"""
    return p["n_mel"] * 2.0 ** -24 * _weighted(logmel_dev, tables32(p)[2])


def logmel_of_mag(p, mag_dev):
    """float64 log-mel rows of the DEVICE's magnitudes: log(mag @ mel + offset), floored where the plan has a floor"""
    t = p["tables"]
    mel = np.asarray(mag_dev, np.float64) @ tables32(p)[1] + np.float64(np.float32(t["log_offset"]))
    if t["log_floor"] > 0.0:
        mel = np.maximum(mel, np.float64(np.float32(t["log_floor"])))
    return np.log(mel)


# ---------------------------------------------------------------------------------------------------------------------------
# the host dispatch, restated
# ---------------------------------------------------------------------------------------------------------------------------
def replay_plan(p):
    """kws_stft_plan_create's band arithmetic (stft.hip): dict(band_start, band_cnt, mel_mc, mel_maxw, mel_ws, clamped,
    shape, lds_bytes): `clamped` = the bands whose tap window the host moved back inside the 260-float row; `shape` =
    stft4_shape's answer, `lds_bytes` = kws_stft4_lds_bytes' (12 waves, groups of 4 quads)"""
    mel = np.asarray(p["tables"]["mel"], np.float32)
    n_mel = p["n_mel"]
    assert mel.shape == (NBINS, n_mel)
    bs, bc = np.zeros(n_mel, int), np.zeros(n_mel, int)
    for m in range(n_mel):
        nz = np.nonzero(mel[:, m])[0]
        if len(nz):
            bs[m], bc[m] = nz[0], nz[-1] - nz[0] + 1
    nb = (n_mel + 15) // 16
    al = 1 if nb >= 5 else 0
    mc = [0] * 8
    for m in range(n_mel):
        mc[m >> 4] = max(mc[m >> 4], (bc[m] + (bs[m] & al) + 3) // 4)
    mc = [max(v, 1) if i < nb else v for i, v in enumerate(mc)]
    maxw = 4 * max(mc)
    ws, clamped = np.zeros(n_mel, int), []
    if maxw > 64:
        maxw = 0
    else:
        for m in range(n_mel):
            ws[m] = bs[m] & ~al
            if ws[m] + maxw > MAGF:
                ws[m] = MAGF - maxw
                clamped.append(m)
    shape = 0
    if maxw > 0:
        for s in (1, 2, 3, 4):
            if len(SHAPES[s]) == nb and all(mc[i] <= v for i, v in enumerate(SHAPES[s])):
                shape = s
                break
    lds = 1 << 30
    if shape:
        nbk, mck = (5, 4) if shape <= 2 else (3, 8)
        lds = 4 * (512 + 512 + 256 + 4 + 16 * nbk * 80 + n_mel * (4 * mck + 4) + 12 * (4 * MAGF + ((16 * (16 * nbk + 1) + 3) & ~3)))
    return dict(band_start=bs, band_cnt=bc, mel_mc=mc[:nb], mel_maxw=maxw, mel_ws=ws, clamped=clamped, shape=shape, lds_bytes=lds)


def kernel_taps(shape, m):
    """taps the stft4 instance `shape` reads for band m (4 x the blocks of its lane group)"""
    return 4 * SHAPES[shape][m >> 4]


def replay_kernel(p, L, kind, aligned16=True, rp=None):
    """kws_stft_mel_kernel (stft.hip) / kws_stft4_kernel_code (stft4.hip): 0 / 1 generic with 4 / 7 waves, 10 + 2 shape + v4, -1"""
    if L < p["frame_len"] or L % 2 or kind not in (0, 1, 2):
        return -1
    rp = rp or replay_plan(p)
    img4 = rp["shape"] != 0 and p["n_mel"] % 4 == 0            # kws_stft4_prepare made an image
    if (kind == 0 and p["n_out"] <= 64 and p["n_mel"] <= 128 and p["n_mel"] % 4 == 0 and p["frame_len"] % 2 == 0 and
            rp["mel_maxw"] > 0 and img4 and rp["lds_bytes"] <= LDS_CAP):
        v4 = L % 4 == 0 and p["step"] % 4 == 0 and aligned16
        return 10 + 2 * rp["shape"] + int(v4)
    return 1 if num_frames(p, L) % 14 == 0 else 0


def expected_kernel(p, L, kind, aligned16=True):
    """the code the TABLE says: from the plan's `shape` entry, not from the replay"""
    if kind == 0 and p["shape"]:
        return 10 + 2 * p["shape"] + int(L % 4 == 0 and p["step"] % 4 == 0 and aligned16)
    return 1 if num_frames(p, L) % 14 == 0 else 0
