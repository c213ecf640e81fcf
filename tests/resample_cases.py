"""The case table of the resampler tests (test_resample_cpu.py, test_resample_kernels_gpu.py): rate pairs, what each one
exercises, the tile of outputs the kernel works in, and the inputs built from them."""
import numpy as np

import resample_oracle as RO

# (rate_in, rate_out, up, down, what the pair exercises)
SCIPY_PAIRS = [(48000, 16000), (44100, 16000), (32000, 16000), (22050, 16000), (11025, 16000), (8000, 16000), (16000, 16000)]

PAIRS = [
    (48000, 16000, 1, 3, "T = 61; up = 1: the decimation loop (one phase, taps from scalar registers)"),
    (8000, 16000, 2, 1, "upsampling"),
    (16000, 48000, 3, 1, "upsampling"),
    (44100, 16000, 160, 441, "T = 56, 36 KB table in LDS"),
    (11025, 16000, 640, 441, "60 KB table (rows padded to 24 floats): in LDS beside a 3 KB tile"),
    (999, 1000, 1000, 999, "20001 taps, 96 KB table: the global-table path"),
    (16000, 2000, 1, 8, "T = 161, up = 1: tiles of 512 outputs (workgroups of 128)"),
    (16000, 1000, 1, 16, "T = 321, up = 1: tiles of 256 outputs (workgroups of 64)"),
    (25000, 2000, 2, 25, "T = 251: tiles of 512 outputs on the general loop"),
    (51000, 2000, 2, 51, "T = 511: tiles of 256 outputs on the general loop"),
    (16000, 100, 1, 160, "T = 3201: the span of 256 outputs does not fit in LDS, the direct kernel"),
    (32000, 32000, 1, 1, "copy"),
]
FILTER_PAIRS = [p for p in PAIRS if (p[2], p[3]) != (1, 1)]
PAIR_IDS = ["%d-%d" % p[:2] for p in PAIRS]
FILTER_IDS = ["%d-%d" % p[:2] for p in FILTER_PAIRS]

# csrc/resample.hip: XS_BYTES, LDS_BYTES, PER and span_floats() - what decides a pair's tile and path
XS_BYTES, LDS_BYTES, PER = 32 * 1024, 64 * 1024, 4


def kernel_path(rate_in, rate_out):
    """(path, tile): 'copy' | 'direct' | 'decimate' | 'lds' | 'global' and the outputs per tile (0 for the untiled kernels),
    as resample_launch() in csrc/resample.hip chooses them ('lds' / 'global': where the general loop's table is)."""
    up, down, _, T = RO.design(rate_in, rate_out)
    if (up, down) == (1, 1):
        return 'copy', 0
    Tp = (T + 3) // 4 * 4
    for nt in (256, 128, 64):
        span = (((PER * nt - 1) * down) // up + 1 + Tp + 3 + 3) // 4 * 4
        if span * 4 <= XS_BYTES:
            if up == 1:
                return 'decimate', PER * nt
            return ('lds' if span * 4 + up * Tp * 4 <= LDS_BYTES else 'global'), PER * nt
    return 'direct', 0


EXPECTED_PATHS = {(48000, 16000): ('decimate', 1024), (8000, 16000): ('lds', 1024), (16000, 48000): ('lds', 1024),
                  (44100, 16000): ('lds', 1024), (11025, 16000): ('lds', 1024), (999, 1000): ('global', 1024),
                  (16000, 2000): ('decimate', 512), (16000, 1000): ('decimate', 256),
                  (25000, 2000): ('lds', 512), (51000, 2000): ('lds', 256),
                  (16000, 100): ('direct', 0), (32000, 32000): ('copy', 0)}


def n_in_for(n_out_wanted, rate_in, rate_out):
    """(largest n_in whose output is shorter than n_out_wanted, smallest n_in whose output has at least n_out_wanted)."""
    up, down, _, _ = RO.design(rate_in, rate_out)
    n = (n_out_wanted * down) // up
    while RO.out_samples(n, rate_in, rate_out) >= n_out_wanted:
        n -= 1
    return n, n + 1


def edge_lengths(rate_in, rate_out):
    """Row lengths of the ragged edge batch: 1, shorter than T, 0, an odd middle, and outputs one short of / equal to /
    one past a tile (the nearest reachable lengths when up > down skips some), longest last but one, a zero row last."""
    _, tile = kernel_path(rate_in, rate_out)
    up, down, _, T = RO.design(rate_in, rate_out)
    tile = tile or 256
    short, exact = n_in_for(tile, rate_in, rate_out)
    past = n_in_for(tile + 1, rate_in, rate_out)[1]
    if (rate_in, rate_out) == (16000, 100):       # T = 3201 samples: one tile of outputs would be 160 * 1024 of them
        return [1, 3000, 0, 777, 8000, 7999, 0]
    return [1, max(T - 1, 1), 0, 777, short, exact, past, 0]


def impulse_positions(n_in, rate_in, rate_out):
    """Input samples further than the filter's span (T samples) apart: 0, n_in - 1, the sample under every multiple of
    256 outputs (every tile size the kernel has; the response of one impulse covers both sides of the boundary), and a
    regular comb between them."""
    up, down, _, T = RO.design(rate_in, rate_out)
    gap = T + 2
    want = [0, n_in - 1]
    n_out = RO.out_samples(n_in, rate_in, rate_out)
    want += [int(round(b * down / up)) for b in range(256, n_out, 256)]
    want += list(range(gap, n_in, gap))
    near = np.zeros(n_in, dtype=bool)             # within the gap of a kept position
    got = []
    for p in want:                                # first come, first kept: edges and boundaries before the comb
        if 0 <= p < n_in and not near[p]:
            got.append(p)
            near[max(p - gap + 1, 0):p + gap] = True
    return sorted(got)


def impulse_row(n_in, rate_in, rate_out, dtype=np.int16):
    """Impulses of value +-2^k, k in (0, 7, 14), at impulse_positions()."""
    x = np.zeros(n_in, dtype=dtype)
    vals = [1, -128, 16384, -1, 128, -16384]
    for c, p in enumerate(impulse_positions(n_in, rate_in, rate_out)):
        x[p] = vals[c % len(vals)]
    return x


def alternating_row(n_in, dtype=np.int16):
    """Full scale, alternating sign: 32767, -32768, ..."""
    x = np.empty(n_in, dtype=dtype)
    x[0::2] = 32767
    x[1::2] = -32768
    return x


def random_row(rng, n_in, dtype=np.int16):
    if dtype == np.int16:
        return rng.randint(-32768, 32768, n_in).astype(np.int16)
    return (rng.randn(n_in) * 0.3).astype(np.float32)
