"""Case tables and NumPy restatements for the shared-frame feature path of the keyword-spotting stream
(stream.Features, kws_stream_gather_f32 in csrc/stream.hip).

gather_ref restates the gather of include/kws_hip.h on 32-bit patterns (the kernel copies bits, so the device's output is
compared as uint32), plan_rows_ref restates stream.plan_rows."""
import numpy as np

GATHER_GRID_THREADS = 2048 * 256   # csrc/stream.hip: MAX_BLOCKS * NT, the most work items one pass of gather_kernel's grid takes
POISON = np.uint32(0x7FC0DEAD)     # a NaN with a payload: neither a zero nor any source word (gather_source keeps it out)


def gather_ref(src, n, start, hop, win, out, out_pitch, W, out_offset=0):
    """A copy of `out` (1-D, viewed as uint32) with out[out_offset + w out_pitch + i] = src[start + w hop + i] for w < W,
    i < win, and 0 where that index is outside [0, n); int64 indexing, nothing else touched."""
    src = np.ascontiguousarray(src).reshape(-1).view(np.uint32)
    out = np.ascontiguousarray(out).reshape(-1).view(np.uint32).copy()
    w = np.arange(W, dtype=np.int64)[:, None]
    i = np.arange(win, dtype=np.int64)[None, :]
    s = np.int64(start) + w * np.int64(hop) + i
    inside = (s >= 0) & (s < np.int64(n))
    vals = np.zeros((W, win), dtype=np.uint32)
    if n:
        vals = np.where(inside, src[np.clip(s, 0, n - 1)], np.uint32(0))
    out[np.int64(out_offset) + w * np.int64(out_pitch) + i] = vals
    return out


def gather_loops(src, n, start, hop, win, out, out_pitch, W, out_offset=0):
    """The definition as an explicit double loop (what gather_ref is checked against)."""
    src = np.ascontiguousarray(src).reshape(-1).view(np.uint32)
    out = np.ascontiguousarray(out).reshape(-1).view(np.uint32).copy()
    for w in range(W):
        for i in range(win):
            s = start + w * hop + i
            out[out_offset + w * out_pitch + i] = src[s] if 0 <= s < n else 0
    return out


def gather_source(words, seed):
    """`words` arbitrary 32-bit patterns: uniform bits (NaNs of every payload among them) with -0.0, +0.0, denormals,
    infinities and signalling / quiet NaNs planted all over; POISON itself is kept out."""
    rng = np.random.RandomState(seed)
    u = rng.randint(0, 1 << 32, words, dtype=np.uint64).astype(np.uint32)
    special = np.array([0x80000000, 0x00000000, 0x00000001, 0x807FFFFF, 0x7F800000, 0xFF800000, 0x7F800001, 0xFFC12345,
                        0x7FFFFFFF, 0x00400000], dtype=np.uint32)
    at = rng.randint(0, words, words // 4)
    u[at] = special[rng.randint(0, len(special), len(at))]
    u[u == POISON] = np.uint32(1)
    return u


def plan_rows_ref(count, hop, win, frame_len, step):
    """(Lc, J, r) of stream.plan_rows: the chunk of `count` windows as one signal of Lc samples (a multiple of 4) with J
    frames, window w taking the F = 1 + (win - frame_len) // step frames from w r on, r = hop / step."""
    if hop % step:
        raise ValueError("hop %d is no multiple of step %d" % (hop, step))
    r = hop // step
    F = 1 + (win - frame_len) // step
    Lc = (count - 1) * hop + win
    while Lc % 4:
        Lc += 1
    return Lc, (count - 1) * r + F, r


# ---- the gather kernel ------------------------------------------------------------------------------------------------------------
# win: below, at and above one 16-byte chunk, two chunks and one over, two spectrogram rows (514), a whole spectrogram (25186,
# not a multiple of 4: with out_pitch = win the rows' alignment rotates)
GATHER_WINS = (1, 2, 3, 4, 5, 7, 8, 9, 514, 25186)
GATHER_PITCH_EXTRA = (0, 1, 3, 16000)          # out_pitch = win + extra; 16000: the raw half of a composite row
GATHER_ROWS = 4


def gather_hops(win):
    return sorted(set((1, 3, 4, win, win + 5)))


def gather_edges(win, hop):
    """(name, start, n, W): where the rows lie against the source's two ends."""
    W = GATHER_ROWS
    half = (win + 1) // 2
    return [
        # row 0 starts up to win before sample 0; row 2 straddles n, and with hop > win / 2 row 3 lies wholly past n
        ('starts_inside_win_before_0', -half, max(0, -half + 2 * hop + win // 2 + 1), W),
        # row 0 (and with a small hop every row) lies wholly before sample 0
        ('starts_more_than_win_before_0', -(win + 3), max(1, -(win + 3) + 3 * hop + half), W),
        ('wholly_inside', 1, 1 + (W - 1) * hop + win + 2, W),
        ('empty_source', 2, 0, W),
        ('one_row', 1, win + 5, 1),
    ]


def gather_cases(win):
    """Every (pitch, hop, edge, source offset mod 4, destination offset mod 4) for one win."""
    for extra in GATHER_PITCH_EXTRA:
        for hop in gather_hops(win):
            for name, start, n, W in gather_edges(win, hop):
                for soff in range(4):
                    for doff in range(4):
                        yield dict(win=win, out_pitch=win + extra, hop=hop, start=start, n=n, W=W, soff=soff, doff=doff, edge=name)


# one case whose W * ceil(win / 4) exceeds one pass of the grid: every thread goes round its loop again, and the stride is
# no whole number of rows (3 chunk slots per row at win = 8), so the (row, chunk) pair carries
GATHER_WRAP = dict(win=8, out_pitch=9, hop=3, start=-5, n=300000 * 3 - 40, W=300000, soff=1, doff=2, edge='grid_wraps')

# ---- Features.rows against Features.windows ------------------------------------------------------------------------------------------
SETTINGS = dict(label_count=12, sample_rate=16000, clip_duration_ms=1000, window_size_ms=30.0, window_stride_ms=10.0,
                dct_coefficient_count=40, num_log_mel_features=40)
WIN, FRAME_LEN, STEP, FRAMES = 16000, 480, 160, 98
ROWS_HOPS = (160, 320, 800)
ROWS_COUNTS = (1, 4, 9)
