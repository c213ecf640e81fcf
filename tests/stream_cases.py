"""Case tables and NumPy restatements for the keyword-spotting stream (speech_recognition_amd/stream.py, csrc/stream.hip).

frames_ref, smooth_ref and detect_ref restate the definitions of include/kws_hip.h / stream.py operation by operation in
the same number formats, so the device's results are compared with them bit for bit."""
import numpy as np


def frames_ref(x, win, hop, W, start=0, scale=None):
    """out[w, i] = float32(scale) * float32(x[start + w hop + i]) - one float32 multiply - and +0.0 outside [0, len(x));
    int64 indexing."""
    x = np.asarray(x)
    if scale is None:
        scale = 1.0 / 32768.0 if x.dtype == np.int16 else 1.0
    n = np.int64(len(x))
    s = np.int64(start) + np.arange(W, dtype=np.int64)[:, None] * np.int64(hop) + np.arange(win, dtype=np.int64)[None, :]
    inside = (s >= 0) & (s < n)
    out = np.zeros((W, win), dtype=np.float32)
    if n:
        vals = x[np.clip(s, 0, n - 1)].astype(np.float32) * np.float32(scale)
        out[inside] = vals[inside]
    return out


def smooth_ref(probs, A):
    """(smoothed, top, top_score): lo = max(0, w - A + 1); the rows lo .. w added one after the other in float32, ascending,
    then ONE float32 division by float32(w - lo + 1); argmax = the first maximum."""
    p = np.asarray(probs, dtype=np.float32)
    W, NC = p.shape
    sm = np.empty((W, NC), dtype=np.float32)
    for w in range(W):
        lo = max(0, w - A + 1)
        acc = p[lo].copy()
        for r in range(lo + 1, w + 1):
            acc = (acc + p[r]).astype(np.float32)
        sm[w] = acc / np.float32(w - lo + 1)
    top = sm.argmax(axis=1).astype(np.int32)
    return sm, top, sm[np.arange(W), top]


def detect_ref(top, top_score, A, hop, win, start=0, threshold=0.7, suppression_samples=16000, minimum_count=3, ignore=(0, 1)):
    """The state machine of stream.detect as one plain loop over the windows -> [(label index, w, end_w, score)]."""
    fires, last = [], None
    thr = np.float32(threshold)
    for w in range(len(top)):
        if min(w + 1, A) < minimum_count or int(top[w]) in ignore or not (np.float32(top_score[w]) >= thr):
            continue
        end_w = start + w * hop + win
        if last is None or end_w - last >= suppression_samples:
            fires.append((int(top[w]), w, end_w, float(top_score[w])))
            last = end_w
    return fires


def plan_windows_ref(n, win, hop, start=0):
    W = 1
    while start + (W - 1) * hop + win < n:
        W += 1
    return W


# ---- frames ---------------------------------------------------------------------------------------------------------------------
# (win, hop, W, start, n): win = 16 at every source alignment, with windows wholly before, across and wholly past both
# ends of the recording, and gaps (hop > win); W covers the recording and two windows past it
SMALL_FRAMES = [(16, hop, max(plan_windows_ref(n, 16, hop, start), 1) + 2, start, n)
                for hop in (1, 3, 4, 5, 16, 23) for start in (0, -7, 3, -16) for n in (0, 5, 16, 17, 100)]
GRID_THREADS = 2048 * 256      # csrc/stream.hip: MAX_BLOCKS * NT, the most work items one pass of frames_kernel's grid takes
NAMED_FRAMES = {
    'win4_hop1': (4, 1, 300, -2, 290),
    'real_shape_padded_tail': (16000, 160, 5, 0, 16500),
    'many_workgroups': (64, 7, 20000, -5, 20000 * 7 + 11),           # 320 000 items = 1250 workgroups, still one pass
    # more items than GRID_THREADS: every thread goes round its loop again, by the stride's (windows, groups) pair
    'grid_wraps_whole_windows': (64, 7, 40000, -5, 40000 * 7 + 11),  # 640 000 items, 16 groups per window: the stride is whole windows
    'grid_wraps_with_carry': (20, 7, 330000, -5, 330000 * 7 + 3),    # 1 650 000 items (4 rounds), 5 groups per window: 3 over, they carry
    'grid_wraps_real_chunk': (16000, 320, 140, 0, 139 * 320 + 15900),  # 560 000 items, 4000 groups per window: 288 over
}
WRAPPING_FRAMES = {'grid_wraps_whole_windows': False, 'grid_wraps_with_carry': True, 'grid_wraps_real_chunk': True}   # name: carries?


def frames_source(n, dtype, seed):
    """n valid samples: int16 kept to |x| <= 1000 (the poison around them is 32767), float32 normal numbers."""
    rng = np.random.RandomState(seed)
    if dtype == np.int16:
        return rng.randint(-1000, 1001, n).astype(np.int16)
    return rng.standard_normal(n).astype(np.float32)


# ---- smooth ---------------------------------------------------------------------------------------------------------------------
SMOOTH_NC = (1, 11, 12, 32, 35, 256)
SMOOTH_A = (1, 2, 3, 8, 50)


def smooth_lengths(A):
    return sorted(set(w for w in (1, A - 1, A, A + 1, 1000) if w > 0))


def softmax_rows(W, NC, seed):
    rng = np.random.RandomState(seed)
    z = rng.standard_normal((W, NC)) * 3.0
    e = np.exp(z - z.max(axis=1, keepdims=True))
    return (e / e.sum(axis=1, keepdims=True)).astype(np.float32)


def dyadic_rows(W, NC, seed):
    """Multiples of 1 / 8 in [0, 1]: every sum of up to 64 rows is exact, and rows tie across classes all the time."""
    rng = np.random.RandomState(seed)
    return (rng.randint(0, 3, (W, NC)) / 8.0).astype(np.float32)
