"""The host side of the keyword-spotting stream (speech_recognition_amd/stream.py): the window plan, the decision state
machine, the scoring and the NumPy restatements the GPU tests compare the kernels with.  No device."""
import numpy as np
import pytest

import stream_cases as SC
from speech_recognition_amd import stream


@pytest.mark.parametrize("n,win,hop,start,W", [
    (0, 16, 4, 0, 1),            # an empty recording is one window of zeros
    (5, 16, 4, 0, 1),            # n < win
    (16, 16, 4, 0, 1),           # n == win
    (17, 16, 4, 0, 2),           # n == win + 1
    (17, 16, 23, 0, 2),          # hop > win
    (40, 16, 23, 0, 3),          # 0..16, 23..39, 46..: sample 39 is the second window's last
    (9, 16, 4, -7, 1),           # left padding: the first window ends at 9 ...
    (10, 16, 4, -7, 2),
    (17, 16, 4, -7, 3),          # ... so 17 samples need -7 + 2 * 4 + 16 = 17
    (16, 16, 4, 3, 1),           # a positive start skips samples: 3 + 16 >= 16
    (20, 16, 4, 3, 2),
    (16000 + 7 * 800 + 123, 16000, 800, 0, 9),
    (600 * 16000, 16000, 320, 0, 29951),
])
def test_plan_windows_at_the_edges(n, win, hop, start, W):
    assert stream.plan_windows(n, win, hop, start) == W
    assert SC.plan_windows_ref(n, win, hop, start) == W


@pytest.mark.parametrize("win,hop,start", [(16, 1, 0), (16, 4, -7), (16, 23, 3), (4, 5, -16), (40, 7, 11)])
def test_plan_windows_is_the_smallest_cover(win, hop, start):
    for n in range(0, 201):
        W = stream.plan_windows(n, win, hop, start)
        assert W == SC.plan_windows_ref(n, win, hop, start), (n, win, hop, start)
        assert W >= 1 and start + (W - 1) * hop + win >= n
        assert W == 1 or start + (W - 2) * hop + win < n


def test_plan_windows_refuses_nonsense():
    for bad in ((10, 0, 1), (10, 16, 0), (-1, 16, 4)):
        with pytest.raises(ValueError):
            stream.plan_windows(*bad)


def run_detect(top, score, A=1, hop=10, win=20, start=0, threshold=0.5, suppression_samples=30, minimum_count=1, ignore=(0, 1)):
    top, score = np.asarray(top, np.int32), np.asarray(score, np.float32)
    got = stream.detect(top, score, stream.counts_ok(len(top), A, minimum_count), hop, win, start=start, threshold=threshold,
                        suppression_samples=suppression_samples, ignore=ignore)
    assert got == SC.detect_ref(top, score, A, hop, win, start=start, threshold=threshold, suppression_samples=suppression_samples,
                                minimum_count=minimum_count, ignore=ignore)
    return got


def test_detect_score_exactly_at_the_threshold_fires():
    thr = 0.7
    at, below = np.float32(thr), np.nextafter(np.float32(thr), np.float32(0))
    got = run_detect([2, 2], [below, at], threshold=thr)
    assert [(c, w) for c, w, _, _ in got] == [(2, 1)]
    assert got[0][2] == 0 + 1 * 10 + 20 and got[0][3] == float(at)


def test_detect_ignored_labels_never_fire():
    got = run_detect([0, 1, 3, 1], [0.9, 0.9, 0.9, 0.9], suppression_samples=0)
    assert [(c, w) for c, w, _, _ in got] == [(3, 2)]
    got = run_detect([0, 1, 3, 1], [0.9, 0.9, 0.9, 0.9], suppression_samples=0, ignore=())
    assert [(c, w) for c, w, _, _ in got] == [(0, 0), (1, 1), (3, 2), (1, 3)]


def test_detect_minimum_count_blocks_the_first_windows():
    top, score = [2] * 6, [0.9] * 6
    assert [w for _, w, _, _ in run_detect(top, score, A=4, minimum_count=3, suppression_samples=0)] == [2, 3, 4, 5]
    assert [w for _, w, _, _ in run_detect(top, score, A=4, minimum_count=4, suppression_samples=0)] == [3, 4, 5]
    # an average that can never hold minimum_count windows never fires
    assert run_detect(top, score, A=2, minimum_count=3, suppression_samples=0) == []


def test_detect_suppression_one_sample_short_and_exactly_at_the_limit():
    top, score = [2] * 5, [0.9] * 5
    # ends 20, 30, 40, 50, 60: with 30 samples of suppression window 3 (50 - 20 = 30) fires, window 2 (20 short by 10) not
    assert [w for _, w, _, _ in run_detect(top, score, suppression_samples=30)] == [0, 3]
    # one sample more and window 3 is one sample short: window 4 fires
    assert [w for _, w, _, _ in run_detect(top, score, suppression_samples=31)] == [0, 4]
    assert [w for _, w, _, _ in run_detect(top, score, hop=1, win=4, suppression_samples=3)] == [0, 3]
    assert [w for _, w, _, _ in run_detect(top, score, hop=1, win=4, suppression_samples=4)] == [0, 4]


def test_detect_two_labels_inside_one_suppression_span():
    """Suppression is about time, not about the label: the second word inside the span is dropped."""
    got = run_detect([2, 3, 3, 3, 3], [0.9] * 5, suppression_samples=30)
    assert [(c, w) for c, w, _, _ in got] == [(2, 0), (3, 3)]


def test_detect_start_moves_the_window_ends_and_an_empty_track_is_empty():
    got = run_detect([2, 2], [0.9, 0.9], start=-7, suppression_samples=0)
    assert [e for _, _, e, _ in got] == [13, 23]
    assert run_detect([], []) == []
    with pytest.raises(ValueError):
        stream.detect(np.zeros(3, np.int32), np.zeros(2, np.float32), np.ones(3, bool), 10, 20)


def test_score_counts():
    det = lambda label, sample: (label, sample / 16000.0, sample, 0.9)
    truth = [('yes', 1000), ('no', 5000), ('up', 9000)]
    assert stream.score([], [], 100) == {'correct': 0, 'wrong_label': 0, 'false_positive': 0, 'missed': 0}
    assert stream.score([], truth, 100) == {'correct': 0, 'wrong_label': 0, 'false_positive': 0, 'missed': 3}
    assert stream.score([det('yes', 1100), det('no', 4900), det('up', 9000)], truth, 100) == \
        {'correct': 3, 'wrong_label': 0, 'false_positive': 0, 'missed': 0}
    # one sample past the tolerance is a false positive and a miss; a wrong label inside it is neither
    assert stream.score([det('yes', 1101), det('down', 5000)], truth, 100) == \
        {'correct': 0, 'wrong_label': 1, 'false_positive': 1, 'missed': 2}
    # one to one: the second detection of the same word finds its truth taken
    assert stream.score([det('yes', 990), det('yes', 1010)], truth, 100) == \
        {'correct': 1, 'wrong_label': 0, 'false_positive': 1, 'missed': 2}
    # time order, not list order; integer labels work like names
    assert stream.score([(7, 0.0, 5000, 1.0), (3, 0.0, 1000, 1.0)], [(3, 1000), (7, 5000)], 0) == \
        {'correct': 2, 'wrong_label': 0, 'false_positive': 0, 'missed': 0}


def test_frames_ref_by_hand():
    x = np.arange(1, 7, dtype=np.int16)
    got = SC.frames_ref(x, 4, 3, 3, start=-2, scale=0.5)
    assert got.dtype == np.float32
    assert np.array_equal(got, np.array([[0, 0, .5, 1], [1, 1.5, 2, 2.5], [2.5, 3, 0, 0]], np.float32))
    assert not np.signbit(SC.frames_ref(x, 4, 3, 3, start=-2, scale=-0.5)[0, 0])       # outside is +0.0, not scale * 0
    assert np.array_equal(SC.frames_ref(np.zeros(0, np.float32), 4, 1, 2), np.zeros((2, 4), np.float32))
    assert SC.frames_ref(np.array([-32768, 32767], np.int16), 4, 4, 1)[0, :2].tolist() == [-1.0, 32767.0 / 32768.0]


@pytest.mark.parametrize("A", [1, 2, 3])
def test_smooth_ref_against_a_float64_mean(A):
    """A sanity check of the restatement.  The bound 2^-22 relative is a proof for A <= 3: k <= 3 positive float32 terms take
    k - 1 roundings to add and one to divide, (1 + 2^-24)^3 - 1 < 2^-22."""
    p = SC.softmax_rows(120, 12, A)
    sm, top, score = SC.smooth_ref(p, A)
    assert sm.dtype == np.float32 and top.dtype == np.int32
    p64 = p.astype(np.float64)
    for w in range(len(p)):
        lo = max(0, w - A + 1)
        mean = p64[lo:w + 1].mean(axis=0)
        assert (np.abs(sm[w] - mean) <= 2.0 ** -22 * mean).all(), w
        assert score[w] == sm[w].max() and top[w] == int(np.argmax(sm[w]))
    if A == 1:
        assert sm.tobytes() == p.tobytes()


@pytest.mark.parametrize("A", [8, 50])
def test_smooth_ref_windowing_at_the_lengths_the_gpu_tests_use(A):
    """lo and the divisor at A = 8 and 50, on tracks shorter than, equal to and longer than A.  k <= A positive float32 terms
    take k - 1 roundings to add and one to divide: (1 + 2^-24)^k - 1 < (k + 1) 2^-24 for k <= 50."""
    for W in (A - 1, A, A + 1, 3 * A):
        p = SC.softmax_rows(W, 12, A + W)
        sm, top, score = SC.smooth_ref(p, A)
        p64 = p.astype(np.float64)
        for w in range(W):
            lo = max(0, w - A + 1)
            mean = p64[lo:w + 1].sum(axis=0) / (w - lo + 1)
            assert (np.abs(sm[w] - mean) <= (w - lo + 2) * 2.0 ** -24 * mean).all(), (W, w)
            # a window one row too long or too short, or a wrong divisor, misses this bound by orders of magnitude
            if w >= 1:
                wrong = p64[max(0, w - A):w + 1].sum(axis=0) / (w - lo + 1)
                assert lo == 0 and w - A < 0 or (np.abs(sm[w] - wrong) > (w - lo + 2) * 2.0 ** -24 * wrong).any()
        assert np.array_equal(top, sm.argmax(axis=1)) and np.array_equal(score, sm.max(axis=1))


def test_smooth_ref_ties_take_the_lowest_class():
    p = SC.dyadic_rows(40, 12, 1)
    sm, top, score = SC.smooth_ref(p, 3)
    ties = 0
    for w in range(40):
        winners = np.nonzero(sm[w] == sm[w].max())[0]
        ties += len(winners) > 1
        assert top[w] == winners[0]
    assert ties > 10
