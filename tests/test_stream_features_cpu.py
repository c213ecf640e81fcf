"""Host-side checks of the shared-frame feature path (stream.plan_rows, stream.Features' argument checks) and of the
restatements the GPU tests trust (stream_feature_cases.gather_ref / plan_rows_ref).  No device is touched."""
import itertools

import numpy as np
import pytest

import stream_feature_cases as FC
from oracle import features as OF
from speech_recognition_amd import stream
from speech_recognition_amd.model import prepare_model_settings


@pytest.mark.parametrize("step,frame_len", [(1, 1), (2, 5), (3, 3), (4, 10), (160, 480)])
def test_plan_rows_against_brute_force(step, frame_len):
    for count, r, extra in itertools.product((1, 2, 3, 7), (1, 2, 5), (0, 1, step - 1, 3 * step + 1)):
        hop, win = r * step, frame_len + extra
        Lc, J, r_got = FC.plan_rows_ref(count, hop, win, frame_len, step)
        assert stream.plan_rows(count, hop, win, frame_len, step) == (Lc, J, r_got)
        assert r_got == r and Lc % 4 == 0 and 0 <= Lc - ((count - 1) * hop + win) < 4
        # the frames of window w, by their first sample inside the chunk: frame k of window w starts at w hop + k step
        F = len(range(0, win - frame_len + 1, step))
        used = set()
        for w in range(count):
            for k in range(F):
                first = w * hop + k * step
                assert first % step == 0                     # ... which is where frame first / step of the chunk's track starts
                assert first // step == w * r + k
                used.add(first // step)
                assert first + frame_len <= (count - 1) * hop + win <= Lc
        assert max(used) == J - 1 and min(used) == 0          # every index used is < J, and J is tight
        assert 1 + (Lc - frame_len) // step >= J              # the track of Lc samples has them all


def test_plan_rows_refuses_a_hop_that_shares_no_frames():
    for fn in (FC.plan_rows_ref, stream.plan_rows):
        with pytest.raises(ValueError, match="step"):
            fn(3, 200, 16000, 480, 160)
    with pytest.raises(ValueError):
        stream.plan_rows(0, 160, 16000, 480, 160)
    with pytest.raises(ValueError):
        stream.plan_rows(1, 160, 400, 480, 160)


@pytest.mark.parametrize("hop", [160, 320, 800])
def test_a_window_is_a_slice_of_the_chunk_track_on_the_oracle(hop):
    """oracle/features.py's path B on a random signal: the features of window w are rows w r .. w r + F - 1 of the features
    of the whole chunk, exactly - the oracle computes a frame from the frame's own samples."""
    win, frame_len, step, count = 2080, 480, 160, 4
    tables = OF.tables_path_b(frame_len, 40, 40)
    Lc, J, r = FC.plan_rows_ref(count, hop, win, frame_len, step)
    x = np.random.RandomState(hop).standard_normal(Lc) * 0.1
    x[(count - 1) * hop + win:] = 0.0
    F = 1 + (win - frame_len) // step
    track = OF.features(x, tables, step)
    assert track.shape[0] >= J and track.shape[1] == 40
    for w in range(count):
        alone = OF.features(x[w * hop:w * hop + win], tables, step)
        assert alone.shape == (F, 40)
        assert alone.tobytes() == track[w * r:w * r + F].tobytes()


@pytest.mark.parametrize("case", [
    dict(n=10, start=0, hop=3, win=4, pitch=4, W=3, off=0),
    dict(n=10, start=-5, hop=1, win=3, pitch=7, W=4, off=2),
    dict(n=10, start=6, hop=4, win=5, pitch=5, W=4, off=1),
    dict(n=0, start=1, hop=2, win=2, pitch=3, W=3, off=0),
    dict(n=33, start=-40, hop=17, win=9, pitch=12, W=6, off=3),
    dict(n=7, start=2, hop=9, win=1, pitch=1, W=1, off=5),
])
def test_gather_ref_against_the_double_loop(case):
    c = case
    src = FC.gather_source(max(c['n'], 1) + 8, 3)
    out = np.full(c['off'] + c['W'] * c['pitch'] + 6, FC.POISON, dtype=np.uint32)
    got = FC.gather_ref(src, c['n'], c['start'], c['hop'], c['win'], out, c['pitch'], c['W'], c['off'])
    want = FC.gather_loops(src, c['n'], c['start'], c['hop'], c['win'], out, c['pitch'], c['W'], c['off'])
    assert got.dtype == np.uint32 and got.tobytes() == want.tobytes()
    assert (out == FC.POISON).all()                                  # the input buffer is left alone
    written = np.zeros(len(out), bool)
    for w in range(c['W']):
        written[c['off'] + w * c['pitch']:c['off'] + w * c['pitch'] + c['win']] = True
    assert (got[~written] == FC.POISON).all() and (got[written] != FC.POISON).all()


def test_gather_case_tables_cover_what_they_claim():
    assert FC.GATHER_WRAP['W'] * -(-FC.GATHER_WRAP['win'] // 4) > FC.GATHER_GRID_THREADS
    for win in FC.GATHER_WINS:
        cases = list(FC.gather_cases(win))
        assert {(c['soff'], c['doff']) for c in cases} == set(itertools.product(range(4), range(4)))
        assert {c['out_pitch'] - win for c in cases} == {0, 1, 3, 16000}
        assert {1, 3, 4, win, win + 5} == {c['hop'] for c in cases}
        assert any(-win <= c['start'] < 0 for c in cases) and any(c['start'] < -win for c in cases)
        assert any(c['n'] == 0 for c in cases) and any(c['W'] == 1 for c in cases)
        ends = [(c['start'] + w * c['hop'], c['n']) for c in cases for w in range(c['W']) if c['n']]
        assert any(s < n < s + win for s, n in ends) or win == 1         # a row straddles n
        assert any(s >= n for s, n in ends)                               # a row wholly past n


def test_features_argument_errors_need_no_device():
    settings = prepare_model_settings(output_representation='mfcc', **FC.SETTINGS)
    assert 'output_representation' not in settings
    with pytest.raises(ValueError, match="output_representation"):
        stream.Features(settings)
    with pytest.raises(ValueError, match="raw"):
        stream.Features(dict(settings, output_representation='raw'))
    with pytest.raises(ValueError, match="raw"):
        stream.Features(settings, output_representation='raw')
    with pytest.raises(ValueError, match="one of"):
        stream.Features(settings, output_representation='mel')
    for key in ('desired_samples', 'window_stride_samples', 'num_log_mel_features'):
        broken = dict(settings, output_representation='spec')
        del broken[key]
        with pytest.raises(ValueError, match=key):
            stream.Features(broken)
