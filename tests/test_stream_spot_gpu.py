"""stream.spot / spot_wav end to end on the headline model with its seeded initialisation: the posterior track against
net.predict of windows cut on the host, the smoothing and the decisions against the NumPy restatements run on the device's
own numbers (the discrete decisions are taken from the device's tracks, as the gradient checks do)."""
import numpy as np
import pytest
import torch

import stream_cases as SC
from net_parity import FAMILY_BARS
from speech_recognition_amd import input_data, resample, stream
from speech_recognition_amd.model import speech_model

pytestmark = pytest.mark.gpu

WIN, HOP, BATCH = 16000, 800, 4
N = 16000 + 7 * 800 + 123           # W = 9: chunks of 4, 4, 1
KW = dict(hop=HOP, average_ms=150, threshold=0.0, suppression_ms=100, minimum_count=2, ignore=())   # A = 3


@pytest.fixture(scope="module")
def model():
    return speech_model('conv_1d_time_sliced_with_attention', 16000, 12)


@pytest.fixture(scope="module")
def recording():
    return np.random.RandomState(20).randint(-3000, 3001, N).astype(np.int16)


@pytest.fixture(scope="module")
def host_chunked_probs(model, recording):
    """net.predict of the windows frames_ref builds on the host, fed in the chunks spot uses with batch = 4."""
    W = stream.plan_windows(N, WIN, HOP)
    assert W == 9
    windows = SC.frames_ref(recording, WIN, HOP, W)
    parts = [model.net.predict(torch.from_numpy(windows[w0:w0 + BATCH]).cuda()).cpu().numpy() for w0 in range(0, W, BATCH)]
    assert [len(p) for p in parts] == [4, 4, 1]
    return np.concatenate(parts)


@pytest.fixture(scope="module")
def spotted(model, recording):
    return stream.spot(model, recording, batch=BATCH, **KW)


def test_probs_are_those_of_host_windows_in_the_same_chunks(spotted, host_chunked_probs):
    assert (spotted.W, spotted.hop, spotted.win, spotted.average_windows) == (9, HOP, WIN, 3)
    assert spotted.probs.shape == (9, 12) and spotted.probs.dtype == np.float32
    assert spotted.probs.tobytes() == host_chunked_probs.tobytes()
    assert np.abs(spotted.probs.sum(axis=1) - 1).max() < 1e-5


def test_one_chunk_agrees_within_the_predict_bar(model, recording, host_chunked_probs):
    one = stream.spot(model, recording, batch=16, **KW)
    err = np.abs(one.probs - host_chunked_probs).max()
    print("batch 16 against chunks of 4: max |dp| = %.3g" % err)
    assert err < FAMILY_BARS['predict']


def test_a_chunk_larger_than_one_pass_of_the_gather_grid(model):
    """151 windows in one chunk are 604 000 work items of the gather, more than its grid takes in one pass: the chunk shape
    of real use (batch 1024 is 8 passes) against host-built windows, bit for bit."""
    hop = 160
    x = np.random.RandomState(21).randint(-3000, 3001, 16000 + 150 * hop - 37).astype(np.int16)
    W = stream.plan_windows(len(x), WIN, hop)
    assert W == 151 and W * (WIN // 4) > SC.GRID_THREADS
    got = stream.spot(model, x, batch=256, **dict(KW, hop=hop))
    windows = SC.frames_ref(x, WIN, hop, W)
    assert stream.frames(x, WIN, hop).cpu().numpy().tobytes() == windows.tobytes()
    assert got.probs.tobytes() == model.net.predict(torch.from_numpy(windows).cuda()).cpu().numpy().tobytes()


def test_smoothing_is_the_restatement_of_the_devices_own_probs(spotted):
    sm, top, score = SC.smooth_ref(spotted.probs, 3)
    assert spotted.smoothed.tobytes() == sm.tobytes()
    assert np.array_equal(spotted.top, top) and spotted.top.dtype == np.int32
    assert spotted.top_score.tobytes() == score.tobytes()


def test_detections_are_the_state_machine_on_the_devices_own_tracks(model, recording, spotted):
    want = SC.detect_ref(spotted.top, spotted.top_score, 3, HOP, WIN, threshold=0.0, suppression_samples=1600, minimum_count=2,
                         ignore=())
    assert [w for _, w, _, _ in want] == [1, 3, 5, 7]          # every second window from the first with two rows under it
    assert spotted.detections == [(c, end / 16000.0, end, s) for c, _, end, s in want]
    assert spotted.fires == want
    named = stream.spot(model, recording, labels=['w%d' % i for i in range(12)], batch=BATCH, **KW)
    assert named.detections == [('w%d' % c, end / 16000.0, end, s) for c, _, end, s in want]
    assert named.probs.tobytes() == spotted.probs.tobytes()
    silent = stream.spot(model, recording, batch=BATCH, **dict(KW, threshold=1.5))
    assert silent.detections == [] and silent.probs.tobytes() == spotted.probs.tobytes()
    # the defaults ignore _silence_ and _unknown_
    assert input_data.prepare_words_list(['yes'])[:2] == [input_data.SILENCE_LABEL, input_data.UNKNOWN_WORD_LABEL]
    ignoring = stream.spot(model, recording, batch=BATCH, **dict(KW, ignore=(0, 1)))
    assert ignoring.fires == SC.detect_ref(spotted.top, spotted.top_score, 3, HOP, WIN, threshold=0.0, suppression_samples=1600,
                                           minimum_count=2, ignore=(0, 1))


def test_float_audio_and_a_device_tensor_give_the_same_track(model, recording, spotted):
    as_float = recording.astype(np.float32) * np.float32(1.0 / 32768.0)       # frames' int16 product, done on the host
    assert stream.spot(model, as_float, batch=BATCH, **KW).probs.tobytes() == spotted.probs.tobytes()
    on_device = torch.from_numpy(recording).cuda()
    assert stream.spot(model, on_device, batch=BATCH, **KW).probs.tobytes() == spotted.probs.tobytes()


def test_transform(model, recording, spotted):
    same = stream.spot(model, recording, batch=BATCH, transform=lambda x: x * 1.0, win=WIN, **KW)
    assert same.probs.tobytes() == spotted.probs.tobytes() and same.detections == spotted.detections
    with pytest.raises(ValueError, match="transform must return"):
        stream.spot(model, recording, batch=BATCH, transform=lambda x: x[:, :100], win=WIN, **KW)
    with pytest.raises(ValueError, match="win"):
        stream.spot(model, recording, batch=BATCH, transform=lambda x: x, **KW)


def test_spot_wav_resamples_on_the_device(model, tmp_path):
    rate = 22050
    t = np.arange(int(1.5 * rate)) / float(rate)
    wave = 0.3 * np.sin(2 * np.pi * 440.0 * t) + 0.05 * np.random.RandomState(3).standard_normal(len(t))
    path = str(tmp_path / "a22050.wav")
    input_data.save_wav_file(path, wave, rate)
    samples, got_rate = input_data._read_wav_int16(path)
    assert got_rate == rate and len(samples) == len(t)
    from_wav = stream.spot_wav(model, path, rate_policy='resample', batch=BATCH, **KW)
    x16k = resample.resample(samples, rate, 16000).reshape(-1)
    direct = stream.spot(model, x16k, batch=BATCH, **KW)
    assert from_wav.W == direct.W == stream.plan_windows(resample.resampled_samples(len(samples), rate, 16000), WIN, HOP) == 11
    assert from_wav.probs.tobytes() == direct.probs.tobytes() and from_wav.detections == direct.detections
    with pytest.raises(ValueError, match="22050"):
        stream.spot_wav(model, path, rate_policy='error', batch=BATCH, **KW)
    with pytest.raises(ValueError, match="rate_policy"):
        stream.spot_wav(model, path, rate_policy='nearest', batch=BATCH, **KW)
    # 'decode_wav' takes the samples as they are, whatever the header says
    as_is = stream.spot_wav(model, path, rate_policy='decode_wav', batch=BATCH, **KW)
    assert as_is.probs.tobytes() == stream.spot(model, samples, batch=BATCH, **KW).probs.tobytes()
