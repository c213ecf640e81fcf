"""Keyword spotting in recordings of any length (csrc/stream.hip, kws_stream_*): which keyword occurs where.

A recording is cut on the device into overlapping windows of the model's input size (`frames`: one gather launch per chunk,
the recording is uploaded once and the windows never exist on the host), every chunk of windows goes through the net's
inference program, the posterior track [W, classes] is averaged over the last `A` windows and reduced to its top class per
window in one launch (`smooth`), and a host-side state machine (`detect`: threshold, minimum count, suppression) turns the
two per-window tracks into detections.  `spot` is the whole chain, `spot_wav` the same from a wav file of any sample rate,
`score` counts detections against a ground truth.

Out of scope: sharing STFT frames between overlapping windows of the feature-input models (a `transform` runs on every
window), data-parallel sharding of one recording, peak picking inside a run of eligible windows (the first eligible window
fires), carrying convolution state from window to window."""
import numpy as np
import torch

from . import _lib

INT16_SCALE = 1.0 / 32768.0       # DecodeWav


def plan_windows(n, win, hop, start=0):
    """The number of windows that covers n samples: the smallest W >= 1 with start + (W - 1) hop + win >= n (host only).
    Every sample from `start` on is then inside some window (hop <= win) and the last window is zero padded."""
    n, win, hop, start = int(n), int(win), int(hop), int(start)
    if win < 1 or hop < 1 or n < 0:
        raise ValueError("plan_windows: n=%d win=%d hop=%d" % (n, win, hop))
    need = n - win - start                     # (W - 1) hop >= need
    return 1 if need <= 0 else 1 + -(-need // hop)


def _device_samples(x, device=None):
    """x as a contiguous 1-D int16 or float32 tensor on the device (uploaded if it is on the host)."""
    dev = torch.device(device) if device is not None else torch.device("cuda", torch.cuda.current_device())
    if not torch.is_tensor(x):
        a = np.asarray(x)
        if a.dtype not in (np.int16, np.float32):
            raise ValueError("stream: samples must be int16 or float32, not %s" % a.dtype)
        x = torch.from_numpy(np.ascontiguousarray(a))
    if x.dtype not in (torch.int16, torch.float32):
        raise ValueError("stream: samples must be int16 or float32, not %s" % x.dtype)
    if x.dim() != 1:
        raise ValueError("stream: samples must be 1-D, not %s" % (tuple(x.shape),))
    if not x.is_cuda:
        x = x.to(dev)
    return x.contiguous()


def frames(x, win, hop, start=0, first=0, count=None, scale=None, out=None):
    """Windows first .. first + count - 1 of the recording x (1-D int16 or float32, tensor or array; uploaded once if it is
    on the host) as a float32 device tensor [count, win]: window w holds scale * x[start + w hop + i], zeros outside x.
    count defaults to the windows from `first` to plan_windows' last; scale to 1 / 32768 for int16 (DecodeWav) and 1 for float.
    out: an optional contiguous float32 device buffer of at least count * win elements that receives the windows."""
    xd = _device_samples(x, out.device if out is not None else None)
    n = xd.shape[0]
    win, hop, start, first = int(win), int(hop), int(start), int(first)
    if count is None:
        count = plan_windows(n, win, hop, start) - first
    count = int(count)
    if count < 1 or first < 0:
        raise ValueError("frames: first=%d count=%d" % (first, count))
    i16 = xd.dtype == torch.int16
    if scale is None:
        scale = INT16_SCALE if i16 else 1.0
    if out is None:
        out = torch.empty((count, win), dtype=torch.float32, device=xd.device)
    elif not (torch.is_tensor(out) and out.is_cuda and out.dtype == torch.float32 and out.is_contiguous()
              and out.numel() >= count * win):
        raise ValueError("frames: out must be a contiguous float32 device tensor of at least count * win elements")
    with torch.cuda.device(xd.device):
        _lib.call("kws_stream_frames_i16" if i16 else "kws_stream_frames_f32", _lib.ptr(xd) if n else None, n,
                  start + first * hop, hop, win, float(scale), _lib.ptr(out), count, _lib.stream_ptr())
    return out.reshape(-1)[:count * win].reshape(count, win)


def smooth(probs, average_windows):
    """probs [W, NC] (float32; uploaded if on the host) -> (smoothed [W, NC] f32, top [W] int32, top_score [W] f32) as device
    tensors: the mean of the last min(w + 1, average_windows) rows, its lowest-index maximum and that maximum's value."""
    if not torch.is_tensor(probs):
        probs = torch.from_numpy(np.ascontiguousarray(probs, dtype=np.float32))
    if not probs.is_cuda:
        probs = probs.to(torch.device("cuda", torch.cuda.current_device()))
    if probs.dim() != 2 or probs.dtype != torch.float32:
        raise ValueError("smooth: probs must be float32 [W, NC]")
    probs = probs.contiguous()
    W, NC = probs.shape
    smoothed = torch.empty_like(probs)
    top = torch.empty(W, dtype=torch.int32, device=probs.device)
    top_score = torch.empty(W, dtype=torch.float32, device=probs.device)
    with torch.cuda.device(probs.device):
        _lib.call("kws_stream_smooth_f32", _lib.ptr(probs), W, NC, int(average_windows), _lib.ptr(smoothed), _lib.ptr(top),
                  _lib.ptr(top_score), _lib.stream_ptr())
    return smoothed, top, top_score


def counts_ok(W, average_windows, minimum_count):
    """[W] bool: window w's average runs over at least minimum_count windows, min(w + 1, A) >= minimum_count (host only)."""
    return np.minimum(np.arange(1, int(W) + 1, dtype=np.int64), int(average_windows)) >= int(minimum_count)


def detect(top, top_score, counts_ok, hop, win, start=0, threshold=0.7, suppression_samples=16000, ignore=(0, 1)):
    """The decision state machine over the per-window tracks (host only, NumPy).  Windows are walked in ascending order;
    window w ends at sample end_w = start + w hop + win and is eligible when counts_ok[w] holds, top[w] is not in `ignore`
    and top_score[w] >= float32(threshold).  An eligible window fires when nothing has fired yet or when
    end_w - (end of the last fire) >= suppression_samples (integers).  -> [(label index, w, end_w, score)]."""
    top = np.asarray(top).reshape(-1)
    top_score = np.asarray(top_score, dtype=np.float32).reshape(-1)
    ok = np.asarray(counts_ok, dtype=bool).reshape(-1)
    if not (len(top) == len(top_score) == len(ok)):
        raise ValueError("detect: top, top_score and counts_ok must have one entry per window")
    eligible = ok & (top_score >= np.float32(threshold))
    if len(ignore):
        eligible &= ~np.isin(top, np.asarray(list(ignore), dtype=top.dtype if top.size else np.int64))
    hop, win, start, suppression_samples = int(hop), int(win), int(start), int(suppression_samples)
    fires, last_end = [], None
    for w in np.nonzero(eligible)[0]:
        end_w = start + int(w) * hop + win
        if last_end is None or end_w - last_end >= suppression_samples:
            fires.append((int(top[w]), int(w), end_w, float(top_score[w])))
            last_end = end_w
    return fires


class Spotted(object):
    """What `spot` returns: detections [(label, time_s, sample, score)] (sample = the firing window's end, label a name when
    labels were given), the tracks probs / smoothed [W, NC], top / top_score [W] as NumPy arrays, and W, hop, win."""

    def __init__(self, **kw):
        self.__dict__.update(kw)

    def __repr__(self):
        return "Spotted(W=%d, hop=%d, win=%d, detections=%r)" % (self.W, self.hop, self.win, self.detections)


def spot(model, audio, labels=None, hop=320, average_ms=500, threshold=0.7, suppression_ms=1000, minimum_count=3, ignore=(0, 1),
         batch=1024, start=0, transform=None, sample_rate=16000, win=None):
    """Keywords in a recording.  audio: 1-D int16 or float32 samples at `sample_rate` (tensor or array; int16 is scaled by
    1 / 32768 like DecodeWav).  The windows (win = the net's input size; with `transform`, a callable from device windows
    [count, win] to model input [count, input_size] such as an AudioProcessor's feature step, `win` is given) are hop samples
    apart and go through the net in chunks of `batch` on one stream without a host synchronisation; the posteriors are averaged
    over A = max(1, average_ms sample_rate // (1000 hop)) windows.  ignore: class indices that never fire - by default
    _silence_ and _unknown_, positions 0 and 1 of input_data.prepare_words_list.  See `detect` for the decision."""
    net = model.net
    if transform is None:
        win = net.input_size if win is None else int(win)
        if win != net.input_size:
            raise ValueError("spot: win=%d but the model takes %d samples (pass a transform)" % (win, net.input_size))
    elif win is None:
        raise ValueError("spot: with a transform, win (the samples per window) must be given")
    win, hop, start, batch = int(win), int(hop), int(start), int(batch)
    if batch < 1:
        raise ValueError("spot: batch=%d" % batch)
    A = max(1, int(average_ms) * int(sample_rate) // (1000 * hop))
    suppression_samples = int(suppression_ms) * int(sample_rate) // 1000
    with torch.cuda.device(net.device):
        xd = _device_samples(audio, net.device)
        W = plan_windows(xd.shape[0], win, hop, start)
        buf = torch.empty((min(batch, W), win), dtype=torch.float32, device=net.device)
        probs = torch.empty((W, net.num_classes), dtype=torch.float32, device=net.device)
        for w0 in range(0, W, batch):
            w1 = min(w0 + batch, W)
            chunk = frames(xd, win, hop, start=start, first=w0, count=w1 - w0, out=buf)
            if transform is not None:
                chunk = transform(chunk)
                if not (torch.is_tensor(chunk) and chunk.is_cuda and chunk.dtype == torch.float32
                        and tuple(chunk.shape) == (w1 - w0, net.input_size)):
                    raise ValueError("spot: transform must return a float32 device tensor [%d, %d], not %s" %
                                     (w1 - w0, net.input_size, tuple(chunk.shape) if torch.is_tensor(chunk) else type(chunk)))
                chunk = chunk.contiguous()
            net.predict(chunk, out=probs[w0:w1])
        smoothed, top, top_score = smooth(probs, A)
        top_h, score_h = top.cpu().numpy(), top_score.cpu().numpy()     # the one wait for the device
    fires = detect(top_h, score_h, counts_ok(W, A, minimum_count), hop, win, start=start, threshold=threshold,
                   suppression_samples=suppression_samples, ignore=ignore)
    names = list(labels) if labels is not None else None
    detections = [(names[c] if names is not None else c, end / float(sample_rate), end, s) for c, _, end, s in fires]
    return Spotted(detections=detections, probs=probs.cpu().numpy(), smoothed=smoothed.cpu().numpy(), top=top_h, top_score=score_h,
                   W=W, hop=hop, win=win, average_windows=A, fires=fires)


def spot_wav(model, filename, labels=None, rate_policy='resample', sample_rate=16000, **kwargs):
    """`spot` on a 16-bit PCM wav file (first channel).  rate_policy, as in input_data.decode_wav_files: 'resample' converts a
    file at another rate to `sample_rate` on the device (resample.py, the recording as one long row; it never comes back to
    the host), 'error' raises ValueError for such a file, 'decode_wav' ignores the header's rate like DecodeWav."""
    from . import input_data
    if rate_policy not in input_data.RATE_POLICIES:
        raise ValueError('rate_policy must be one of %r, not %r' % (input_data.RATE_POLICIES, rate_policy))
    samples, rate = input_data._read_wav_int16(filename)
    if rate_policy == 'error':
        input_data.check_wav_rates([filename], sample_rate)
    device = model.net.device
    x = torch.from_numpy(np.ascontiguousarray(samples, dtype=np.int16)).to(device)
    if rate_policy == 'resample' and rate != sample_rate and x.shape[0]:
        from . import resample as rs
        keep = rs.resampled_samples(x.shape[0], rate, sample_rate)
        x = rs.resample_rows(x.reshape(1, -1), None, rate, sample_rate, keep)[0].reshape(-1)
    return spot(model, x, labels=labels, sample_rate=sample_rate, **kwargs)


def score(detections, truth, tolerance_samples):
    """Detections against a ground truth (host only): greedy one-to-one matching in time order.  detections: `spot`'s
    [(label, time_s, sample, score)]; truth: [(label, sample)].  Each detection, earliest first, takes the earliest still
    unmatched truth within tolerance_samples of it: 'correct' when the labels agree, 'wrong_label' when not; a detection
    with no such truth is a 'false_positive', a truth nothing took is 'missed'.  -> dict of the four counts."""
    tol = int(tolerance_samples)
    dets = sorted(((int(d[2]), d[0]) for d in detections), key=lambda t: t[0])
    tru = sorted(((int(t[1]), t[0]) for t in truth), key=lambda t: t[0])
    taken = [False] * len(tru)
    out = {'correct': 0, 'wrong_label': 0, 'false_positive': 0, 'missed': 0}
    for sample, label in dets:
        hit = next((k for k, (ts, _) in enumerate(tru) if not taken[k] and abs(ts - sample) <= tol), None)
        if hit is None:
            out['false_positive'] += 1
            continue
        taken[hit] = True
        out['correct' if tru[hit][1] == label else 'wrong_label'] += 1
    out['missed'] = taken.count(False)
    return out
