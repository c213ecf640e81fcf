"""Keyword spotting in recordings of any length (csrc/stream.hip, kws_stream_*): which keyword occurs where.

A recording is cut on the device into overlapping windows of the model's input size (`frames`: one gather launch per chunk,
the recording is uploaded once and the windows never exist on the host), every chunk of windows goes through the net's
inference program, the posterior track [W, classes] is averaged over the last `A` windows and reduced to its top class per
window in one launch (`smooth`), and a host-side state machine (`detect`: threshold, minimum count, suppression) turns the
two per-window tracks into detections.  `spot` is the whole chain, `spot_wav` the same from a wav file of any sample rate,
`score` counts detections against a ground truth.

The feature-input models ('mfcc', 'spec', 'mfcc_and_raw') take `spot(..., features=Features(model_settings))`: every chunk
of windows is one signal to the STFT, and window w is frames w r .. w r + F - 1 of the chunk's feature track, cut out by
kws_stream_gather_f32 (`Features.rows`) - a frame depends on its own samples only, so the rows are those of the per-window
feature step (`Features.windows`) bit for bit.

Out of scope: shared STFT frames for a hop that is no multiple of the frame step (`share_frames=False` computes every
window's own) and across chunk seams (the F - r frames two neighbouring chunks have in common are computed by both: 96 of
2144 at hop 320, batch 1024), data-parallel sharding of one recording, peak picking inside a run of eligible windows (the
first eligible window fires), carrying convolution state from window to window."""
import ctypes

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


def gather(src, n, start, hop, win, out, out_pitch, count, out_offset=0):
    """kws_stream_gather_f32 on device float32 tensors: out.flat[out_offset + w out_pitch + i] = src.flat[start + w hop + i]
    for w < count, i < win, +0.0 where that index is outside [0, n); a copy of bits, nothing else of `out` is written."""
    if not (src.is_cuda and out.is_cuda and src.dtype == torch.float32 and out.dtype == torch.float32
            and src.is_contiguous() and out.is_contiguous()):
        raise ValueError("gather: src and out must be contiguous float32 device tensors")
    n, count, win, out_pitch, out_offset = int(n), int(count), int(win), int(out_pitch), int(out_offset)
    if n > src.numel() or out_offset < 0 or (count >= 1 and out_offset + (count - 1) * out_pitch + win > out.numel()):
        raise ValueError("gather: n=%d of %d source floats, rows up to %d of %d output floats" %
                         (n, src.numel(), out_offset + (count - 1) * out_pitch + win, out.numel()))
    with torch.cuda.device(out.device):
        _lib.call("kws_stream_gather_f32", _lib.ptr(src) if n else None, n, int(start), int(hop), win,
                  ctypes.c_void_p(out.data_ptr() + 4 * out_offset), out_pitch, count, _lib.stream_ptr())
    return out


def plan_rows(count, hop, win, frame_len, step):
    """The chunk of `count` windows, `hop` apart, as ONE signal for the STFT (host only) -> (Lc, J, r): Lc samples =
    (count - 1) hop + win rounded up to a multiple of 4, r = hop / step frames between two windows, J = (count - 1) r + F
    frames of which window w takes w r .. w r + F - 1, F = 1 + (win - frame_len) // step.  Frame w r + k of the signal
    starts at sample w hop + k step, where frame k of window w starts: the same frame_len samples."""
    count, hop, win, frame_len, step = int(count), int(hop), int(win), int(frame_len), int(step)
    if count < 1 or hop < 1 or step < 1 or frame_len < 1 or win < frame_len:
        raise ValueError("plan_rows: count=%d hop=%d win=%d frame_len=%d step=%d" % (count, hop, win, frame_len, step))
    if hop % step:
        raise ValueError("plan_rows: hop=%d is not a multiple of the frame step=%d, so overlapping windows share no STFT "
                         "frames (spot(..., share_frames=False) computes every window's own)" % (hop, step))
    r = hop // step
    F = 1 + (win - frame_len) // step
    return -(-((count - 1) * hop + win) // 4) * 4, (count - 1) * r + F, r


class Features(object):
    """The feature step of the feature-input models for `spot`: the path-B STFT / mel / DCT features AudioProcessor feeds
    them (the same plan: features.path_b_plan), per window (`windows`) or once per chunk on a track the overlapping windows
    share (`rows`).  model_settings: model.prepare_model_settings' dict; the representation - 'mfcc', 'spec' or
    'mfcc_and_raw' - is its 'output_representation' entry or the keyword (prepare_model_settings takes it and does not
    return it).  win = desired_samples, frame_len / step = the framing, F frames per window of `width` values, row = the
    model's input size: F width, and the window's win samples behind them for 'mfcc_and_raw'.
    The plan and the reused chunk buffers belong to one stream at a time; close() frees the plan."""
    OUT_KINDS = {'mfcc': 0, 'spec': 1, 'mfcc_and_raw': 0}        # kws_stft_mel_f32's out_kind, as AudioProcessor.get_data
    _KEYS = ('desired_samples', 'window_size_samples', 'window_stride_samples', 'dct_coefficient_count',
             'num_log_mel_features', 'sample_rate')

    def __init__(self, model_settings, device=None, output_representation=None):
        self._plan = None
        rep = output_representation if output_representation is not None else model_settings.get('output_representation')
        if rep is None:
            raise ValueError("Features: model_settings has no 'output_representation' (one of %s)" % sorted(self.OUT_KINDS))
        if rep not in self.OUT_KINDS:
            raise ValueError("Features: output_representation=%r - the raw-waveform models take the windows themselves; "
                             "one of %s" % (rep, sorted(self.OUT_KINDS)))
        for k in self._KEYS:
            if k not in model_settings:
                raise ValueError("Features: model_settings has no %r" % k)
        self.representation = rep
        self.out_kind = self.OUT_KINDS[rep]
        self.win = int(model_settings['desired_samples'])
        self.frame_len = int(model_settings['window_size_samples'])
        self.step = int(model_settings['window_stride_samples'])
        self.width = 257 if rep == 'spec' else int(model_settings['num_log_mel_features'])
        if self.step < 1 or self.win < self.frame_len or self.frame_len < 1:
            raise ValueError("Features: a window of %d samples holds no frame of %d (step %d)" % (self.win, self.frame_len, self.step))
        self.device = torch.device(device) if device is not None else torch.device("cuda", torch.cuda.current_device())
        self.lib = _lib.load()
        from .features import path_b_plan
        with torch.cuda.device(self.device):
            self._plan = path_b_plan(model_settings)
        self.F = self.lib.kws_stft_num_frames(self._plan, self.win)
        self.row = self.F * self.width + (self.win if rep == 'mfcc_and_raw' else 0)
        self._P = self._track = None

    def close(self):
        if getattr(self, '_plan', None):
            self.lib.kws_stft_plan_destroy(self._plan)
            self._plan = None
        self._P = self._track = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def kernel_code(self, L, x=None):
        """kws_stft_mel_kernel: which kernel the feature launch over signals of L samples at x (default: a 16-byte aligned
        buffer, as every buffer of this class is) answers to."""
        return self.lib.kws_stft_mel_kernel(self._plan, _lib.ptr(x) if x is not None else ctypes.c_void_p(16), int(L), self.out_kind)

    def _stft(self, x, B, L, out):
        if self._plan is None:
            raise _lib.KwsError("Features is closed: its STFT plan is gone")
        _lib.call("kws_stft_mel_f32", self._plan, _lib.ptr(x), B, L, _lib.ptr(out), self.out_kind, _lib.stream_ptr())

    def _out(self, out, count):
        if out is None:
            return torch.empty((count, self.row), dtype=torch.float32, device=self.device)
        if not (torch.is_tensor(out) and out.is_cuda and out.dtype == torch.float32 and out.is_contiguous()
                and out.numel() >= count * self.row):
            raise ValueError("Features: out must be a contiguous float32 device tensor of at least count * row elements")
        return out

    def windows(self, chunk, out=None):
        """The per-window definition: device float32 windows [count, win] -> model input [count, row] by one
        kws_stft_mel_f32 over the count windows (what AudioProcessor feeds the model); for 'mfcc_and_raw' the features land
        in a dense buffer and two gathers lay them and the window's samples into the composite rows."""
        if not (torch.is_tensor(chunk) and chunk.is_cuda and chunk.dtype == torch.float32 and chunk.dim() == 2
                and chunk.shape[1] == self.win):
            raise ValueError("Features.windows: a float32 device tensor [count, %d] is needed" % self.win)
        chunk = chunk.contiguous()
        count, fw = chunk.shape[0], self.F * self.width
        out = self._out(out, count)
        with torch.cuda.device(self.device):
            if self.row == fw:
                self._stft(chunk, count, self.win, out)
            else:
                dense = torch.empty((count, fw), dtype=torch.float32, device=self.device)
                self._stft(chunk, count, self.win, dense)
                gather(dense, count * fw, 0, fw, fw, out, self.row, count)
                gather(chunk, count * self.win, 0, self.win, self.win, out, self.row, count, out_offset=fw)
        return out.reshape(-1)[:count * self.row].reshape(count, self.row)

    def rows(self, x, hop, start, first, count, out=None):
        """The shared path: the model input [count, row] of windows first .. first + count - 1 (window w starts at sample
        start + w hop of the recording x; zeros outside it), bit for bit windows(frames(...)) of them, with every STFT frame
        of the chunk computed once.  hop must be a multiple of the frame step.  The chunk's Lc samples (plan_rows) are
        gathered as one window into a reused buffer (the per-window gather's own multiply and zero fill), one
        kws_stft_mel_f32 turns them into a reused track [J', width], J' >= J, and kws_stream_gather_f32 cuts window w's F
        frames out of it from frame w r on; for 'mfcc_and_raw' a second gather puts the window's samples behind them."""
        hop, start, first, count = int(hop), int(start), int(first), int(count)
        if hop % self.step:
            raise ValueError("Features.rows: hop=%d is not a multiple of the frame step=%d, so overlapping windows share no "
                             "STFT frames (share_frames=False computes every window's own)" % (hop, self.step))
        if first < 0:
            raise ValueError("Features.rows: first=%d count=%d" % (first, count))
        Lc, J, r = plan_rows(count, hop, self.win, self.frame_len, self.step)
        if Lc >= 1 << 31:
            raise ValueError("Features.rows: a chunk of %d windows is %d samples, more than one STFT launch takes" % (count, Lc))
        xd = _device_samples(x, self.device)
        out = self._out(out, count)
        with torch.cuda.device(self.device):
            Jt = self.lib.kws_stft_num_frames(self._plan, Lc)       # >= J: the rounding of Lc may add a frame
            if self._P is None or self._P.numel() < Lc:
                self._P = torch.empty(Lc, dtype=torch.float32, device=self.device)
            if self._track is None or self._track.numel() < Jt * self.width:
                self._track = torch.empty(Jt * self.width, dtype=torch.float32, device=self.device)
            P, track = self._P, self._track
            frames(xd, Lc, Lc, start=start + first * hop, first=0, count=1, out=P)
            self._stft(P, 1, Lc, track)
            fw = self.F * self.width
            gather(track, J * self.width, 0, r * self.width, fw, out, self.row, count)
            if self.row != fw:
                gather(P, Lc, 0, hop, self.win, out, self.row, count, out_offset=fw)
        return out.reshape(-1)[:count * self.row].reshape(count, self.row)


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
         batch=1024, start=0, transform=None, sample_rate=16000, win=None, features=None, share_frames=True):
    """Keywords in a recording.  audio: 1-D int16 or float32 samples at `sample_rate` (tensor or array; int16 is scaled by
    1 / 32768 like DecodeWav).  The windows (win = the net's input size; with `transform`, a callable from device windows
    [count, win] to model input [count, input_size] such as an AudioProcessor's feature step, `win` is given) are hop samples
    apart and go through the net in chunks of `batch` on one stream without a host synchronisation; the posteriors are averaged
    over A = max(1, average_ms sample_rate // (1000 hop)) windows.  ignore: class indices that never fire - by default
    _silence_ and _unknown_, positions 0 and 1 of input_data.prepare_words_list.  See `detect` for the decision.
    features: a `Features` for a feature-input model (win = features.win).  With share_frames (the default; hop must be a
    multiple of the frame step) every chunk is features.rows - each STFT frame of the chunk computed once - otherwise
    features.windows runs on every window as a transform would; the posteriors are the same bit for bit."""
    net = model.net
    shared = False
    if features is not None:
        if transform is not None:
            raise ValueError("spot: features and transform are two ways to say the same thing - pass one")
        if features.row != net.input_size:
            raise ValueError("spot: features.row=%d but the model takes rows of %d" % (features.row, net.input_size))
        if win is not None and int(win) != features.win:
            raise ValueError("spot: win=%d but features.win=%d" % (int(win), features.win))
        win = features.win
        shared = bool(share_frames)
        if shared:
            plan_rows(1, hop, features.win, features.frame_len, features.step)      # refuses a hop that shares no frames
        else:
            transform = features.windows
    if transform is None and not shared:
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
        buf = torch.empty((min(batch, W), features.row if shared else win), dtype=torch.float32, device=net.device)
        probs = torch.empty((W, net.num_classes), dtype=torch.float32, device=net.device)
        for w0 in range(0, W, batch):
            w1 = min(w0 + batch, W)
            if shared:
                net.predict(features.rows(xd, hop, start, w0, w1 - w0, out=buf), out=probs[w0:w1])
                continue
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
