"""AudioProcessor: dataset index, sampler and batched on-GPU augmentation / feature extraction.

Host-side mirror of the reference's `input_data.py` interface (same names, argument meaning and
error behaviour; reference input_data.py:49-610) for the accelerated path:

  * index construction (`which_set`, `prepare_data_index`) is host glue, restated here;
  * every wav of the index is decoded ONCE into an HBM-resident int16 clip bank (DecodeWav
    semantics: int16/32768, mono, pad/crop to desired_samples; reference input_data.py:335-336);
  * `get_data` draws the per-clip augmentation parameters on the host in exactly the reference's
    NumPy-global-RNG order (input_data.py:457-514) and then issues ONE
    `kws_augment_*` launch (+ ONE `kws_stft_mel_f32` launch for 'mfcc'/'spec') for the whole batch
    instead of one `sess.run` per clip; the batch stays on the GPU (DeviceArray).
"""
from __future__ import absolute_import, division, print_function

import glob
import hashlib
import math
import os
import os.path
import random
import re
import struct
import sys
import threading

import numpy as np
import torch

from . import _lib
from .device_array import DeviceArray, Labels

from .sampler import (BACKGROUND_NOISE_DIR_NAME, MAX_NUM_WAVS_PER_CLASS, RANDOM_SEED, SILENCE_INDEX,  # noqa: F401
                      SILENCE_LABEL, UNKNOWN_WORD_INDEX, UNKNOWN_WORD_LABEL, DataIndex, prepare_words_list,
                      which_set)


_TLS = threading.local()      # which _lib.Profiler the current thread is attached to (AudioProcessor.get_data)


# ---- wav I/O (host glue; TF DecodeWav / EncodeWav semantics for 16-bit PCM) ------------------------
def _read_wav_int16(filename):
    with open(filename, 'rb') as f:
        data = f.read()
    if len(data) < 12 or data[:4] != b'RIFF' or data[8:12] != b'WAVE':
        raise ValueError('%s is not a RIFF/WAVE file' % filename)
    pos, fmt, pcm = 12, None, None
    while pos + 8 <= len(data):
        cid, size = data[pos:pos + 4], struct.unpack('<I', data[pos + 4:pos + 8])[0]
        body = data[pos + 8:pos + 8 + size]
        if cid == b'fmt ':
            fmt = struct.unpack('<HHIIHH', body[:16])
        elif cid == b'data':
            pcm = body
            break
        pos += 8 + size + (size & 1)
    if fmt is None or pcm is None:
        raise ValueError('%s: missing fmt/data chunk' % filename)
    audio_format, channels, rate, _, _, bits = fmt
    if audio_format != 1 or bits != 16:
        raise ValueError('%s: only 16-bit PCM is supported (DecodeWav)' % filename)
    a = np.frombuffer(pcm[:len(pcm) // (2 * channels) * 2 * channels], dtype='<i2').reshape(-1, channels)
    return a[:, 0].copy(), rate


def load_wav_file(filename):
    """float PCM in [-1, 1): int16 / 32768 (reference input_data.py:117-132)."""
    a, _ = _read_wav_int16(filename)
    return a.astype(np.float32) / np.float32(32768.0)


def save_wav_file(filename, wav_data, sample_rate):
    """EncodeWav: clamp(x)*32767 -> int16 (reference input_data.py:135-156)."""
    x = np.clip(np.asarray(wav_data, dtype=np.float32).reshape(-1), -1.0, 1.0)
    pcm = (x * 32767.0).astype('<i2').tobytes()
    with open(filename, 'wb') as f:
        f.write(b'RIFF' + struct.pack('<I', 36 + len(pcm)) + b'WAVE' + b'fmt ' +
                struct.pack('<IHHIIHH', 16, 1, 1, int(sample_rate), int(sample_rate) * 2, 2, 16) +
                b'data' + struct.pack('<I', len(pcm)) + pcm)


def bank_from_files(file_row, desired_samples):
    """Host image of the int16 clip bank: row r = the first `desired_samples` samples of file r's first channel,
    zero padded (DecodeWav with desired_channels=1, desired_samples; reference input_data.py:335-336)."""
    bank = np.zeros((max(len(file_row), 1), desired_samples), dtype=np.int16)
    for fn, r in file_row.items():
        a, _ = _read_wav_int16(fn)
        n = min(len(a), desired_samples)
        bank[r, :n] = a[:n]
    return bank


RATE_POLICIES = ('decode_wav', 'error', 'resample')
RESAMPLE_CHUNK_FILES = 2048      # files per kws_resample_i16 launch of decode_wav_files


def group_files_by_rate(filenames):
    """[(rate, [(position in `filenames`, int16 samples)])] in ascending rate order; every file is read once."""
    groups = {}
    for k, fn in enumerate(filenames):
        a, rate = _read_wav_int16(fn)
        groups.setdefault(int(rate), []).append((k, a))
    return sorted(groups.items())


def check_wav_rates(filenames, sample_rate):
    """rate_policy='error': ValueError naming the first file whose header rate differs from `sample_rate`."""
    for fn in filenames:
        rate = _read_wav_int16(fn)[1]
        if rate != sample_rate:
            raise ValueError('%s has a sample rate of %d Hz, not %d (wav_rate_policy=\'error\'; \'resample\' converts it, '
                             '\'decode_wav\' ignores the header like DecodeWav)' % (fn, rate, sample_rate))


def decode_wav_files(filenames, desired_samples, sample_rate, device, rate_policy='decode_wav'):
    """The int16 clip bank rows of `filenames` as a device tensor [n, desired_samples] (row k = file k, first channel,
    cropped / zero padded).  rate_policy:
      'decode_wav'  the header's sample rate is ignored (DecodeWav; the bytes of bank_from_files);
      'error'       ValueError for the first file whose rate is not `sample_rate`;
      'resample'    files at another rate are resampled to `sample_rate` on the device (resample.py): each rate's files
                    go up padded, with their lengths, in chunks of at most RESAMPLE_CHUNK_FILES and every chunk is one
                    kws_resample_i16 launch that crops / pads to desired_samples; files already at `sample_rate` take the
                    'decode_wav' path."""
    if rate_policy not in RATE_POLICIES:
        raise ValueError('rate_policy must be one of %r, not %r' % (RATE_POLICIES, rate_policy))
    filenames = list(filenames)
    if rate_policy == 'error':
        check_wav_rates(filenames, sample_rate)
    if rate_policy != 'resample':
        bank = bank_from_files({fn: k for k, fn in enumerate(filenames)}, desired_samples)[:len(filenames)]
        return torch.from_numpy(bank).to(device)
    from . import resample as rs
    out = torch.zeros((len(filenames), desired_samples), dtype=torch.int16, device=device)
    for rate, files in group_files_by_rate(filenames):
        if rate != sample_rate:
            rs.design(rate, sample_rate)          # a rate the library refuses fails before anything is uploaded
        for c in range(0, len(files), RESAMPLE_CHUNK_FILES):
            chunk = files[c:c + RESAMPLE_CHUNK_FILES]
            rows = torch.tensor([k for k, _ in chunk], dtype=torch.int64, device=device)
            if rate == sample_rate:
                host = np.zeros((len(chunk), desired_samples), dtype=np.int16)
                for i, (_, a) in enumerate(chunk):
                    host[i, :min(len(a), desired_samples)] = a[:desired_samples]
                out[rows] = torch.from_numpy(host).to(device)
                continue
            # only the samples the first desired_samples outputs depend on travel: ceil(desired_samples down / up) plus the
            # filter's reach on the right; the row's true length (capped there) still decides where the zeros start
            up, down, half, _ = rs.design(rate, sample_rate)
            need = -(-(desired_samples * down + half) // up) + 1
            lens = np.array([min(len(a), need) for _, a in chunk], dtype=np.int32)
            host = np.zeros((len(chunk), max(int(lens.max()), 1)), dtype=np.int16)
            for i, (_, a) in enumerate(chunk):
                host[i, :lens[i]] = a[:lens[i]]
            o16, _ = rs.resample_rows(torch.from_numpy(host).to(device), torch.from_numpy(lens).to(device), rate, sample_rate,
                                      desired_samples)
            out[rows] = o16
    return out


def resample_recording(samples_i16, rate, sample_rate, device):
    """One int16 recording of any length (a background noise file) at `sample_rate`, resampled as ONE long row: the int16
    host array a file converted to `sample_rate` would hold (rounded half to even, saturated)."""
    from . import resample as rs
    x = torch.from_numpy(np.ascontiguousarray(samples_i16, dtype=np.int16).reshape(1, -1)).to(device)
    keep = rs.resampled_samples(x.shape[1], rate, sample_rate)
    o16, _ = rs.resample_rows(x, None, rate, sample_rate, keep)
    return o16.reshape(-1).cpu().numpy()


class _Placeholder(object):
    """Opaque feed key standing in for a tf.placeholder of the reference's processing graph."""

    def __init__(self, name):
        self.name = name

    def __repr__(self):
        return '<placeholder %s>' % self.name


class _Fetch(object):
    def __init__(self, owner, kind):
        self.owner, self.kind = owner, kind


class ClipBank(object):
    """HBM-resident clips [n, L] (int16 PCM or f32) + background recordings, plus the metadata the
    index needs.  `from_arrays` builds the synthetic banks used by bench.py and the tests."""

    def __init__(self, clips, noise_list, device):
        self.device = device
        self.clips = clips                      # torch tensor on device, int16 or float32
        self.noise_host = [np.asarray(n, dtype=np.float32) for n in noise_list]
        self.noise_starts = np.cumsum([0] + [len(n) for n in self.noise_host])[:-1].astype(np.int64)
        if self.noise_host:
            self.noise = torch.from_numpy(np.concatenate(self.noise_host)).to(device)
        else:
            self.noise = None

    @property
    def n_clips(self):
        return self.clips.shape[0]

    @property
    def samples(self):
        return self.clips.shape[1]


class AudioProcessor(object):
    """Handles loading, partitioning, and preparing audio training data (reference
    input_data.py:159-610); see the module docstring for what runs where."""

    def __init__(self, data_dirs, silence_percentage, unknown_percentage, wanted_words, validation_percentage,
                 testing_percentage, model_settings, output_representation=False, device=None,
                 wav_rate_policy='decode_wav'):
        """wav_rate_policy (not in the reference): what a wav whose header rate is not model_settings['sample_rate'] means -
        'decode_wav' ignores the header like the reference's DecodeWav (the default), 'error' refuses the file, 'resample'
        converts it on the device (decode_wav_files)."""
        if wav_rate_policy not in RATE_POLICIES:
            raise ValueError('wav_rate_policy must be one of %r, not %r' % (RATE_POLICIES, wav_rate_policy))
        self.wav_rate_policy = wav_rate_policy
        if not torch.cuda.is_available():
            raise _lib.KwsError("AudioProcessor needs an MI355X: augmentation and features run on the GPU "
                                "(no CPU fallback)")
        self.lib = _lib.load()
        self.device = torch.device(device if device is not None else "cuda:%d" % torch.cuda.current_device())
        self.data_dirs = data_dirs
        assert output_representation in {'raw', 'spec', 'mfcc', 'mfcc_and_raw'}
        self.output_representation = output_representation
        self.model_settings = model_settings
        # the generator's own stream, LOW priority: augment + STFT fill the CUs the training stream leaves idle instead of
        # co-running with its MFMA kernels (round 2 measured low / normal / high: the step time does not move, the
        # generator's own kernels run 40 % shorter on the low one).  The handle is ours: close() destroys it.
        self._own_stream = _lib.OwnedStream(self.device, -1)
        self._stream_obj = self._own_stream.stream
        self.profiler = None            # a _lib.Profiler: get_data() attaches the calling (generator) thread to it
        self._plan = None
        self._synthetic = isinstance(data_dirs, dict)
        if self._synthetic:
            self._init_synthetic(data_dirs, wanted_words)
        else:
            for data_dir in self.data_dirs:
                self.maybe_download_and_extract_dataset(data_dir)
            self.prepare_data_index(silence_percentage, unknown_percentage, wanted_words, validation_percentage,
                                    testing_percentage)
            self.prepare_background_data()
            self._build_bank()
        self.prepare_processing_graph(model_settings)

    def close(self):
        """Drain the generator stream, then free the STFT plan and the stream this processor created."""
        own = getattr(self, '_own_stream', None)
        if own is not None and own.stream is not None:
            try:
                import torch
                own.stream.synchronize()
                # torch's pinned-memory cache holds events recorded on this stream (the non_blocking parameter uploads of
                # _augment): they must be retired while the stream still exists - a later query of an event whose stream is gone,
                # or whose handle a NEW stream got, fails ("event last recorded in a capturing stream", round 5).  Explicitly:
                # the device is drained (every such event has completed) and the pinned cache is emptied (it processes and
                # frees its events); an allocation through the cache is the fallback on a torch without that entry point.
                torch.cuda.synchronize(self.device)
                empty = getattr(torch._C, "_host_emptyCache", None)
                if empty is not None:
                    empty()
                else:
                    torch.empty(16).pin_memory()
            except Exception as ex:       # closing must not raise - but a failure here is the round-5 bug coming back: say so
                sys.stderr.write("AudioProcessor.close(): retiring the generator stream's pinned-memory events failed: %r\n" % (ex,))
        if getattr(self, '_plan', None):
            self.lib.kws_stft_plan_destroy(self._plan)
            self._plan = None
        self._stream_obj = None          # a later get_data() fails cleanly instead of launching on a destroyed stream
        if own is not None:
            own.close()
            self._own_stream = None

    @property
    def _stream(self):
        s = self.__dict__.get('_stream_obj')
        if s is None:
            raise _lib.KwsError("AudioProcessor is closed: its generator stream and STFT plan are gone")
        return s

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    # -- index ---------------------------------------------------------------------------------------
    def maybe_download_and_extract_dataset(self, data_dir):
        if not os.path.exists(data_dir):
            print("Please download the dataset!")
            sys.exit(0)

    def prepare_data_index(self, silence_percentage, unknown_percentage, wanted_words, validation_percentage,
                           testing_percentage):
        """reference input_data.py:182-272; the host logic lives in sampler.DataIndex.from_dirs."""
        self._adopt_index(DataIndex.from_dirs(self.data_dirs, silence_percentage, unknown_percentage, wanted_words,
                                              validation_percentage, testing_percentage))

    def _adopt_index(self, idx):
        self._index = idx
        self.data_index = idx.data_index
        self.word_to_index = idx.word_to_index
        self.words_list = idx.words_list
        self._file_row = idx.file_row
        self._rows, self._labels, self._silence = idx.rows, idx.labels, idx.silence

    def prepare_background_data(self):
        """reference input_data.py:274-309"""
        self.background_data = []
        background_dir = os.path.join(self.data_dirs[0], BACKGROUND_NOISE_DIR_NAME)
        if not os.path.exists(background_dir):
            return self.background_data
        search_path = os.path.join(background_dir, '*.wav')
        paths = sorted(glob.glob(search_path))
        policy = getattr(self, 'wav_rate_policy', 'decode_wav')
        rate_out = self.model_settings['sample_rate'] if policy != 'decode_wav' else None
        if policy == 'error':
            check_wav_rates(paths, rate_out)
        for wav_path in paths:
            if policy == 'resample':
                a, rate = _read_wav_int16(wav_path)
                if rate != rate_out:
                    a = resample_recording(a, rate, rate_out, self.device)
                self.background_data.append(a.astype(np.float32) / np.float32(32768.0))
            else:
                self.background_data.append(load_wav_file(wav_path))
        if not self.background_data:
            raise Exception('No background wav files were found in ' + search_path)

    def _build_bank(self):
        """Decode every distinct file of the index once into the int16 HBM clip bank."""
        L = self.model_settings['desired_samples']
        if self.wav_rate_policy == 'decode_wav':
            clips = torch.from_numpy(bank_from_files(self._file_row, L)).to(self.device)
        else:
            files = sorted(self._file_row, key=self._file_row.get)          # row r = file r
            assert [self._file_row[fn] for fn in files] == list(range(len(files)))
            clips = decode_wav_files(files, L, self.model_settings['sample_rate'], self.device, self.wav_rate_policy)
            if not files:
                clips = torch.zeros((1, L), dtype=torch.int16, device=self.device)
        self.bank = ClipBank(clips, self.background_data, self.device)

    def _init_synthetic(self, spec, wanted_words):
        """Synthetic source (bench.py / tests): spec = {'bank': ClipBank, 'index': {set: [(row, word)]}}.
        No files are touched; everything downstream (sampler, kernels) is the production path."""
        self.bank = spec['bank']
        self.background_data = self.bank.noise_host
        self._adopt_index(DataIndex.from_entries(spec['index'], wanted_words))

    # -- processing "graph" ----------------------------------------------------------------------
    def prepare_processing_graph(self, model_settings):
        """Creates the feed keys / fetch handles of the reference graph (input_data.py:311-381) and
        the STFT plan (tables follow tf.contrib.signal)."""
        self.wav_filename_placeholder_ = _Placeholder('filename')
        self.foreground_volume_placeholder_ = _Placeholder('foreground_volme')
        self.time_shift_placeholder_ = _Placeholder('timeshift')
        self.background_data_placeholder_ = _Placeholder('background_data')
        self.background_volume_placeholder_ = _Placeholder('background_volume')
        self.background_clamp_ = _Fetch(self, 'raw')
        self.spectrogram_ = _Fetch(self, 'spec')
        self.mfcc_ = _Fetch(self, 'mfcc')
        from .features import path_b_plan
        self._n_mel = model_settings['dct_coefficient_count']
        self._n_out = model_settings['num_log_mel_features']
        plan = path_b_plan(model_settings)
        self._plan = plan
        self._n_frames = self.lib.kws_stft_num_frames(plan, model_settings['desired_samples'])

    def set_size(self, mode):
        """reference input_data.py:383-393"""
        return len(self.data_index[mode])

    # -- sampler (host, reference RNG order) -----------------------------------------------------------
    def _draw(self, mode, offset, sample_count, how_many, *aug):
        """Per-clip parameters in the reference's draw order (sampler.DataIndex.draw)."""
        return self._index.draw(mode, offset, sample_count, how_many, self.model_settings['desired_samples'],
                                [len(b) for b in self.background_data],
                                self.bank.noise_starts if self.background_data else [], *aug)

    # -- device side -----------------------------------------------------------------------------------
    def _augment(self, rows, shift, bg_off, bg_vol, fg_vol):
        """One kws_augment launch for the whole batch on the processor's own stream."""
        B = len(rows)
        L = self.model_settings['desired_samples']
        packed_i = np.concatenate([rows.astype(np.int32), shift.astype(np.int32)])
        packed_f = np.concatenate([fg_vol.astype(np.float32), bg_vol.astype(np.float32)])
        st = self._stream
        with torch.cuda.stream(st):
            di = torch.from_numpy(packed_i).pin_memory().to(self.device, non_blocking=True)
            df = torch.from_numpy(packed_f).pin_memory().to(self.device, non_blocking=True)
            do = torch.from_numpy(bg_off.astype(np.int64)).pin_memory().to(self.device, non_blocking=True)
            out = torch.empty((B, L), dtype=torch.float32, device=self.device)
            bank = self.bank
            fn = "kws_augment_i16" if bank.clips.dtype == torch.int16 else "kws_augment_f32"
            noise = bank.noise if bank.noise is not None else None
            _lib.call(fn, _lib.ptr(bank.clips), bank.n_clips, L, _lib.ptr(di[:B]), _lib.ptr(df[:B]),
                      _lib.ptr(di[B:]), _lib.ptr(noise), 0 if noise is None else noise.numel(),
                      _lib.ptr(do) if noise is not None else None, _lib.ptr(df[B:]), _lib.ptr(out), B,
                      _lib.stream_ptr(st))
            self._keep = (di, df, do)     # alive until the next call on this stream
        return out

    def _features(self, raw, out_kind):
        B, L = raw.shape
        width = {0: self._n_out, 1: 257, 2: self._n_mel}[out_kind]
        st = self._stream
        with torch.cuda.stream(st):
            out = torch.empty((B, self._n_frames * width), dtype=torch.float32, device=self.device)
            _lib.call("kws_stft_mel_f32", self._plan, _lib.ptr(raw), B, L, _lib.ptr(out), out_kind,
                      _lib.stream_ptr(st))
        return out

    def get_data(self, how_many, offset, background_frequency, background_volume_range, foreground_frequency,
                 foreground_volume_range, time_shift_frequency, time_shift_range, mode, sess,
                 pseudo_frequency=0.0, flip_frequency=0.0, silence_volume_range=0.0):
        """reference input_data.py:395-541.  Returns (data, labels): data is a DeviceArray
        [n, D] (or [mfcc, raw] for 'mfcc_and_raw'), labels a float64 one-hot matrix that also
        carries its device copy.  `sess` is accepted and ignored (there is no TF session)."""
        candidates = self.data_index[mode]
        prof = self.profiler
        if prof is not getattr(_TLS, 'prof', None):       # the generator runs on its own thread: attach THAT thread
            if prof is None:
                _lib.Profiler.detach()
            else:
                prof.attach()
            _TLS.prof = prof
        if how_many == -1:
            sample_count = len(candidates)
        else:
            sample_count = max(0, min(how_many, len(candidates) - offset))
        label_count = self.model_settings['label_count']
        if sample_count == 0:
            D = {'raw': self.model_settings['desired_samples'],
                 'spec': self._n_frames * 257}.get(self.output_representation, self._n_frames * self._n_out)
            return np.zeros((0, D)), np.zeros((0, label_count))
        rows, labels, shift, bg_off, bg_vol, fg_vol = self._draw(
            mode, offset, sample_count, how_many, background_frequency, background_volume_range,
            foreground_frequency, foreground_volume_range, time_shift_frequency, time_shift_range,
            pseudo_frequency, flip_frequency, silence_volume_range)
        raw = self._augment(rows, shift, bg_off, bg_vol, fg_vol)
        rep = self.output_representation
        if rep == 'raw':
            data = raw
        elif rep == 'spec':
            data = self._features(raw, 1)
        else:
            data = self._features(raw, 0)
        onehot = np.zeros((sample_count, label_count))
        onehot[np.arange(sample_count), labels] = 1
        with torch.cuda.stream(self._stream):
            dlab = torch.from_numpy(onehot.astype(np.float32)).pin_memory().to(self.device, non_blocking=True)
            ev = torch.cuda.Event()
            ev.record(self._stream)
        lab = Labels(onehot, dlab, ev)
        if rep != 'mfcc_and_raw':
            return DeviceArray(data, ev), lab
        return [DeviceArray(data, ev), DeviceArray(raw, ev)], lab

    def run_fetch(self, fetch, feed_dict):
        """Single-clip evaluation of one graph output, for reference-style `sess.run(ap.mfcc_, feed)`
        call sites (make_submission.py:86-115)."""
        L = self.model_settings['desired_samples']
        fn = feed_dict[self.wav_filename_placeholder_]
        if fn in self._file_row:
            row = self._file_row[fn]
            clip = self.bank.clips[row:row + 1]
        else:
            a, _ = _read_wav_int16(fn)
            buf = np.zeros((1, L), np.int16)
            buf[0, :min(len(a), L)] = a[:L]
            clip = torch.from_numpy(buf).to(self.device)
        bg = np.asarray(feed_dict.get(self.background_data_placeholder_, np.zeros(L)), dtype=np.float32).reshape(-1)
        st = self._stream
        with torch.cuda.stream(st):
            one_i = torch.tensor([0, int(feed_dict.get(self.time_shift_placeholder_, 0))], dtype=torch.int32,
                                 device=self.device)
            one_f = torch.tensor([float(feed_dict.get(self.foreground_volume_placeholder_, 1.0)),
                                  float(feed_dict.get(self.background_volume_placeholder_, 0.0))],
                                 dtype=torch.float32, device=self.device)
            noise = torch.from_numpy(bg).to(self.device)
            off = torch.zeros(1, dtype=torch.int64, device=self.device)
            out = torch.empty((1, L), dtype=torch.float32, device=self.device)
            name = "kws_augment_i16" if clip.dtype == torch.int16 else "kws_augment_f32"
            _lib.call(name, _lib.ptr(clip), 1, L, _lib.ptr(one_i[:1]), _lib.ptr(one_f[:1]), _lib.ptr(one_i[1:]),
                      _lib.ptr(noise), noise.numel(), _lib.ptr(off), _lib.ptr(one_f[1:]), _lib.ptr(out), 1,
                      _lib.stream_ptr(st))
        if fetch.kind == 'raw':
            res = out
        else:
            res = self._features(out, 1 if fetch.kind == 'spec' else 0)
            res = res.reshape(1, self._n_frames, -1)
        st.synchronize()
        return res.cpu().numpy()

    def get_unprocessed_data(self, how_many, model_settings, mode):
        """reference input_data.py:543-589 (no transformations; silence rows are zeroed)."""
        candidates = self.data_index[mode]
        sample_count = len(candidates) if how_many == -1 else how_many
        idx = np.arange(sample_count) if how_many == -1 else \
            np.array([np.random.randint(len(candidates)) for _ in range(sample_count)])
        rows = self._rows[mode][idx]
        fg = np.where(self._silence[mode][idx], 0.0, 1.0).astype(np.float32)
        z = np.zeros(sample_count)
        raw = self._augment(rows, z.astype(np.int32), z.astype(np.int64), z.astype(np.float32), fg)
        self._stream.synchronize()
        labels = [self.words_list[i] for i in self._labels[mode][idx]]
        return raw.cpu().numpy().astype(np.float64), labels

    def summary(self):
        """reference input_data.py:591-610"""
        set_counts = {}
        print("There are %d classes." % (len(self.word_to_index)))
        print("1%% <-> %d samples in 'training'" % int(self.set_size('training') / 100))
        for set_index in ['training', 'validation', 'testing', 'pseudo']:
            counts = {k: 0 for k in sorted(self.word_to_index.keys())}
            num_total = self.set_size(set_index)
            for data_point in self.data_index[set_index]:
                counts[data_point['label']] += (1.0 / num_total) * 100.0
            set_counts[set_index] = counts
        print("%-13s%-6s%-6s%-6s%-6s" % ('', 'Train', 'Val', 'Test', 'Pseudo'))
        for label_name in sorted(self.word_to_index.keys(), key=self.word_to_index.get):
            line = "%02d %-12s: " % (self.word_to_index[label_name], label_name)
            for set_index in ['training', 'validation', 'testing', 'pseudo']:
                line += "%.1f%% " % (set_counts[set_index][label_name])
            print(line)
