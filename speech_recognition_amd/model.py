"""Host-side mirror of the reference's model.py for the accelerated models: `speech_model`
dispatch (reference model.py:1729-1781), `prepare_model_settings` (model.py:1785-1829) and the two
symbols checkpoints name as custom objects (`relu6` model.py:30-31, `overlapping_time_slice_stack`
model.py:67-76).  The layer graphs themselves are native network programs in csrc/net*.hip (conv_1d_time_sliced:
csrc/net_time_sliced.hip, whose first convolution is csrc/frame_conv.hip and whose pooled head is csrc/gap.hip)."""
from . import _lib
from .keras_api import SGD, Adam, Model, RMSprop
from .net import DeviceNet

ACCELERATED = ('conv_1d_time_sliced_with_attention', 'conv_1d_log_mfcc', 'conv_1d_spectrogram', 'steffeNet', 'conv_1d_residual', 'conv_1d_mfcc_and_raw',
               'conv_1d_fast', 'conv_1d_spec', 'conv_1d_time_stacked', 'conv_1d_heavy', 'conv_1d_gru', 'conv_1d_multi_time_sliced', 'conv_1d_simple',
               'xception_with_attention', 'inception_d1', 'conv_2d_mobile', 'conv_2d_fast', 'conv_1d_time_sliced', 'conv_1d_learned_spec', 'conv_1d_top_down')
REFERENCE_MODEL_TYPES = (
    'simple', 'snn', 'conv_1d_time_stacked', 'conv_1d_multi_time_sliced', 'conv_1d_time_sliced',
    'conv_1d_time_sliced_group', 'conv_1d_heavy', 'conv_1d_simple', 'conv_1d_gru', 'conv_2d', 'conv_2d_fast',
    'conv_2d_mobile', 'inception', 'inception_d1', 'conv_1d_learned_spec', 'conv_1d_spec', 'conv_1d_fast',
    'conv_1d_top_down', 'conv_1d_residual', 'xception_with_attention', 'conv_1d_time_sliced_with_attention',
    'conv_1d_log_mfcc', 'conv_1d_spectrogram', 'conv_1d_mfcc_and_raw', 'steffeNet')


def relu6(x):
    """K.relu(x, max_value=6).  On the device ReLU6 is fused into the consumer of every BatchNorm
    (csrc/dwconv.hip, csrc/tail.hip); this callable exists for checkpoint custom_objects."""
    return x.clamp(0, 6) if hasattr(x, 'clamp') else min(max(x, 0), 6)


def overlapping_time_slice_stack(x, ksize, stride, padding='SAME'):
    """extract_image_patches framing.  On the device it is fused into the first convolution's
    gathered A-operand (kws_gemm_gather_f32); calling it on host data is not part of the hot path."""
    raise _lib.KwsError("overlapping_time_slice_stack is fused into kws_gemm_gather_f32 on the device")


def class_map_32_to_12(all_classes=None, wanted_classes=None):
    """int32 map [len(all_classes) + 2] -> slot of the 12-class head, as freeze_graph_32_classes.py:55-69 walks it:
    silence -> 0, the unknown-unknown class and every word outside `wanted_classes` -> 1 (their MAXIMUM becomes the
    unknown probability), wanted words -> 2.. in the order they appear in `all_classes`."""
    import numpy as np
    from .classes import get_classes
    all_classes = get_classes(wanted_only=False) if all_classes is None else list(all_classes)
    wanted_classes = get_classes(wanted_only=True) if wanted_classes is None else list(wanted_classes)
    mp = np.zeros(len(all_classes) + 2, np.int32)
    mp[1], slot = 1, 2
    for i, c in enumerate(all_classes):
        if c in wanted_classes:
            mp[i + 2] = slot
            slot += 1
        else:
            mp[i + 2] = 1
    return mp, slot


_HEAD_MAPS = {}


def head32to12(all_probs, all_classes=None, wanted_classes=None, out=None):
    """The 32 -> 12 class head of the reference's frozen graph (freeze_graph_32_classes.py:55-69, BASELINE config C3)
    on the device: `all_probs` [B, 32] softmax outputs of a 32-class model (CUDA tensor / DeviceArray / array) ->
    [B, 12] = softmax over (silence, max over the unknown words, the wanted words).  One `kws_head32to12` launch."""
    import torch
    from .device_array import as_device_f32
    dev = all_probs.device if isinstance(all_probs, torch.Tensor) and all_probs.is_cuda else \
        torch.device("cuda", torch.cuda.current_device())
    p = as_device_f32(all_probs, dev)
    key = (tuple(all_classes) if all_classes is not None else None,
           tuple(wanted_classes) if wanted_classes is not None else None, str(dev))
    if key not in _HEAD_MAPS:
        mp, n_out = class_map_32_to_12(all_classes, wanted_classes)
        _HEAD_MAPS[key] = (torch.from_numpy(mp).to(dev), n_out)
    dmap, n_out = _HEAD_MAPS[key]
    if p.dim() != 2 or p.shape[1] != dmap.numel():
        raise ValueError("head32to12: expected [B, %d] probabilities, got %s" % (dmap.numel(), tuple(p.shape)))
    B = p.shape[0]
    if out is None:
        out = torch.empty((B, n_out), dtype=torch.float32, device=dev)
    with torch.cuda.device(dev):
        _lib.call("kws_head32to12", _lib.ptr(p), p.shape[1], _lib.ptr(dmap), n_out, _lib.ptr(out), B, _lib.stream_ptr())
    return out


def conv_1d_time_sliced_with_attention_model(input_size=16000, num_classes=11, filter_mult=1):
    """reference model.py:775-838: 12-block depthwise/pointwise 1-D CNN on raw waveform, attention-pooled
    head, RMSprop(1e-3), label-smoothed CE (0.1), categorical accuracy."""
    net = DeviceNet(_lib.KWS_NET_TS_ATTENTION, num_classes, filter_mult=filter_mult, input_size=input_size)
    return Model(net, RMSprop(lr=1e-3), name='conv_1d_time_sliced_with_attention')


def conv_1d_time_sliced_model(input_size=16000, num_classes=11, filter_mult=1):
    """reference model.py:716-772: the model the attention net grew out of - the same time-slice front end at 32 * filter_mult
    filters (Conv1D(3, strides=2) over overlapping_time_slice_stack(x, 40, 20)), thirteen 3-tap depthwise / pointwise blocks
    (64 ... 512 * filter_mult) -> GlobalAveragePooling1D -> Dropout(.4) -> Dense(256 * filter_mult, no bias) + relu6 -> Dropout(.3)
    -> Dense (no bias, l2 1e-5); RMSprop(1e-3), categorical CE."""
    net = DeviceNet(_lib.KWS_NET_CONV_1D_TIME_SLICED, num_classes, filter_mult=filter_mult, input_size=input_size)
    return Model(net, RMSprop(lr=1e-3), name='conv_1d_time_sliced', loss='cce')


def conv_1d_log_mfcc_model(input_size=16000, num_classes=11, *args, **kwargs):
    """reference model.py:1400-1479: residual depthwise 1-D CNN on [spectrogram_length, num_log_mel_features]
    features, softmax-over-time attention, RMSprop(6e-4), categorical CE."""
    time_size = kwargs.get('spectrogram_length', 65)
    frequency_size = kwargs.get('num_log_mel_features', 40)
    net = DeviceNet(_lib.KWS_NET_LOG_MFCC, num_classes, input_size=input_size, spectrogram_length=time_size,
                    num_features=frequency_size)
    return Model(net, RMSprop(lr=6e-4), name='conv_1d_log_mfcc', loss='cce')


def conv_1d_spectrogram_model(input_size=16000, num_classes=11, *args, **kwargs):
    """reference model.py:1482-1561: the conv_1d_log_mfcc architecture on the generator's 'spec' output
    ([spectrogram_length, spectrogram_frequencies = 257] magnitudes), RMSprop(3e-4), categorical CE."""
    time_size = kwargs.get('spectrogram_length', 65)
    frequency_size = kwargs.get('spectrogram_frequencies', 257)
    net = DeviceNet(_lib.KWS_NET_LOG_MFCC, num_classes, input_size=input_size, spectrogram_length=time_size,
                    num_features=frequency_size)
    return Model(net, RMSprop(lr=3e-4), name='conv_1d_spectrogram', loss='cce')


def steffeNet(input_size=16000, num_classes=11, *args, **kwargs):
    """reference model.py:1663-1726: raw waveform -> Conv1D(256, 75, strides=50) -> context block -> 12 residual
    depthwise blocks (320 ... 1536 wide, the first depthwise of every other block strided) -> global max ++
    average pooling -> Dropout(.5) -> Dense, RMSprop(1e-3), label-smoothed CE (0.1)."""
    net = DeviceNet(_lib.KWS_NET_STEFFE, num_classes, input_size=input_size)
    return Model(net, RMSprop(lr=1e-3), name='steffeNet')


def conv_1d_residual_model(input_size=16000, num_classes=11, filter_mult=1):
    """reference model.py:841-908: raw waveform -> time-slice stack -> Conv1D(64, 3, strides=2) -> 13 residual blocks
    with 3-wide max-pool joins -> reduce block (1024) -> global average pooling -> Dropout(.5) -> Dense,
    RMSprop(1e-4), categorical CE."""
    net = DeviceNet(_lib.KWS_NET_RESIDUAL, num_classes, filter_mult=filter_mult, input_size=input_size)
    return Model(net, RMSprop(lr=1e-4), name='conv_1d_residual', loss='cce')


def conv_1d_mfcc_and_raw_model(input_size=16000, num_classes=11, *args, **kwargs):
    """reference model.py:1563-1660: the two-input model fed by the generator's 'mfcc_and_raw' output - log-mel
    features -> Conv1D(64, 3) and raw frames (480 / 160, VALID) -> Conv1D(96, 3), concatenated, 10 residual blocks
    with 3-wide max-pool joins, global average pooling, Dropout(.3), Dense; RMSprop(5e-4), categorical CE.
    `input_size` is the feature input's size (as the reference passes it); batches are `[mfcc, raw]`."""
    time_size = kwargs.get('spectrogram_length', 65)
    frequency_size = kwargs.get('num_log_mel_features', 40)
    raw_size = kwargs.get('desired_samples', 16000)
    if kwargs.get('window_size_samples', 480) != 480 or kwargs.get('window_stride_samples', 160) != 160:
        raise NotImplementedError("conv_1d_mfcc_and_raw: only the 30 ms / 10 ms framing (480 / 160 samples) is built")
    net = DeviceNet(_lib.KWS_NET_MFCC_AND_RAW, num_classes, input_size=time_size * frequency_size + raw_size,
                    spectrogram_length=time_size, num_features=frequency_size)
    return Model(net, RMSprop(lr=5e-4), name='conv_1d_mfcc_and_raw', loss='cce')


def conv_1d_fast_model(input_size=16000, num_classes=11, *args, **kwargs):
    """reference model.py:642-713: raw waveform -> Conv1D(252, 479, strides=160, l2 1e-4; no BN, no activation) -> two
    grouped reduce blocks (300 filters, k 15, 6 groups over 252 channels; 360, k 7, 5 groups over 300), each group its
    own Conv1D + BatchNormalization + relu6 -> Flatten -> Dropout(.3) -> Dense; RMSprop(3e-3), categorical CE.  The
    reference names the Keras model 'conv_1d_learned_spec'."""
    net = DeviceNet(_lib.KWS_NET_CONV_1D_FAST, num_classes, input_size=input_size)
    return Model(net, RMSprop(lr=3e-3), name='conv_1d_learned_spec', loss='cce')


def conv_1d_learned_spec_model(input_size=16000, num_classes=11, *args, **kwargs):
    """reference model.py:1159-1246: raw waveform -> a learned filterbank of six Conv1D(40, k, strides=160, SAME, no bias, l2 1e-4)
    layers, k = 479, 383, 319, 255, 191, 161, concatenated to [ceil(input_size / 160), 240] (no BN, no activation; one
    kws_fbank_conv_* launch, csrc/fbank_conv.hip) -> four grouped reduce (k 3, stride 2, 3 groups) / context (k 3, 2 groups) pairs
    of 300 ... 480 filters, each group its own Conv1D + BatchNormalization + relu6 - the first context block slices 360 channels
    of 300, so its groups read 180 and 120 - -> Flatten -> Dropout(.3) -> Dense; RMSprop(2e-3), categorical CE.  input_size: any
    even size of at least 14402 samples (91 rows)."""
    net = DeviceNet(_lib.KWS_NET_CONV_1D_LEARNED_SPEC, num_classes, input_size=input_size)
    return Model(net, RMSprop(lr=2e-3), name='conv_1d_learned_spec', loss='cce')


def conv_1d_top_down_model(input_size=16000, num_classes=11, *args, **kwargs):
    """reference model.py:1326-1397: raw waveform -> Conv1D(480, 479, strides=160, with bias; no BN, no activation) -> four grouped
    reduce (stride 2, 3 groups over slices of 480, 300 of 420, 360 and 300 channels) / context (2 groups, EACH reading all channels:
    the reference hands them x, not the slice) pairs of 420, 360, 300, 240 filters, k 3 VALID, every group its own DepthwiseConv2D
    -> Conv1D(F / g, 1) -> BatchNormalization -> relu6 with l2 1e-5 (the depthwise halves of a block one kws_gdwconv_* launch,
    csrc/gdwconv.hip) -> Flatten -> Dropout(.05) -> Dense; RMSprop(3e-3), categorical CE.  input_size: any even size of at least
    14879 samples (91 rows), so 14880 is the first."""
    net = DeviceNet(_lib.KWS_NET_CONV_1D_TOP_DOWN, num_classes, input_size=input_size)
    return Model(net, RMSprop(lr=3e-3), name='conv_1d_top_down', loss='cce')


def conv_1d_spec_model(input_size=16000, num_classes=11, *args, **kwargs):
    """reference model.py:1249-1323: the generator's 'spec' output as [98, 257] (the reference fixes Input(shape=[98 * 257])
    and ignores input_size) -> four grouped reduce (k 3, stride 2, 4 groups) / context (k 3, 3 groups) pairs of 300 ... 480
    filters -> Flatten -> Dropout(.3) -> Dense; RMSprop(2e-3), categorical CE."""
    net = DeviceNet(_lib.KWS_NET_CONV_1D_SPEC, num_classes, input_size=98 * 257)
    return Model(net, RMSprop(lr=2e-3), name='conv_1d_spec', loss='cce')


def _raw_16000(model_type, input_size):
    if int(input_size) != 16000:
        raise ValueError("%s: input_size %s - the reference reshapes exactly 16000 samples" % (model_type, input_size))


def conv_1d_time_stacked_model(input_size=16000, num_classes=11, *args, **kwargs):
    """reference model.py:257-309: raw waveform as [800, 20] -> Conv1D(32, 1) -> six pairs of Conv1D(F, 3, VALID, l2 1e-5) +
    BatchNormalization + relu6, the first of a pair followed by MaxPool1D(3, strides=2, 'valid') (F = 48 ... 256) -> Dropout(.3)
    -> Conv1D(num_classes, 5, softmax); Adam(3e-4), categorical CE."""
    _raw_16000('conv_1d_time_stacked', input_size)
    net = DeviceNet(_lib.KWS_NET_CONV_1D_TIME_STACKED, num_classes, input_size=16000)
    return Model(net, Adam(lr=3e-4), name='conv_1d_time_stacked', loss='cce')


def conv_1d_heavy_model(input_size=16000, num_classes=11, *args, **kwargs):
    """reference model.py:409-467: raw waveform as [1600, 10], the conv_1d_time_stacked ladder with a seventh pair (320) ->
    Dropout(.3) -> Conv1D(128, 5) + BatchNormalization + relu6 -> Dropout(.1) -> Conv1D(num_classes, 1, softmax, no bias);
    Adam(3e-4), categorical CE.  The reference names this Keras model 'conv_1d_time_stacked' as well."""
    _raw_16000('conv_1d_heavy', input_size)
    net = DeviceNet(_lib.KWS_NET_CONV_1D_HEAVY, num_classes, input_size=16000)
    return Model(net, Adam(lr=3e-4), name='conv_1d_time_stacked', loss='cce')


def conv_1d_gru_model(input_size=16000, num_classes=11, *args, **kwargs):
    """reference model.py:470-512: raw waveform as [16000, 1] -> six depthwise blocks (DepthwiseConv2D((1, k), strides=s) ->
    Conv1D(F, 1) -> BatchNormalization -> relu6, l2 1e-5): k 63 / 31 / 15 / 7 / 5 SAME at strides 16 / 4 / 4 / 4 / 2, then k 8
    VALID; F = 128 ... 512 -> Flatten -> Dropout(.3) -> Dense(256) + relu6 -> Dropout(.3) -> Dense; RMSprop(1e-3), categorical
    CE.  No recurrent layer, despite the name; the reference names the Keras model 'conv_1d_bigru'."""
    _raw_16000('conv_1d_gru', input_size)
    net = DeviceNet(_lib.KWS_NET_CONV_1D_GRU, num_classes, input_size=16000)
    return Model(net, RMSprop(lr=1e-3), name='conv_1d_bigru', loss='cce')


def conv_1d_multi_time_sliced_model(input_size=16000, num_classes=11, *args, **kwargs):
    """reference model.py:1080-1156: raw waveform viewed as [4000, 4], [3200, 5] and [640, 25], each view a ladder of depthwise
    blocks (DepthwiseConv2D((1, k), VALID) -> Conv1D(F, 1) -> BatchNormalization -> relu6, l2 1e-5), a reduce block followed by
    MaxPool1D(3, strides=2, 'same'); five one-step branch ends of 64 channels concatenated -> Dropout(.1) -> a one-tap block (128)
    -> Dropout(.1) -> Conv1D(num_classes, 1, softmax); RMSprop(3e-3), categorical CE."""
    _raw_16000('conv_1d_multi_time_sliced', input_size)
    net = DeviceNet(_lib.KWS_NET_CONV_1D_MULTI_TIME_SLICED, num_classes, input_size=16000)
    return Model(net, RMSprop(lr=3e-3), name='conv_1d_multi_time_sliced', loss='cce')


def conv_1d_simple_model(input_size=16000, num_classes=11, *args, **kwargs):
    """reference model.py:116-156: raw waveform as [16000, 1] -> fourteen VALID depthwise blocks (k 31 at stride 16, then k 3 at
    strides 1, 2, 1, ...; F = 32, 32, 64, 64 ... 224, 224; l2 1e-5) ending at [10, 224] -> Bidirectional(GRU(128, dropout=.2,
    recurrent_dropout=.2)) -> Dense; Adam() at the Keras defaults (lr 1e-3), categorical CE.  The reference names the Keras model
    'conv_1d_time_stacked'."""
    _raw_16000('conv_1d_simple', input_size)
    net = DeviceNet(_lib.KWS_NET_CONV_1D_SIMPLE, num_classes, input_size=16000)
    return Model(net, Adam(lr=1e-3), name='conv_1d_time_stacked', loss='cce')


def inception_d1_model(input_size=16000, num_classes=11, *args, **kwargs):
    """reference model.py:312-406 (conv_inception_d1_model): raw waveform as [800, 20] -> Conv1D(32, 1) -> three stride-1
    reduce (MaxPool1D(3, 2) behind) / context pairs (64, 128, 256; k 3 VALID) -> eight inception blocks (1x1 | 1x1 -> k3 dil 2 |
    1x1 -> k3 -> k3 | AveragePooling1D(3, 1, 'same') -> 1x1, concatenated to 256 channels) with a reduce block (496 channels,
    half the steps) behind every second one -> [6, 496] -> Dropout(.2) -> Conv1D(num_classes, 6, softmax); every convolution
    BatchNormalization + relu6, l2 1e-5; Adam(1e-3), categorical CE."""
    _raw_16000('inception_d1', input_size)
    net = DeviceNet(_lib.KWS_NET_INCEPTION_D1, num_classes, input_size=16000)
    return Model(net, Adam(lr=1e-3), name='inception_d1', loss='cce')


def _mfcc_3920(model_type, input_size):
    if int(input_size) != 3920:
        raise ValueError("%s: input_size %s - the reference reshapes exactly 98 x 40 mfcc features (3920)" % (model_type, input_size))


def conv_2d_mobile_model(input_size=3920, num_classes=11, *args, **kwargs):
    """reference model.py:547-594: the generator's 'mfcc' output as an image [98, 40, 1] -> Preprocess -> eight Conv2D(F, 3 x 3,
    SAME, bias) + BatchNormalization + relu6 (F = 32, 32, 64, 64, 128, 128, 256, 256; the odd-numbered ones at stride 2), Dropout(.05)
    behind every pair -> GlobalAveragePooling2D -> Dropout(.1) -> Dense; SGD(1e-3, momentum .95), categorical CE."""
    _mfcc_3920('conv_2d_mobile', input_size)
    net = DeviceNet(_lib.KWS_NET_CONV_2D_MOBILE, num_classes, input_size=3920)
    return Model(net, SGD(lr=1e-3, momentum=0.95), name='conv_2d_mobile', loss='cce')


def conv_2d_fast_model(input_size=3920, num_classes=11, *args, **kwargs):
    """reference model.py:597-639: the 'mfcc' image [98, 40, 1] -> Preprocess -> four Conv2D(SAME, bias, dilation) +
    BatchNormalization + relu + MaxPool2D() (16 x (11, 5) and 32 x (5, 3) at dilation (2, 1), 64 and 128 x (3, 3)) ->
    GlobalAveragePooling2D -> Dense; SGD(1e-3, momentum .9), categorical CE."""
    _mfcc_3920('conv_2d_fast', input_size)
    net = DeviceNet(_lib.KWS_NET_CONV_2D_FAST, num_classes, input_size=3920)
    return Model(net, SGD(lr=1e-3, momentum=0.9), name='conv_2d_fast', loss='cce')


def xception_with_attention_model(input_size=16000, num_classes=11, filter_mult=1):
    """reference model.py:911-983: raw waveform -> time-slice stack -> Conv1D(64, 3, strides=2) -> eleven residual blocks with 3-wide
    max-pool joins (128, 256, 8 x 256, 384) ending at [50, 384] -> attention gate (a 5-tap depthwise block of one filter, softmax over
    time, multiplied onto the sequence) -> Bidirectional(GRU(192, dropout=.2, recurrent_dropout=.2, l2 1e-5 on the kernels)) -> Dense;
    RMSprop(5e-4), categorical CE."""
    net = DeviceNet(_lib.KWS_NET_XCEPTION_ATTENTION, num_classes, filter_mult=filter_mult, input_size=input_size)
    return Model(net, RMSprop(lr=5e-4), name='xception_with_attention', loss='cce')


def speech_model(model_type, input_size, num_classes=11, *args, **kwargs):
    if model_type == 'conv_1d_time_sliced_with_attention':
        return conv_1d_time_sliced_with_attention_model(input_size, num_classes)
    if model_type == 'conv_1d_time_sliced':
        return conv_1d_time_sliced_model(input_size, num_classes)
    if model_type == 'conv_1d_log_mfcc':
        return conv_1d_log_mfcc_model(input_size, num_classes, *args, **kwargs)
    if model_type == 'conv_1d_spectrogram':
        return conv_1d_spectrogram_model(input_size, num_classes, *args, **kwargs)
    if model_type == 'steffeNet':
        return steffeNet(input_size, num_classes, *args, **kwargs)
    if model_type == 'conv_1d_residual':
        return conv_1d_residual_model(input_size, num_classes)
    if model_type == 'conv_1d_mfcc_and_raw':
        return conv_1d_mfcc_and_raw_model(input_size, num_classes, *args, **kwargs)
    if model_type == 'conv_1d_fast':
        return conv_1d_fast_model(input_size, num_classes)
    if model_type == 'conv_1d_spec':
        return conv_1d_spec_model(input_size, num_classes)
    if model_type == 'conv_1d_learned_spec':
        return conv_1d_learned_spec_model(input_size, num_classes)
    if model_type == 'conv_1d_top_down':
        return conv_1d_top_down_model(input_size, num_classes)
    if model_type == 'conv_1d_time_stacked':
        return conv_1d_time_stacked_model(input_size, num_classes)
    if model_type == 'conv_1d_heavy':
        return conv_1d_heavy_model(input_size, num_classes)
    if model_type == 'conv_1d_gru':
        return conv_1d_gru_model(input_size, num_classes)
    if model_type == 'conv_1d_multi_time_sliced':
        return conv_1d_multi_time_sliced_model(input_size, num_classes)
    if model_type == 'conv_1d_simple':
        return conv_1d_simple_model(input_size, num_classes)
    if model_type == 'xception_with_attention':
        return xception_with_attention_model(input_size, num_classes)
    if model_type == 'inception_d1':
        return inception_d1_model(input_size, num_classes)
    if model_type == 'conv_2d_mobile':
        return conv_2d_mobile_model(input_size, num_classes)
    if model_type == 'conv_2d_fast':
        return conv_2d_fast_model(input_size, num_classes)
    if model_type in REFERENCE_MODEL_TYPES:
        raise NotImplementedError(
            "model '%s' has no native network program yet (built natively: %s)"
            % (model_type, ', '.join(ACCELERATED)))
    raise ValueError("Invalid model: %s" % model_type)


def prepare_model_settings(label_count, sample_rate, clip_duration_ms, window_size_ms, window_stride_ms,
                           dct_coefficient_count, num_log_mel_features, output_representation='raw'):
    """Settings arithmetic of reference model.py:1785-1829 (truncating int() conversions included)."""
    desired_samples = int(sample_rate * clip_duration_ms / 1000)
    window_size_samples = int(sample_rate * window_size_ms / 1000)
    window_stride_samples = int(sample_rate * window_stride_ms / 1000)
    length_minus_window = desired_samples - window_size_samples
    spectrogram_frequencies = 257
    spectrogram_length = 0 if length_minus_window < 0 else 1 + int(length_minus_window / window_stride_samples)
    fingerprint_size = {
        'mfcc': num_log_mel_features * spectrogram_length,
        'raw': desired_samples,
        'spec': spectrogram_frequencies * spectrogram_length,
        'mfcc_and_raw': num_log_mel_features * spectrogram_length,
    }[output_representation]
    return {
        'desired_samples': desired_samples,
        'window_size_samples': window_size_samples,
        'window_stride_samples': window_stride_samples,
        'spectrogram_length': spectrogram_length,
        'spectrogram_frequencies': spectrogram_frequencies,
        'dct_coefficient_count': dct_coefficient_count,
        'fingerprint_size': fingerprint_size,
        'label_count': label_count,
        'sample_rate': sample_rate,
        'num_log_mel_features': num_log_mel_features,
    }
