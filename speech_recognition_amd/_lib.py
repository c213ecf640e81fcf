"""ctypes binding of libkws_hip.so (the C ABI declared in include/kws_hip.h).

The product path has NO CPU fallback: if the shared library is missing or a call fails, a
KwsError is raised.  PyTorch-ROCm is used only to own device memory and streams; every
pointer handed to the library is a tensor's ``data_ptr()``.
"""
import ctypes
import os

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.environ.get("KWS_LIB_PATH") or os.path.join(_HERE, "libkws_hip.so")  # override: kernel A/B experiments

ABI_VERSION = 5    # include/kws_hip.h: KWS_ABI_VERSION

KWS_NET_TS_ATTENTION = 1
KWS_NET_LOG_MFCC = 2
KWS_NET_STEFFE = 3
KWS_NET_RESIDUAL = 4
KWS_NET_MFCC_AND_RAW = 5
KWS_NET_CONV_1D_FAST = 6
KWS_NET_CONV_1D_SPEC = 7
KWS_NET_CONV_1D_TIME_STACKED = 8
KWS_NET_CONV_1D_HEAVY = 9
KWS_NET_CONV_1D_GRU = 10
KWS_NET_CONV_1D_MULTI_TIME_SLICED = 11
KWS_NET_CONV_1D_SIMPLE = 12
KWS_NET_XCEPTION_ATTENTION = 13
KWS_NET_INCEPTION_D1 = 14
KWS_NET_CONV_2D_MOBILE = 15
KWS_NET_CONV_2D_FAST = 16
KWS_NET_CONV_1D_TIME_SLICED = 17
KWS_NET_CONV_1D_LEARNED_SPEC = 18
KWS_NET_CONV_1D_TOP_DOWN = 19


class KwsError(RuntimeError):
    pass


class GatherDesc(ctypes.Structure):
    _fields_ = [("L_out", ctypes.c_int), ("cin", ctypes.c_int), ("taps", ctypes.c_int),
                ("stride_t", ctypes.c_int), ("stride_j", ctypes.c_int), ("base_off", ctypes.c_int),
                ("x_len", ctypes.c_int), ("x_batch_stride", ctypes.c_int64)]


class GconvDesc(ctypes.Structure):
    """kws_gconv_t: grouped Conv1D over [B, L, C] -> [B, Lout, g * Ng]."""
    _fields_ = [("B", ctypes.c_int), ("L", ctypes.c_int), ("C", ctypes.c_int), ("Lout", ctypes.c_int),
                ("k", ctypes.c_int), ("stride", ctypes.c_int), ("g", ctypes.c_int), ("gs", ctypes.c_int),
                ("Ng", ctypes.c_int), ("w_group_stride", ctypes.c_int64)]


class GdwconvDesc(ctypes.Structure):
    """kws_gdwconv_t: grouped depthwise Conv1D from the channel windows [x0 + q * x_step, + gs) of [B, L, C] to [B, Lout, g * gs];
    act (GDW_ACT_*) is what a value goes through on load."""
    _fields_ = [(n, ctypes.c_int) for n in ("B", "L", "C", "Lout", "k", "stride", "g", "gs", "x0", "x_step", "act", "bn_group")] + \
               [("w_group_stride", ctypes.c_int64)]


GDW_ACT_NONE = 0       # include/kws_hip.h: KWS_GDW_ACT_*
GDW_ACT_BN_RELU6 = 1
GDW_ACT_BIAS = 2


class Conv1dDesc(ctypes.Structure):
    """kws_conv1d_t: dense Conv1D (stride 1) from the columns [x0, x0 + Cin) of [B, L, Cx] to the columns [y0, y0 + F) of
    [B, Lout, Cy]."""
    _fields_ = [("B", ctypes.c_int), ("L", ctypes.c_int), ("Lout", ctypes.c_int), ("k", ctypes.c_int),
                ("dil", ctypes.c_int), ("pad_l", ctypes.c_int), ("Cx", ctypes.c_int), ("x0", ctypes.c_int),
                ("Cin", ctypes.c_int), ("Cy", ctypes.c_int), ("y0", ctypes.c_int), ("F", ctypes.c_int)]


class Conv2dDesc(ctypes.Structure):
    """kws_conv2d_t: dense NHWC Conv2D from [B, H, W, Cin] to [B, Hout, Wout, F]; act (ACT_RELU6 / ACT_RELU) is the activation
    applied on load when a table is given."""
    _fields_ = [(n, ctypes.c_int) for n in ("B", "H", "W", "Hout", "Wout", "kh", "kw", "sh", "sw", "dh", "dw", "pad_t",
                                            "pad_l", "Cin", "F", "act")]


class FrameConvDesc(ctypes.Structure):
    """kws_frame_conv_t: overlapping_time_slice_stack(ksize, hop, SAME) + Conv1D(N, taps, strides=stride) over B clips of L
    samples -> [B, Lout, N]."""
    _fields_ = [(n, ctypes.c_int) for n in ("B", "L", "Lout", "ksize", "hop", "pad_l", "taps", "stride", "N")] + \
               [("x_batch_stride", ctypes.c_int64)]


class FbankConvDesc(ctypes.Structure):
    """kws_fbank_conv_t: nbanks Conv1D(N, ksize[q], strides=stride) layers over B clips of L samples, concatenated ->
    [B, Lout, nbanks * N]; bank q's kernel [ksize[q], 1, N] lies w_off[q] floats behind the weight pointer."""
    _fields_ = [(n, ctypes.c_int) for n in ("B", "L", "Lout", "stride", "nbanks", "N")] + \
               [("ksize", ctypes.c_int * 8), ("pad_l", ctypes.c_int * 8), ("w_off", ctypes.c_int64 * 8),
                ("x_batch_stride", ctypes.c_int64)]


ACT_RELU6 = 0   # include/kws_hip.h: KWS_ACT_*
ACT_RELU = 1


class SamplerSet(ctypes.Structure):
    _fields_ = [("rows", ctypes.c_void_p), ("labels", ctypes.c_void_p), ("silence", ctypes.c_void_p),
                ("n", ctypes.c_int32)]


class SamplerArgs(ctypes.Structure):
    _fields_ = [("deterministic", ctypes.c_int32), ("offset", ctypes.c_int32), ("count", ctypes.c_int32),
                ("use_background", ctypes.c_int32), ("n_bg", ctypes.c_int32), ("bg_len", ctypes.c_void_p),
                ("bg_start", ctypes.c_void_p), ("desired_samples", ctypes.c_int32), ("shift_lo", ctypes.c_int32),
                ("shift_hi", ctypes.c_int32), ("background_frequency", ctypes.c_double),
                ("background_volume_range", ctypes.c_double), ("foreground_frequency", ctypes.c_double),
                ("foreground_volume_range", ctypes.c_double), ("time_shift_frequency", ctypes.c_double),
                ("pseudo_frequency", ctypes.c_double), ("flip_frequency", ctypes.c_double),
                ("silence_volume_range", ctypes.c_double)]


class NetConfig(ctypes.Structure):
    _fields_ = [("kind", ctypes.c_int), ("num_classes", ctypes.c_int), ("filter_mult", ctypes.c_int),
                ("input_size", ctypes.c_int), ("spectrogram_length", ctypes.c_int),
                ("num_features", ctypes.c_int)]


class TensorInfo(ctypes.Structure):
    _fields_ = [("name", ctypes.c_char * 64), ("offset", ctypes.c_int64), ("size", ctypes.c_int64),
                ("ndim", ctypes.c_int), ("shape", ctypes.c_int64 * 4), ("is_state", ctypes.c_int),
                ("l2", ctypes.c_float), ("fan_in", ctypes.c_int), ("fan_out", ctypes.c_int),
                ("init", ctypes.c_float)]


_P = ctypes.c_void_p
_I = ctypes.c_int
_I64 = ctypes.c_int64
_F = ctypes.c_float

# name -> (restype, argtypes); every symbol include/kws_hip.h declares
SIGNATURES = {
    "kws_abi_version": (_I, []),
    "kws_last_error": (ctypes.c_char_p, []),
    "kws_device_name": (_I, [ctypes.c_char_p, _I]),
    "kws_stream_create": (_I, [_I, ctypes.POINTER(_P)]),
    "kws_stream_destroy": (_I, [_P]),
    "kws_profiler_create": (_I, [ctypes.POINTER(_P)]),
    "kws_profiler_destroy": (_I, [_P]),
    "kws_profiler_attach": (_I, [_P]),
    "kws_profiler_collect": (_I, [_P]),
    "kws_profiler_get": (_I, [_P, _I, ctypes.c_char_p, _I, ctypes.POINTER(ctypes.c_double), ctypes.POINTER(_I64),
                              ctypes.POINTER(ctypes.c_double), ctypes.POINTER(ctypes.c_double)]),
    "kws_sampler_draw": (_I, [_P, ctypes.POINTER(_I), ctypes.POINTER(SamplerSet), ctypes.POINTER(SamplerSet),
                              ctypes.POINTER(SamplerArgs), _P, _P, _P, _P, _P, _P]),
    "kws_augment_f32": (_I, [_P, _I64, _I, _P, _P, _P, _P, _I64, _P, _P, _P, _I, _P]),
    "kws_augment_i16": (_I, [_P, _I64, _I, _P, _P, _P, _P, _I64, _P, _P, _P, _I, _P]),
    "kws_tta_transform": (_I, [_P, _P, _I, _I, _I, _P]),
    "kws_tta_combine": (_I, [ctypes.POINTER(_P), _I, _F, _P, _P, _I, _I, _P]),
    "kws_head32to12": (_I, [_P, _I, _P, _I, _P, _I, _P]),
    "kws_dropout_fwd": (_I, [_P, _P, _I, _I, _F, ctypes.c_uint64, ctypes.c_uint32, ctypes.c_uint32, _I64, _P]),
    "kws_dropout_bwd": (_I, [_P, _P, _I, _I, _F, ctypes.c_uint64, ctypes.c_uint32, ctypes.c_uint32, _I64, _P]),
    "kws_attn_pool_fwd": (_I, [_P, _P, _P, _I, _I, _I, _P]),
    "kws_attn_pool_bwd_workspace_floats": (_I64, [_I, _I, _I]),
    "kws_attn_pool_bwd": (_I, [_P, _P, _P, _P, _P, _P, _I, _I, _I, _P]),
    "kws_softmax_xent_smooth_fwd": (_I, [_P, _P, _P, _P, _I, _I, _F, _P]),
    "kws_softmax_xent_smooth_bwd": (_I, [_P, _P, _P, _P, _I, _I, _F, _F, _P]),
    "kws_comm_unique_id": (_I, [_P]),
    "kws_comm_create": (_I, [_I, _I, _P, ctypes.POINTER(_P)]),
    "kws_comm_destroy": (_I, [_P]),
    "kws_allreduce_grads": (_I, [_P, _P, _I64, _P]),
    "kws_stretch_plan_create": (_I, [_I, ctypes.c_double, ctypes.POINTER(_P)]),
    "kws_stretch_plan_destroy": (_I, [_P]),
    "kws_stretch_out_samples": (_I, [_P]),
    "kws_time_stretch_f32": (_I, [_P, _P, _F, _P, _I, _I, _I, _P]),
    "kws_time_stretch_i16": (_I, [_P, _P, _P, _I, _I, _I, _P]),
    "kws_resample_design": (_I, [_I, _I, ctypes.POINTER(_I), ctypes.POINTER(_I), ctypes.POINTER(_I), ctypes.POINTER(_I)]),
    "kws_resample_taps": (_I, [_I, _I, _P, _I64]),
    "kws_resample_out_samples": (_I64, [_I, _I, _I64]),
    "kws_resample_plan_create": (_I, [_I, _I, ctypes.POINTER(_P)]),
    "kws_resample_plan_destroy": (_I, [_P]),
    "kws_resample_i16": (_I, [_P, _P, _I64, _P, _I, _P, _P, _I, _I, _P]),
    "kws_resample_f32": (_I, [_P, _P, _I64, _P, _I, _P, _I, _I, _P]),
    "kws_stream_frames_i16": (_I, [_P, _I64, _I64, _I, _I, _F, _P, _I, _P]),
    "kws_stream_frames_f32": (_I, [_P, _I64, _I64, _I, _I, _F, _P, _I, _P]),
    "kws_stream_gather_f32": (_I, [_P, _I64, _I64, _I64, _I, _P, _I64, _I, _P]),
    "kws_stream_smooth_f32": (_I, [_P, _I, _I, _I, _P, _P, _P, _P]),
    "kws_stft_plan_create": (_I, [_I, _I, _I, _I, _I, _P, _P, _P, _F, _F, ctypes.POINTER(_P)]),
    "kws_stft_plan_destroy": (_I, [_P]),
    "kws_stft_num_frames": (_I, [_P, _I]),
    "kws_stft_mel_f32": (_I, [_P, _P, _I, _I, _P, _I, _P]),
    "kws_stft_mel_kernel": (_I, [_P, _P, _I, _I]),
    "kws_gemm_num_row_tiles": (_I, [_I64]),
    "kws_gemm_nn_stats_rows": (_I, [_I64, _I, _I]),
    "kws_gemm_gather_stats_rows": (_I, [_I64]),
    "kws_gemm_nn_f32": (_I, [_P, _P, _P, _I64, _I, _I, _P, _P]),
    "kws_net_get_gemm_mode": (_I, [_P]),
    "kws_net_set_gemm_mode": (_I, [_P, _I]),
    "kws_gemm_nn_f16x2_supported": (_I, [_I64, _I, _I]),
    "kws_gemm_tn_f16x2_supported": (_I, [_I64, _I, _I]),
    "kws_gemm_nn_f16x2_stats_rows": (_I, [_I64]),
    "kws_absmax_batch_f32": (_I, [_P, _P, _P, _I, _P]),
    "kws_dwconv_fwd_amax_f32": (_I, [_P, _P, _P, _P, _I, _I, _I, _I, _I, _I, _P, _P]),
    "kws_dwconv_bwd_bn_amax_f32": (_I, [_P, _P, _P, _P, _P, _P, _P, _I, _I, _I, _I, _I, _I, _I, _P, _P]),
    "kws_bn_bwd_apply_amax": (_I, [_P, _P, _P, _P, _P, _I64, _I, _P, _P]),
    "kws_f16x2_split_batch": (_I, [_P, _P, _P, _P, _P, _P, _I, _P]),
    "kws_gemm_nn_f16x2_f32": (_I, [_P, _P, _P, _I64, _I, _I, _P, _P, _P, _P]),
    "kws_gemm_tn_f16x2_workspace_floats": (_I64, [_I64, _I, _I]),
    "kws_gemm_tn_f16x2_f32": (_I, [_P, _P, _P, _I64, _I, _I, _P, _P, _P, _P]),
    "kws_gemm_gather_f32": (_I, [_P, ctypes.POINTER(GatherDesc), _P, _P, _I, _I, _P, _P]),
    "kws_gemm_tn_workspace_floats": (_I64, [_I64, _I, _I]),
    "kws_gemm_tn_f32": (_I, [_P, _P, _P, _I64, _I, _I, _P, _P]),
    "kws_gemm_tn_gather_f32": (_I, [_P, ctypes.POINTER(GatherDesc), _P, _P, _I, _I, _P, _P]),
    "kws_gconv_stats_rows": (_I, [ctypes.POINTER(GconvDesc)]),
    "kws_gconv_fwd_f32": (_I, [_P, _P, _I, _P, _P, _P, ctypes.POINTER(GconvDesc), _P]),
    "kws_gconv_dgrad_f32": (_I, [_P, _P, _P, ctypes.POINTER(GconvDesc), _P]),
    "kws_gconv_wgrad_workspace_floats": (_I64, [ctypes.POINTER(GconvDesc)]),
    "kws_gconv_wgrad_f32": (_I, [_P, _P, _I, _P, _P, _P, ctypes.POINTER(GconvDesc), _P]),
    "kws_gdwconv_fwd_f32": (_I, [_P, _P, _P, _P, ctypes.POINTER(GdwconvDesc), _P]),
    "kws_gdwconv_bwd_part_rows": (_I, [ctypes.POINTER(GdwconvDesc)]),
    "kws_gdwconv_bwd_workspace_floats": (_I64, [ctypes.POINTER(GdwconvDesc)]),
    "kws_gdwconv_bwd_f32": (_I, [_P, _P, _P, _P, _P, _P, _P, _P, ctypes.POINTER(GdwconvDesc), _P]),
    "kws_pool3s2_out_len": (_I, [_I]),
    "kws_pool3s2_fwd_f32": (_I, [_P, _P, _P, _I, _I, _I, _P]),
    "kws_pool3s2_bwd_part_rows": (_I, [_I, _I, _I]),
    "kws_pool3s2_bwd_part_floats": (_I64, [_I, _I, _I]),
    "kws_pool3s2_bwd_f32": (_I, [_P, _P, _P, _P, _P, _I, _I, _I, _P]),
    "kws_pool3s2_same_out_len": (_I, [_I]),
    "kws_pool3s2_same_fwd_f32": (_I, [_P, _P, _P, _I, _I, _I, _P]),
    "kws_pool3s2_same_bwd_part_rows": (_I, [_I, _I, _I]),
    "kws_pool3s2_same_bwd_part_floats": (_I64, [_I, _I, _I]),
    "kws_pool3s2_same_bwd_f32": (_I, [_P, _P, _P, _P, _P, _I, _I, _I, _P]),
    "kws_conv1d_stats_rows": (_I, [ctypes.POINTER(Conv1dDesc)]),
    "kws_conv1d_fwd_f32": (_I, [_P, _P, _P, _P, _P, ctypes.POINTER(Conv1dDesc), _P]),
    "kws_conv1d_dgrad_f32": (_I, [_P, _P, _P, _I, ctypes.POINTER(Conv1dDesc), _P]),
    "kws_conv1d_wgrad_workspace_floats": (_I64, [ctypes.POINTER(Conv1dDesc)]),
    "kws_conv1d_wgrad_f32": (_I, [_P, _P, _P, _P, _P, ctypes.POINTER(Conv1dDesc), _P]),
    "kws_conv2d_stats_rows": (_I, [ctypes.POINTER(Conv2dDesc)]),
    "kws_conv2d_fwd_f32": (_I, [_P, _P, _P, _P, _P, ctypes.POINTER(Conv2dDesc), _P]),
    "kws_conv2d_dgrad_f32": (_I, [_P, _P, _P, ctypes.POINTER(Conv2dDesc), _P]),
    "kws_conv2d_wgrad_workspace_floats": (_I64, [ctypes.POINTER(Conv2dDesc)]),
    "kws_conv2d_wgrad_f32": (_I, [_P, _P, _P, _P, _P, ctypes.POINTER(Conv2dDesc), _P]),
    "kws_pool2x2_fwd_f32": (_I, [_P, _P, _P, _I, _I, _I, _I, _I, _P]),
    "kws_pool2x2_bwd_part_rows": (_I, [_I, _I, _I, _I]),
    "kws_pool2x2_bwd_part_floats": (_I64, [_I, _I, _I, _I]),
    "kws_pool2x2_bwd_f32": (_I, [_P, _P, _P, _P, _P, _I, _I, _I, _I, _I, _P]),
    "kws_frame_conv_stats_rows": (_I, [ctypes.POINTER(FrameConvDesc)]),
    "kws_frame_conv_fwd_f32": (_I, [_P, _P, _P, _P, ctypes.POINTER(FrameConvDesc), _P]),
    "kws_frame_conv_wgrad_workspace_floats": (_I64, [ctypes.POINTER(FrameConvDesc)]),
    "kws_frame_conv_wgrad_f32": (_I, [_P, _P, _P, _P, ctypes.POINTER(FrameConvDesc), _P]),
    "kws_fbank_conv_fwd_f32": (_I, [_P, _P, _P, ctypes.POINTER(FbankConvDesc), _P]),
    "kws_fbank_conv_wgrad_workspace_floats": (_I64, [ctypes.POINTER(FbankConvDesc)]),
    "kws_fbank_conv_wgrad_f32": (_I, [_P, _P, _P, _P, ctypes.POINTER(FbankConvDesc), _P]),
    "kws_gap_drop_fwd_f32": (_I, [_P, _P, _P, _P, _I, _I, _I, _F, ctypes.c_uint64, ctypes.c_uint32, ctypes.c_uint32, _I64, _P]),
    "kws_gap_drop_bwd_part_rows": (_I, [_I, _I, _I]),
    "kws_gap_drop_bwd_f32": (_I, [_P, _P, _P, _P, _P, _I, _I, _I, _F, ctypes.c_uint64, ctypes.c_uint32, ctypes.c_uint32, _I64,
                                  _P]),
    "kws_avgpool3_same_fwd_f32": (_I, [_P, _P, _P, _I, _I, _I, _P]),
    "kws_avgpool3_same_bwd_f32": (_I, [_P, _P, _I, _I, _I, _I, _P]),
    "kws_stem_stats_rows": (_I, [_I, _I]),
    "kws_stem_fwd_f32": (_I, [_P, _P, _P, _P, _I, _I, _I, _I, _P, _P]),
    "kws_stem_bwd_workspace_floats": (_I64, [_I, _I, _I, _I]),
    "kws_stem_bwd_f32": (_I, [_P, _P, _P, _P, _P, _P, _I, _I, _I, _I, _P, _P]),
    "kws_dwconvk_fwd_f32": (_I, [_P, _P, _P, _P, _I, _I, _I, _I, _I, _I, _I, _P]),
    "kws_dwconvk_bwd_part_rows": (_I, [_I, _I, _I, _I, _I]),
    "kws_dwconvk_bwd_part_floats": (_I64, [_I, _I, _I, _I, _I]),
    "kws_dwconvk_bwd_f32": (_I, [_P, _P, _P, _P, _P, _P, _I, _I, _I, _I, _I, _I, _I, _P]),
    "kws_dwconvk_bwd_finalize": (_I, [_P, _I, _I64, _I, _I, _P, _P, _P, _P, _P]),
    "kws_dwconvk_pw1_stats_rows": (_I, [_I64]),
    "kws_dwconvk_pw1_fwd_f32": (_I, [_P, _P, _P, _I64, _I, _P, _P]),
    "kws_dwconvk_pw1_bwd_workspace_floats": (_I64, [_I64, _I]),
    "kws_dwconvk_pw1_bwd_f32": (_I, [_P, _P, _P, _P, _P, _I64, _I, _P, _P]),
    "kws_gru_save_floats": (_I64, [_I, _I, _I]),
    "kws_gru_workspace_floats": (_I64, [_I, _I, _I, _I, _I]),
    "kws_gru_masks": (_I, [_P, _P, _I, _I, _I, _F, ctypes.c_uint64, ctypes.c_uint32, _I64, _P]),
    "kws_gru_seq_fwd_f32": (_I, [_P, _I64, _I64, _I, _P, _P, _P, _P, _P, _P, _P, _I, _I, _I, _P]),
    "kws_gru_seq_bwd_f32": (_I, [_P, _P, _P, _P, _P, _P, _I, _I, _I, _P]),
    "kws_gru_fwd_f32": (_I, [_P] * 12 + [_I, _I, _I, _I, _P]),
    "kws_gru_bwd_f32": (_I, [_P] * 17 + [_I, _I, _I, _I, _P]),
    "kws_attn_gate_fwd_floats": (_I64, [_I, _I, _I, _I]),
    "kws_attn_gate_bwd_floats": (_I64, [_I, _I, _I, _I]),
    "kws_attn_gate_fwd_f32": (_I, [_P] * 12 + [_I, _I, _I, _I, _I, _P]),
    "kws_attn_gate_bwd_f32": (_I, [_P] * 14 + [_I, _I, _I, _I, _I, _P]),
    "kws_transpose_f32": (_I, [_P, _P, _I, _I, _P]),
    "kws_bn_stats_finalize": (_I, [_P, _I, _I64, _I, _P, _P, _F, _F, _P, _P, _P, _P, _P]),
    "kws_bn_infer_prepare": (_I, [_P, _P, _P, _P, _F, _I, _P, _P]),
    "kws_bn_relu6_apply": (_I, [_P, _P, _P, _I64, _I, _I, _P]),
    "kws_dwconv_fwd_f32": (_I, [_P, _P, _P, _P, _I, _I, _I, _I, _I, _I, _P]),
    "kws_dwconv_bwd_part_floats": (_I64, [_I, _I, _I]),
    "kws_dwconv_bwd_f32": (_I, [_P, _P, _P, _P, _P, _P, _I, _I, _I, _I, _I, _I, _P]),
    "kws_dwconv_bwd_bn_f32": (_I, [_P, _P, _P, _P, _P, _P, _P, _I, _I, _I, _I, _I, _I, _I, _P]),
    "kws_dw_bwd_finalize": (_I, [_P, _I, _I64, _I, _P, _P, _P, _P, _P, _P]),
    "kws_bn_bwd_apply": (_I, [_P, _P, _P, _P, _P, _I64, _I, _P]),
    "kws_rmsprop_step": (_I, [_P, _P, _P, _P, _I64, _F, _F, _F, _F, _P]),
    "kws_sgd_momentum_step": (_I, [_P, _P, _P, _P, _I64, _F, _F, _F, _P]),
    "kws_adam_step": (_I, [_P, _P, _P, _P, _P, _I64, _F, _F, _F, _F, _F, _P]),
    "kws_l2_loss": (_I, [_P, _P, _I64, _P, _P]),
    "kws_net_create": (_I, [ctypes.POINTER(NetConfig), ctypes.POINTER(_P)]),
    "kws_net_destroy": (_I, [_P]),
    "kws_net_num_params": (_I64, [_P]),
    "kws_net_num_state": (_I64, [_P]),
    "kws_net_num_tensors": (_I, [_P]),
    "kws_net_tensor_info": (_I, [_P, _I, ctypes.POINTER(TensorInfo)]),
    "kws_net_workspace_bytes": (_I64, [_P, _I, _I]),
    "kws_net_debug_view": (_I, [_P, _I, _I, _I, _I, ctypes.POINTER(_I64), ctypes.POINTER(_I64)]),
    "kws_net_predict": (_I, [_P, _P, _P, _P, _I, _P, _P, _I64, _P]),
    "kws_net_train_fwd_bwd": (_I, [_P, _P, _P, _P, _P, _I, _P, _P, _P, ctypes.c_uint64, ctypes.c_uint32,
                                   _I64, _I, _P, _I64, _P]),
    "kws_net_num_blocks": (_I, [_P]),
    "kws_net_grad_ready_offset": (_I64, [_P, _I]),
    "kws_net_train_fwd_bwd_part": (_I, [_P, _P, _P, _P, _P, _I, _P, _P, _P, ctypes.c_uint64, ctypes.c_uint32,
                                        _I64, _I, _P, _I64, _I, _I, _P]),
}

_lib = None


def load():
    """Load libkws_hip.so (built in-tree by __graft_entry__.build() / csrc/Makefile)."""
    global _lib
    if _lib is not None:
        return _lib
    if not os.path.exists(LIB_PATH):
        raise KwsError("libkws_hip.so not found at %s - build it with "
                       "`python -c 'import __graft_entry__ as g; g.build()'` "
                       "(there is no CPU fallback)" % LIB_PATH)
    lib = ctypes.CDLL(LIB_PATH)
    lib.kws_abi_version.restype = _I
    if lib.kws_abi_version() != ABI_VERSION:      # before any other symbol is bound: a stale library says so itself
        raise KwsError("%s has ABI version %d, this package expects %d - rebuild it (__graft_entry__.build())" %
                       (LIB_PATH, lib.kws_abi_version(), ABI_VERSION))
    for name, (res, args) in SIGNATURES.items():
        fn = getattr(lib, name)  # AttributeError here = header/library mismatch
        fn.restype = res
        fn.argtypes = args
    _lib = lib
    return lib


def check(rc, what=""):
    if rc != 0:
        msg = load().kws_last_error()
        raise KwsError("%s failed (%d): %s" % (what or "libkws_hip call", rc,
                                               msg.decode() if msg else "?"))


def ptr(t):
    """Device pointer of a torch tensor (or None)."""
    if t is None:
        return None
    return ctypes.c_void_p(t.data_ptr())


def stream_ptr(stream=None):
    import torch
    s = stream if stream is not None else torch.cuda.current_stream()
    return ctypes.c_void_p(s.cuda_stream)


class OwnedStream(object):
    """A HIP stream of scheduling class `cls` (-1 low, 0 normal, +1 high) created by kws_stream_create, viewed by torch as
    an ExternalStream (which does not own the handle) and destroyed by close() / the finaliser after a synchronise."""

    def __init__(self, device, cls):
        import torch
        self.device = device
        with torch.cuda.device(device):
            h = ctypes.c_void_p()
            check(load().kws_stream_create(int(cls), ctypes.byref(h)), "kws_stream_create")
            self.handle = h.value
            self.stream = torch.cuda.ExternalStream(h.value, device=device)

    def close(self):
        h, self.handle = self.handle, None
        if h and _lib is not None:
            try:
                import torch
                with torch.cuda.device(self.device):
                    self.stream.synchronize()
                    _lib.kws_stream_destroy(ctypes.c_void_p(h))
            except Exception:      # interpreter shutdown: the runtime may be gone already
                pass
        self.stream = None

    def __del__(self):
        self.close()


class Profiler(object):
    """Per-kernel-family HIP-event profiler (kws_profiler_*): a handle that threads attach to.  attach() makes the CALLING
    thread's launches record into it, detach() stops that; collect() -> {family: {"ms", "count", "flops", "bytes"}} of
    everything recorded since the last collect()."""

    def __init__(self):
        h = ctypes.c_void_p()
        check(load().kws_profiler_create(ctypes.byref(h)), "kws_profiler_create")
        self.handle = h

    def attach(self):
        check(load().kws_profiler_attach(self.handle), "kws_profiler_attach")

    @staticmethod
    def detach():
        check(load().kws_profiler_attach(None), "kws_profiler_attach")

    def collect(self):
        lib = load()
        out = {}
        n = lib.kws_profiler_collect(self.handle)
        for i in range(n):
            name = ctypes.create_string_buffer(64)
            ms, fl, by = ctypes.c_double(), ctypes.c_double(), ctypes.c_double()
            cnt = ctypes.c_int64()
            check(lib.kws_profiler_get(self.handle, i, name, 64, ctypes.byref(ms), ctypes.byref(cnt), ctypes.byref(fl),
                                       ctypes.byref(by)), "kws_profiler_get")
            out[name.value.decode()] = {"ms": ms.value, "count": cnt.value, "flops": fl.value, "bytes": by.value}
        return out

    def close(self):
        """Destroys the handle.  Raises (and keeps the handle) while another thread is still attached to it."""
        h = self.handle
        if h is not None and _lib is not None:
            check(_lib.kws_profiler_destroy(h), "kws_profiler_destroy")
        self.handle = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


def call(name, *args):
    lib = load()
    rc = getattr(lib, name)(*args)
    check(rc, name)
