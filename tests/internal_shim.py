"""Builds and loads libkws_internal_test.so: the library's own objects (csrc/build/*.o) plus tests/native/internal_shim.cpp, whose
kwst_* forwarders expose the hidden launchers of the residual-network programs (resblock.hip, dwconv.hip, gemm.hip), the fused
backward GEMM pair (gemm.hip kws_gemm_dgrad_wgrad_f32), the classifier tails (tail.hip, gconv.hip kws_flat_tail_launch), the
BatchNorm bookkeeping shared by the grouped, depthwise, multi-slice and inception programs (bncols.hip kws_gbn_*), the
raw-waveform net's first convolution (conv1.hip kws_conv1_*) and the two batch launchers of bn.hip (kws_dw_grad_finalize_batch,
kws_bn_infer_prepare_batch) to ctypes; built once per process, whichever test module asks first.
The public kws_* entry points come from the same library (-Wl,-Bsymbolic keeps its calls inside its own copy), so every kernel a
test compares comes from one build.  Also: the join / shortcut shapes the residual programs launch, read from the planner of
net_logmfcc.hip through the public net API (host-side only: no GPU needed)."""
import ctypes
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "speech_recognition_amd", "csrc")
HIPCC = "/opt/rocm/bin/hipcc"
SHIM_SRC = os.path.join(ROOT, "tests", "native", "internal_shim.cpp")

_P = ctypes.c_void_p
_I = ctypes.c_int
_I64 = ctypes.c_int64
_F = ctypes.c_float

KWST_SIGNATURES = {
    "kwst_block_out_fwd": (_I, [_P, _P, _P, _P, _P, _I, _I, _I, _I, _P]),
    "kwst_block_out_dw_fwd": (_I, [_P, _P, _P, _P, _P, _P, _P, _I, _I, _I, _I, _P]),
    "kwst_block_out_bwd_part_floats": (_I64, [_I, _I, _I, _I]),
    "kwst_block_out_bwd": (_I, [_P, _P, _P, _P, _P, _I, _I, _I, _I, _I, _P]),
    "kwst_block_join_bwd_parts": (_I, [_I, _I, _I, _I]),
    "kwst_block_join_bwd": (_I, [_P, _P, _P, _P, _P, _P, _P, _I, _I, _I, _I, _I, _I, _P]),
    "kwst_block_out3_fwd": (_I, [_P, _P, _P, _P, _P, _I, _I, _I, _I, _I, _I, _P]),
    "kwst_block_out3_bwd_part_floats": (_I64, [_I, _I, _I]),
    "kwst_block_out3_bwd": (_I, [_P, _P, _P, _P, _P, _I, _I, _I, _I, _I, _I, _P]),
    "kwst_add_f32": (_I, [_P, _P, _P, _I64, _P]),
    "kwst_add_strided_f32": (_I, [_P, _P, _I, _I, _I, _I, _I, _P]),
    "kwst_dwconv_bwd_acc_f32": (_I, [_P, _P, _P, _P, _P, _P, _I, _I, _I, _I, _I, _I, _P]),
    "kwst_dwconv_bwd_acc_strided_f32": (_I, [_P, _P, _P, _P, _I, _I, _P, _P, _I, _I, _I, _I, _I, _I, _P]),
    "kwst_gather_strided_rows": (ctypes.c_bool, [_P, ctypes.POINTER(_I)]),
    "kwst_gemm_nn_strided_f32": (_I, [_P, _I, _P, _P, _I64, _I, _I, _P, _P]),
    "kwst_gemm_tn_slabs_strided_f32": (_I, [_P, _I, _P, _I64, _I, _I, _P, ctypes.POINTER(_I), _P]),
    "kwst_gemm_tn_slabs_f32": (_I, [_P, _P, _I64, _I, _I, _P, ctypes.POINTER(_I), _P]),
    "kwst_gemm_dgrad_wgrad_f32": (_I, [_P, _P, _P, _P, _I64, _I, _I, _P, ctypes.POINTER(_I), _P]),
    "kwst_reduce_slabs_batch": (_I, [_P, _P, _P, _P, _I, _P]),
    "kwst_ts_tail_launch": (_I, [_P, _P]),
    "kwst_small_wgrad_launch": (_I, [_P, _P, _P, _P, _I, _I, _I, _P, _P]),
    "kwst_metrics_launch": (_I, [_P, _P, _I, _P, _P]),
    "kwst_tail_post_launch": (_I, [_P, ctypes.POINTER(_I), _P]),
    "kwst_flat_tail_launch": (_I, [_P, _I, _P]),
    "kwst_reduce_slabs_f32": (_I, [_P, _P, _I64, _I, _P]),
    "kwst_tail_struct_layout": (None, [ctypes.POINTER(_I64)]),
    "kwst_gbn_finalize": (_I, [_P, _I, _I64, _P, _P, _F, _F, _P, _P]),
    "kwst_gbn_infer": (_I, [_P, _P, _F, _P, _P]),
    "kwst_gbn_bwd_rows": (_I, [_I64]),
    "kwst_gbn_bwd": (_I, [_P, _P, _P, _P, _I64, _P, _P, _P, _P, _I64, _I64, _P]),
    "kwst_gbn_bwd_finish": (_I, [_P, _P, _P, _I64, _P, _P, _I, _P, _P, _I64, _I64, _P]),
    "kwst_gbn_struct_layout": (None, [ctypes.POINTER(_I64)]),
    "kwst_conv1_supported": (ctypes.c_bool, [_P, _P, _I]),
    "kwst_conv1_stats_rows": (_I, [_I64]),
    "kwst_conv1_wgrad_workspace_floats": (_I64, [_I64]),
    "kwst_conv1_fwd": (_I, [_P, _P, _P, _P, _P, _I, _I, _P, _P]),
    "kwst_conv1_wgrad": (_I, [_P, _P, _P, _P, _P, _I, _I, _P, _P]),
    "kwst_conv1_wgrad_slabs": (_I, [_P, _P, _P, _P, _P, _I, _I, _P, _P, _P, _P, _P, _I, _P]),
    "kwst_reduce_slab_groups_f32": (_I, [_P, _I64, _I, _I, _P]),
    "kwst_dw_grad_finalize_batch": (_I, [_P, _P, _P, _P, _I, _P]),
    "kwst_bn_infer_prepare_batch": (_I, [_P, _P, _P, _P, _F, _P, _P, _I, _P]),
}
# the public entry points the tests compare against, taken from the same library
PUBLIC = ["kws_last_error", "kws_dwconv_fwd_f32", "kws_dwconv_bwd_f32", "kws_dwconv_bwd_part_floats", "kws_dw_bwd_finalize",
          "kws_bn_bwd_apply", "kws_bn_relu6_apply", "kws_gemm_nn_f32", "kws_gemm_nn_stats_rows", "kws_gemm_num_row_tiles",
          "kws_gemm_tn_f32", "kws_gemm_tn_workspace_floats", "kws_gemm_gather_f32", "kws_gemm_tn_gather_f32", "kws_net_create", "kws_net_destroy", "kws_net_num_tensors",
          "kws_net_tensor_info", "kws_net_debug_view", "kws_dwconv_fwd_amax_f32", "kws_dwconv_bwd_bn_f32", "kws_dwconv_bwd_bn_amax_f32",
          "kws_bn_bwd_apply_amax", "kws_bn_stats_finalize", "kws_bn_infer_prepare"]


_BUILT = None    # the library this process has already built: every test module after the first reuses it


def build(out_dir):
    """make the library's objects, compile the shim against the internal headers and link both; returns the .so path.  Built
    once per process: a later call returns the first call's library, whatever its out_dir."""
    global _BUILT
    if _BUILT is None:
        _BUILT = _build(out_dir)
    return _BUILT


def _build(out_dir):
    subprocess.check_call(["make", "-C", CSRC, "-j8"], stdout=subprocess.DEVNULL)
    shim_o = os.path.join(out_dir, "internal_shim.o")
    r = subprocess.run([HIPCC, "-O3", "-std=c++17", "-fPIC", "-fvisibility=hidden", "--offload-arch=gfx950", "-Wall", "-Werror",
                        "-Wno-unused-function", "-I", CSRC, "-x", "hip", "-c", SHIM_SRC, "-o", shim_o],
                       capture_output=True, text=True, timeout=600)
    if r.returncode != 0:
        raise RuntimeError("internal_shim.cpp failed to compile:\n" + r.stderr[-4000:])
    objs = sorted(os.path.join(CSRC, "build", f) for f in os.listdir(os.path.join(CSRC, "build")) if f.endswith(".o"))
    so = os.path.join(out_dir, "libkws_internal_test.so")
    r = subprocess.run([HIPCC, "--offload-arch=gfx950", "-shared", "-fPIC", "-Wl,-Bsymbolic", "-o", so, shim_o] + objs,
                       capture_output=True, text=True, timeout=600)
    if r.returncode != 0:
        raise RuntimeError("libkws_internal_test.so failed to link:\n" + r.stderr[-4000:])
    return so


def load(so):
    from speech_recognition_amd import _lib
    lib = ctypes.CDLL(so)
    for name, (res, args) in KWST_SIGNATURES.items():
        fn = getattr(lib, name)
        fn.restype, fn.argtypes = res, args
    for name in PUBLIC:
        res, args = _lib.SIGNATURES[name]
        fn = getattr(lib, name)
        fn.restype, fn.argtypes = res, args
    return lib


def exported_symbols(so):
    out = subprocess.check_output(["nm", "-D", "--defined-only", so], text=True)
    return set(line.split()[-1] for line in out.splitlines() if line.strip())


class Gather(ctypes.Structure):
    _fields_ = [("L_out", _I), ("cin", _I), ("taps", _I), ("stride_t", _I), ("stride_j", _I), ("base_off", _I),
                ("x_len", _I), ("x_batch_stride", _I64)]


# ctypes mirrors of the tails' argument structs (csrc/internal.h); tail_struct_layout() below is what the library itself says
class TsTailArgs(ctypes.Structure):
    _fields_ = [(n, _P) for n in ("y", "bn", "W1", "b1", "W2", "labels", "probs", "g", "part", "xd", "fd", "dl1", "dl2",
                                  "per_loss", "per_correct", "att")] + \
               [("B", _I), ("T", _I), ("C", _I), ("NC", _I), ("seed", ctypes.c_uint64), ("step", ctypes.c_uint32),
                ("keep_prob", _F), ("label_smoothing", _F), ("loss_batch", _I), ("row_offset", _I64), ("train", _I)]


class TailPostArgs(ctypes.Structure):
    _fields_ = [("X2", _P), ("D2", _P), ("ws2", _P), ("K2", _I), ("N2", _I), ("X1", _P), ("D1", _P), ("ws1", _P), ("K1", _I),
                ("N1", _I), ("bias1", _P), ("per_loss", _P), ("per_correct", _P), ("metrics", _P), ("B", _I)]


class FlatTailArgs(ctypes.Structure):
    _fields_ = [("y", _P), ("bn", _P), ("Ng", _I), ("Wd", _P), ("bd", _P), ("labels", _P), ("probs", _P), ("fd", _P), ("dl", _P),
                ("dA", _P), ("per_loss", _P), ("per_correct", _P), ("B", _I), ("D", _I), ("F", _I), ("NC", _I),
                ("seed", ctypes.c_uint64), ("step", ctypes.c_uint32), ("keep_prob", _F), ("loss_batch", _I), ("row_offset", _I64),
                ("layer_id", ctypes.c_uint32), ("raw", _I)]


# (mirror, its last member) in the order of kwst_tail_struct_layout
TAIL_STRUCTS = [(TsTailArgs, "train"), (TailPostArgs, "B"), (FlatTailArgs, "raw")]


def tail_struct_layout(lib):
    """[(sizeof, offsetof last member)] of kws_ts_tail_args, kws_tail_post_args, kws_flat_tail_args as the library was compiled"""
    out = (_I64 * 6)()
    lib.kwst_tail_struct_layout(out)
    return [(int(out[2 * i]), int(out[2 * i + 1])) for i in range(3)]


# ctypes mirrors of bncols.hip's two descriptors (csrc/internal.h)
class GbnCols(ctypes.Structure):
    _fields_ = [("g", _I), ("Ng", _I), ("pitch", _I), ("c0", _I)]


class GbnRefs(ctypes.Structure):
    _fields_ = [("gamma", _P), ("pstride", _I64), ("boff", _I64), ("mm", _P), ("sstride", _I64), ("voff", _I64)]


GBN_STRUCTS = [(GbnCols, "c0"), (GbnRefs, "voff")]


def gbn_struct_layout(lib):
    """[(sizeof, offsetof last member)] of kws_gbn_cols, kws_gbn_refs as the library was compiled"""
    out = (_I64 * 4)()
    lib.kwst_gbn_struct_layout(out)
    return [(int(out[2 * i]), int(out[2 * i + 1])) for i in range(2)]


# the four residual programs of net_logmfcc.hip, configured as speech_model() builds them (model.py); C3 = conv_1d_log_mfcc at
# 98 x 40 features, the flagship of the bench
PROGRAMS = {
    "conv_1d_log_mfcc": dict(kind=2, nc=32, input_size=98 * 40, T=98, F=40, stem=1, pool3=False, B=2048),
    "conv_1d_spectrogram": dict(kind=2, nc=32, input_size=65 * 257, T=65, F=257, stem=1, pool3=False, B=1024),
    "conv_1d_residual": dict(kind=4, nc=12, input_size=16000, T=0, F=0, stem=1, pool3=True, B=1024),
    "conv_1d_mfcc_and_raw": dict(kind=5, nc=11, input_size=98 * 40 + 16000, T=98, F=40, stem=2, pool3=True, B=1024),
}


def planner_blocks(lib, name):
    """The residual blocks of program `name` as its planner lays them out: one dict per block with the join input (L = the
    second BatchNorm's rows per clip, C), the join's output length Lo, the pool / stride and, for a strided block, its shortcut
    (cin, the gather descriptor the planner builds).  Read from the net's tensor table (BN widths) and its debug views (rows of
    every BN input), which is the planner's own layout; the walk stops at the first BN run that is not a block."""
    from speech_recognition_amd import _lib
    p = PROGRAMS[name]
    B = p["B"]
    net = _P()
    cfg = _lib.NetConfig(p["kind"], p["nc"], 1, p["input_size"], p["T"], p["F"])
    assert lib.kws_net_create(ctypes.byref(cfg), ctypes.byref(net)) == 0, lib.kws_last_error()
    try:
        widths = {}
        info = _lib.TensorInfo()
        for i in range(lib.kws_net_num_tensors(net)):
            assert lib.kws_net_tensor_info(net, i, ctypes.byref(info)) == 0
            nm = info.name.decode()
            if nm.startswith("batch_normalization_") and nm.endswith("/gamma"):
                widths[int(nm[len("batch_normalization_"):-len("/gamma")])] = int(info.shape[0])
        views = []
        off, cnt = _I64(), _I64()
        for idx in sorted(widths):
            if lib.kws_net_debug_view(net, B, 1, 0, idx, ctypes.byref(off), ctypes.byref(cnt)) != 0:
                break
            C = widths[idx]
            assert cnt.value % (B * C) == 0
            views.append((cnt.value // (B * C), C))
    finally:
        lib.kws_net_destroy(net)
    stem = views[:p["stem"]]
    cin = sum(c for _, c in stem)
    k, blocks = p["stem"], []
    while k + 1 < len(views):
        short = views[k][0] != views[k + 1][0]
        j = k + 1 if short else k
        if j + 1 >= len(views) or views[j] != views[j + 1]:
            break
        L, C = views[j]
        if short:
            stride = 2
            Lo = views[k][0]
            if views[k][1] != C or Lo != -(-L // 2):
                break
        else:
            stride, Lo = 1, L
            if C != cin:
                break
        blk = dict(L=L, C=C, Lo=Lo, pool=stride, cin=cin, B=B)
        if p["pool3"]:
            pad = max((Lo - 1) * stride + 3 - L, 0)
            blk["pad_l"] = pad // 2
        if short:
            # the planner's shortcut gather (net_logmfcc.hip): row (b, t) of the 1 x 1 stride-2 convolution reads input row 2 t
            blk["gather"] = dict(L_out=Lo, cin=cin, taps=1, stride_t=stride * cin, stride_j=0, base_off=0, x_len=L * cin,
                                 x_batch_stride=L * cin)
        blocks.append(blk)
        cin = C
        k = j + 2
    return blocks
