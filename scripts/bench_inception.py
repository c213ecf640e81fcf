"""inception_d1: one training step at batch 1024 (forward + backward + Adam, HIP events, warm-up excluded) and the new kernels at
the shapes the model runs them at - the dense Conv1D's three (kws_conv1d_*; each distinct convolution of the twelve blocks once) and
the average pool's two (kws_avgpool3_same_*) - each against its own floor: algorithmic bytes over the measured copy rate (6.3 TB/s,
DESIGN.md) and, for the convolutions, FLOPs over the f32 matrix peak.  Asserts nothing; prints one JSON object.
usage: python3 scripts/bench_inception.py [--steps 20] [--warmup 5] [--out FILE] [--no-layers]"""
import argparse
import ctypes
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch  # noqa: E402

from speech_recognition_amd import _lib  # noqa: E402
from speech_recognition_amd.model import speech_model  # noqa: E402

PEAK_TF = 157.3   # MI355X dense f32 matrix peak, TFLOP/s
COPY_TBS = 6.3    # measured device copy rate, TB/s
B = 1024


def block_convs():
    """The distinct (L, Cx, Cin, Cy, y0, F, k, dil) of the blocks, as net_inception.hip builds them, with how often each runs."""
    seen = {}
    L, C = 93, 256
    for kind, d in (('inc', 2), ('inc', 2), ('red', 0), ('inc', 2), ('inc', 1), ('red', 0), ('inc', 1), ('inc', 1), ('red', 0), ('inc', 1),
                    ('inc', 1), ('red', 0)):
        if kind == 'inc':
            convs = [(L, C, C, 256, 0, 64, 1, 1), (L, C, C, 48, 0, 48, 1, 1), (L, 48, 48, 256, 64, 64, 3, 2), (L, C, C, 64, 0, 64, 1, 1),
                     (L, 64, 64, 96, 0, 96, 3, d), (L, 96, 96, 256, 128, 96, 3, d), (L, C, C, 256, 224, 32, 1, 1)]
            pool = (L, C)
            C = 256
        else:
            convs = [(L, C, C, 192, 0, 192, 3, 1), (L, C, C, 32, 0, 32, 1, 1), (L, 32, 32, 48, 0, 48, 3, 1), (L, 48, 48, 48, 0, 48, 3, 1)]
            pool = None
            L, C = (L + 1) // 2, 192 + 48 + C
        for c in convs:
            seen[('conv',) + c] = seen.get(('conv',) + c, 0) + 1
        if pool:
            seen[('avg',) + pool] = seen.get(('avg',) + pool, 0) + 1
    return seen


def timed(fn, steps, warmup):
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(steps):
        fn()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b) / steps


def step_time(steps, warmup):
    model = speech_model('inception_d1', 16000, num_classes=12)
    g = torch.Generator(device="cuda")
    g.manual_seed(1)
    x = torch.randn((B, 16000), generator=g, device="cuda") * 0.0774
    y = torch.eye(12, device="cuda")[torch.randint(0, 12, (B,), generator=g, device="cuda")].contiguous()
    row = torch.zeros(4, device="cuda")
    ms = timed(lambda: model._train_step_async(x, y, row), steps, warmup)
    ws = int(model.net.lib.kws_net_workspace_bytes(model.net.handle, B, 1))
    return {'ms_per_step': ms, 'clips_per_s': B / ms * 1e3, 'loss_last': float(row[0].item()) / B, 'workspace_gib': ws / 2.0 ** 30}


def conv_times(shape, count, steps, warmup):
    L, Cx, Cin, Cy, y0, F, k, dil = shape
    d = _lib.Conv1dDesc(B, L, L, k, dil, dil * (k - 1) // 2, Cx, 0, Cin, Cy, y0, F)
    lib = _lib.load()
    gen = torch.Generator(device="cuda")
    gen.manual_seed(2)
    X = torch.randn((B, L, Cx), generator=gen, device="cuda")
    W = torch.randn((k, Cin, F), generator=gen, device="cuda") * 0.05
    dY = torch.randn((B, L, Cy), generator=gen, device="cuda")
    Y = torch.empty((B, L, Cy), device="cuda")
    dX = torch.zeros((B, L, Cx), device="cuda")
    dW = torch.empty_like(W)
    st = torch.empty(lib.kws_conv1d_stats_rows(ctypes.byref(d)) * 2 * F, device="cuda")
    ws = torch.empty(int(lib.kws_conv1d_wgrad_workspace_floats(ctypes.byref(d))), device="cuda")
    bn = torch.rand(4 * Cx, generator=gen, device="cuda")
    S = _lib.stream_ptr()
    fwd = lambda: _lib.call("kws_conv1d_fwd_f32", _lib.ptr(X), _lib.ptr(bn), _lib.ptr(W), _lib.ptr(Y), _lib.ptr(st), ctypes.byref(d), S)  # noqa: E731
    dgr = lambda: _lib.call("kws_conv1d_dgrad_f32", _lib.ptr(dY), _lib.ptr(W), _lib.ptr(dX), 0, ctypes.byref(d), S)  # noqa: E731
    dga = lambda: _lib.call("kws_conv1d_dgrad_f32", _lib.ptr(dY), _lib.ptr(W), _lib.ptr(dX), 1, ctypes.byref(d), S)  # noqa: E731
    wgr = lambda: _lib.call("kws_conv1d_wgrad_f32", _lib.ptr(X), _lib.ptr(bn), _lib.ptr(dY), _lib.ptr(dW), _lib.ptr(ws), ctypes.byref(d), S)  # noqa: E731
    flops = 2.0 * B * L * k * Cin * F
    nbytes = 4.0 * (B * L * Cin + B * L * F + k * Cin * F)      # each operand once
    floor_us = max(flops / (PEAK_TF * 1e12), nbytes / (COPY_TBS * 1e12)) * 1e6
    out = {'op': 'conv1d', 'shape': 'L%d Cin%d/%d F%d@%d/%d k%d dil%d' % (L, Cin, Cx, F, y0, Cy, k, dil), 'runs_per_step': count,
           'gflop': flops / 1e9, 'mbytes': nbytes / 1e6, 'floor_us': floor_us,
           'floor_is': 'flops' if flops / (PEAK_TF * 1e12) > nbytes / (COPY_TBS * 1e12) else 'bytes'}
    for name, fn in (('fwd', fwd), ('dgrad', dgr), ('dgrad_accumulate', dga), ('wgrad', wgr)):
        us = timed(fn, steps, warmup) * 1e3
        out[name + '_us'] = us
        out[name + '_floor_ratio'] = floor_us / us
    return out


def avg_times(shape, count, steps, warmup):
    L, C = shape
    gen = torch.Generator(device="cuda")
    gen.manual_seed(3)
    X = torch.randn((B, L, C), generator=gen, device="cuda")
    bn = torch.rand(4 * C, generator=gen, device="cuda") - 0.3
    Z = torch.empty_like(X)
    dX = torch.zeros_like(X)
    S = _lib.stream_ptr()
    out = {'op': 'avgpool3_same', 'shape': 'L%d C%d' % (L, C), 'runs_per_step': count}
    n = 4.0 * B * L * C
    for name, fn, nb in (
            ('fwd', lambda: _lib.call("kws_avgpool3_same_fwd_f32", _lib.ptr(X), _lib.ptr(bn), _lib.ptr(Z), B, L, C, S), 2 * n),
            ('bwd', lambda: _lib.call("kws_avgpool3_same_bwd_f32", _lib.ptr(Z), _lib.ptr(dX), 0, B, L, C, S), 2 * n),
            ('bwd_accumulate', lambda: _lib.call("kws_avgpool3_same_bwd_f32", _lib.ptr(Z), _lib.ptr(dX), 1, B, L, C, S), 3 * n)):
        us = timed(fn, steps, warmup) * 1e3
        out[name + '_us'] = us
        out[name + '_tbs'] = nb / (us * 1e-6) / 1e12
        out[name + '_floor_ratio'] = (nb / (COPY_TBS * 1e12) * 1e6) / us
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--steps', type=int, default=20)
    ap.add_argument('--warmup', type=int, default=5)
    ap.add_argument('--out', default=None)
    ap.add_argument('--no-layers', action='store_true')
    a = ap.parse_args()
    torch.cuda.set_device(0)
    res = {'batch': B, 'peak_tflops_f32': PEAK_TF, 'copy_tbs': COPY_TBS, 'device': torch.cuda.get_device_name(0),
           'inception_d1': step_time(a.steps, a.warmup)}
    if not a.no_layers:
        res['kernels'] = [(conv_times if key[0] == 'conv' else avg_times)(key[1:], n, a.steps, a.warmup)
                          for key, n in block_convs().items()]
    line = json.dumps(res)
    print(line)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, 'w') as f:
            f.write(line + '\n')


if __name__ == '__main__':
    main()
