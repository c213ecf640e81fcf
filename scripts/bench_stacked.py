"""conv_1d_time_stacked / conv_1d_heavy: one training step at batch 1024 (forward + backward + Adam, HIP events, warm-up
excluded) and, per ladder layer, the dense Conv1D's three kernels (kws_gconv_* with one group) and the pool's two
(kws_pool3s2_*), each against its own floor: algorithmic bytes over the measured copy rate (6.3 TB/s) and, for the
convolutions, FLOPs over the f32 matrix peak.  Prints one JSON object.
usage: python3 scripts/bench_stacked.py [--steps 20] [--warmup 5] [--out FILE] [--no-layers]"""
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
WIDTHS = {'time_stacked': ((800, 20), (48, 96, 128, 160, 192, 256)), 'heavy': ((1600, 10), (48, 96, 128, 160, 192, 256, 320))}


def ladder(kind):
    """(model, L, C, k, F, pooled, producer BN on load) per layer, as net_grouped.hip builds it."""
    (L, C), widths = WIDTHS[kind]
    out = [(kind, L, C, 1, 32, False, False)]
    L, C, on_load = L, 32, True
    for F in widths:
        out.append((kind, L, C, 3, F, True, on_load))
        L, C = (L - 2 - 3) // 2 + 1, F
        out.append((kind, L, C, 3, F, False, False))
        L, on_load = L - 2, True
    return out


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


def step_time(model_type, steps, warmup):
    model = speech_model(model_type, 16000, num_classes=12)
    g = torch.Generator(device="cuda")
    g.manual_seed(1)
    x = torch.randn((B, 16000), generator=g, device="cuda") * 0.0774
    y = torch.eye(12, device="cuda")[torch.randint(0, 12, (B,), generator=g, device="cuda")].contiguous()
    row = torch.zeros(4, device="cuda")
    ms = timed(lambda: model._train_step_async(x, y, row), steps, warmup)
    return {'ms_per_step': ms, 'clips_per_s': B / ms * 1e3, 'loss_last': float(row[0].item()) / B}


def layer_times(layer, steps, warmup):
    kind, L, C, k, F, pooled, on_load = layer
    Lout = L - k + 1
    d = _lib.GconvDesc(B, L, C, Lout, k, 1, 1, C, F, 0)
    lib = _lib.load()
    gen = torch.Generator(device="cuda")
    gen.manual_seed(2)
    X = torch.randn((B, L, C), generator=gen, device="cuda")
    W = torch.randn((k, C, F), generator=gen, device="cuda") * 0.05
    dY = torch.randn((B, Lout, F), generator=gen, device="cuda")
    Y = torch.empty((B, Lout, F), device="cuda")
    dX = torch.empty((B, L, C), device="cuda")
    dW = torch.empty_like(W)
    st = torch.empty(lib.kws_gconv_stats_rows(ctypes.byref(d)) * 2 * F, device="cuda")
    ws = torch.empty(int(lib.kws_gconv_wgrad_workspace_floats(ctypes.byref(d))), device="cuda")
    bn = torch.rand(4 * C, generator=gen, device="cuda") if on_load else None
    S = _lib.stream_ptr()
    bnp, bg = _lib.ptr(bn), (C if on_load else 0)
    fwd = lambda: _lib.call("kws_gconv_fwd_f32", _lib.ptr(X), bnp, bg, _lib.ptr(W), _lib.ptr(Y), _lib.ptr(st), ctypes.byref(d), S)  # noqa: E731
    dgr = lambda: _lib.call("kws_gconv_dgrad_f32", _lib.ptr(dY), _lib.ptr(W), _lib.ptr(dX), ctypes.byref(d), S)  # noqa: E731
    wgr = lambda: _lib.call("kws_gconv_wgrad_f32", _lib.ptr(X), bnp, bg, _lib.ptr(dY), _lib.ptr(dW), _lib.ptr(ws), ctypes.byref(d), S)  # noqa: E731
    flops = 2.0 * B * Lout * k * C * F
    nbytes = 4.0 * (B * L * C + B * Lout * F + k * C * F)      # each operand once
    floor_us = max(flops / (PEAK_TF * 1e12), nbytes / (COPY_TBS * 1e12)) * 1e6
    out = {'model': kind, 'shape': 'L%d C%d k%d F%d' % (L, C, k, F), 'gflop': flops / 1e9, 'mbytes': nbytes / 1e6,
           'conv_floor_us': floor_us, 'conv_floor_is': 'flops' if flops / (PEAK_TF * 1e12) > nbytes / (COPY_TBS * 1e12) else 'bytes'}
    for name, fn in (('fwd', fwd), ('dgrad', dgr), ('wgrad', wgr)):
        us = timed(fn, steps, warmup) * 1e3
        out[name + '_us'] = us
        out[name + '_floor_ratio'] = floor_us / us
    if pooled:
        Lp = lib.kws_pool3s2_out_len(Lout)
        table = torch.rand(4 * F, generator=gen, device="cuda") - 0.3       # some negative scales
        Z = torch.empty((B, Lp, F), device="cuda")
        dZ = torch.randn((B, Lp, F), generator=gen, device="cuda")
        G = torch.empty((B, Lout, F), device="cuda")
        part = torch.empty(int(lib.kws_pool3s2_bwd_part_floats(B, Lout, F)), device="cuda")
        pf = lambda: _lib.call("kws_pool3s2_fwd_f32", _lib.ptr(dY), _lib.ptr(table), _lib.ptr(Z), B, Lout, F, S)  # noqa: E731
        pb = lambda: _lib.call("kws_pool3s2_bwd_f32", _lib.ptr(dZ), _lib.ptr(dY), _lib.ptr(table), _lib.ptr(G), _lib.ptr(part), B,  # noqa: E731
                               Lout, F, S)
        for name, fn, nb in (('pool_fwd', pf, 4.0 * B * F * (Lout + Lp)), ('pool_bwd', pb, 4.0 * B * F * (2 * Lout + Lp))):
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
    res = {'batch': B, 'peak_tflops_f32': PEAK_TF, 'copy_tbs': COPY_TBS, 'device': torch.cuda.get_device_name(0)}
    for mt in ('conv_1d_time_stacked', 'conv_1d_heavy'):
        res[mt] = step_time(mt, a.steps, a.warmup)
    if not a.no_layers:
        res['layers'] = [layer_times(l, a.steps, a.warmup) for k in ('time_stacked', 'heavy') for l in ladder(k)]
    line = json.dumps(res)
    print(line)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, 'w') as f:
            f.write(line + '\n')


if __name__ == '__main__':
    main()
