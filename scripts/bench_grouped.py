"""conv_1d_fast / conv_1d_spec: one training step at batch 1024 (forward + backward + RMSprop, HIP events, warm-up excluded)
and, per grouped layer, the library's three grouped-Conv1D kernels against the same-run torch.nn.functional.conv1d(groups=g)
forward and backward (a yardstick only: torch is never on the product path).  Prints one JSON object.
usage: python3 scripts/bench_grouped.py [--steps 20] [--warmup 5] [--out FILE]
       rocprofv3 --kernel-trace --stats -d DIR -- python3 scripts/bench_grouped.py --steps 5 --warmup 2 --no-layers"""
import argparse
import ctypes
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch  # noqa: E402
import torch.nn.functional as Fn  # noqa: E402

from speech_recognition_amd import _lib  # noqa: E402
from speech_recognition_amd.model import speech_model  # noqa: E402

PEAK_TF = 157.3   # MI355X dense f32 matrix peak, TFLOP/s
B = 1024
# (model, B, L, C, k, stride, g, gs, Ng, producer BN width or 0)
LAYERS = [('fast', 98, 252, 15, 2, 6, 42, 50, 0), ('fast', 42, 300, 7, 2, 5, 60, 72, 50),
          ('spec', 98, 257, 3, 2, 4, 63, 75, 0), ('spec', 48, 300, 3, 1, 3, 100, 100, 75),
          ('spec', 46, 300, 3, 2, 4, 75, 90, 100), ('spec', 22, 360, 3, 1, 3, 120, 120, 90),
          ('spec', 20, 360, 3, 2, 4, 90, 105, 120), ('spec', 9, 420, 3, 1, 3, 120, 140, 105),
          ('spec', 7, 420, 3, 2, 4, 105, 120, 140), ('spec', 3, 480, 3, 1, 3, 160, 160, 120)]


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
    D = 16000 if model_type == 'conv_1d_fast' else 98 * 257
    g = torch.Generator(device="cuda")
    g.manual_seed(1)
    x = torch.randn((B, D), generator=g, device="cuda") * (0.0774 if model_type == 'conv_1d_fast' else 1.0)
    if model_type == 'conv_1d_spec':
        x = x.abs_()
    y = torch.eye(12, device="cuda")[torch.randint(0, 12, (B,), generator=g, device="cuda")].contiguous()
    row = torch.zeros(4, device="cuda")
    ms = timed(lambda: model._train_step_async(x, y, row), steps, warmup)
    return {'ms_per_step': ms, 'clips_per_s': B / ms * 1e3, 'loss_last': float(row[0].item()) / B}


def layer_times(layer, steps, warmup):
    kind, L, C, k, s, g, gs, Ng, bg = layer
    Lout = (L - k) // s + 1
    F = g * Ng
    d = _lib.GconvDesc(B, L, C, Lout, k, s, g, gs, Ng, 0)
    lib = _lib.load()
    gen = torch.Generator(device="cuda")
    gen.manual_seed(2)
    X = torch.randn((B, L, C), generator=gen, device="cuda")
    W = torch.randn((g, k, gs, Ng), generator=gen, device="cuda") * 0.05
    dY = torch.randn((B, Lout, F), generator=gen, device="cuda")
    Y = torch.empty((B, Lout, F), device="cuda")
    dX = torch.empty((B, L, C), device="cuda")
    dW = torch.empty_like(W)
    st = torch.empty(lib.kws_gconv_stats_rows(ctypes.byref(d)) * 2 * F, device="cuda")
    ws = torch.empty(int(lib.kws_gconv_wgrad_workspace_floats(ctypes.byref(d))), device="cuda")
    bn = None
    if bg:
        bn = torch.rand(C // bg, 4, bg, generator=gen, device="cuda").reshape(-1)
    S = _lib.stream_ptr()
    bnp = _lib.ptr(bn)
    fwd = lambda: _lib.call("kws_gconv_fwd_f32", _lib.ptr(X), bnp, bg, _lib.ptr(W), _lib.ptr(Y), _lib.ptr(st), ctypes.byref(d), S)  # noqa: E731
    dgr = lambda: _lib.call("kws_gconv_dgrad_f32", _lib.ptr(dY), _lib.ptr(W), _lib.ptr(dX), ctypes.byref(d), S)  # noqa: E731
    wgr = lambda: _lib.call("kws_gconv_wgrad_f32", _lib.ptr(X), bnp, bg, _lib.ptr(dY), _lib.ptr(dW), _lib.ptr(ws), ctypes.byref(d), S)  # noqa: E731
    flops = 2.0 * B * Lout * k * gs * Ng * g          # algorithmic, per operation
    out = {'model': kind, 'shape': 'L%d C%d k%d s%d g%d gs%d Ng%d' % (L, C, k, s, g, gs, Ng), 'gflop': flops / 1e9}
    for name, fn in (('fwd', fwd), ('dgrad', dgr), ('wgrad', wgr)):
        ms = timed(fn, steps, warmup)
        out[name + '_us'] = ms * 1e3
        out[name + '_pct_peak'] = 100.0 * flops / (ms * 1e-3) / (PEAK_TF * 1e12)
    # yardstick: torch conv1d(groups=g) on the channels the groups read, NCL layout, its forward and both backward products
    xt = X[:, :, :g * gs].permute(0, 2, 1).contiguous().requires_grad_(True)
    wt = W.permute(0, 3, 2, 1).reshape(F, gs, k).contiguous().requires_grad_(True)
    gy = dY.permute(0, 2, 1).contiguous()
    out['torch_fwd_us'] = timed(lambda: Fn.conv1d(xt, wt, stride=s, groups=g), steps, warmup) * 1e3

    def tb():
        yt = Fn.conv1d(xt, wt, stride=s, groups=g)
        torch.autograd.grad(yt, (xt, wt), gy)
    out['torch_fwd_bwd_us'] = timed(tb, steps, warmup) * 1e3
    out['ours_fwd_bwd_us'] = out['fwd_us'] + out['dgrad_us'] + out['wgrad_us']
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--steps', type=int, default=20)
    ap.add_argument('--warmup', type=int, default=5)
    ap.add_argument('--out', default=None)
    ap.add_argument('--no-layers', action='store_true')
    a = ap.parse_args()
    torch.cuda.set_device(0)
    res = {'batch': B, 'peak_tflops_f32': PEAK_TF, 'device': torch.cuda.get_device_name(0)}
    for mt in ('conv_1d_fast', 'conv_1d_spec'):
        res[mt] = step_time(mt, a.steps, a.warmup)
    if not a.no_layers:
        res['layers'] = [layer_times(l, a.steps, a.warmup) for l in LAYERS]
    line = json.dumps(res)
    print(line)
    if a.out:
        with open(a.out, 'w') as f:
            f.write(line + '\n')


if __name__ == '__main__':
    main()
