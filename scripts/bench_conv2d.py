"""conv_2d_mobile / conv_2d_fast: one training step at batch 1024 (forward + backward + SGD, HIP events, warm-up excluded) and the new
kernels at the shapes the models run them at - the Conv2D's three (kws_conv2d_*; every layer of both ladders) as a fraction of the
f32 matrix peak, next to torch.nn.functional.conv2d forward and forward + backward at the same shape on the same card; the pool's two
(kws_pool2x2_*) and conv_2d_mobile's activation + Dropout pass against the measured copy rate (6.3 TB/s).  Asserts
nothing; prints one JSON object.
usage: python3 scripts/bench_conv2d.py [--steps 20] [--warmup 5] [--out FILE] [--no-layers]"""
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
COPY_TBS = 6.3    # measured device copy rate, TB/s
B = 1024
# F, (kh, kw), stride, (dh, dw), pooled, Dropout behind: the two ladders as net_conv2d.hip builds them
LADDERS = {
    'conv_2d_mobile': [(32, (3, 3), 2, (1, 1), False, False), (32, (3, 3), 1, (1, 1), False, True),
                       (64, (3, 3), 2, (1, 1), False, False), (64, (3, 3), 1, (1, 1), False, True),
                       (128, (3, 3), 2, (1, 1), False, False), (128, (3, 3), 1, (1, 1), False, True),
                       (256, (3, 3), 2, (1, 1), False, False), (256, (3, 3), 1, (1, 1), False, True)],
    'conv_2d_fast': [(16, (11, 5), 1, (2, 1), True, False), (32, (5, 3), 1, (2, 1), True, False), (64, (3, 3), 1, (1, 1), True, False),
                     (128, (3, 3), 1, (1, 1), True, False)],
}


def same(n, k, s, d):
    out = -(-n // s)
    total = max((out - 1) * s + d * (k - 1) + 1 - n, 0)
    return out, total // 2, total - total // 2


def layers(name):
    H, W, C = 98, 40, 1
    for F, (kh, kw), s, (dh, dw), pool, drop in LADDERS[name]:
        Ho, pt, pb = same(H, kh, s, dh)
        Wo, pl, pr = same(W, kw, s, dw)
        yield dict(model=name, H=H, W=W, C=C, F=F, kh=kh, kw=kw, s=s, dh=dh, dw=dw, Ho=Ho, Wo=Wo, pads=(pt, pb, pl, pr), pool=pool, drop=drop)
        H, W, C = (Ho // 2, Wo // 2, F) if pool else (Ho, Wo, F)


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


def step_time(name, steps, warmup):
    model = speech_model(name, 3920, num_classes=12)
    g = torch.Generator(device="cuda")
    g.manual_seed(1)
    x = torch.randn((B, 3920), generator=g, device="cuda") * 12.0
    y = torch.eye(12, device="cuda")[torch.randint(0, 12, (B,), generator=g, device="cuda")].contiguous()
    row = torch.zeros(4, device="cuda")
    ms = timed(lambda: model._train_step_async(x, y, row), steps, warmup)
    ws = int(model.net.lib.kws_net_workspace_bytes(model.net.handle, B, 1))
    return {'ms_per_step': ms, 'clips_per_s': B / ms * 1e3, 'loss_last': float(row[0].item()) / B, 'workspace_gib': ws / 2.0 ** 30}


def conv_times(l, steps, warmup):
    lib = _lib.load()
    act = _lib.ACT_RELU6 if l['model'] == 'conv_2d_mobile' else _lib.ACT_RELU
    d = _lib.Conv2dDesc(B, l['H'], l['W'], l['Ho'], l['Wo'], l['kh'], l['kw'], l['s'], l['s'], l['dh'], l['dw'], l['pads'][0], l['pads'][2],
                        l['C'], l['F'], act)
    gen = torch.Generator(device="cuda")
    gen.manual_seed(2)
    X = torch.randn((B, l['H'], l['W'], l['C']), generator=gen, device="cuda")
    W = torch.randn((l['kh'], l['kw'], l['C'], l['F']), generator=gen, device="cuda") * 0.05
    dY = torch.randn((B, l['Ho'], l['Wo'], l['F']), generator=gen, device="cuda")
    Y = torch.empty_like(dY)
    dX = torch.empty_like(X)
    dW = torch.empty_like(W)
    st = torch.empty(lib.kws_conv2d_stats_rows(ctypes.byref(d)) * 2 * l['F'], device="cuda")
    ws = torch.empty(int(lib.kws_conv2d_wgrad_workspace_floats(ctypes.byref(d))), device="cuda")
    # the table is applied on load only where nothing stands between two convolutions (conv_2d_mobile's even-numbered layers)
    on_load = l['model'] == 'conv_2d_mobile' and l['s'] == 1
    bn = torch.rand(4 * l['C'], generator=gen, device="cuda") if on_load else None
    bnp = _lib.ptr(bn) if on_load else None
    S = _lib.stream_ptr()
    fwd = lambda: _lib.call("kws_conv2d_fwd_f32", _lib.ptr(X), bnp, _lib.ptr(W), _lib.ptr(Y), _lib.ptr(st), ctypes.byref(d), S)  # noqa: E731
    dgr = lambda: _lib.call("kws_conv2d_dgrad_f32", _lib.ptr(dY), _lib.ptr(W), _lib.ptr(dX), ctypes.byref(d), S)  # noqa: E731
    wgr = lambda: _lib.call("kws_conv2d_wgrad_f32", _lib.ptr(X), bnp, _lib.ptr(dY), _lib.ptr(dW), _lib.ptr(ws), ctypes.byref(d), S)  # noqa: E731
    M, K = B * l['Ho'] * l['Wo'], l['kh'] * l['kw'] * l['C']
    flops = 2.0 * M * K * l['F']
    nbytes = 4.0 * (X.numel() + Y.numel() + W.numel())          # each operand once
    out = {'op': 'conv2d', 'model': l['model'], 'shape': '%dx%d C%d -> %dx%d F%d k%dx%d s%d d%d,%d' %
           (l['H'], l['W'], l['C'], l['Ho'], l['Wo'], l['F'], l['kh'], l['kw'], l['s'], l['dh'], l['dw']), 'M': M, 'K': K,
           'gflop': flops / 1e9, 'mbytes': nbytes / 1e6, 'bn_on_load': on_load}
    for name, fn in (('fwd', fwd), ('dgrad', dgr), ('wgrad', wgr)):
        if name == 'dgrad' and l['C'] == 1:
            continue                                            # the input has no gradient: the model never makes this call
        us = timed(fn, steps, warmup) * 1e3
        out[name + '_us'] = us
        out[name + '_peak_fraction'] = flops / (us * 1e-6) / (PEAK_TF * 1e12)
    # yardstick: torch conv2d at the same shape (NCHW, explicit padding), forward and forward + both backward products
    pt, pb, pl, pr = l['pads']
    xt = Fn.pad(X.permute(0, 3, 1, 2), (pl, pr, pt, pb)).contiguous().requires_grad_(l['C'] > 1)
    wt = W.permute(3, 2, 0, 1).contiguous().requires_grad_(True)
    gt = dY.permute(0, 3, 1, 2).contiguous()
    out['torch_fwd_us'] = timed(lambda: Fn.conv2d(xt, wt, stride=l['s'], dilation=(l['dh'], l['dw'])), steps, warmup) * 1e3

    def fwd_bwd():
        yt = Fn.conv2d(xt, wt, stride=l['s'], dilation=(l['dh'], l['dw']))
        yt.backward(gt)
        xt.grad = None
        wt.grad = None

    out['torch_fwd_bwd_us'] = timed(fwd_bwd, steps, warmup) * 1e3
    out['ours_fwd_bwd_us'] = out['fwd_us'] + out.get('dgrad_us', 0.0) + out['wgrad_us']
    return out


def pool_times(l, steps, warmup):
    H, W, C = l['Ho'], l['Wo'], l['F']
    gen = torch.Generator(device="cuda")
    gen.manual_seed(3)
    Y = torch.randn((B, H, W, C), generator=gen, device="cuda")
    bn = torch.rand(4 * C, generator=gen, device="cuda") - 0.3
    Z = torch.empty((B, H // 2, W // 2, C), device="cuda")
    dZ = torch.randn((B, H // 2, W // 2, C), generator=gen, device="cuda")
    G = torch.empty_like(Y)
    part = torch.empty(int(_lib.load().kws_pool2x2_bwd_part_floats(B, H, W, C)), device="cuda")
    S = _lib.stream_ptr()
    n, nz = 4.0 * Y.numel(), 4.0 * Z.numel()
    out = {'op': 'pool2x2', 'model': l['model'], 'shape': '%dx%d C%d' % (H, W, C)}
    for name, fn, nb in (
            ('fwd', lambda: _lib.call("kws_pool2x2_fwd_f32", _lib.ptr(Y), _lib.ptr(bn), _lib.ptr(Z), B, H, W, C, _lib.ACT_RELU, S), n + nz),
            ('bwd', lambda: _lib.call("kws_pool2x2_bwd_f32", _lib.ptr(dZ), _lib.ptr(Y), _lib.ptr(bn), _lib.ptr(G), _lib.ptr(part), B, H, W, C,
                                      _lib.ACT_RELU, S), 2 * n + nz)):
        us = timed(fn, steps, warmup) * 1e3
        out[name + '_us'] = us
        out[name + '_tbs'] = nb / (us * 1e-6) / 1e12
        out[name + '_copy_rate_fraction'] = (nb / (COPY_TBS * 1e12) * 1e6) / us
    return out


def dropout_pass_times(l, steps, warmup):
    """conv_2d_mobile's Dropout(.05) as the program runs it: kws_bn_relu6_apply into a scratch tensor, kws_dropout_fwd out of it"""
    M, C = B * l['Ho'] * l['Wo'], l['F']
    gen = torch.Generator(device="cuda")
    gen.manual_seed(4)
    Y = torch.randn((M, C), generator=gen, device="cuda")
    bn = torch.rand(4 * C, generator=gen, device="cuda")
    A, O = torch.empty_like(Y), torch.empty_like(Y)
    S = _lib.stream_ptr()

    def both():
        _lib.call("kws_bn_relu6_apply", _lib.ptr(Y), _lib.ptr(bn), _lib.ptr(A), M, C, 1, S)
        _lib.call("kws_dropout_fwd", _lib.ptr(A), _lib.ptr(O), B, l['Ho'] * l['Wo'] * C, 0.95, 1, 0, 2, 0, S)

    us = timed(both, steps, warmup) * 1e3
    nb = 4.0 * 4.0 * Y.numel()                                   # two reads, two writes; fused on load it would be none
    return {'op': 'bn_relu6_apply + dropout_fwd', 'model': l['model'], 'shape': '%dx%d C%d' % (l['Ho'], l['Wo'], C), 'us': us,
            'tbs': nb / (us * 1e-6) / 1e12, 'copy_rate_fraction': (nb / (COPY_TBS * 1e12) * 1e6) / us}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--steps', type=int, default=20)
    ap.add_argument('--warmup', type=int, default=5)
    ap.add_argument('--out', default=None)
    ap.add_argument('--no-layers', action='store_true')
    a = ap.parse_args()
    torch.cuda.set_device(0)
    res = {'batch': B, 'peak_tflops_f32': PEAK_TF, 'copy_tbs': COPY_TBS, 'device': torch.cuda.get_device_name(0)}
    for name in LADDERS:
        res[name] = step_time(name, a.steps, a.warmup)
    if not a.no_layers:
        res['kernels'] = []
        for name in LADDERS:
            for l in layers(name):
                res['kernels'].append(conv_times(l, a.steps, a.warmup))
                if l['pool']:
                    res['kernels'].append(pool_times(l, a.steps, a.warmup))
                if l['drop']:
                    res['kernels'].append(dropout_pass_times(l, a.steps, a.warmup))
    line = json.dumps(res)
    print(line)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, 'w') as f:
            f.write(line + '\n')


if __name__ == '__main__':
    main()
