"""conv_1d_gru: one training step at batch 1024 (forward + backward + RMSprop, HIP events, warm-up excluded) and, per block,
the general depthwise kernels (kws_dwconvk_fwd_f32 / kws_dwconvk_bwd_f32 + finalize) and block 1's one-channel pointwise pair,
each against its own floor: algorithmic bytes over the measured copy rate (6.3 TB/s) - 4 B C (L_in + L_out) forward,
4 B C (2 L_in + L_out) backward (y and dz read, g written).  As the in-run yardstick the shipped 3-tap kws_dwconv_fwd_f32 is
timed on a stride-2 shape of the headline net, and the general kernel on the same shape: what generality costs.
Prints one JSON object.
usage: python3 scripts/bench_dwk.py [--steps 20] [--warmup 5] [--out FILE] [--no-layers]"""
import argparse
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch  # noqa: E402

from speech_recognition_amd import _lib  # noqa: E402
from speech_recognition_amd.model import speech_model  # noqa: E402

COPY_TBS = 6.3    # measured device copy rate, TB/s
B = 1024
# (L_in, C, k, stride, pad_l, L_out, producer BN on load) per block, as net_dwk.hip builds it
BLOCKS = [(16000, 1, 63, 16, 23, 1000, False), (1000, 128, 31, 4, 13, 250, True), (250, 256, 15, 4, 6, 63, True),
          (63, 384, 7, 4, 2, 16, True), (16, 448, 5, 2, 1, 8, True), (8, 512, 8, 1, 0, 1, True)]
YARDSTICK = (397, 128, 3, 2, 1, 199, True)   # the headline net's first strided depthwise layer (SAME: pad_l 1)


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
    model = speech_model('conv_1d_gru', 16000, num_classes=12)
    g = torch.Generator(device="cuda")
    g.manual_seed(1)
    x = torch.randn((B, 16000), generator=g, device="cuda") * 0.0774
    y = torch.eye(12, device="cuda")[torch.randint(0, 12, (B,), generator=g, device="cuda")].contiguous()
    row = torch.zeros(4, device="cuda")
    ms = timed(lambda: model._train_step_async(x, y, row), steps, warmup)
    return {'ms_per_step': ms, 'clips_per_s': B / ms * 1e3, 'loss_last': float(row[0].item()) / B}


def block_times(blk, steps, warmup, three_tap=False):
    L, C, k, s, pad_l, Lout, on_load = blk
    lib = _lib.load()
    gen = torch.Generator(device="cuda")
    gen.manual_seed(2)
    Y = torch.randn((B, L, C), generator=gen, device="cuda")
    W = torch.randn((k, C), generator=gen, device="cuda") * 0.2
    dZ = torch.randn((B, Lout, C), generator=gen, device="cuda")
    Z = torch.empty((B, Lout, C), device="cuda")
    G = torch.empty((B, L, C), device="cuda")
    bn = (torch.rand(4 * C, generator=gen, device="cuda") - 0.3) if on_load else None
    part = torch.empty(int(lib.kws_dwconvk_bwd_part_floats(B, L, C, k, s)), device="cuda")
    rows = lib.kws_dwconvk_bwd_part_rows(B, L, C, k, s)
    fin = torch.empty((k + 4) * C, device="cuda")
    S = _lib.stream_ptr()
    fwd = lambda: _lib.call("kws_dwconvk_fwd_f32", _lib.ptr(Y), _lib.ptr(bn), _lib.ptr(W), _lib.ptr(Z), B, L, Lout, C, k, s, pad_l, S)  # noqa: E731
    bwd = lambda: _lib.call("kws_dwconvk_bwd_f32", _lib.ptr(dZ), _lib.ptr(Y), _lib.ptr(bn), _lib.ptr(W), _lib.ptr(G), _lib.ptr(part), B,  # noqa: E731
                            L, Lout, C, k, s, pad_l, S)
    fz = lambda: _lib.call("kws_dwconvk_bwd_finalize", _lib.ptr(part), rows, B * L, C, k, _lib.ptr(fin[:k * C]),  # noqa: E731
                           _lib.ptr(fin[k * C:(k + 1) * C]), _lib.ptr(fin[(k + 1) * C:(k + 2) * C]), _lib.ptr(fin[(k + 2) * C:]), S)
    fb, bb = 4.0 * B * C * (L + Lout), 4.0 * B * C * (2 * L + Lout)
    out = {'shape': 'L%d C%d k%d s%d' % (L, C, k, s), 'fwd_mbytes': fb / 1e6, 'bwd_mbytes': bb / 1e6, 'part_rows': rows}
    for name, fn, nb in (('fwd', fwd, fb), ('bwd', bwd, bb), ('finalize', fz, None)):
        us = timed(fn, steps, warmup) * 1e3
        out[name + '_us'] = us
        if nb:
            out[name + '_tbs'] = nb / (us * 1e-6) / 1e12
            out[name + '_floor_ratio'] = (nb / (COPY_TBS * 1e12) * 1e6) / us
    if three_tap:
        f3 = lambda: _lib.call("kws_dwconv_fwd_f32", _lib.ptr(Y), _lib.ptr(bn), _lib.ptr(W), _lib.ptr(Z), B, L, Lout, C, s, pad_l, S)  # noqa: E731
        us = timed(f3, steps, warmup) * 1e3
        out['three_tap_fwd_us'] = us
        out['three_tap_fwd_floor_ratio'] = (fb / (COPY_TBS * 1e12) * 1e6) / us
    return out


def pw1_times(steps, warmup):
    lib = _lib.load()
    M, N = B * 1000, 128
    gen = torch.Generator(device="cuda")
    gen.manual_seed(3)
    z = torch.randn(M, generator=gen, device="cuda")
    p = torch.randn(N, generator=gen, device="cuda")
    dy = torch.randn((M, N), generator=gen, device="cuda")
    y = torch.empty((M, N), device="cuda")
    st = torch.empty(lib.kws_dwconvk_pw1_stats_rows(M) * 2 * N, device="cuda")
    ws = torch.empty(int(lib.kws_dwconvk_pw1_bwd_workspace_floats(M, N)), device="cuda")
    dz, dp = torch.empty(M, device="cuda"), torch.empty(N, device="cuda")
    S = _lib.stream_ptr()
    fwd = lambda: _lib.call("kws_dwconvk_pw1_fwd_f32", _lib.ptr(z), _lib.ptr(p), _lib.ptr(y), M, N, _lib.ptr(st), S)  # noqa: E731
    bwd = lambda: _lib.call("kws_dwconvk_pw1_bwd_f32", _lib.ptr(dy), _lib.ptr(z), _lib.ptr(p), _lib.ptr(dz), _lib.ptr(dp), M, N,  # noqa: E731
                            _lib.ptr(ws), S)
    out = {'shape': 'M%d N%d' % (M, N)}
    for name, fn, nb in (('fwd', fwd, 4.0 * (M + M * N)), ('bwd', bwd, 4.0 * (2 * M + M * N))):
        us = timed(fn, steps, warmup) * 1e3
        out[name + '_us'] = us
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
    res = {'batch': B, 'copy_tbs': COPY_TBS, 'device': torch.cuda.get_device_name(0)}
    res['conv_1d_gru'] = step_time(a.steps, a.warmup)
    if not a.no_layers:
        res['blocks'] = [block_times(blk, a.steps, a.warmup) for blk in BLOCKS]
        res['pointwise_1'] = pw1_times(a.steps, a.warmup)
        res['yardstick_3tap_s2'] = block_times(YARDSTICK, a.steps, a.warmup, three_tap=True)
    line = json.dumps(res)
    print(line)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, 'w') as f:
            f.write(line + '\n')


if __name__ == '__main__':
    main()
