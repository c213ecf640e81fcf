"""conv_1d_multi_time_sliced: one training step at batch 1024 (forward + backward + RMSprop, HIP events, warm-up excluded) and
every kernel the model added, each against its own floor: algorithmic bytes over the measured copy rate (6.3 TB/s).
  kws_pool3s2_same_fwd_f32   4 B C (L + Lp): y read, the pooled tensor written            (the seven xs4 shapes)
  kws_pool3s2_same_bwd_f32   4 B C (2 L + Lp): dz and y read, g written
  kws_stem_fwd_f32           4 B (L C + (L - 2) N): x read once, y written                (the three stems)
  kws_stem_bwd_f32           4 B (L C + (L - 2) N): x and dy read once
Prints one JSON object.
usage: python3 scripts/bench_mts.py [--steps 20] [--warmup 5] [--out FILE] [--no-layers]"""
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
POOLS = [(3998, 16), (1997, 32), (997, 48), (497, 64), (247, 96), (122, 128), (59, 160)]   # (L, C) of the xs4 reduce blocks
STEMS = [(4000, 4, 16), (3200, 5, 16), (640, 25, 32)]                                      # (L, C, N)


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
    model = speech_model('conv_1d_multi_time_sliced', 16000, num_classes=12)
    g = torch.Generator(device="cuda")
    g.manual_seed(1)
    x = torch.randn((B, 16000), generator=g, device="cuda") * 0.0774
    y = torch.eye(12, device="cuda")[torch.randint(0, 12, (B,), generator=g, device="cuda")].contiguous()
    row = torch.zeros(4, device="cuda")
    ms = timed(lambda: model._train_step_async(x, y, row), steps, warmup)
    return {'ms_per_step': ms, 'clips_per_s': B / ms * 1e3, 'loss_last': float(row[0].item()) / B}


def _ratio(out, name, fn, nbytes, steps, warmup):
    us = timed(fn, steps, warmup) * 1e3
    out[name + '_us'] = us
    out[name + '_tbs'] = nbytes / (us * 1e-6) / 1e12
    out[name + '_floor_ratio'] = (nbytes / (COPY_TBS * 1e12) * 1e6) / us


def pool_times(L, C, steps, warmup):
    lib = _lib.load()
    Lp = lib.kws_pool3s2_same_out_len(L)
    gen = torch.Generator(device="cuda")
    gen.manual_seed(2)
    Y = torch.randn((B, L, C), generator=gen, device="cuda")
    bn = torch.rand(4 * C, generator=gen, device="cuda") - 0.3
    dZ = torch.randn((B, Lp, C), generator=gen, device="cuda")
    Z = torch.empty((B, Lp, C), device="cuda")
    G = torch.empty((B, L, C), device="cuda")
    part = torch.empty(int(lib.kws_pool3s2_same_bwd_part_floats(B, L, C)), device="cuda")
    S = _lib.stream_ptr()
    fwd = lambda: _lib.call("kws_pool3s2_same_fwd_f32", _lib.ptr(Y), _lib.ptr(bn), _lib.ptr(Z), B, L, C, S)  # noqa: E731
    bwd = lambda: _lib.call("kws_pool3s2_same_bwd_f32", _lib.ptr(dZ), _lib.ptr(Y), _lib.ptr(bn), _lib.ptr(G), _lib.ptr(part), B, L, C, S)  # noqa: E731
    fb, bb = 4.0 * B * C * (L + Lp), 4.0 * B * C * (2 * L + Lp)
    out = {'shape': 'L%d C%d' % (L, C), 'fwd_mbytes': fb / 1e6, 'bwd_mbytes': bb / 1e6}
    _ratio(out, 'fwd', fwd, fb, steps, warmup)
    _ratio(out, 'bwd', bwd, bb, steps, warmup)
    return out


def stem_times(L, C, N, steps, warmup):
    lib = _lib.load()
    gen = torch.Generator(device="cuda")
    gen.manual_seed(3)
    X = torch.randn((B, L, C), generator=gen, device="cuda")
    W = torch.randn((3, C), generator=gen, device="cuda") * 0.5
    P = torch.randn((C, N), generator=gen, device="cuda") * 0.3
    dY = torch.randn((B, L - 2, N), generator=gen, device="cuda")
    Y = torch.empty((B, L - 2, N), device="cuda")
    st = torch.empty(lib.kws_stem_stats_rows(B, L) * 2 * N, device="cuda")
    ws = torch.empty(int(lib.kws_stem_bwd_workspace_floats(B, L, C, N)), device="cuda")
    dW, dP = torch.empty(3 * C, device="cuda"), torch.empty(C * N, device="cuda")
    S = _lib.stream_ptr()
    fwd = lambda: _lib.call("kws_stem_fwd_f32", _lib.ptr(X), _lib.ptr(W), _lib.ptr(P), _lib.ptr(Y), B, L, C, N, _lib.ptr(st), S)  # noqa: E731
    bwd = lambda: _lib.call("kws_stem_bwd_f32", _lib.ptr(dY), _lib.ptr(X), _lib.ptr(W), _lib.ptr(P), _lib.ptr(dW), _lib.ptr(dP), B, L, C,  # noqa: E731
                            N, _lib.ptr(ws), S)
    nb = 4.0 * B * (L * C + (L - 2) * N)
    out = {'shape': 'L%d C%d N%d' % (L, C, N), 'mbytes': nb / 1e6}
    _ratio(out, 'fwd', fwd, nb, steps, warmup)
    _ratio(out, 'bwd', bwd, nb, steps, warmup)
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
    res['conv_1d_multi_time_sliced'] = step_time(a.steps, a.warmup)
    if not a.no_layers:
        res['pool_same'] = [pool_times(L, C, a.steps, a.warmup) for L, C in POOLS]
        res['stems'] = [stem_times(L, C, N, a.steps, a.warmup) for L, C, N in STEMS]
    line = json.dumps(res)
    print(line)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, 'w') as f:
            f.write(line + '\n')


if __name__ == '__main__':
    main()
