"""adam_kernel against rmsprop_kernel and sgd_kernel on one 1.2 M-parameter buffer (about the flagship's): HIP events over
back-to-back launches, warm-up excluded.  At this size a launch moves 29 - 38 MB, which stays in the last-level cache between
repeats: the figures are launch-sized times, not HBM rates.  Prints one JSON object.
usage: python3 scripts/bench_optimizers.py [--steps 50] [--warmup 10] [--n 1200000] [--out FILE]"""
import argparse
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch  # noqa: E402

from speech_recognition_amd import _lib  # noqa: E402


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


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--steps', type=int, default=50)
    ap.add_argument('--warmup', type=int, default=10)
    ap.add_argument('--n', type=int, default=1200000)
    ap.add_argument('--out', default=None)
    a = ap.parse_args()
    torch.cuda.set_device(0)
    n = a.n
    gen = torch.Generator(device="cuda")
    gen.manual_seed(4)
    p = torch.randn(n, generator=gen, device="cuda")
    g = torch.randn(n, generator=gen, device="cuda") * 1e-2
    m, v, l2 = torch.zeros(n, device="cuda"), torch.zeros(n, device="cuda"), torch.full((n,), 1e-5, device="cuda")
    S, P = _lib.stream_ptr(), _lib.ptr
    kernels = (
        ('adam', 32.0, lambda: _lib.call("kws_adam_step", P(p), P(g), P(m), P(v), P(l2), n, 3e-4, 0.9, 0.999, 1e-8, 1.0, S)),
        ('rmsprop', 24.0, lambda: _lib.call("kws_rmsprop_step", P(p), P(g), P(v), P(l2), n, 1e-3, 0.9, 1e-8, 1.0, S)),
        ('sgd', 24.0, lambda: _lib.call("kws_sgd_momentum_step", P(p), P(g), P(m), P(l2), n, 1e-2, 0.9, 1.0, S)),
    )
    res = {'n_params': n, 'device': torch.cuda.get_device_name(0), 'steps': a.steps, 'warmup': a.warmup}
    for name, bytes_per_param, fn in kernels:
        ms = timed(fn, a.steps, a.warmup)
        res[name + '_us'] = ms * 1e3
        res[name + '_bytes_per_param'] = bytes_per_param
        res[name + '_TBps'] = bytes_per_param * n / (ms * 1e-3) / 1e12
    res['adam_over_rmsprop'] = res['adam_us'] / res['rmsprop_us']
    line = json.dumps(res)
    print(line)
    if a.out:
        with open(a.out, 'w') as f:
            f.write(line + '\n')


if __name__ == '__main__':
    main()
