"""xception_with_attention: one training step at batch 1024 (forward + backward + RMSprop, HIP events, warm-up excluded) and the new
kernels of csrc/attgate.hip on their own at the model's shape (B 1024, T 50, C 384, k 5): the gate's forward call (logits, table,
apply: 3 B T C 4 bytes) and backward call (gate gradient, fold, dx, weight fold: 5 B T C 4 bytes plus the partial rows), each
against its own byte count at the copy rate measured in the same run (a device-to-device copy of one [B, T, C] tensor: read +
write); and the GRU's recurrence launches at T 50, H 192.  Reports what the run measured; there is no bar.
Prints one JSON object.
usage: python3 scripts/bench_xception.py [--steps 20] [--warmup 5] [--out FILE] [--no-layers]"""
import argparse
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch  # noqa: E402

from speech_recognition_amd import _lib  # noqa: E402
from speech_recognition_amd.model import speech_model  # noqa: E402

B, T, C, K, H = 1024, 50, 384, 5, 192


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
    model = speech_model('xception_with_attention', 16000, num_classes=12)
    g = torch.Generator(device="cuda")
    g.manual_seed(1)
    x = torch.randn((B, 16000), generator=g, device="cuda") * 0.0774
    y = torch.eye(12, device="cuda")[torch.randint(0, 12, (B,), generator=g, device="cuda")].contiguous()
    row = torch.zeros(4, device="cuda")
    ms = timed(lambda: model._train_step_async(x, y, row), steps, warmup)
    return {'ms_per_step': ms, 'clips_per_s': B / ms * 1e3, 'loss_last': float(row[0].item()) / B}


def gate_times(steps, warmup):
    lib = _lib.load()
    P, S = _lib.ptr, _lib.stream_ptr()
    gen = torch.Generator(device="cuda")
    gen.manual_seed(2)
    rnd = lambda *shape: torch.randn(shape, generator=gen, device="cuda")  # noqa: E731
    x, dy = rnd(B, T, C).clamp(0, 6), rnd(B, T, C) * 0.1
    wa, Wa = rnd(K, C) * 0.1, rnd(C) * 0.1
    gamma, beta = torch.full((1,), 1.5, device="cuda"), torch.full((1,), 2.0, device="cuda")
    mm, mv = torch.zeros(1, device="cuda"), torch.ones(1, device="cuda")
    u, att, tab = torch.empty(B * T, device="cuda"), torch.empty(B * T, device="cuda"), torch.empty(4, device="cuda")
    y, dx = torch.empty_like(x), torch.empty_like(x)
    dwa, dWa, dg, db = torch.empty_like(wa), torch.empty_like(Wa), torch.empty(1, device="cuda"), torch.empty(1, device="cuda")
    n_b = int(lib.kws_attn_gate_bwd_floats(B, T, C, K))
    wf = torch.empty(int(lib.kws_attn_gate_fwd_floats(B, T, C, K)), device="cuda")
    wb = torch.empty(n_b, device="cuda")
    fwd = lambda: _lib.call("kws_attn_gate_fwd_f32", P(x), P(wa), P(Wa), P(gamma), P(beta), P(mm), P(mv), P(u), P(tab), P(att), P(y), P(wf),  # noqa: E731
                            B, T, C, K, 1, S)
    bwd = lambda: _lib.call("kws_attn_gate_bwd_f32", P(dy), P(x), P(u), P(att), P(tab), P(wa), P(Wa), P(gamma), P(dx), P(dwa), P(dWa), P(dg),  # noqa: E731
                            P(db), P(wb), B, T, C, K, 1, S)
    tensor = 4.0 * B * T * C
    copy_us = timed(lambda: y.copy_(x), steps, warmup) * 1e3
    rate = 2.0 * tensor / (copy_us * 1e-6)
    rows_bytes = 2.0 * 4.0 * (n_b - B * T - 2 * B)      # the partial rows are written once and read once
    res = {'shape': 'B%d T%d C%d k%d' % (B, T, C, K), 'copy_us': copy_us, 'copy_GBps': rate / 1e9,
           'fwd_bytes': 3.0 * tensor, 'bwd_bytes': 5.0 * tensor + rows_bytes}
    for name, fn, nbytes in (('fwd', fwd, res['fwd_bytes']), ('bwd', bwd, res['bwd_bytes'])):
        us = timed(fn, steps, warmup) * 1e3
        res[name + '_us'] = us
        res[name + '_floor_us'] = nbytes / rate * 1e6
        res[name + '_over_floor'] = us / res[name + '_floor_us']
    return res


def gru_times(steps, warmup):
    lib = _lib.load()
    P, S = _lib.ptr, _lib.stream_ptr()
    gen = torch.Generator(device="cuda")
    gen.manual_seed(3)
    rnd = lambda *shape: torch.randn(shape, generator=gen, device="cuda")  # noqa: E731
    U = [rnd(H, 3 * H) * 0.1 for _ in range(2)]
    b = [rnd(3 * H) * 0.1 for _ in range(2)]
    dout, out = rnd(B, 2 * H), torch.empty(B, 2 * H, device="cuda")
    mh = torch.ones(6 * B * H, device="cuda")
    save = torch.empty(int(lib.kws_gru_save_floats(B, T, H)), device="cuda")
    a = rnd(2, 3, B * T, H)
    ut = rnd(2, 3, H, H) * 0.1
    da, lop = torch.empty(6 * B * T * H, device="cuda"), torch.empty(6 * B * T * H, device="cuda")
    seq_f = lambda: _lib.call("kws_gru_seq_fwd_f32", P(a), 3 * B * T * H, B * T * H, H, P(U[0]), P(U[1]), P(b[0]), P(b[1]), P(mh), P(out),  # noqa: E731
                              P(save), B, T, H, S)
    seq_b = lambda: _lib.call("kws_gru_seq_bwd_f32", P(dout), P(ut), P(mh), P(save), P(da), P(lop), B, T, H, S)  # noqa: E731
    res = {'shape': 'B%d T%d H%d' % (B, T, H)}
    flops = 2.0 * 2 * B * T * H * 3 * H
    for name, fn in (('seq_fwd', seq_f), ('seq_bwd', seq_b)):
        res[name + '_us'] = timed(fn, steps, warmup) * 1e3
        res[name + '_tflops'] = flops / (res[name + '_us'] * 1e-6) / 1e12
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--steps', type=int, default=20)
    ap.add_argument('--warmup', type=int, default=5)
    ap.add_argument('--out', default=None)
    ap.add_argument('--no-layers', action='store_true')
    a = ap.parse_args()
    torch.cuda.set_device(0)
    res = {'batch': B, 'device': torch.cuda.get_device_name(0)}
    res['xception_with_attention'] = step_time(a.steps, a.warmup)
    if not a.no_layers:
        res['gate'] = gate_times(a.steps, a.warmup)
        res['gru'] = gru_times(a.steps, a.warmup)
    line = json.dumps(res)
    print(line)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, 'w') as f:
            f.write(line + '\n')


if __name__ == '__main__':
    main()
