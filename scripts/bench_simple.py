"""conv_1d_simple: one training step at batch 1024 (forward + backward + Adam, HIP events, warm-up excluded) and the new kernels of
csrc/gru.hip on their own at the model's shape (B 1024, T 10, I 224, H 128): the recurrence forward and backward launches, the
whole op forward and backward (projections, weight gradients and dx included), and the mask draw.  Beside the two recurrence
launches: torch.nn.GRU(224, 128, bidirectional=True) forward + backward on the same card at the same shape - a TIMING yardstick
only (its cell is the reset_after variant and it includes its own input projections, so no values are compared); if the
library behind it will not run here the column is left out and the reason recorded.
Prints one JSON object.
usage: python3 scripts/bench_simple.py [--steps 20] [--warmup 5] [--out FILE] [--no-layers]"""
import argparse
import ctypes
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch  # noqa: E402

from speech_recognition_amd import _lib  # noqa: E402
from speech_recognition_amd.model import speech_model  # noqa: E402

B, T, I, H = 1024, 10, 224, 128


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
    model = speech_model('conv_1d_simple', 16000, num_classes=12)
    g = torch.Generator(device="cuda")
    g.manual_seed(1)
    x = torch.randn((B, 16000), generator=g, device="cuda") * 0.0774
    y = torch.eye(12, device="cuda")[torch.randint(0, 12, (B,), generator=g, device="cuda")].contiguous()
    row = torch.zeros(4, device="cuda")
    ms = timed(lambda: model._train_step_async(x, y, row), steps, warmup)
    return {'ms_per_step': ms, 'clips_per_s': B / ms * 1e3, 'loss_last': float(row[0].item()) / B}


def gru_times(steps, warmup):
    lib = _lib.load()
    P, S = _lib.ptr, _lib.stream_ptr()
    gen = torch.Generator(device="cuda")
    gen.manual_seed(2)
    rnd = lambda *shape: torch.randn(shape, generator=gen, device="cuda")  # noqa: E731
    x = rnd(B, T, I).clamp(0, 6)
    W = [rnd(I, 3 * H) * 0.1 for _ in range(2)]
    U = [rnd(H, 3 * H) * 0.1 for _ in range(2)]
    b = [rnd(3 * H) * 0.1 for _ in range(2)]
    dout = rnd(B, 2 * H)
    mx, mh = torch.empty(6 * B * I, device="cuda"), torch.empty(6 * B * H, device="cuda")
    ws = torch.empty(int(lib.kws_gru_workspace_floats(B, T, I, H, 1)), device="cuda")
    save = torch.empty(int(lib.kws_gru_save_floats(B, T, H)), device="cuda")
    out, dx = torch.empty(B, 2 * H, device="cuda"), torch.empty(B, T, I, device="cuda")
    g = [torch.empty_like(t) for t in (W[0], U[0], b[0], W[1], U[1], b[1])]
    a = rnd(2, 3, B * T, H)
    ut = rnd(2, 3, H, H) * 0.1
    da, lop = torch.empty(6 * B * T * H, device="cuda"), torch.empty(6 * B * T * H, device="cuda")
    masks = lambda: _lib.call("kws_gru_masks", P(mx), P(mh), B, I, H, ctypes.c_float(0.8), ctypes.c_uint64(1), ctypes.c_uint32(0), 0, S)  # noqa: E731
    fwd = lambda: _lib.call("kws_gru_fwd_f32", P(x), P(W[0]), P(U[0]), P(b[0]), P(W[1]), P(U[1]), P(b[1]), P(mx), P(mh), P(out), P(save),  # noqa: E731
                            P(ws), B, T, I, H, S)
    bwd = lambda: _lib.call("kws_gru_bwd_f32", P(dout), P(x), P(W[0]), P(U[0]), P(W[1]), P(U[1]), P(mx), P(mh), P(save), P(dx), P(g[0]),  # noqa: E731
                            P(g[1]), P(g[2]), P(g[3]), P(g[4]), P(g[5]), P(ws), B, T, I, H, S)
    seq_f = lambda: _lib.call("kws_gru_seq_fwd_f32", P(a), 3 * B * T * H, B * T * H, H, P(U[0]), P(U[1]), P(b[0]), P(b[1]), P(mh), P(out),  # noqa: E731
                              P(save), B, T, H, S)
    seq_b = lambda: _lib.call("kws_gru_seq_bwd_f32", P(dout), P(ut), P(mh), P(save), P(da), P(lop), B, T, H, S)  # noqa: E731
    masks()
    res = {'shape': 'B%d T%d I%d H%d' % (B, T, I, H)}
    for name, fn in (('masks', masks), ('seq_fwd', seq_f), ('seq_bwd', seq_b), ('op_fwd', fwd), ('op_bwd', bwd)):
        res[name + '_us'] = timed(fn, steps, warmup) * 1e3
    flops = 2.0 * 2 * B * T * H * 3 * H
    res['seq_fwd_tflops'] = flops / (res['seq_fwd_us'] * 1e-6) / 1e12
    res['seq_bwd_tflops'] = flops / (res['seq_bwd_us'] * 1e-6) / 1e12
    try:
        gru = torch.nn.GRU(I, H, batch_first=True, bidirectional=True).cuda()
        xt = x.clone().requires_grad_(True)

        def torch_step():
            o, hn = gru(xt)
            hn.backward(dout.view(B, 2, H).transpose(0, 1).contiguous())
        res['torch_gru_fwd_bwd_us'] = timed(torch_step, steps, warmup) * 1e3
        res['torch_gru_note'] = 'reset_after cell, input projections included: timing yardstick only'
        res['seq_fwd_plus_bwd_over_torch'] = (res['seq_fwd_us'] + res['seq_bwd_us']) / res['torch_gru_fwd_bwd_us']
        res['op_fwd_plus_bwd_over_torch'] = (res['op_fwd_us'] + res['op_bwd_us']) / res['torch_gru_fwd_bwd_us']
    except Exception as e:   # the library behind torch.nn.GRU would not run here: the column is left out
        res['torch_gru_error'] = '%s: %s' % (type(e).__name__, str(e)[:200])
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
    res['conv_1d_simple'] = step_time(a.steps, a.warmup)
    if not a.no_layers:
        res['gru'] = gru_times(a.steps, a.warmup)
    line = json.dumps(res)
    print(line)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, 'w') as f:
            f.write(line + '\n')


if __name__ == '__main__':
    main()
