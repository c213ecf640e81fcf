"""conv_1d_top_down at batch 1024: one training step (forward + backward + RMSprop, HIP events, warm-up excluded) and, per block,
the calls the step is made of against their floors.

  copy rate   measured in this run (a device-to-device copy of 1 GiB: bytes read + bytes written over its time); every byte floor
              below is algorithmic bytes over THIS rate
  depthwise   kws_gdwconv_fwd_f32 and kws_gdwconv_bwd_f32 (csrc/gdwconv.hip) against their byte counts.  forward: the channels
              the groups read of X once (the shared form of a context block counts X ONCE, though g groups filter it) + Z written.
              backward: dZ and the read channels of X once, dA [B, L, C] written - the floor of a pass that saw each tensor once;
              the kernels read dZ twice (input gradient, weight gradient) and the shared form reads X once per group in the
              weight-gradient pass, which the ratio shows.
  pointwise   the k = 1 kws_gconv_fwd_f32 / kws_gconv_wgrad_f32 / kws_gconv_dgrad_f32 calls against the larger of their FLOP floor
              at the f32 matrix peak and their byte floor
Prints one JSON object.
usage: python3 scripts/bench_top_down.py [--steps 20] [--warmup 5] [--out profiles/top_down_bench_b1024.json]"""
import argparse
import ctypes
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch  # noqa: E402

from speech_recognition_amd import _lib  # noqa: E402
from speech_recognition_amd.model import conv_1d_top_down_model  # noqa: E402

B = 1024
L = 16000
ROWS = 98
C0 = 480
F32_MFMA_TFLOPS = 157.3    # MI355X f32 matrix peak (spec): 256 CUs x 4 SIMDs x 64 FLOP/clk at 2.4 GHz (bench.py's figure)
# (filters, groups, num_channels, stride, shared) per block
BLOCKS = [(420, 3, 480, 2, False), (420, 2, 420, 1, True), (360, 3, 300, 2, False), (360, 2, 360, 1, True),
          (300, 3, 360, 2, False), (300, 2, 300, 1, True), (240, 3, 300, 2, False), (240, 2, 240, 1, True)]


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


def copy_rate(steps, warmup):
    n = 1 << 28
    src, dst = torch.empty(n, device="cuda"), torch.empty(n, device="cuda")
    src.normal_()
    ms = timed(lambda: dst.copy_(src), steps, warmup)
    return 8.0 * n / (ms * 1e-3) / 1e12


def entry(us, nbytes, flops, tbs):
    byte_us = nbytes / (tbs * 1e12) * 1e6
    flop_us = flops / (F32_MFMA_TFLOPS * 1e12) * 1e6
    return {'us': us, 'mbytes': nbytes / 1e6, 'mflop': flops / 1e6, 'tbs': nbytes / (us * 1e-6) / 1e12, 'byte_floor_us': byte_us,
            'flop_floor_us': flop_us, 'bound': 'bytes' if byte_us >= flop_us else 'flops', 'floor_ratio': max(byte_us, flop_us) / us}


def step_time(steps, warmup):
    model = conv_1d_top_down_model(L, 12)
    g = torch.Generator(device="cuda")
    g.manual_seed(1)
    x = torch.randn((B, L), generator=g, device="cuda") * 0.0774
    y = torch.eye(12, device="cuda")[torch.randint(0, 12, (B,), generator=g, device="cuda")].contiguous()
    row = torch.zeros(4, device="cuda")
    ms = timed(lambda: model._train_step_async(x, y, row), steps, warmup)
    out = {'ms_per_step': ms, 'clips_per_s': B / ms * 1e3, 'loss_last': float(row[0].item()) / B}
    del model
    torch.cuda.empty_cache()
    return out


def block_times(steps, warmup, tbs):
    lib = _lib.load()
    S = _lib.stream_ptr()
    gen = torch.Generator(device="cuda")
    gen.manual_seed(6)
    out = []
    Lin, C, prev_ng = ROWS, C0, 0
    for i, (F, g, nch, s, shared) in enumerate(BLOCKS):
        Lout = (Lin - 3) // s + 1
        M = B * Lout
        gs, Ng = (C if shared else nch // g), F // g
        Fz = g * gs
        read = C if shared else g * gs                      # channels of X some group reads
        xin = torch.randn((B, Lin, C), generator=gen, device="cuda")
        tab = torch.rand(4 * C, generator=gen, device="cuda") + 0.2      # block 0: its first C floats are the bias
        w = torch.randn(g * 3 * gs, generator=gen, device="cuda") * 0.1
        dw = torch.empty_like(w)
        z, dz = torch.empty((M, Fz), device="cuda"), torch.randn((M, Fz), generator=gen, device="cuda")
        dA = torch.empty((B, Lin, C), device="cuda")
        dd = _lib.GdwconvDesc(B=B, L=Lin, C=C, Lout=Lout, k=3, stride=s, g=g, gs=gs, x0=0, x_step=0 if shared else gs,
                              act=_lib.GDW_ACT_BN_RELU6 if i else _lib.GDW_ACT_BIAS, bn_group=prev_ng, w_group_stride=0)
        dws = torch.empty(int(lib.kws_gdwconv_bwd_workspace_floats(ctypes.byref(dd))), device="cuda")
        W = torch.randn(g * gs * Ng, generator=gen, device="cuda") * 0.1
        dW = torch.empty_like(W)
        yout, dy = torch.empty((M, F), device="cuda"), torch.randn((M, F), generator=gen, device="cuda")
        pd = _lib.GconvDesc(B=B, L=Lout, C=Fz, Lout=Lout, k=1, stride=1, g=g, gs=gs, Ng=Ng, w_group_stride=0)
        stats = torch.empty(lib.kws_gconv_stats_rows(ctypes.byref(pd)) * 2 * F, device="cuda")
        pws = torch.empty(int(lib.kws_gconv_wgrad_workspace_floats(ctypes.byref(pd))), device="cuda")

        def dw_fwd():
            _lib.call("kws_gdwconv_fwd_f32", _lib.ptr(xin), _lib.ptr(tab), _lib.ptr(w), _lib.ptr(z), ctypes.byref(dd), S)

        def dw_bwd():
            _lib.call("kws_gdwconv_bwd_f32", _lib.ptr(xin), _lib.ptr(tab), _lib.ptr(dz), _lib.ptr(w), _lib.ptr(dA), _lib.ptr(dw),
                      None, _lib.ptr(dws), ctypes.byref(dd), S)   # no dbias, as in the program: the front bias's gradient is 0

        def pw_fwd():
            _lib.call("kws_gconv_fwd_f32", _lib.ptr(z), None, 0, _lib.ptr(W), _lib.ptr(yout), _lib.ptr(stats), ctypes.byref(pd), S)

        def pw_wgrad():
            _lib.call("kws_gconv_wgrad_f32", _lib.ptr(z), None, 0, _lib.ptr(dy), _lib.ptr(dW), _lib.ptr(pws), ctypes.byref(pd), S)

        def pw_dgrad():
            _lib.call("kws_gconv_dgrad_f32", _lib.ptr(dy), _lib.ptr(W), _lib.ptr(dz), ctypes.byref(pd), S)

        rec = {'block': i, 'shape': 'L%d->%d s%d C%d (%d read) -> %d x %d -> %d' % (Lin, Lout, s, C, read, g, gs, F),
               'form': 'shared' if shared else 'sliced', 'part_rows': int(lib.kws_gdwconv_bwd_part_rows(ctypes.byref(dd)))}
        rec['dw_fwd'] = entry(timed(dw_fwd, steps, warmup) * 1e3, 4.0 * (B * Lin * read + M * Fz), 2.0 * M * Fz * 3, tbs)
        rec['dw_bwd'] = entry(timed(dw_bwd, steps, warmup) * 1e3, 4.0 * (M * Fz + B * Lin * read + B * Lin * C), 4.0 * M * Fz * 3, tbs)
        pflops = 2.0 * M * gs * Ng * g
        pio = 4.0 * (M * Fz + M * F + W.numel())
        rec['pw_fwd'] = entry(timed(pw_fwd, steps, warmup) * 1e3, pio, pflops, tbs)
        rec['pw_wgrad'] = entry(timed(pw_wgrad, steps, warmup) * 1e3, pio, pflops, tbs)
        rec['pw_dgrad'] = entry(timed(pw_dgrad, steps, warmup) * 1e3, pio, pflops, tbs)
        out.append(rec)
        Lin, C, prev_ng = Lout, F, Ng
        del xin, z, dz, dA, dws, yout, dy, pws
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--steps', type=int, default=20)
    ap.add_argument('--warmup', type=int, default=5)
    ap.add_argument('--out', default=None)
    ap.add_argument('--no-layers', action='store_true')
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_top_down: no GPU visible - nothing is measured without one")
    torch.cuda.set_device(0)
    tbs = copy_rate(a.steps, a.warmup)
    res = {'batch': B, 'input_size': L, 'copy_tbs_measured': tbs, 'f32_mfma_tflops_peak': F32_MFMA_TFLOPS,
           'device': torch.cuda.get_device_name(0), 'steps': a.steps, 'warmup': a.warmup}
    res['step'] = step_time(a.steps, a.warmup)
    if not a.no_layers:
        res['blocks'] = block_times(a.steps, a.warmup, tbs)
        for k in ('dw_fwd', 'dw_bwd', 'pw_fwd', 'pw_wgrad', 'pw_dgrad'):
            res['sum_us_' + k] = sum(r[k]['us'] for r in res['blocks'])
    line = json.dumps(res)
    print(line)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, 'w') as f:
            f.write(line + '\n')


if __name__ == '__main__':
    main()
