"""conv_1d_time_sliced at batch 1024 (filter_mult 1 and 2): one training step (forward + backward + RMSprop, HIP events, warm-up
excluded) and, per layer, the calls the step is made of against their floors.

  copy rate     measured in this run (a device-to-device copy of 1 GiB: bytes read + bytes written over its time); every byte
                floor below is algorithmic bytes over THIS rate
  new kernels   kws_frame_conv_fwd_f32 / _wgrad_f32 at N = 32 and 64 (4 B (B L + M N) bytes: the waveform read once, y written / G
                read once) and kws_gap_drop_fwd_f32 / _bwd_f32 at [1024, 3, 512 fm]
  blocks        per block the depthwise forward, the two passes of the fused depthwise + BatchNorm backward, and the pointwise
                forward / input-gradient / weight-gradient GEMMs (K = 32 and 64 are the project's narrowest), each against the
                larger of its byte floor and its FLOP floor at the f32 MFMA peak
  A/B           kws_frame_conv_fwd_f32 + kws_frame_conv_wgrad_f32 against what the net would otherwise run - kws_gemm_gather_f32
                and kws_gemm_tn_gather_f32 on the folded 80-sample descriptor - alternating in this process, medians after
                warm-up.  The generic side is timed WITHOUT its fold_taps / unfold_taps launches (they are not public entry
                points): the comparison favours the generic path by two small launches.
Prints one JSON object.
usage: python3 scripts/bench_time_sliced.py [--steps 20] [--warmup 5] [--reps 9] [--out profiles/time_sliced_bench_b1024.json]"""
import argparse
import ctypes
import json
import os
import statistics
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch  # noqa: E402

from speech_recognition_amd import _lib  # noqa: E402
from speech_recognition_amd.model import conv_1d_time_sliced_model  # noqa: E402

B = 1024
L = 16000
F32_MFMA_TFLOPS = 157.3    # MI355X f32 matrix peak (spec): 256 CUs x 4 SIMDs x 64 FLOP/clk at 2.4 GHz
SPEC = [(1, 64), (2, 128), (1, 128), (2, 192), (1, 192), (2, 256), (1, 256), (2, 320), (1, 320), (2, 384), (1, 384), (2, 512), (1, 512)]


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


def step_time(fm, steps, warmup):
    model = conv_1d_time_sliced_model(L, 12, filter_mult=fm)
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


def frame_desc(N):
    d = _lib.FrameConvDesc(B=B, L=L, Lout=399, ksize=40, hop=20, pad_l=10, taps=3, stride=2, N=N, x_batch_stride=L)
    g = _lib.GatherDesc()
    g.L_out, g.cin, g.taps, g.stride_t, g.stride_j, g.base_off, g.x_len, g.x_batch_stride = 399, 80, 1, 40, 0, -10, L, L
    return d, g


def frame_conv_ab(N, steps, warmup, reps, tbs):
    """the new kernels and the generic gathered GEMMs on the same buffers, alternating; medians of `reps` windows of `steps` calls"""
    lib = _lib.load()
    d, gd = frame_desc(N)
    M = B * 399
    gen = torch.Generator(device="cuda")
    gen.manual_seed(4)
    x = torch.randn((B, L), generator=gen, device="cuda") * 0.0774
    W = torch.randn((3, 40, N), generator=gen, device="cuda") * 0.1
    G = torch.randn((M, N), generator=gen, device="cuda") * 0.1
    Weff = torch.zeros((80, N), device="cuda")
    for j in range(3):
        Weff[20 * j:20 * j + 40] += W[j]
    y, y2 = torch.empty((M, N), device="cuda"), torch.empty((M, N), device="cuda")
    dW, dWeff = torch.empty((3, 40, N), device="cuda"), torch.empty((80, N), device="cuda")
    rows = lib.kws_frame_conv_stats_rows(ctypes.byref(d))
    part = torch.empty(max(rows, lib.kws_gemm_num_row_tiles(M)) * 2 * N, device="cuda")
    ws = torch.empty(int(lib.kws_frame_conv_wgrad_workspace_floats(ctypes.byref(d))), device="cuda")
    ws2 = torch.empty(int(lib.kws_gemm_tn_workspace_floats(M, 80, N)), device="cuda")
    S = _lib.stream_ptr()
    calls = {
        'frame_conv_fwd': lambda: _lib.call("kws_frame_conv_fwd_f32", _lib.ptr(x), _lib.ptr(W), _lib.ptr(y), _lib.ptr(part), ctypes.byref(d), S),
        'frame_conv_wgrad': lambda: _lib.call("kws_frame_conv_wgrad_f32", _lib.ptr(x), _lib.ptr(G), _lib.ptr(dW), _lib.ptr(ws), ctypes.byref(d), S),
        'generic_fwd': lambda: _lib.call("kws_gemm_gather_f32", _lib.ptr(x), ctypes.byref(gd), _lib.ptr(Weff), _lib.ptr(y2), B, N, _lib.ptr(part), S),
        'generic_wgrad': lambda: _lib.call("kws_gemm_tn_gather_f32", _lib.ptr(x), ctypes.byref(gd), _lib.ptr(G), _lib.ptr(dWeff), B, N, _lib.ptr(ws2), S),
    }
    for fn in calls.values():
        for _ in range(warmup):
            fn()
    samples = {k: [] for k in calls}
    for _ in range(reps):
        for k, fn in calls.items():
            samples[k].append(timed(fn, steps, 0) * 1e3)
    # the two paths computed the same thing
    torch.cuda.synchronize()
    agree_y = float((y - y2).abs().max() / y2.abs().max())
    unf = torch.stack([dWeff[20 * j:20 * j + 40] for j in range(3)])
    agree_dw = float((dW - unf).abs().max() / unf.abs().max())
    med = {k: statistics.median(v) for k, v in samples.items()}
    nbytes, flops = 4.0 * (B * L + M * N), 2.0 * M * 80 * N
    out = {'N': N, 'reps': reps, 'calls_per_rep': steps, 'median_us': med, 'min_us': {k: min(v) for k, v in samples.items()},
           'max_us': {k: max(v) for k, v in samples.items()},
           'frame_conv_fwd_plus_wgrad_us': med['frame_conv_fwd'] + med['frame_conv_wgrad'],
           'generic_fwd_plus_wgrad_us': med['generic_fwd'] + med['generic_wgrad'],
           'fwd': entry(med['frame_conv_fwd'], nbytes, flops, tbs), 'wgrad': entry(med['frame_conv_wgrad'], nbytes, flops, tbs),
           'generic_fwd': entry(med['generic_fwd'], nbytes, flops, tbs), 'generic_wgrad': entry(med['generic_wgrad'], nbytes, flops, tbs),
           'max_rel_diff_y': agree_y, 'max_rel_diff_dW': agree_dw}
    out['frame_conv_no_slower'] = out['frame_conv_fwd_plus_wgrad_us'] <= out['generic_fwd_plus_wgrad_us']
    return out


def gap_times(fm, steps, warmup, tbs):
    T, C = 3, 512 * fm
    lib = _lib.load()
    gen = torch.Generator(device="cuda")
    gen.manual_seed(5)
    y = torch.randn((B, T, C), generator=gen, device="cuda")
    bn = torch.rand(4 * C, generator=gen, device="cuda") + 0.2
    dfd = torch.randn((B, C), generator=gen, device="cuda")
    feat, fd, g = torch.empty((B, C), device="cuda"), torch.empty((B, C), device="cuda"), torch.empty((B, T, C), device="cuda")
    part = torch.empty(lib.kws_gap_drop_bwd_part_rows(B, T, C) * 2 * C, device="cuda")
    S = _lib.stream_ptr()
    fwd = lambda: _lib.call("kws_gap_drop_fwd_f32", _lib.ptr(y), _lib.ptr(bn), _lib.ptr(feat), _lib.ptr(fd), B, T, C, 0.6, 7, 1, 1, 0, S)  # noqa: E731
    bwd = lambda: _lib.call("kws_gap_drop_bwd_f32", _lib.ptr(dfd), _lib.ptr(y), _lib.ptr(bn), _lib.ptr(g), _lib.ptr(part), B, T, C, 0.6, 7, 1,  # noqa: E731
                            1, 0, S)
    return {'shape': 'B%d T%d C%d' % (B, T, C),
            'fwd': entry(timed(fwd, steps, warmup) * 1e3, 4.0 * B * C * (T + 2), 4.0 * B * T * C, tbs),
            'bwd': entry(timed(bwd, steps, warmup) * 1e3, 4.0 * B * C * (2 * T + 1), 8.0 * B * T * C, tbs)}


def block_times(fm, steps, warmup, tbs):
    lib = _lib.load()
    S = _lib.stream_ptr()
    out = []
    Lin, cin = 399, 32 * fm
    gen = torch.Generator(device="cuda")
    gen.manual_seed(6)
    for i, (s, F) in enumerate(SPEC):
        cout = F * fm
        if s == 2:
            Lout = -(-Lin // 2)
            pad_l = max((Lout - 1) * 2 + 3 - Lin, 0) // 2
        else:
            Lout, pad_l = Lin - 2, 0
        M = B * Lout
        yin = torch.randn((B, Lin, cin), generator=gen, device="cuda")
        bn = torch.rand(4 * cin, generator=gen, device="cuda") + 0.2
        w = torch.randn((3, cin), generator=gen, device="cuda") * 0.3
        z = torch.empty((M, cin), device="cuda")
        Wp = torch.randn((cin, cout), generator=gen, device="cuda") * 0.1
        WT = Wp.t().contiguous()
        yout = torch.empty((M, cout), device="cuda")
        dy = torch.randn((M, cout), generator=gen, device="cuda")
        dz = torch.randn((M, cin), generator=gen, device="cuda")
        dyin = torch.empty((B, Lin, cin), device="cuda")
        dWp = torch.empty((cin, cout), device="cuda")
        stats = torch.empty(lib.kws_gemm_num_row_tiles(M) * 2 * cout, device="cuda")
        part = torch.empty(int(lib.kws_dwconv_bwd_part_floats(B, Lin, cin)), device="cuda")
        coef = torch.rand(2 * cin, generator=gen, device="cuda") * 0.01
        tn = torch.empty(int(lib.kws_gemm_tn_workspace_floats(M, cin, cout)), device="cuda")
        calls = [
            ('dw_fwd', lambda: _lib.call("kws_dwconv_fwd_f32", _lib.ptr(yin), _lib.ptr(bn), _lib.ptr(w), _lib.ptr(z), B, Lin, Lout, cin, s, pad_l, S),
             4.0 * B * cin * (Lin + Lout), 6.0 * M * cin),
            ('dw_bwd_pass1', lambda: _lib.call("kws_dwconv_bwd_bn_f32", _lib.ptr(dz), _lib.ptr(yin), _lib.ptr(bn), _lib.ptr(w), None, None,
                                               _lib.ptr(part), 1, B, Lin, Lout, cin, s, pad_l, S),
             4.0 * B * cin * (Lin + Lout), 12.0 * B * Lin * cin),
            ('dw_bwd_pass2', lambda: _lib.call("kws_dwconv_bwd_bn_f32", _lib.ptr(dz), _lib.ptr(yin), _lib.ptr(bn), _lib.ptr(w), _lib.ptr(coef),
                                               _lib.ptr(dyin), None, 2, B, Lin, Lout, cin, s, pad_l, S),
             4.0 * B * cin * (2 * Lin + Lout), 12.0 * B * Lin * cin),
            ('pw_fwd', lambda: _lib.call("kws_gemm_nn_f32", _lib.ptr(z), _lib.ptr(Wp), _lib.ptr(yout), M, cin, cout, _lib.ptr(stats), S),
             4.0 * (M * cin + cin * cout + M * cout), 2.0 * M * cin * cout),
            ('pw_dgrad', lambda: _lib.call("kws_gemm_nn_f32", _lib.ptr(dy), _lib.ptr(WT), _lib.ptr(dz), M, cout, cin, None, S),
             4.0 * (M * cin + cin * cout + M * cout), 2.0 * M * cin * cout),
            ('pw_wgrad', lambda: _lib.call("kws_gemm_tn_f32", _lib.ptr(z), _lib.ptr(dy), _lib.ptr(dWp), M, cin, cout, _lib.ptr(tn), S),
             4.0 * (M * cin + cin * cout + M * cout), 2.0 * M * cin * cout),
        ]
        rec = {'block': i, 'shape': 'L%d->%d s%d C%d->%d' % (Lin, Lout, s, cin, cout),
               'pw_flop_per_byte': 2.0 * M * cin * cout / (4.0 * (M * cin + cin * cout + M * cout))}
        for name, fn, nbytes, flops in calls:
            rec[name] = entry(timed(fn, steps, warmup) * 1e3, nbytes, flops, tbs)
        out.append(rec)
        Lin, cin = Lout, cout
        del yin, z, yout, dy, dz, dyin, tn
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--steps', type=int, default=20)
    ap.add_argument('--warmup', type=int, default=5)
    ap.add_argument('--reps', type=int, default=9)
    ap.add_argument('--out', default=None)
    ap.add_argument('--no-layers', action='store_true')
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_time_sliced: no GPU visible - nothing is measured without one")
    torch.cuda.set_device(0)
    tbs = copy_rate(a.steps, a.warmup)
    res = {'batch': B, 'input_size': L, 'copy_tbs_measured': tbs, 'f32_mfma_tflops_peak': F32_MFMA_TFLOPS,
           'device': torch.cuda.get_device_name(0), 'steps': a.steps, 'warmup': a.warmup}
    res['step'] = {'fm%d' % fm: step_time(fm, a.steps, a.warmup) for fm in (1, 2)}
    res['frame_conv_ab'] = {'N%d' % N: frame_conv_ab(N, a.steps, a.warmup, a.reps, tbs) for N in (32, 64)}
    res['gap_drop'] = {'fm%d' % fm: gap_times(fm, a.steps, a.warmup, tbs) for fm in (1, 2)}
    if not a.no_layers:
        res['blocks'] = {'fm%d' % fm: block_times(fm, a.steps, a.warmup, tbs) for fm in (1, 2)}
    line = json.dumps(res)
    print(line)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, 'w') as f:
            f.write(line + '\n')


if __name__ == '__main__':
    main()
