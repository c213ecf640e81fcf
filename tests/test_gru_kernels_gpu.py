"""GPU parity of the stand-alone bidirectional GRU op (kws_gru_masks / kws_gru_fwd_f32 / kws_gru_bwd_f32, csrc/gru.hip) against the
float64 oracle tests/gru_oracle.py, forward and backward, with and without dropout masks.

Shapes: T = 1 (only h0 = 0: the recurrent term must vanish), 2 (first real recurrence), 10 (the model's); B = 1, 5, 37 (a partial
16-row tile, and two full tiles plus a partial one); (I, H) = (8, 16) smallest, (224, 128) conv_1d_simple's, (384, 192) the
follow-up model's (three column tiles per wave).

Bars.  Forward values (z, r, c, h, output) are bounded by 1 and every pre-activation is an f32 sum of at most I + H <= 576 products
of magnitude below about 0.5: worst-case linear growth is 576 * 2^-24 * 0.5 = 1.7e-5, and the state update z h + (1 - z) c does not
amplify what it carries; the bar is 2e-5 absolute (the sibling nets' predict bar).  Gradients: the siblings' 2e-4 of the tensor's
maximum.  Hard-sigmoid decisions of the backward pass are the device's own (a gate is in its linear region iff its saved value is
strictly between 0 and 1); gate values are compared only where the float64 pre-activation is farther than 1e-5 from +-2.5, and at
most 0.1 % of the elements may be left out."""
import ctypes
import functools

import numpy as np
import pytest
import torch

from gru_oracle import KEEP, KERNEL_CASES, bigru_bwd, bigru_fwd, draw_masks, kernel_inputs
from speech_recognition_amd import _lib

pytestmark = pytest.mark.gpu

CASES = KERNEL_CASES
SEED, STEP, ROW0 = 1234567, 3, 0
_inputs = kernel_inputs


def _dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def _device_run(B, T, I, H, masked, x, ws, dout):
    st = _lib.stream_ptr()
    P = _lib.ptr
    dx_, dw = _dev(x), [[_dev(t) for t in w] for w in ws]
    mx = mh = None
    if masked:
        mx = torch.empty(6 * B * I, dtype=torch.float32, device='cuda')
        mh = torch.empty(6 * B * H, dtype=torch.float32, device='cuda')
        _lib.call("kws_gru_masks", P(mx), P(mh), B, I, H, ctypes.c_float(KEEP), ctypes.c_uint64(SEED), ctypes.c_uint32(STEP), ROW0, st)
    lib = _lib.load()
    n_ws = int(lib.kws_gru_workspace_floats(B, T, I, H, 1))
    n_save = int(lib.kws_gru_save_floats(B, T, H))
    assert n_ws > 0 and n_save == 8 * B * T * H
    wsb = torch.zeros(n_ws, dtype=torch.float32, device='cuda')
    save = torch.zeros(n_save, dtype=torch.float32, device='cuda')
    out = torch.zeros(B, 2 * H, dtype=torch.float32, device='cuda')
    _lib.call("kws_gru_fwd_f32", P(dx_), P(dw[0][0]), P(dw[0][1]), P(dw[0][2]), P(dw[1][0]), P(dw[1][1]), P(dw[1][2]), P(mx), P(mh),
              P(out), P(save), P(wsb), B, T, I, H, st)
    g = [torch.zeros_like(t) for w in dw for t in w]
    gx = torch.zeros_like(dx_)
    _lib.call("kws_gru_bwd_f32", P(_dev(dout)), P(dx_), P(dw[0][0]), P(dw[0][1]), P(dw[1][0]), P(dw[1][1]), P(mx), P(mh), P(save), P(gx),
              P(g[0]), P(g[1]), P(g[2]), P(g[3]), P(g[4]), P(g[5]), P(wsb), B, T, I, H, st)
    torch.cuda.synchronize()
    res = {'out': out.cpu().numpy(), 'save': save.cpu().numpy().reshape(2, 4, B, T, H), 'dx': gx.cpu().numpy(),
           'grads': [t.cpu().numpy() for t in g]}
    if masked:
        res['mx'] = mx.cpu().numpy().reshape(2, 3, B, I)
        res['mh'] = mh.cpu().numpy().reshape(2, 3, B, H)
    # inference form of the same call: no save, one product per direction when there is no mask
    out2 = torch.zeros_like(out)
    _lib.call("kws_gru_fwd_f32", P(dx_), P(dw[0][0]), P(dw[0][1]), P(dw[0][2]), P(dw[1][0]), P(dw[1][1]), P(dw[1][2]), P(mx), P(mh),
              P(out2), None, P(wsb), B, T, I, H, st)
    torch.cuda.synchronize()
    res['out_nosave'] = out2.cpu().numpy()
    return res


@functools.lru_cache(maxsize=None)
def _case(B, T, I, H, masked):
    x, ws, dout = _inputs(B, T, I, H)
    dev = _device_run(B, T, I, H, masked, x, ws, dout)
    dev2 = _device_run(B, T, I, H, masked, x, ws, dout)
    x64 = x.astype(np.float64)
    w64 = [tuple(t.astype(np.float64) for t in w) for w in ws]
    mx = mh = None
    if masked:
        mx, mh = draw_masks(SEED, STEP, B, I, H, KEEP, ROW0, T)
    ref_out, caches = bigru_fwd(x64, w64, mx, mh)
    decisions = {}
    for d in range(2):
        decisions[(d, 'z')] = (dev['save'][d, 0] > 0) & (dev['save'][d, 0] < 1)
        decisions[(d, 'r')] = (dev['save'][d, 1] > 0) & (dev['save'][d, 1] < 1)
    ref_dx, ref_g = bigru_bwd(dout.astype(np.float64), x64, w64, caches, decisions)
    return dev, dev2, ref_out, caches, ref_dx, ref_g, (mx, mh)


@pytest.mark.parametrize("masked", [False, True])
@pytest.mark.parametrize("B,T,I,H", CASES)
def test_forward_matches_oracle(B, T, I, H, masked):
    dev, _, ref_out, caches, _, _, (mx, mh) = _case(B, T, I, H, masked)
    if masked:   # the device's masks are the oracle's, bit for bit
        for d in range(2):
            for g in range(3):
                assert np.array_equal(dev['mx'][d, g], mx[d][g][:, 0].astype(np.float32))
                assert np.array_equal(dev['mh'][d, g], mh[d][g][:, 0].astype(np.float32))
    left_out = total = 0
    worst = {}
    for d in range(2):
        c = caches[d]
        for q, (name, pre) in enumerate((('z', c['pz']), ('r', c['pr']))):
            far = np.abs(np.abs(pre) - 2.5) > 1e-5
            left_out += (~far).sum()
            total += far.size
            worst[(d, name)] = np.abs(dev['save'][d, q] - c[name])[far].max() if far.any() else 0.0
        worst[(d, 'c')] = np.abs(dev['save'][d, 2] - c['c']).max()
        worst[(d, 'h')] = np.abs(dev['save'][d, 3] - c['h']).max()
        # the final state is the last (forward) / first (backward) row of the saved sequence
        assert np.array_equal(dev['out'][:, d * H:(d + 1) * H], dev['save'][d, 3][:, 0 if d else T - 1])
    err = np.abs(dev['out'] - ref_out).max()
    print("gru fwd B=%d T=%d I=%d H=%d masked=%d: out %.3g, steps %s, left out %d / %d" %
          (B, T, I, H, masked, err, ' '.join('%s%d %.2g' % (k[1], k[0], v) for k, v in sorted(worst.items())), left_out, total))
    assert left_out <= 1e-3 * total
    assert err < 2e-5
    for k, v in worst.items():
        assert v < 2e-5, (k, v)
    assert np.abs(dev['out_nosave'] - ref_out).max() < 2e-5
    if T == 1:   # h0 = 0: z, r, c are functions of the input projection alone, whatever U holds
        assert np.abs(dev['save'][:, 3] - (1 - dev['save'][:, 0]) * dev['save'][:, 2]).max() < 1e-6


@pytest.mark.parametrize("masked", [False, True])
@pytest.mark.parametrize("B,T,I,H", CASES)
def test_backward_matches_oracle(B, T, I, H, masked):
    dev, _, _, _, ref_dx, ref_g, _ = _case(B, T, I, H, masked)
    names = ['dW0', 'dU0', 'db0', 'dW1', 'dU1', 'db1']
    refs = [t for g in ref_g for t in g]
    errs = {'dx': np.abs(dev['dx'] - ref_dx).max() / max(np.abs(ref_dx).max(), 1e-7)}
    for nm, got, ref in zip(names, dev['grads'], refs):
        if T == 1 and nm.startswith('dU'):
            assert not got.any() and not ref.any()     # h0 = 0: no gradient reaches the recurrent kernel
            continue
        errs[nm] = np.abs(got - ref).max() / max(np.abs(ref).max(), 1e-7)
    print("gru bwd B=%d T=%d I=%d H=%d masked=%d: %s" % (B, T, I, H, masked, ' '.join('%s %.2g' % kv for kv in errs.items())))
    for k, v in errs.items():
        assert v < 2e-4, (k, v)


@pytest.mark.parametrize("B,T,I,H", [CASES[2], CASES[5], CASES[8]])
def test_two_runs_are_bit_identical(B, T, I, H):
    a, b = _case(B, T, I, H, True)[:2]
    assert np.array_equal(a['out'], b['out']) and np.array_equal(a['save'], b['save']) and np.array_equal(a['dx'], b['dx'])
    for x, y in zip(a['grads'], b['grads']):
        assert np.array_equal(x, y)
