"""GPU parity of the stand-alone attention-gate op (kws_attn_gate_fwd_f32 / kws_attn_gate_bwd_f32, csrc/attgate.hip) against the
float64 oracle tests/xception_oracle.py, forward and backward, with the training table (batch statistics) and the inference table
(moving statistics).

Shapes (B, T, C, k): (1, 1, 4, 5) one step - every tap but the centre is padding, att == 1 and nothing passes the softmax backward;
(3, 2, 8, 5) T smaller than the taps; (37, 7, 132, 3) odd T, C no multiple of 64, three taps, NEGATIVE gamma; (5, 50, 384, 5) the
model's tail; (2, 128, 64, 5) the domain's largest T (two time steps per lane in the softmax wave, four time-step groups).

Every output and workspace is pre-filled with NaN inside a buffer whose guard bands (256 floats each side) must come back
untouched.  The ReLU6 decisions handed to the oracle's backward pass are the device's (from its u and table, in the kernels' f32
arithmetic pre = fmaf(u, scale, shift)); elements of att whose float64 pre-activation lies within 1e-5 of 0 or 6 are left out, at
most 1e-3 of them.

Bars: the GRU kernel test's - forward values 2e-5, gradients 2e-4, each relative to the reference tensor's largest magnitude
(dgamma / dbeta: to the sum of the magnitudes of their terms, which cancel).  The gate oracle in float32 against itself in float64
on the CPU, at these shapes and seeds and on the float64 run's decisions (tests/test_xception_cpu.py prints them): worst forward
figure 5.5e-7 (y, (5, 50, 384, 5)), worst gradient 7.5e-7 (dwa, (3, 2, 8, 5)); no element within 1e-5 of a corner.  Both are under
half their bars, so the bars stand."""
import ctypes
import functools

import numpy as np
import pytest
import torch

from speech_recognition_amd import _lib
from xception_oracle import GATE_BWD_KEYS, GATE_CASES, GATE_FWD_KEYS, gate_errors, gate_inputs, gate_reference

pytestmark = pytest.mark.gpu

GUARD = 256
SENTINEL = 12345.678
NEG_GAMMA_CASE = GATE_CASES[2]
FWD_BAR, BWD_BAR = 2e-5, 2e-4


class Guarded(object):
    """A device buffer of n floats filled with `fill` between two guard bands of a sentinel."""

    def __init__(self, n, fill=float('nan')):
        self.n = int(n)
        self.buf = torch.full((self.n + 2 * GUARD,), SENTINEL, dtype=torch.float32, device='cuda')
        self.buf[GUARD:GUARD + self.n] = fill
        self.view = self.buf[GUARD:GUARD + self.n]

    def ptr(self):
        return ctypes.c_void_p(self.view.data_ptr())

    def set(self, a):
        self.view.copy_(torch.from_numpy(np.ascontiguousarray(a, dtype=np.float32).reshape(-1)))
        return self

    def numpy(self):
        return self.view.cpu().numpy()

    def intact(self):
        b = self.buf.cpu().numpy()
        return bool(np.all(b[:GUARD] == np.float32(SENTINEL)) and np.all(b[GUARD + self.n:] == np.float32(SENTINEL)))


def _dev(a):
    return torch.from_numpy(np.ascontiguousarray(a, dtype=np.float32)).cuda()


def _device_run(B, T, C, k, training, neg):
    x, dy, wa, Wa, gamma, beta, mm, mv = gate_inputs(B, T, C, k, neg)
    lib = _lib.load()
    st = _lib.stream_ptr()
    P = _lib.ptr
    n_f, n_b = int(lib.kws_attn_gate_fwd_floats(B, T, C, k)), int(lib.kws_attn_gate_bwd_floats(B, T, C, k))
    assert n_f > 0 and n_b > 0
    dxx, ddy, dwa_, dWa_ = _dev(x), _dev(dy), _dev(wa), _dev(Wa)
    dgam, dbet = _dev(np.array([gamma])), _dev(np.array([beta]))
    out = {k_: Guarded(n) for k_, n in (('u', B * T), ('table', 4), ('att', B * T), ('y', B * T * C), ('dx', B * T * C), ('dwa', k * C),
                                       ('dWa', C), ('dgamma', 1), ('dbeta', 1), ('ws_f', n_f), ('ws_b', n_b))}
    out['mm'] = Guarded(1).set(np.array([mm]))
    out['mv'] = Guarded(1).set(np.array([mv]))
    _lib.call("kws_attn_gate_fwd_f32", P(dxx), P(dwa_), P(dWa_), P(dgam), P(dbet), out['mm'].ptr(), out['mv'].ptr(), out['u'].ptr(),
              out['table'].ptr(), out['att'].ptr(), out['y'].ptr(), out['ws_f'].ptr(), B, T, C, k, int(training), st)
    _lib.call("kws_attn_gate_bwd_f32", P(ddy), P(dxx), out['u'].ptr(), out['att'].ptr(), out['table'].ptr(), P(dwa_), P(dWa_), P(dgam),
              out['dx'].ptr(), out['dwa'].ptr(), out['dWa'].ptr(), out['dgamma'].ptr(), out['dbeta'].ptr(), out['ws_b'].ptr(), B, T, C, k,
              int(training), st)
    torch.cuda.synchronize()
    res = {k_: v.numpy() for k_, v in out.items() if not k_.startswith('ws_')}
    res['guards'] = {k_: v.intact() for k_, v in out.items()}
    return res


@functools.lru_cache(maxsize=None)
def _case(B, T, C, k, training):
    neg = (B, T, C, k) == NEG_GAMMA_CASE
    dev = _device_run(B, T, C, k, training, neg)
    dev2 = _device_run(B, T, C, k, training, neg)
    # the device's ReLU6 decisions, in the kernels' arithmetic: pre = fmaf(u, scale, shift) rounded once
    pre_dev = (dev['u'].astype(np.float64) * np.float64(dev['table'][0]) + np.float64(dev['table'][1])).astype(np.float32)
    mask = ((pre_dev > 0) & (pre_dev <= 6)).astype(np.float64).reshape(B, T)
    ref = gate_reference(B, T, C, k, training, neg, mask=mask)
    near = (np.abs(ref['pre']) < 1e-5) | (np.abs(ref['pre'] - 6.0) < 1e-5)
    return dev, dev2, ref, near


@pytest.mark.parametrize("training", [True, False])
@pytest.mark.parametrize("B,T,C,k", GATE_CASES)
def test_gate_matches_oracle(B, T, C, k, training):
    dev, dev2, ref, near = _case(B, T, C, k, training)
    assert all(dev['guards'].values()), dev['guards']
    assert all(dev2['guards'].values()), dev2['guards']
    for key in GATE_FWD_KEYS + GATE_BWD_KEYS:
        assert np.all(np.isfinite(dev[key])), key          # every element was written (the buffers started as NaN)
    errs = gate_errors(dev, ref, near)
    print("gate B=%d T=%d C=%d k=%d training=%d: %s; left out %d / %d" %
          (B, T, C, k, training, ' '.join('%s %.2g' % kv for kv in errs.items()), near.sum(), near.size))
    assert near.sum() <= 1e-3 * near.size
    for key in GATE_FWD_KEYS:
        assert errs[key] < FWD_BAR, (key, errs[key])
    for key in GATE_BWD_KEYS:
        assert errs[key] < BWD_BAR, (key, errs[key])
    att = dev['att'].reshape(B, T)
    assert np.abs(att.sum(axis=1) - 1.0).max() < 1e-5
    if T == 1:   # one step: the softmax is 1 whatever the logit, and its backward passes nothing on
        x, dy = gate_inputs(B, T, C, k)[:2]
        assert np.all(att == 1.0) and np.array_equal(dev['y'], x.reshape(-1))
        assert not dev['dwa'].any() and not dev['dWa'].any() and dev['dgamma'][0] == 0 and dev['dbeta'][0] == 0
        assert np.array_equal(dev['dx'], dy.reshape(-1))
    if not training:   # the moving statistics stay what they were
        mm, mv = gate_inputs(B, T, C, k, (B, T, C, k) == NEG_GAMMA_CASE)[6:]
        assert dev['mm'][0] == mm and dev['mv'][0] == mv


@pytest.mark.parametrize("B,T,C,k", GATE_CASES)
def test_two_runs_are_bit_identical(B, T, C, k):
    a, b = _case(B, T, C, k, True)[:2]
    for key in GATE_FWD_KEYS + GATE_BWD_KEYS:
        assert np.array_equal(a[key], b[key]), key
