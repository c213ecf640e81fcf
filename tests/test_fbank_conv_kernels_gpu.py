"""The banked strided first convolution (csrc/fbank_conv.hip: kws_fbank_conv_fwd_f32, kws_fbank_conv_wgrad_f32 and the workspace
planner), called through the public C ABI, against the float64 bank-by-bank references of tests/fbank_conv_cases.py.  The method
is test_frame_conv_kernels_gpu.py's.

Every device buffer is a window of a sentinel-guarded allocation (test_resblock_kernels_gpu.Guarded) - the INPUTS too.  The
banks' kernels (and their gradients) lie GAP floats apart in one buffer: the gaps of W hold 1000.0 (a read outside a bank changes
an integer), the gaps of dW must keep the sentinel.  The slack between L and x_batch_stride holds 1000.0.  The workspace is
exactly what the planner asks for.  Every launch runs twice and must give the same bits.

  exact    integer x, W, G in [-3, 3] (every case of fbank_conv_cases.CASES): y and every bank's dW equal float64 bit for bit;
           host-side controls (one row dropped / counted twice) do not match.
  floats   random normal inputs at the model's banks: every element within the a-priori bound of a float32 sum of n products in
           any order, gamma_n * sum |a b| with gamma_n = n u / (1 - n u), u = 2^-24 (Higham, Accuracy and Stability, (3.5)):
           n = the widest K range (forward), n = M + the number of slabs (weight gradient: products, then the slab sums).
Descriptors outside the domain return non-zero and leave the guarded outputs untouched."""
import ctypes

import numpy as np
import pytest
import torch

import fbank_conv_cases as FB
from speech_recognition_amd import _lib
from test_resblock_kernels_gpu import GUARD, SENT, Guarded, ok, twice

pytestmark = pytest.mark.gpu
GAP = 33           # floats between two banks' tensors (odd: a bank's tensor need not be 16-byte aligned)
U = 2.0 ** -24


@pytest.fixture(scope="module")
def lib():
    assert torch.cuda.is_available(), "these tests need an MI355X"
    return _lib.load()


def st():
    return _lib.stream_ptr()


def fdesc(c, w_off):
    d = _lib.FbankConvDesc()
    for k, v in FB.desc_fields(c, w_off):
        if isinstance(v, list):
            for i, e in enumerate(v):
                getattr(d, k)[i] = e
        else:
            setattr(d, k, v)
    return d


def gapped_offsets(c):
    out, at = [], 0
    for k in c["ksize"]:
        out.append(at)
        at += k * c["N"] + GAP
    return out, at - GAP


class Case(object):
    """the device side of one case: guarded x (with its slack), W (banks GAP apart) and G, and the descriptor"""

    def __init__(self, name, exact):
        self.c = c = (FB.CASES if exact else FB.FLOAT_CASES)[name]
        self.r = r = FB.reference(name, exact)
        self.M, self.F, self.N = FB.rows_of(c), FB.F_of(c), c["N"]
        self.w_off, self.w_floats = gapped_offsets(c)
        self.d = fdesc(c, self.w_off)
        Wall = np.full(self.w_floats, FB.SLACK, np.float32)
        for q, o in enumerate(self.w_off):
            Wall[o:o + r["W"][q].size] = r["W"][q].reshape(-1)
        self.x = Guarded(c["B"] * c["x_batch_stride"], init=FB.x_with_slack(r["x"], c))
        self.W = Guarded(self.w_floats, init=Wall)
        self.G = Guarded(r["G"].size, init=r["G"].copy())        # (a copy: the shared reference arrays are read-only)
        self.inputs = [self.x, self.W, self.G]
        self.before = [g.bits() for g in self.inputs]

    def inputs_intact(self):
        for g, b in zip(self.inputs, self.before):
            g.check("an input")
            assert np.array_equal(g.bits(), b), "a kernel wrote into one of its inputs"

    def forward(self, lib):
        y = Guarded(self.M * self.F)
        ok(lib, lib.kws_fbank_conv_fwd_f32(self.x.ptr(), self.W.ptr(), y.ptr(), ctypes.byref(self.d), st()), "fbank_conv_fwd")
        y.check("fbank_conv_fwd y")
        return y

    def wgrad(self, lib):
        """-> dW (all banks and the gaps between them), workspace of exactly the planner's size"""
        n_ws = lib.kws_fbank_conv_wgrad_workspace_floats(ctypes.byref(self.d))
        assert n_ws == FB.workspace_floats(self.c) > 0
        dW, ws = Guarded(self.w_floats), Guarded(n_ws)
        ok(lib, lib.kws_fbank_conv_wgrad_f32(self.x.ptr(), self.G.ptr(), dW.ptr(), ws.ptr(), ctypes.byref(self.d), st()),
           "fbank_conv_wgrad")
        ws.check("fbank_conv_wgrad workspace")                   # every slab written, nothing behind them (the guard)
        bits = dW.bits()
        written = np.zeros(self.w_floats, bool)
        for q, o in enumerate(self.w_off):
            written[o:o + self.c["ksize"][q] * self.N] = True
        assert (bits[written] != SENT).all(), "fbank_conv_wgrad left elements of a bank's dW unwritten"
        assert (bits[~written] == SENT).all(), "fbank_conv_wgrad wrote between the banks"
        assert bool((dW.buf[:GUARD] == SENT).all()) and bool((dW.buf[-GUARD:] == SENT).all()), "fbank_conv_wgrad wrote around the banks"
        return dW, ws

    def banks_of(self, dW_bits):
        a = dW_bits.view(np.float32)
        return [a[o:o + k * self.N].reshape(k, self.N) for o, k in zip(self.w_off, self.c["ksize"])]


def same_bits(got, ref64):
    return got.dtype == np.float32 and got.shape == ref64.shape and np.array_equal(got.astype(np.float64), ref64)


def assert_exact(got, ref64, what):
    if not same_bits(got, ref64):
        bad = np.argwhere(got.astype(np.float64) != ref64)
        raise AssertionError("%s differs from the float64 reference in %d of %d elements; first at %s: %r, reference %r" % (
            what, len(bad), got.size, tuple(bad[0]), got[tuple(bad[0])], ref64[tuple(bad[0])]))


def test_case_table_reaches_every_corner():
    reached = set()
    for name, c in FB.CASES.items():
        assert FB.in_domain(c), name
        assert c["corners"] <= FB.edges(c), (name, c["corners"] - FB.edges(c))
        reached |= c["corners"]
    assert reached == FB.CORNERS


# ---------------------------------------------------------------------------------------------------------------------------
# exact runs
# ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", list(FB.CASES))
def test_fbank_conv_is_exact_on_integer_inputs(lib, name):
    k = Case(name, True)
    c, r, M, F, N = k.c, k.r, k.M, k.F, k.N
    FB.premise(r)
    y_bits, = twice(lambda: [k.forward(lib)])
    assert_exact(y_bits.view(np.float32).reshape(M, F), r["y"], "y")
    dW_bits, _ = twice(lambda: list(k.wgrad(lib)))
    got = k.banks_of(dW_bits)
    for q in range(c["nbanks"]):
        assert_exact(got[q], r["dW"][q], "dW of bank %d" % q)
    # controls on host data: a gradient that lost one row of M, or counted it twice
    q = c["nbanks"] - 1
    Fq, Gq = FB.windows(r["x"], c, q), np.asarray(r["G"], dtype=np.float64)[:, q * N:(q + 1) * N]
    row = int(np.nonzero(np.abs(Fq).sum(axis=1) * np.abs(Gq).sum(axis=1))[0][-1])
    for sign in (-1.0, 1.0):
        assert not same_bits(got[q], r["dW"][q] + sign * np.outer(Fq[row], Gq[row]))
    k.inputs_intact()


# ---------------------------------------------------------------------------------------------------------------------------
# random floats
# ---------------------------------------------------------------------------------------------------------------------------
def gamma(n):
    return n * U / (1.0 - n * U)


@pytest.mark.parametrize("name", sorted(FB.FLOAT_CASES))
def test_fbank_conv_on_random_floats(lib, name):
    k = Case(name, False)
    c, r, M, F = k.c, k.r, k.M, k.F
    y_bits, dW_bits, _ = twice(lambda: [k.forward(lib)] + list(k.wgrad(lib)))
    y = y_bits.view(np.float32).reshape(M, F).astype(np.float64)
    p = FB.plan(c)
    n_fwd = max(b - a for a, b in zip(p["k0"], p["k1"]))
    e_y = np.abs(y - r["y"])
    print("\nfbank_conv %-12s M=%-5d y: max err %.3e (of max |y| %.3e), worst err / bound %.3f" % (
        name, M, e_y.max(), np.abs(r["y"]).max(), (e_y / (gamma(n_fwd) * r["abs_y"] + 1e-300)).max()))
    assert (e_y <= gamma(n_fwd) * r["abs_y"]).all()
    n_wg = M + p["S"]
    for q, got in enumerate(k.banks_of(dW_bits)):
        e = np.abs(got.astype(np.float64) - r["dW"][q])
        print("  dW bank %d: max err %.3e (of max %.3e), worst err / bound %.3f" % (
            q, e.max(), np.abs(r["dW"][q]).max(), (e / (gamma(n_wg) * r["abs_dW"][q] + 1e-300)).max()))
        assert (e <= gamma(n_wg) * r["abs_dW"][q]).all()
    k.inputs_intact()


# ---------------------------------------------------------------------------------------------------------------------------
# refusals
# ---------------------------------------------------------------------------------------------------------------------------
def test_fbank_conv_rejects_bad_arguments(lib):
    k = Case("short_clip", True)
    y = Guarded(k.M * k.F)
    dW, ws = Guarded(k.w_floats), Guarded(FB.workspace_floats(k.c))
    good = ctypes.byref(k.d)
    fwd_good = [k.x.ptr(), k.W.ptr(), y.ptr(), good, st()]
    wg_good = [k.x.ptr(), k.G.ptr(), dW.ptr(), ws.ptr(), good, st()]
    for i in (0, 1, 2, 3):                                       # x, W, y, the descriptor
        a = list(fwd_good)
        a[i] = None
        assert lib.kws_fbank_conv_fwd_f32(*a) != 0, i
    for i in (0, 1, 2, 3, 4):                                    # x, G, dW, workspace, the descriptor
        a = list(wg_good)
        a[i] = None
        assert lib.kws_fbank_conv_wgrad_f32(*a) != 0, i
    for changes, why in FB.REFUSED:
        bad = FB.refused(changes)
        assert not FB.in_domain(bad), why
        d = fdesc(bad, FB.packed_offsets(bad)[:8])
        assert lib.kws_fbank_conv_wgrad_workspace_floats(ctypes.byref(d)) == 0, why
        a = list(fwd_good)
        a[3] = ctypes.byref(d)
        assert lib.kws_fbank_conv_fwd_f32(*a) != 0, why
        a = list(wg_good)
        a[4] = ctypes.byref(d)
        assert lib.kws_fbank_conv_wgrad_f32(*a) != 0, why
    assert y.untouched() and dW.untouched() and ws.untouched()
    k.inputs_intact()
