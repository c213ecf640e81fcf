"""The framed first convolution at narrow widths (csrc/frame_conv.hip: kws_frame_conv_fwd_f32, kws_frame_conv_wgrad_f32 and their
planners), called through the public C ABI, against the float64 frame-by-frame references of tests/frame_conv_cases.py.  The
method is test_conv1_kernels_gpu.py's.

Every device buffer is a window of a sentinel-guarded allocation (test_resblock_kernels_gpu.Guarded) - the INPUTS too: a read in
front of the first clip or behind the last one (or outside W or G) brings back the NaN sentinel, and the slack between L and
x_batch_stride holds 1000.0, so a read past L changes an integer.  Every launch runs twice and must give the same bits.

  exact    ternary x, W, G (every case of frame_conv_cases.CASES, N = 32 and 64): y, the fold of the statistics rows and
           dW[taps][ksize][N] equal float64 bit for bit; exactly rows * 2 * N statistics floats and exactly the promised workspace
           floats are written; host-side controls (one row dropped / counted twice) do not match.
  floats   random normal inputs (B = 1 and B = 5 at 16000 samples): y and dW within the bars of the same operation on the generic
           kernel (2e-6 and 5e-6 of the reference's maximum, test_conv1_kernels_gpu.py); the generic gathered GEMMs' errors on the
           same inputs (folded descriptor, weights folded on the host) are printed beside them.
Descriptors outside the domain return non-zero and leave the guarded outputs untouched."""
import ctypes

import numpy as np
import pytest
import torch

import frame_conv_cases as FC
import gemm_exact as GE
from speech_recognition_amd import _lib
from test_kernels_gpu import _check_stats_exact
from test_resblock_kernels_gpu import Guarded, ok, twice

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def lib():
    assert torch.cuda.is_available(), "these tests need an MI355X"
    return _lib.load()


def st():
    return _lib.stream_ptr()


def fdesc(c):
    return _lib.FrameConvDesc(**FC.desc_fields(c))


def gdesc(c):
    g = _lib.GatherDesc()
    for k, v in FC.folded_gather(c).items():
        setattr(g, k, v)
    return g


def rel_err(a, b):
    return np.abs(a - b).max() / max(np.abs(b).max(), 1e-30)


class Case(object):
    """the device side of one case: guarded x (with its slack), W and G, and the descriptor"""

    def __init__(self, name, exact):
        self.c = c = (FC.CASES if exact else FC.FLOAT_CASES)[name]
        self.r = r = FC.reference(name, exact)
        self.M, self.N = FC.rows_of(c), c["N"]
        self.d = fdesc(c)
        self.x = Guarded(c["B"] * c["x_batch_stride"], init=FC.x_with_slack(r["x"], c))
        self.W = Guarded(r["W"].size, init=r["W"].copy())        # (copies: the shared reference arrays are read-only)
        self.G = Guarded(r["G"].size, init=r["G"].copy())
        self.inputs = [self.x, self.W, self.G]
        self.before = [g.bits() for g in self.inputs]

    def inputs_intact(self):
        for g, b in zip(self.inputs, self.before):
            g.check("an input")
            assert np.array_equal(g.bits(), b), "a kernel wrote into one of its inputs"

    def forward(self, lib, stats=True):
        rows = FC.stats_rows(self.c)
        y = Guarded(self.M * self.N)
        part = Guarded((rows + 3) * 2 * self.N) if stats else None
        ok(lib, lib.kws_frame_conv_fwd_f32(self.x.ptr(), self.W.ptr(), y.ptr(), part.ptr() if stats else None, ctypes.byref(self.d),
                                           st()), "frame_conv_fwd")
        y.check("frame_conv_fwd y")
        if stats:
            part.check("frame_conv_fwd statistics", written=rows * 2 * self.N)
        return y, part

    def wgrad(self, lib):
        """-> dW, workspace; the workspace is exactly what kws_frame_conv_wgrad_workspace_floats asks for"""
        n_ws = lib.kws_frame_conv_wgrad_workspace_floats(ctypes.byref(self.d))
        assert n_ws == FC.workspace_floats(self.c)
        dW, ws = Guarded(self.r["W"].size), Guarded(n_ws)
        ok(lib, lib.kws_frame_conv_wgrad_f32(self.x.ptr(), self.G.ptr(), dW.ptr(), ws.ptr(), ctypes.byref(self.d), st()),
           "frame_conv_wgrad")
        dW.check("frame_conv_wgrad dW")
        ws.check("frame_conv_wgrad workspace")                   # every slab written, nothing behind them (the guard)
        return dW, ws

    def generic(self, lib):
        """the generic gathered GEMMs on the folded descriptor with host-folded weights -> C, dWeff"""
        c, K = self.c, FC.span_of(self.c)
        g = gdesc(c)
        Weff = Guarded(K * self.N, init=FC.fold32(self.r["W"], c))
        C, dWeff = Guarded(self.M * self.N), Guarded(K * self.N)
        ok(lib, lib.kws_gemm_gather_f32(self.x.ptr(), ctypes.byref(g), Weff.ptr(), C.ptr(), c["B"], self.N, None, st()), "gemm_gather")
        C.check("gemm_gather C")
        ws = Guarded(lib.kws_gemm_tn_workspace_floats(self.M, K, self.N))
        ok(lib, lib.kws_gemm_tn_gather_f32(self.x.ptr(), ctypes.byref(g), self.G.ptr(), dWeff.ptr(), c["B"], self.N, ws.ptr(), st()),
           "gemm_tn_gather")
        dWeff.check("gemm_tn_gather dW")
        return C, dWeff


def test_case_table_reaches_every_corner():
    reached = set()
    for name, c in FC.CASES.items():
        assert FC.in_domain(c), name
        assert c["corners"] <= FC.edges(c), (name, c["corners"] - FC.edges(c))
        reached |= c["corners"]
    assert reached == FC.CORNERS


# ---------------------------------------------------------------------------------------------------------------------------
# exact runs
# ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", FC.EXACT_CASES)
def test_frame_conv_is_exact_on_integer_inputs(lib, name):
    k = Case(name, True)
    c, r, M, N = k.c, k.r, k.M, k.N
    GE.premise_columns(r["y"])
    GE.premise_tn(r["F"], r["G"])
    rows = lib.kws_frame_conv_stats_rows(ctypes.byref(k.d))
    assert rows == FC.stats_rows(c) and 0 < rows <= FC.tiles_of(c)

    def fwd():
        return list(k.forward(lib))
    y_bits, part_bits = twice(fwd)
    y, part = k.forward(lib)
    GE.assert_exact(y.get().reshape(M, N), r["y"], "y")
    _check_stats_exact(part, rows, N, r["y"], "frame_conv_fwd")
    # ... and without statistics: the same bits
    y2, _ = k.forward(lib, stats=False)
    assert np.array_equal(y.bits(), y2.bits()) and np.array_equal(y.bits(), y_bits)
    # weight gradient
    dW_bits, _ = twice(lambda: list(k.wgrad(lib)))
    got = dW_bits.view(np.float32).reshape(c["taps"], c["ksize"], N)
    GE.assert_exact(got, r["dW"], "dW")
    # controls on host data: a gradient that lost one row of M, or counted it twice
    row = GE.tn_controls_row(r["F"], r["G"])
    flat = r["dW"].reshape(-1, N)
    for wrong in (GE.tn_without_row(flat, r["F"], r["G"], row), GE.tn_with_row_twice(flat, r["F"], r["G"], row)):
        assert not GE.same_bits(got.reshape(-1, N), wrong)
    k.inputs_intact()


# ---------------------------------------------------------------------------------------------------------------------------
# random floats
# ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", sorted(FC.FLOAT_CASES))
def test_frame_conv_on_random_floats(lib, name):
    k = Case(name, False)
    c, r, M, N = k.c, k.r, k.M, k.N

    def run():
        y, part = k.forward(lib)
        dW, ws = k.wgrad(lib)
        return [y, part, dW, ws]
    y_bits, part_bits, dW_bits, _ = twice(run)                   # y, statistics, dW and the workspace: the same bits twice
    y = y_bits.view(np.float32).reshape(M, N)
    dW = dW_bits.view(np.float32).reshape(c["taps"], c["ksize"], N)
    rows = FC.stats_rows(c)
    p = part_bits.view(np.float32)[:rows * 2 * N].reshape(rows, 2, N).astype(np.float64).sum(axis=0)
    want = GE.stats_ref(r["y"])
    # the generic kernel on the same inputs (folded descriptor, weights folded on the host in float32)
    C, dWeff = k.generic(lib)
    e_y, g_y = rel_err(y, r["y"]), rel_err(C.get().reshape(M, N), r["y"])
    e_dw = rel_err(dW, r["dW"])
    g_dw = rel_err(FC.unfold(GE.f64(dWeff.get().reshape(FC.span_of(c), N)), c), r["dW"])
    print("\nframe_conv %-12s M=%-6d    y (bar 2e-6)   dW (bar 5e-6)" % (name, M))
    print("  frame_conv.hip        %12.3e   %12.3e" % (e_y, e_dw))
    print("  generic gathered GEMM %12.3e   %12.3e" % (g_y, g_dw))
    assert e_y < 2e-6
    assert e_dw < 5e-6
    # the statistics rows: the bars of test_conv1_kernels_gpu.py (test_gemm_nn_and_stats')
    np.testing.assert_allclose(p[0], want[0], rtol=0, atol=2e-4 * np.abs(r["y"]).sum(axis=0).max())
    np.testing.assert_allclose(p[1], want[1], rtol=2e-5, atol=1e-5 * want[1].max())
    k.inputs_intact()


# ---------------------------------------------------------------------------------------------------------------------------
# refusals
# ---------------------------------------------------------------------------------------------------------------------------
def test_frame_conv_rejects_bad_arguments(lib):
    k = Case("L1600_B3_n32", True)
    rows = FC.stats_rows(k.c)
    y, part = Guarded(k.M * k.N), Guarded(rows * 2 * k.N)
    dW, ws = Guarded(k.r["W"].size), Guarded(FC.workspace_floats(k.c))
    good = ctypes.byref(k.d)
    fwd_good = [k.x.ptr(), k.W.ptr(), y.ptr(), part.ptr(), good, st()]
    wg_good = [k.x.ptr(), k.G.ptr(), dW.ptr(), ws.ptr(), good, st()]
    for i in (0, 1, 2, 4):                                       # x, W, y, the descriptor
        a = list(fwd_good)
        a[i] = None
        assert lib.kws_frame_conv_fwd_f32(*a) != 0, i
    for i in (0, 1, 2, 3, 4):                                    # x, G, dW, workspace, the descriptor
        a = list(wg_good)
        a[i] = None
        assert lib.kws_frame_conv_wgrad_f32(*a) != 0, i
    for changes, why in FC.REFUSED:
        bad = FC.refused(changes)
        assert not FC.in_domain(bad), why
        d = fdesc(bad)
        assert lib.kws_frame_conv_stats_rows(ctypes.byref(d)) == 0, why
        assert lib.kws_frame_conv_wgrad_workspace_floats(ctypes.byref(d)) == 0, why
        a = list(fwd_good)
        a[4] = ctypes.byref(d)
        assert lib.kws_frame_conv_fwd_f32(*a) != 0, why
        a = list(wg_good)
        a[4] = ctypes.byref(d)
        assert lib.kws_frame_conv_wgrad_f32(*a) != 0, why
    assert y.untouched() and part.untouched() and dW.untouched() and ws.untouched()
    k.inputs_intact()
