"""kws_gemm_dgrad_wgrad_f32 (csrc/gemm.hip gemm_dgrad_wgrad_kernel: a layer's input-gradient GEMM dZ = dY WT and the slabs of its
weight-gradient GEMM dW = Z^T dY in one launch), called directly through the test-only forwarder of tests/internal_shim.py.

Three kinds of check per case (M, cin, cout) of tests/gemm_exact.py PAIR_CASES, which reaches all seven instantiations
<BN, KB, BKO, BNO> the planner can launch and the corners of both walks (half tiles with and without a full round, a last tile
of fewer than 64 / of 65 .. 127 rows, idle XCDs, M = 1, M below one TN stage, S = 1, a ragged last split):

  exact     ternary inputs: dZ and the float64 sum of the S slabs are BIT-equal to float64 (every partial sum is an integer below
            2^24, so no order of summation may change it); dZ fully written; exactly the first S cin cout workspace floats
            written; guards intact; kws_reduce_slabs_batch over the same slabs gives the same matrix.  Host-side controls: the
            reference with one row of M removed, or counted twice, is not bit-equal to what the device gave.
  identity  random normal inputs: dZ, S and every slab are bit-identical to the separate launches kws_gemm_nn_f32 (no
            statistics) and kws_gemm_tn_slabs_f32, and within their max-norm bars against float64 (2e-6 for dZ, 5e-6 for dW).
  twice     every run is made twice and must give the same bits.

Shapes the pair does not take return 1 and write nothing; NULL pointers and a width that is no multiple of 4 are errors."""
import ctypes

import numpy as np
import pytest
import torch

import gemm_exact as GE
import internal_shim
from speech_recognition_amd import _lib
from test_resblock_kernels_gpu import Guarded, P, ok, twice

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def lib(tmp_path_factory):
    assert torch.cuda.is_available(), "these tests need an MI355X"
    return internal_shim.load(internal_shim.build(str(tmp_path_factory.mktemp("kwst"))))


def st():
    return _lib.stream_ptr()


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a, dtype=np.float32)).cuda()


def rel_err(a, b):
    return np.abs(a - b).max() / max(np.abs(b).max(), 1e-30)


def run_pair(lib, d_dY, d_WT, d_Z, M, cin, cout):
    """one launch into fresh guarded buffers -> (dZ, workspace, S); checks rc, full dZ, exactly S slabs, guards"""
    dZ = Guarded(M * cin)
    ws = Guarded(lib.kws_gemm_tn_workspace_floats(M, cin, cout))
    S = ctypes.c_int(-1)
    ok(lib, lib.kwst_gemm_dgrad_wgrad_f32(P(d_dY), P(d_WT), dZ.ptr(), P(d_Z), M, cin, cout, ws.ptr(), ctypes.byref(S), st()),
       "gemm_dgrad_wgrad")
    assert 0 < S.value and S.value * cin * cout <= ws.n
    dZ.check("gemm_dgrad_wgrad dZ")
    ws.check("gemm_dgrad_wgrad workspace", written=S.value * cin * cout)
    return dZ, ws, S.value


def slab_sum(lib, ws, S, n):
    out = Guarded(n)
    wsv, outv = (ctypes.c_void_p * 1)(ws.view.data_ptr()), (ctypes.c_void_p * 1)(out.view.data_ptr())
    ok(lib, lib.kwst_reduce_slabs_batch(wsv, outv, (ctypes.c_int64 * 1)(n), (ctypes.c_int * 1)(S), 1, st()), "reduce_slabs_batch")
    out.check("reduce_slabs_batch")
    return out


@pytest.mark.parametrize("M,cin,cout", [c[:3] for c in GE.PAIR_CASES])
def test_pair_is_exact_on_integer_inputs(lib, M, cin, cout):
    # the instantiation this case is in the table for: the restated planner says so, and the library's own statistics-row count
    # (which reveals BN wherever an XCD has fewer than 32 slots) agrees with the restatement
    assert GE.pair_form(M, cin, cout) == dict((c[:3], c[3]) for c in GE.PAIR_CASES)[(M, cin, cout)]
    assert lib.kws_gemm_nn_stats_rows(M, cout, cin) == GE.nn_plan(M, cout, cin)["rows"]
    dY, WT, Z = GE.pair_inputs(M, cin, cout, exact=True)
    GE.premise_tn(Z, dY)
    dZ_ref = GE.f64(dY) @ GE.f64(WT)
    dW_ref = GE.f64(Z).T @ GE.f64(dY)
    assert np.abs(dZ_ref).max() < GE.LIMIT
    d_dY, d_WT, d_Z = dev(dY), dev(WT), dev(Z)
    seen = []

    def run():
        dZ, ws, S = run_pair(lib, d_dY, d_WT, d_Z, M, cin, cout)
        seen.append(S)
        return [dZ, ws, slab_sum(lib, ws, S, cin * cout)]
    dZ_bits, ws_bits, dW_bits = twice(run)
    S = seen[0]
    assert seen[1] == S == GE.tn_plan(M, cin, cout, True)["S"]            # the restated planner labels the case rightly
    GE.assert_exact(dZ_bits.view(np.float32).reshape(M, cin), dZ_ref, "dZ")
    slabs = ws_bits.view(np.float32)[:S * cin * cout].reshape(S, cin, cout)
    folded = GE.f64(slabs).sum(axis=0)
    GE.assert_exact(folded.astype(np.float32), dW_ref, "the float64 sum of the slabs")
    assert np.array_equal(folded, dW_ref)                                 # (no rounding hidden by the conversion above)
    GE.assert_exact(dW_bits.view(np.float32).reshape(cin, cout), dW_ref, "kws_reduce_slabs_batch of the slabs")
    # controls on host data: a weight gradient that lost one row of M, or counted it twice, is not what the device gave
    r = GE.tn_controls_row(Z, dY)
    assert not GE.same_bits(folded.astype(np.float32), GE.tn_without_row(dW_ref, Z, dY, r))
    assert not GE.same_bits(folded.astype(np.float32), GE.tn_with_row_twice(dW_ref, Z, dY, r))


@pytest.mark.parametrize("M,cin,cout", [c[:3] for c in GE.PAIR_CASES])
def test_pair_is_bit_identical_to_the_separate_launches(lib, M, cin, cout):
    dY, WT, Z = GE.pair_inputs(M, cin, cout, exact=False)
    d_dY, d_WT, d_Z = dev(dY), dev(WT), dev(Z)
    seen = []

    def run():
        dZ, ws, S = run_pair(lib, d_dY, d_WT, d_Z, M, cin, cout)
        seen.append(S)
        return [dZ, ws, slab_sum(lib, ws, S, cin * cout)]
    dZ_bits, ws_bits, dW_bits = twice(run)
    S = seen[0]
    assert seen[1] == S
    # the two separate launches of the same library
    dZ2 = Guarded(M * cin)
    ok(lib, lib.kws_gemm_nn_f32(P(d_dY), P(d_WT), dZ2.ptr(), M, cout, cin, None, st()), "gemm_nn")
    dZ2.check("gemm_nn")
    ws2 = Guarded(lib.kws_gemm_tn_workspace_floats(M, cin, cout))
    S2 = ctypes.c_int(-1)
    ok(lib, lib.kwst_gemm_tn_slabs_f32(P(d_Z), P(d_dY), M, cin, cout, ws2.ptr(), ctypes.byref(S2), st()), "gemm_tn_slabs")
    assert S2.value == S
    n = S * cin * cout
    ws2.check("gemm_tn_slabs", written=n)
    assert np.array_equal(dZ_bits, dZ2.bits()), "dZ of the pair differs from kws_gemm_nn_f32"
    diff = ws_bits[:n] != ws2.bits()[:n]
    assert not diff.any(), "slabs %s of the pair differ from kws_gemm_tn_slabs_f32" % sorted(set(np.nonzero(diff)[0] // (cin * cout)))
    # the bars the separate launches are held to (tests/test_kernels_gpu.py), max-norm against float64
    assert rel_err(dZ_bits.view(np.float32).reshape(M, cin), GE.f64(dY) @ GE.f64(WT)) < 2e-6
    assert rel_err(dW_bits.view(np.float32).reshape(cin, cout), GE.f64(Z).T @ GE.f64(dY)) < 5e-6


@pytest.mark.parametrize("M,cin,cout", GE.PAIR_REFUSED)
def test_pair_refuses_shapes_it_does_not_take(lib, M, cin, cout):
    dY, WT, Z = GE.pair_inputs(M, cin, cout, exact=True)
    dZ = Guarded(M * cin)
    ws = Guarded(lib.kws_gemm_tn_workspace_floats(M, cin, cout))
    S = ctypes.c_int(-7)
    rc = lib.kwst_gemm_dgrad_wgrad_f32(P(dev(dY)), P(dev(WT)), dZ.ptr(), P(dev(Z)), M, cin, cout, ws.ptr(), ctypes.byref(S), st())
    assert rc == 1 and S.value == -7
    assert dZ.untouched() and ws.untouched()


def test_pair_rejects_bad_arguments(lib):
    M, cin, cout = 256, 128, 128
    dY, WT, Z = GE.pair_inputs(M, cin, cout, exact=True)
    d_dY, d_WT, d_Z = dev(dY), dev(WT), dev(Z)
    dZ = Guarded(M * cin)
    ws = Guarded(lib.kws_gemm_tn_workspace_floats(M, cin, cout))
    S = ctypes.c_int(-7)
    good = [P(d_dY), P(d_WT), dZ.ptr(), P(d_Z), M, cin, cout, ws.ptr(), ctypes.byref(S), st()]
    for i in (0, 1, 2, 3, 7, 8):                                           # each pointer in turn
        args = list(good)
        args[i] = None
        assert lib.kwst_gemm_dgrad_wgrad_f32(*args) < 0, i
    for bad in (dict(cin=126), dict(cout=126), dict(M=0), dict(cin=0)):    # widths that are no multiple of 4, empty shapes
        a = dict(dict(M=M, cin=cin, cout=cout), **bad)
        assert lib.kwst_gemm_dgrad_wgrad_f32(P(d_dY), P(d_WT), dZ.ptr(), P(d_Z), a["M"], a["cin"], a["cout"], ws.ptr(),
                                             ctypes.byref(S), st()) < 0, bad
    assert S.value == -7 and dZ.untouched() and ws.untouched()
