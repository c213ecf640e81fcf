"""tests/conv1_cases.py on the build machine (no GPU): the restated planners against the library's own host functions
(kwst_conv1_stats_rows, kwst_conv1_wgrad_workspace_floats), the corners the case table claims, the premises of the exact method
for every exact case, the Toeplitz-and-fold reference against the frame + Conv1D oracle, and the accept / refuse table of
kwst_conv1_supported."""
import ctypes
import os

import numpy as np
import pytest

import conv1_cases as CC
import gemm_exact as GE
import internal_shim
from speech_recognition_amd import _lib

pytestmark = pytest.mark.skipif(not os.path.exists(internal_shim.HIPCC), reason="no hipcc")


@pytest.fixture(scope="module")
def lib(tmp_path_factory):
    return internal_shim.load(internal_shim.build(str(tmp_path_factory.mktemp("kwst"))))


def _sweep():
    """M around every step of the two planners: the 64-row tiles up to and past the 768-workgroup grid, the 32-row units, and
    every growth of the chunk (at multiples of 768 x 32 rows)"""
    ms = set(range(1, 200)) | set(CC.rows_of(c) for c in CC.CASES.values())
    for centre in [64 * 767, 64 * 768, 64 * 769, 2 * 64 * 768] + [768 * 32 * k for k in range(1, 7)]:
        ms |= set(range(centre - 70, centre + 71))
    rng = np.random.RandomState(1)
    ms |= set(int(m) for m in rng.randint(1, 400000, size=300))
    return sorted(ms)


def test_planners_restated(lib):
    for M in _sweep():
        assert lib.kwst_conv1_stats_rows(M) == CC.fwd_plan(M)["rows"], M
        assert lib.kwst_conv1_wgrad_workspace_floats(M) == CC.workspace_floats(M), M
    # what the issue's table says of the model's cases, in numbers
    assert [CC.fwd_plan(399 * b)["tiles"] for b in (1, 64, 124, 200)] == [7, 399, 774, 1247]
    assert [(p["chunk"], p["S"], p["groups"]) for p in (CC.wgrad_plan(399 * b) for b in (1, 64, 124, 200))] == \
        [(32, 13, 1), (64, 399, 13), (96, 516, 17), (128, 624, 20)]
    assert 399 * 124 - 773 * 64 == 4 and 399 * 124 - 515 * 96 == 36 and 516 - 16 * 32 == 4 and 399 - 12 * 32 == 15


def test_case_table_reaches_its_corners():
    reached = set()
    for name, c in CC.CASES.items():
        e = CC.edges(c)
        assert c["corners"] <= e, (name, sorted(c["corners"] - e))
        reached |= e
    assert CC.CORNERS <= reached, sorted(CC.CORNERS - reached)
    assert set(CC.FLOAT_CASES) <= set(CC.EXACT_CASES) == set(CC.CASES)
    # the gathers no product configuration builds are labelled so (ts_build: input_size >= 1600, a multiple of 4, taps 3 x 40)
    for name, c in CC.CASES.items():
        builds = c["x_len"] >= 1600 and c["x_len"] % 4 == 0 and c["x_batch_stride"] == c["x_len"] and \
            (c["taps"], c["cin"], c["hop"], c["stride_t"]) == (3, 40, 20, 40)
        assert c["product"] == builds, name
    # the clip-end zero fill of input_size 1604: row 39 reads samples 1542 .. 1621
    c = CC.CASES["in1604"]
    assert c["stride_t"] * 39 + c["base_off"] == 1542 and 1542 + CC.KF - 1 == 1621 > c["x_len"]


@pytest.mark.parametrize("name", CC.EXACT_CASES)
def test_exact_premises_hold(name):
    r = CC.reference(name, True)
    GE.premise_columns(r["C"])
    GE.premise_tn(r["A"], r["G"])
    assert np.abs(r["C"]).max() < GE.LIMIT and np.abs(r["Weff"]).max() <= CC.CASES[name]["taps"]
    # every case's controls have a row to work on
    GE.controls_row(r["C"])
    GE.tn_controls_row(r["A"], r["G"])


def test_toeplitz_and_fold_is_frame_plus_conv1d():
    """for the model's gather the definition-level reference equals the existing oracle (frame_same + conv1d_fwd) exactly, in
    the forward result and in the weight gradient"""
    x, W, G = GE.gather_inputs(3)
    c = dict(CC.CASES["B1"], B=3)
    assert CC.unfolded_desc(c) == GE.GATHER_DESC
    A = CC.toeplitz(x, CC.folded_desc(c))
    y_ref, cols = GE.gather_ref(x, W)
    assert np.array_equal(A @ CC.fold(W, 20), y_ref)
    dW = CC.unfold(A.T @ GE.f64(G), 3, 40, 20)
    assert np.array_equal(dW.reshape(120, CC.NOUT), cols.T @ GE.f64(G))
    # and on floats, where the two orders of summation differ only by rounding
    rng = np.random.RandomState(2)
    xf, Wf = rng.randn(3, 16000), rng.randn(3, 40, CC.NOUT)
    yf, colsf = GE.gather_ref(xf, Wf)
    Af = CC.toeplitz(xf, CC.folded_desc(c))
    np.testing.assert_allclose(Af @ CC.fold(Wf, 20), yf, rtol=0, atol=1e-12 * np.abs(yf).max())
    # the unfolded operand itself: column (j, c) of cols is column 20 j + c of A
    for j in range(3):
        assert np.array_equal(colsf[:, 40 * j:40 * j + 40], Af[:, 20 * j:20 * j + 40])


def test_references_on_a_hand_made_clip():
    """toeplitz / fold / unfold against values written out by hand"""
    g = dict(L_out=2, stride_t=4, base_off=-2, x_len=81)
    x = np.arange(1, 82, dtype=np.float64)[None]              # sample i holds i + 1
    A = CC.toeplitz(x, g)
    assert A.shape == (2, 80)
    assert list(A[0, :4]) == [0, 0, 1, 2] and A[0, 79] == 78                     # row 0 starts two samples in front of the clip
    assert list(A[1, :2]) == [3, 4] and list(A[1, 77:]) == [80, 81, 0]           # row 1 ends one sample past it
    W = np.zeros((3, 40, 1))
    W[0, 39], W[1, 19], W[1, 0], W[2, 0] = 1, 2, 4, 8
    Weff = CC.fold(W, 20)
    assert Weff.shape == (80, 1) and Weff[39, 0] == 3 and Weff[20, 0] == 4 and Weff[40, 0] == 8 and Weff.sum() == 15
    d = np.arange(80, dtype=np.float64)[:, None]
    u = CC.unfold(d, 3, 40, 20)
    assert u.shape == (3, 40, 1) and u[0, 39, 0] == 39 and u[1, 19, 0] == 39 and u[2, 0, 0] == 40 and u[2, 39, 0] == 79


def _desc(d):
    g = _lib.GatherDesc()
    for k, v in d.items():
        setattr(g, k, v)
    return g


def test_conv1_supported_accepts_and_refuses(lib):
    seen = set()
    for row in CC.SUPPORTED_TABLE:
        f, u, N, want = CC.supported_args(row)
        got = lib.kwst_conv1_supported(ctypes.byref(_desc(f)), ctypes.byref(_desc(u)), N)
        assert bool(got) == want, row
        seen.add(want)
    assert seen == {True, False}
    good = _desc(CC.folded_desc(CC.CASES["B1"])), _desc(CC.unfolded_desc(CC.CASES["B1"]))
    assert not lib.kwst_conv1_supported(None, ctypes.byref(good[1]), 128)
    assert not lib.kwst_conv1_supported(ctypes.byref(good[0]), None, 128)
    # every case of the table is a pair the predicate takes
    for name, c in CC.CASES.items():
        assert lib.kwst_conv1_supported(ctypes.byref(_desc(CC.folded_desc(c))), ctypes.byref(_desc(CC.unfolded_desc(c))), 128), name
        assert c["hop"] * (c["taps"] - 1) + c["cin"] == CC.KF
