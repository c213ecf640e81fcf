"""The grouped depthwise Conv1D kernels (csrc/gdwconv.hip: kws_gdwconv_fwd_f32, kws_gdwconv_bwd_f32 and the planner), called
through the public C ABI, against the float64 references of tests/gdwconv_cases.py.

The inputs are integers / short dyadics on which float32 is exact in any order, so Z, dA, every group's dw and (bias mode) dbias
must equal float64 BIT FOR BIT.  Every device buffer is a window of a sentinel-guarded allocation
(test_resblock_kernels_gpu.Guarded), the inputs too.  The groups' kernels (and their gradients) lie w_group_stride floats apart in
one buffer: the gaps of w hold 1000.0 (a read outside a kernel changes an integer), the gaps of dW must keep the sentinel.  The
table's mean / rstd rows hold 1000.0 as well.  The workspace is exactly what the planner asks for.  Every launch runs twice and
must give the same bits."""
import ctypes

import numpy as np
import pytest
import torch

import gdwconv_cases as GD
from speech_recognition_amd import _lib
from test_resblock_kernels_gpu import GUARD, SENT, Guarded, ok, twice

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def lib():
    assert torch.cuda.is_available(), "these tests need an MI355X"
    return _lib.load()


def st():
    return _lib.stream_ptr()


def gdesc(c):
    d = _lib.GdwconvDesc()
    for k, v in GD.desc_fields(c):
        setattr(d, k, v)
    return d


def assert_exact(got, ref64, what):
    assert got.dtype == np.float32 and got.shape == ref64.shape, what
    if not np.array_equal(got.astype(np.float64), ref64):
        bad = np.argwhere(got.astype(np.float64) != ref64)
        raise AssertionError("%s differs from the float64 reference in %d of %d elements; first at %s: %r, reference %r" % (
            what, len(bad), got.size, tuple(bad[0]), got[tuple(bad[0])], ref64[tuple(bad[0])]))


class Case(object):
    """the device side of one case: guarded X, table / bias, kernels (w_group_stride apart) and dZ, and the descriptor"""

    def __init__(self, name):
        self.c = c = GD.CASES[name]
        self.r = r = GD.reference(name)
        self.d = gdesc(c)
        self.ws_, self.kg = GD.wstride(c), c["k"] * c["gs"]
        self.w_floats = (c["g"] - 1) * self.ws_ + self.kg
        Wall = np.full(self.w_floats, GD.SLACK, np.float32)
        for q in range(c["g"]):
            Wall[q * self.ws_:q * self.ws_ + self.kg] = r["w"][q].reshape(-1)
        self.X = Guarded(r["x"].size, init=r["x"].copy())
        self.W = Guarded(self.w_floats, init=Wall)
        self.dZ = Guarded(r["dz"].size, init=r["dz"].copy())
        self.tab = Guarded(r["tab"].size, init=r["tab"].copy()) if r["tab"] is not None else None
        self.inputs = [g for g in (self.X, self.W, self.dZ, self.tab) if g is not None]
        self.before = [g.bits() for g in self.inputs]

    def tab_ptr(self):
        return self.tab.ptr() if self.tab is not None else None

    def inputs_intact(self):
        for g, b in zip(self.inputs, self.before):
            g.check("an input")
            assert np.array_equal(g.bits(), b), "a kernel wrote into one of its inputs"

    def forward(self, lib):
        Z = Guarded(self.r["Z"].size)
        ok(lib, lib.kws_gdwconv_fwd_f32(self.X.ptr(), self.tab_ptr(), self.W.ptr(), Z.ptr(), ctypes.byref(self.d), st()), "gdwconv_fwd")
        Z.check("gdwconv_fwd Z")
        return [Z]

    def backward(self, lib):
        c = self.c
        n_ws = lib.kws_gdwconv_bwd_workspace_floats(ctypes.byref(self.d))
        assert n_ws == GD.workspace_floats(c) > 0
        assert lib.kws_gdwconv_bwd_part_rows(ctypes.byref(self.d)) == GD.part_rows(c)
        dA, dW, ws = Guarded(self.r["dA"].size), Guarded(self.w_floats), Guarded(n_ws)
        dbias = Guarded(c["C"]) if c["act"] == GD.ACT_BIAS else None
        ok(lib, lib.kws_gdwconv_bwd_f32(self.X.ptr(), self.tab_ptr(), self.dZ.ptr(), self.W.ptr(), dA.ptr(), dW.ptr(),
                                        dbias.ptr() if dbias else None, ws.ptr(), ctypes.byref(self.d), st()), "gdwconv_bwd")
        dA.check("gdwconv_bwd dA")                               # every element written, zeros included
        ws.check("gdwconv_bwd workspace")                        # every partial row written, nothing behind them
        if dbias:
            dbias.check("gdwconv_bwd dbias")
        bits = dW.bits()
        written = np.zeros(self.w_floats, bool)
        for q in range(c["g"]):
            written[q * self.ws_:q * self.ws_ + self.kg] = True
        assert (bits[written] != SENT).all(), "gdwconv_bwd left elements of a group's dw unwritten"
        assert (bits[~written] == SENT).all(), "gdwconv_bwd wrote between the groups' kernels"
        assert bool((dW.buf[:GUARD] == SENT).all()) and bool((dW.buf[-GUARD:] == SENT).all()), "gdwconv_bwd wrote around dW"
        return [dA, dW] + ([dbias] if dbias else [])

    def groups_of(self, dW_bits):
        a = dW_bits.view(np.float32)
        return [a[q * self.ws_:q * self.ws_ + self.kg].reshape(self.c["k"], self.c["gs"]) for q in range(self.c["g"])]


@pytest.mark.parametrize("name", sorted(GD.CASES))
def test_forward_equals_float64(lib, name):
    case = Case(name)
    (z,) = twice(lambda: case.forward(lib))
    assert_exact(z.view(np.float32).reshape(case.r["Z"].shape), case.r["Z"], "Z of %s" % name)
    case.inputs_intact()


@pytest.mark.parametrize("name", sorted(GD.CASES))
def test_backward_equals_float64(lib, name):
    case = Case(name)
    c, r = case.c, case.r
    out = twice(lambda: case.backward(lib))
    dA = out[0].view(np.float32).reshape(r["dA"].shape)
    assert_exact(dA, r["dA"], "dA of %s" % name)
    for q, (got, ref) in enumerate(zip(case.groups_of(out[1]), r["dw"])):
        assert_exact(got, ref, "dw of group %d of %s" % (q, name))
    if c["act"] == GD.ACT_BIAS:
        assert_exact(out[2].view(np.float32), r["dbias"], "dbias of %s" % name)
        assert np.abs(r["dbias"]).max() > 0
    case.inputs_intact()
    # what the case is there for
    read = np.zeros(c["C"], bool)
    for q in range(c["g"]):
        read[c["x0"] + q * c["x_step"]:c["x0"] + q * c["x_step"] + c["gs"]] = True
    reach = c["stride"] * (c["Lout"] - 1) + c["k"]
    assert not dA[:, reach:].any() and not dA[:, :, ~read].any()          # exact zeros, and +0.0 at that
    assert not np.signbit(dA[:, reach:]).any() and not np.signbit(dA[:, :, ~read]).any()
    assert np.abs(dA[:, :reach][:, :, read]).max() > 0
    if name == "sliced_unread":
        assert reach == 9 and c["L"] == 10 and list(np.flatnonzero(~read)) == list(range(12, 20))
    if name == "many_rows":
        assert GD.part_rows(c) >= 2 and c["B"] * c["Lout"] > 4 * 16
    if name == "model_block3":
        assert int(read.sum()) == 300 and GD.part_rows(c) >= 2


def test_shared_form_sums_the_groups_and_overlap_sums_the_windows(lib):
    """dA of the shared case is the sum of what each group alone would give; the same for the overlapping windows"""
    for name in ("shared", "overlap"):
        c, r = GD.CASES[name], GD.reference(name)
        gs, reach = c["gs"], c["stride"] * (c["Lout"] - 1) + 1
        dz = r["dz"].astype(np.float64)
        per_group = []
        for q in range(c["g"]):
            one = np.zeros(r["dA"].shape)
            lo = c["x0"] + q * c["x_step"]
            for j in range(c["k"]):
                one[:, j:j + reach:c["stride"], lo:lo + gs] += r["w"][q][j].astype(np.float64) * dz[:, :, q * gs:(q + 1) * gs]
            per_group.append(one)
        assert all(np.abs(one).max() > 0 for one in per_group)
        assert np.array_equal(sum(per_group), r["dA"]) and not np.array_equal(per_group[0], r["dA"])


def test_table_is_indexed_per_channel():
    """the straddle case really has a vector under two tables, with different entries, and elements on both kinks"""
    c, r = GD.CASES["table_straddle"], GD.reference("table_straddle")
    assert c["bn_group"] == 6 and c["gs"] == 4 and 4 // 6 != 7 // 6
    tab = r["tab"]
    assert not np.array_equal(tab[0, :2, 4:6], tab[1, :2, 0:2])
    # a kernel that took the vector's first channel's table for all four would compute something else
    sc, sh = tab[:, 0].reshape(-1).astype(np.float64), tab[:, 1].reshape(-1).astype(np.float64)
    wrong = np.clip(r["x"][:, :, 4:8].astype(np.float64) * np.r_[sc[4:6], tab[0, 0, 0:2]] + np.r_[sh[4:6], tab[0, 1, 0:2]], 0, 6)
    assert not np.array_equal(wrong, GD.activated(c, r)[:, :, 4:8])
