"""tests/bn_cols_cases.py on the build machine (no GPU): the premises under which the float64 references of the BatchNorm
backward are exact hold for the chosen inputs, both edges of the relu6 gate are met, the three wrong-on-purpose references differ
from the right one in an output the device is held to bit for bit (so that no control of tests/test_bn_cols_kernels_gpu.py is
vacuous), the index helpers describe the two layouts of kws_gbn_cols, and a fused double step cannot reach the forward bars."""
import numpy as np
import pytest

import bn_cols_cases as BC


@pytest.mark.parametrize("with_add", [False, True])
@pytest.mark.parametrize("name", list(BC.LAYOUTS))
def test_backward_premises_hold(name, with_add):
    inp = BC.bwd_inputs(name)
    ref = BC.bwd_ref(inp, with_add)
    at0, at6 = BC.premise_bwd(inp, ref)
    assert at0 >= 8 and at6 >= 8, (at0, at6)            # pre == 0 (gate closed) and pre == 6 (gate open) at several elements
    sc = inp["table"][0]
    assert abs((sc < 0).mean() - 1.0 / 3) < 0.02 and set(np.abs(sc)) == {0.5, 1.0, 2.0}
    assert set(inp["table"][3]) == {0.5, 1.0, 2.0} and np.abs(inp["table"][2]).max() == 2
    M = BC.LAYOUTS[name]["M"]
    assert ref["part"].shape[0] == -(-M // BC.CHUNK) and M % BC.CHUNK     # a short last chunk
    assert np.abs(ref["part"][-1]).sum() > 0                              # ... that counts
    assert (ref["dy_bar"] > 0).mean() > 0.9 and ref["dy_bar"].max() < 1e-4


@pytest.mark.parametrize("name", list(BC.LAYOUTS))
@pytest.mark.parametrize("mutate", BC.MUTATIONS)
def test_wrong_references_differ_in_an_exact_output(mutate, name):
    inp = BC.bwd_inputs(name)
    right, wrong = BC.bwd_ref(inp, True), BC.bwd_ref(inp, True, mutate=mutate)
    BC.premise_bwd(inp, wrong)                           # (exact as well: the device could not differ from it by rounding)
    assert BC.differs_exactly(right, wrong)
    assert not BC.differs_exactly(right, BC.bwd_ref(inp, True))


def test_layout_indices():
    for name, lay in BC.LAYOUTS.items():
        F, M = BC.width(lay), lay["M"]
        d = BC.data_idx(lay)
        assert d.shape == (M, F) and d.min() == lay["c0"] and d.max() == (M - 1) * lay["pitch"] + lay["c0"] + F - 1 < M * lay["pitch"]
        t = BC.table_idx(lay)
        assert t.shape == (4, F) and len(set(t.reshape(-1))) == 4 * F and t.min() >= 0 and t.max() < BC.table_size(lay)
        r = BC.refs_layout(lay)
        both = np.concatenate([r["first"], r["second"]])
        assert len(set(both)) == 2 * F and both.min() >= 0 and both.max() < r["size"]
        assert r["size"] > 2 * F                          # there is something beside the layer's own two tensors
        if lay["g"] > 1:
            assert r["pstride"] > 2 * lay["Ng"] and r["boff"] > lay["Ng"] and not BC.is_window(lay)
            assert np.array_equal(t[:, lay["Ng"]], 4 * lay["Ng"] + np.arange(4) * lay["Ng"])     # group 1's table: [4][Ng] behind group 0's
        elif BC.is_window(lay):
            assert np.array_equal(t[:, 0], lay["c0"] + np.arange(4) * lay["pitch"])              # [4][pitch], from the first column
    # the g = 1 dense layout is the window with pitch F and first column 0: one formula, and the same inputs as "window"
    lay = BC.LAYOUTS["plain"]
    assert np.array_equal(BC.table_idx(lay), np.arange(4)[:, None] * 20 + np.arange(20)[None, :])
    assert BC.bwd_inputs("plain")["dA"] is not None and np.array_equal(BC.bwd_inputs("plain")["y"], BC.bwd_inputs("window")["y"])
    assert BC.width(BC.LAYOUTS["grouped"]) % 16 and BC.width(BC.LAYOUTS["wide_window"]) > 256


@pytest.mark.parametrize("rows", BC.FIN_ROWS)
@pytest.mark.parametrize("name", list(BC.LAYOUTS))
def test_forward_inputs_are_exact_and_well_conditioned(name, rows):
    inp = BC.fin_inputs(name, rows)
    part = BC.f64(inp["part"])
    assert np.array_equal(part, np.rint(part)) and np.abs(part).sum(axis=0).max() < 2 ** 24      # s and ss exact, in any order
    val, bar = BC.fin_ref(inp)
    ss = part[:, 1].sum(axis=0) / inp["count"]
    assert (ss > 0).all() and np.abs(val["mean"]).max() <= 4
    # the device may fuse a step of var = ss / n - mean^2: that moves var by at most 2^-52 ss / n, absolutely.  Behind eps = 1e-3 it is
    # a relative 0.5 * that / eps of rstd, and a hundredth of it reaches the moving variance: both far below one float32 roundoff
    delta = 2.0 ** -52 * ss.max()
    assert 0.5 * delta / float(BC.BN_EPS) < 1e-3 * BC.U and 0.01 * delta < 1e-3 * BC.U * inp["mv"].min()
    for k in bar:
        assert (bar[k] <= 1e-5 * (1 + np.abs(val[k]))).all(), k
    assert (np.sign(inp["gamma"]) < 0).any() and (np.sign(inp["gamma"]) > 0).any()
