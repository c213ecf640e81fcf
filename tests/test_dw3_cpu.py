"""tests/dw3_cases.py on the build machine (no GPU): the restated launch geometry reaches every labelled corner, the premise of
the exact inputs holds at every shape, the ReLU6 corners pre == 0 and pre == 6 carry the share of the elements the draws give
them, and every wrong-on-purpose reference (the exclusive ReLU6 mask, a unit row lost, a unit row counted twice) differs from
the right one - so that no negative control of tests/test_dw3_kernels_gpu.py is vacuous."""
import numpy as np
import pytest

import dw3_cases as DC
from oracle import layers as OL


def test_geometry_restatement_reaches_every_labelled_corner():
    seen = set()
    for c in DC.CASES:
        got = DC.corners_of(c)
        assert c[7] <= got, (DC.case_id(c), c[7] - got)
        seen |= got
    assert DC.CORNERS <= seen, DC.CORNERS - seen
    assert all(c[7] <= DC.CORNERS for c in DC.CASES)
    # the figures the case table names
    g = DC.bwd_geom
    assert (g(2, 1, 4)["R"], g(2, 1, 4)["block"]) == (512, 512)
    assert (g(3, 8, 320)["R"], g(3, 8, 320)["block"]) == (6, 480)
    assert g(3, 17, 1000)["block"] == 500 and 500 % 64 != 0
    assert (g(2, 11, 1536)["ny"], g(2, 11, 1536)["Cb"]) == (2, 768)
    assert (g(2, 10, 2048)["ny"], g(2, 10, 2048)["Cb"]) == (2, 1024)
    big = g(820, 33, 512)
    assert (big["R"], 820 * big["nchunks"], big["groups"], big["grid"]) == (4, 4100, 1025, 256)
    assert DC.cdiv(big["groups"], big["grid"]) == 5                              # the row-writing modes take five strides
    assert g(820, 33, 512, parts=False)["grid"] == 1024 and big["groups"] - 1024 == 1   # pass 2: a second stride in workgroup 0 only
    for c in DC.CASES[-2:]:
        assert DC.fwd_threads(c[0], c[5], c[2]) == (1064960, 4096) and 4096 * 256 == 1048576
    # the cases the older direct test calls its striding ones: only the row-writing modes stride there
    assert DC.fwd_threads(300, 38, 512)[0] <= 750 * 256 and g(300, 40, 512, parts=False)["groups"] == 375
    assert g(300, 40, 512)["groups"] > DC.BWD_PARTS


def test_part_floats_restated():
    for c in DC.CASES:
        B, Lin, C = c[:3]
        n = DC.part_floats(B, Lin, C)
        assert DC.bwd_geom_ok(C) and n > 0 and n % (5 * C) == 0 and n // (5 * C) <= DC.BWD_PARTS, DC.case_id(c)
    assert not DC.bwd_geom_ok(1028) and not DC.bwd_geom_ok(6)


def test_pad_and_uncovered_rows():
    for c in DC.CASES:
        DC.pad_of(c)                                                             # (asserts that the windows give L_out)
    c = [c for c in DC.CASES if "uncovered_rows" in c[7]][0]
    ref = DC.bwd_ref(c, True)
    inp = DC.inputs(c)
    assert c[1] == 12 and not ref["g"][:, 11].any()                              # row 11 is under no window: g is exactly 0 ...
    co, bn = DC.f64(inp["coef"]), DC.f64(inp["bn"])
    assert np.array_equal(ref["dy"][:, 11], bn[0] * (-co[0] - ref["xhat"][:, 11] * co[1]))   # ... and dy what is left
    assert ref["dy"][:, 11].any()


@pytest.mark.parametrize("c", DC.BWD_CASES, ids=DC.case_id)
def test_premise_shares_and_controls(c):
    C = c[2]
    for with_bn in (True, False):
        ref = DC.bwd_ref(c, with_bn)
        assert DC.premise(ref) < 4e5                                             # (measured: 3.7e5 at the 27060 rows of B = 820)
        lost, twice = DC.control_sums(c, with_bn)
        assert not np.array_equal(lost, ref["sums"]) and not np.array_equal(twice, ref["sums"])
        # the rows' own contributions do add up to the sums (so the controls remove / add what a kernel would)
        if c[0] * c[1] <= 64:
            total = sum(DC.row_terms(c, with_bn, b, u) for b in range(c[0]) for u in range(c[1]))
            assert np.array_equal(total, ref["sums"])
        z, pre = DC.fwd_ref(c, with_bn)
        assert np.array_equal(z, DC.fwd_ref_int(c, with_bn)) and np.array_equal(DC.f64(z.astype(np.float32)), z)
        if not with_bn:
            assert not ref["sums"][1].any()                                      # no table: xhat = 0
            continue
        # the finalise kernel's coefficients are float32 values of their own (nothing to assert but the restated arithmetic)
        co = DC.coef_of(ref["sums"], ref["count"])
        assert co.dtype == np.float32 and co.shape == (2, C)
        if C >= 64:
            on0, on6 = DC.edge_shares(pre)
            assert abs(on0 - 5 / 54.0) < 0.02 and abs(on6 - 7 / 162.0) < 0.012, (on0, on6)   # 9.3 % and 4.3 % by the draws
            wrong = DC.bwd_ref(c, True, "exclusive")
            assert int((wrong["g"] != ref["g"]).sum()) >= 33
            assert not np.array_equal(wrong["sums"][0], ref["sums"][0])


def test_forward_only_cases_are_integer_references():
    c = DC.CASES[-1]
    assert c[6] and DC.inputs(c)["y"].nbytes <= 52 * 2 ** 20
    z = DC.fwd_ref_int(c, True)
    assert z.shape == (c[0], c[5], c[2]) and np.abs(z).max() <= 3 * 2 * 6 and z.any()


def test_fold_plans_restated():
    assert sorted(set(n for n, _ in DC.FOLD_CASES)) == [1, 255, 256, 257, 1000, 1024, 3001]
    assert sorted(set(C for _, C in DC.FOLD_CASES)) == [4, 20, 64] and 20 % 16 != 0
    pl = DC.pre_reduce_plan
    assert all(pl(n, True) is None for n in (1, 255, 256)) and all(pl(n, False) is None for n in DC.FOLD_N)
    assert pl(257, True) == (9, 29) and pl(1000, True) == (32, 32) and pl(1024, True) == (32, 32) and pl(3001, True) == (94, 32)
    assert all(pl(n, True)[1] <= DC.REDUCE_SLICES for n in range(257, 5000))      # the scratch bound callers allocate by
    assert DC.scratch_floats(257, 5 * 20, True) == 29 * 100 and DC.scratch_floats(256, 5 * 20, True) == 0
    for n, C in DC.FOLD_CASES:
        DC.premise_fold(DC.dw_fold_inputs(n, C)[0])
        st = DC.stats_fold_inputs(n, C)
        DC.premise_fold(st["part"])
        s = DC.f64(st["part"]).sum(0) / st["count"]
        assert np.abs(s[0]).max() <= 2 and (s[1] - s[0] ** 2).min() >= 6
    for C, rows in DC.BATCH_LAYERS:
        assert rows <= DC.PRE_REDUCE_MIN                                          # what kws_dw_grad_finalize_batch takes


def test_infer_bars():
    for C in DC.INFER_C:
        inp = DC.infer_inputs(C)
        assert inp["mv"].min() >= 0.5 and inp["mv"].max() <= 2.0
        table, bars = DC.infer_ref(inp)
        # the table is the oracle's inference BatchNorm: applied to y = 1 it gives scale + shift
        one = OL.bn_infer_fwd(np.ones((1, 1, C)), DC.f64(inp["gamma"]), DC.f64(inp["beta"]), DC.f64(inp["mm"]), DC.f64(inp["mv"]),
                              eps=float(np.float32(DC.BN_EPS)))[0, 0]
        assert np.allclose(one, table[0] + table[1], rtol=1e-13, atol=1e-13)
        assert (bars[0] > 0).all() and (bars[3] > 0).all() and not bars[2].any() and bars.max() < 1e-5
