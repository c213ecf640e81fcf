"""tests/tail_cases.py on the build machine (no GPU): the restated slice planner reaches every labelled corner, the premises of
the exact and the grid inputs hold, the wrong-on-purpose references differ from the right one by more than the bars (so that no
negative control of tests/test_tail_kernels_gpu.py is vacuous), and the planner-facing fact ts_tail_kernel relies on without
checking it: dense_2/kernel (W2, read as float4 rows when NC <= 16 and NC % 4 == 0) starts on a multiple of 4 floats in the flat
parameter buffer of every headline configuration."""
import ctypes
import os

import numpy as np
import pytest

import tail_cases as TC
from oracle import layers as OL
from speech_recognition_amd import _lib


def test_planner_restatement_reaches_every_labelled_corner():
    seen = set()
    for B, K, N, scratch, bias, corners in TC.WGRAD_CASES:
        got = TC.wgrad_corners(B, K, N, scratch, bias)
        assert corners <= got, (B, K, N, corners - got)
        seen |= got
    for B, N, form in TC.COLSUM_CASES:
        assert TC.small_wgrad_plan(B, TC.COLSUM_K, N, True)["colsum"] == form
    assert TC.WGRAD_CORNERS <= seen, TC.WGRAD_CORNERS - seen
    # the figures the issue's table names
    pl = TC.small_wgrad_plan
    assert pl(1, 260, 12, True)["S"] == 1
    assert (pl(31, 260, 12, True)["rows_per"], pl(31, 260, 12, True)["S"]) == (1, 31)
    assert (pl(33, 260, 12, True)["rows_per"], pl(33, 260, 12, True)["S"]) == (2, 17)
    assert pl(100, 1024, 12, True)["rows_per"] == 4
    assert (pl(1000, 516, 9, True)["rows_per"], pl(1000, 516, 9, True)["S"]) == (32, 32) and 1000 - 31 * 32 == 8
    assert pl(2048, 64, 16, True)["rows_per"] == 64 and pl(2048, 64, 16, True)["kernel"] == "rows"
    assert pl(2049, 64, 12, True)["rows_per"] == 65 and pl(2049, 64, 12, True)["kernel"] == "generic"
    assert pl(70, 37, 11, True)["slab"] == "slab_sum" and pl(70, 37, 11, True)["kernel"] == "rows"
    assert pl(70, 37, 17, True)["slab"] == "slab_sum" and pl(70, 37, 17, True)["kernel"] == "generic"
    assert pl(40, 260, 12, False) == dict(S=1, rows_per=40, kernel="rows", slab="none", colsum=(16, 256))
    assert pl(70, 260, 12, False)["kernel"] == "generic"
    # the scratch bound every planner allocates by: S never exceeds KWS_SMALL_WGRAD_SLICES
    assert all(pl(B, 4, 4, True)["S"] <= TC.SLICES for B in range(1, 4100))


def test_tail_post_eligibility_restated():
    h = TC.TAIL_POST_HEADLINE
    for B in TC.TAIL_POST_B:
        assert TC.tail_post_eligible(B, h["K1"], h["N1"], h["K2"], h["N2"])
    for B, K1, N1, K2, N2, why in TC.TAIL_POST_REFUSED:
        assert not TC.tail_post_eligible(B, K1, N1, K2, N2), why
    assert TC.tail_post_eligible(2048, 36, 9, 64, 12)                      # the last batch size it takes


def test_exact_premises_hold():
    for B, K, N, _, _, _ in TC.WGRAD_CASES:
        TC.premise_wgrad(*TC.wgrad_inputs(B, K, N))
    for B, N, _ in TC.COLSUM_CASES:
        TC.premise_wgrad(*TC.wgrad_inputs(B, TC.COLSUM_K, N))
    for B in TC.METRICS_B:
        pl, pc = TC.metrics_inputs(B)
        assert float(np.float32(TC.f64(pl).sum())) == TC.f64(pl).sum()


@pytest.fixture(scope="module")
def ts_refs():
    out = {}
    for c in TC.TS_CASES:
        inp = TC.ts_inputs(c[0])
        out[c[0]] = (inp, TC.ts_tail_ref(inp, 0))
    return out


def test_ts_grid_premises_hold(ts_refs):
    zero_ties = pair_ties = 0
    for name, (inp, ref) in ts_refs.items():
        z, p = TC.premise_ts(inp, ref)                                     # (asserts the pool-winner premise)
        zero_ties += z
        pair_ties += p
        on0, on6 = TC.edge_shares(ref["pre"])
        assert on0 > 0.002 and on6 > 0.002, (name, on0, on6)
        T, C = inp["y"].shape[1:]
        if T >= 2 and C >= 320 and name != "saturated":                     # (saturated: every gradient is 0)
            assert z > 0 and p > 0, name                                   # structural ties with a non-zero gradient occur
        if name == "saturated":
            TC.premise_saturated(ref)
            assert not ref["dl2"].any()
    assert zero_ties > 0 and pair_ties > 0
    B, T, C = ts_refs["big_lds"][0]["y"].shape
    assert 64 * 1024 < TC.ts_lds_bytes(T, C) <= 160 * 1024
    assert all(TC.ts_lds_bytes(c[2], c[3]) <= 64 * 1024 for c in TC.TS_CASES if c[0] != "big_lds")


def test_flat_premises_hold():
    for c in TC.FLAT_CASES:
        inp = TC.flat_inputs(c[0])
        ref = TC.flat_tail_ref(c[0], inp)
        TC.premise_flat(ref)
        if not c[7] and c[2] >= 128:
            on0, on6 = TC.edge_shares(ref["pre"])
            assert on0 > 0.002 and on6 > 0.002, (c[0], on0, on6)


def test_losses_agree_with_the_oracle_inside_the_clip_edges():
    """tail_cases restates the two losses only to give the clip its float32 edges: where no probability is outside them the
    restatements are oracle.layers' functions, value for value."""
    rng = np.random.RandomState(5)
    p = OL.softmax(rng.randn(7, 12))
    y = np.eye(12)[rng.randint(0, 12, 7)]
    _, per, dp = OL.smooth_cce_fwd_bwd(p, y, 0.1)
    per2, dp2 = TC.smooth_cce(p, y, 0.1, 7)
    assert np.allclose(per, per2, rtol=1e-14, atol=0) and np.allclose(dp, dp2, rtol=1e-14, atol=0)
    _, per, dp = OL.cce_fwd_bwd(p, y)
    per2, dp2 = TC.keras_cce(p, y, 7)
    assert np.allclose(per, per2, rtol=1e-14, atol=0) and np.allclose(dp, dp2, rtol=1e-12, atol=1e-18)


# which output each wrong reference is compared on, and on which case (tests/test_tail_kernels_gpu.py uses the same table)
def test_wrong_references_miss_by_more_than_the_bars(ts_refs):
    for mutate, name, key in TC.TS_CONTROLS:
        inp, ref = ts_refs[name]
        ro = 3 if mutate == "row_offset_ignored" else 0
        right = TC.ts_tail_ref(inp, ro) if ro else ref
        wrong = TC.ts_tail_ref(inp, ro, mutate=mutate)
        scale = max(np.abs(right[key]).max(), np.abs(wrong[key]).max())
        assert np.abs(wrong[key] - right[key]).max() > 100 * TC.CEILING * scale, (mutate, name, key)
    for mutate, name, key in TC.FLAT_CONTROLS:
        inp = TC.flat_inputs(name)
        right, wrong = TC.flat_tail_ref(name, inp), TC.flat_tail_ref(name, inp, mutate=mutate)
        assert np.abs(wrong[key] - right[key]).max() > 100 * TC.CEILING * np.abs(right[key]).max(), (mutate, name, key)


def test_bars_are_set_and_below_the_whole_net_bar():
    for bars in (TC.TS_BARS, TC.FLAT_BARS):
        for k, v in bars.items():
            assert v is not None and 0 < v <= TC.CEILING, k


@pytest.mark.skipif(not os.path.exists(_lib.LIB_PATH), reason="libkws_hip.so not built")
@pytest.mark.parametrize("nc", [12, 32])
@pytest.mark.parametrize("mult", [1, 2])
@pytest.mark.parametrize("input_size", [12000, 16000, 20000])
def test_headline_planner_aligns_the_dense_kernels(nc, mult, input_size):
    """ts_tail_kernel reads W1 (fast-9 path, host-checked) and W2 (NC <= 16, NOT host-checked) as float4: both must start on a
    multiple of 4 floats of the flat parameter buffer; and T is what TS_T says."""
    lib = _lib.load()
    net = ctypes.c_void_p()
    cfg = _lib.NetConfig(_lib.KWS_NET_TS_ATTENTION, nc, mult, input_size, 0, 0)
    assert lib.kws_net_create(ctypes.byref(cfg), ctypes.byref(net)) == 0, lib.kws_last_error()
    try:
        info = _lib.TensorInfo()
        seen = {}
        for i in range(lib.kws_net_num_tensors(net)):
            assert lib.kws_net_tensor_info(net, i, ctypes.byref(info)) == 0
            seen[info.name.decode()] = (int(info.offset), [int(info.shape[k]) for k in range(info.ndim)], int(info.is_state))
    finally:
        lib.kws_net_destroy(net)
    off1, shape1, st1 = seen["dense_1/kernel"]
    off2, shape2, st2 = seen["dense_2/kernel"]
    assert not st1 and not st2
    T = TC.TS_T[input_size]
    assert shape1 == [T * 512 * mult, T] and shape2 == [2 * 512 * mult, nc]
    assert off1 % 4 == 0, "dense_1/kernel at float %d of the parameter buffer" % off1
    assert off2 % 4 == 0, "dense_2/kernel at float %d of the parameter buffer" % off2
