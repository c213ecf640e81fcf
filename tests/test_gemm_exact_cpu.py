"""The exact-integer GEMM tests (tests/gemm_exact.py) on the build machine, no GPU: the Python restatement of gemm.hip's planners
against the library's own host functions on every case (so that the instantiation labels of the tables hold), the corners the
tables must reach, the premise of every exact case (integer sums below 2^24) together with numpy's float32 product equalling the
float64 one, and the sensitivity controls: a reference with one row removed or counted twice is NOT bit-equal."""
import random

import numpy as np
import pytest

import gemm_exact as GE
from speech_recognition_amd import _lib


@pytest.fixture(scope="module")
def lib():
    return _lib.load()


def test_planner_restatement_matches_the_library(lib):
    shapes = set(GE.NN_EXACT_CASES + GE.TN_CASES + [c[:3] for c in GE.BN_CASES])
    shapes |= set((M, cout, cin) for M, cin, cout, _, _ in GE.PAIR_CASES) | set((M, cin, cout) for M, cin, cout, _, _ in GE.PAIR_CASES)
    rnd = random.Random(1)
    for _ in range(400):
        M = rnd.choice([1, 63, 64, 127, 128, 129, 1100, 4096, 5120, 8192, 33692, rnd.randint(1, 300000)])
        if rnd.random() < 0.7:
            shapes.add((M, 64 * rnd.randint(1, 16), 64 * rnd.randint(1, 17)))
        else:
            shapes.add((M, 4 * rnd.randint(1, 300), 4 * rnd.randint(1, 300)))
    for M, K, N in sorted(shapes):
        assert lib.kws_gemm_nn_stats_rows(M, K, N) == GE.nn_plan(M, K, N)["rows"], (M, K, N)
        assert lib.kws_gemm_tn_workspace_floats(M, K, N) == GE.tn_workspace_floats(M, K, N), (M, K, N)


def test_pair_table_labels_and_corners():
    forms, nn_corners, tn_corners = set(), set(), set()
    for M, cin, cout, form, corners in GE.PAIR_CASES:
        assert GE.pair_form(M, cin, cout) == form, (M, cin, cout)
        edges = GE.nn_edges(M, cout, cin)
        assert corners <= edges, (M, cin, cout, edges)
        forms.add(form)
        nn_corners |= edges
        tn_corners |= GE.tn_edges(M, cin, cout)
        assert M * max(cin, cout) <= 6e6                      # about a second per case
    assert forms == set(GE.PAIR_REACHABLE)                    # all seven instantiations the planner can reach
    assert GE.PAIR_NN_CORNERS <= nn_corners and GE.PAIR_TN_CORNERS <= tn_corners
    for M, cin, cout in GE.PAIR_REFUSED:
        assert GE.pair_form(M, cin, cout) is None
    # kws_gemm_nn_stats_rows reveals BN where an XCD has fewer than 32 slots (rows = 8 ceil(m_tiles / 8) cin / BN); with the
    # comparison of test_planner_restatement_matches_the_library that pins the BN of those cases, and (128, 64 | 128, 128) pin
    # the rule that keeps BN = 128 for cout = 64
    for M, cin, cout, form, _ in GE.PAIR_CASES:
        pl = GE.nn_plan(M, cout, cin)
        if pl["wgs"] < 32 * GE.NXCD:
            assert pl["rows"] * form[0] == GE.NXCD * GE.ceil_div(pl["m_tiles"], GE.NXCD) * cin
    assert GE.nn_plan(128, 64, 128)["rows"] == 8 and GE.nn_plan(128, 128, 128)["rows"] == 16


def test_only_seven_pair_instantiations_are_reachable():
    seen = set()
    for M in [1, 100, 128, 1000, 1100, 2048, 4096, 5120, 8192, 24000, 24704, 32768, 33692, 100000, 262144, 817152]:
        for cin in range(64, 1025, 64):
            for cout in range(64, 1025, 64):
                f = GE.pair_form(M, cin, cout)
                assert f is not None
                seen.add(f)
    assert seen == set(GE.PAIR_REACHABLE) and not seen & set(GE.PAIR_UNREACHABLE)


def test_nn_and_bn_tables_cover_every_form():
    assert {GE.nn_form(*c) for c in GE.NN_EXACT_CASES} == {"wide", "64/64", "64/32", "persistent"}
    for M, K, N, form in GE.BN_CASES:
        assert GE.nn_form(M, K, N) == form
    assert {c[3] for c in GE.BN_CASES} == {"wide", "64/64", "64/32", "persistent"}
    assert {64, 1024} <= {c[2] for c in GE.BN_CASES} and any(c[0] % 64 for c in GE.BN_CASES)
    corners = set().union(*[GE.nn_edges(*c) for c in GE.NN_EXACT_CASES])
    assert {"halves_only", "halves_after_full_round", "half_last_lt64", "half_last_65_127", "idle_xcd"} <= corners


def _controls_bite(got, ref, without, twice):
    assert GE.same_bits(got, ref)
    assert not GE.same_bits(got, without) and not GE.same_bits(got, twice)
    with pytest.raises(AssertionError):
        GE.assert_exact(got, without, "control")
    with pytest.raises(AssertionError):
        GE.assert_exact(got, twice, "control")


@pytest.mark.parametrize("M,K,N", GE.NN_EXACT_CASES)
def test_nn_exact_premise_and_controls(M, K, N):
    A, W = GE.nn_inputs(M, K, N)
    C = GE.f64(A) @ GE.f64(W)
    GE.premise_columns(C)
    C32 = A @ W
    assert GE.same_bits(C32, C)
    st32 = np.stack([C32.sum(axis=0, dtype=np.float32), (C32 * C32).sum(axis=0, dtype=np.float32)])
    r = GE.controls_row(C)
    _controls_bite(st32, GE.stats_ref(C), GE.stats_without_row(C, r), GE.stats_with_row_twice(C, r))


@pytest.mark.parametrize("B", GE.GATHER_B)
def test_gather_exact_premise_and_controls(B):
    x, W, G = GE.gather_inputs(B)
    C, cols = GE.gather_ref(x, W)
    assert C.shape == (B * 399, 128) and cols.shape == (B * 399, 120)
    GE.premise_columns(C)
    assert GE.same_bits(cols.astype(np.float32) @ W.reshape(120, 128), C)
    r = GE.controls_row(C)
    st32 = GE.stats_ref(C).astype(np.float32)
    _controls_bite(st32, GE.stats_ref(C), GE.stats_without_row(C, r), GE.stats_with_row_twice(C, r))
    GE.premise_tn(cols, G)
    dW = cols.T @ GE.f64(G)
    r = GE.tn_controls_row(cols, G)
    _controls_bite(cols.astype(np.float32).T @ G, dW, GE.tn_without_row(dW, cols, G, r), GE.tn_with_row_twice(dW, cols, G, r))


@pytest.mark.parametrize("M,K,N", GE.TN_CASES)
def test_tn_exact_premise_and_controls(M, K, N):
    A, G = GE.tn_inputs(M, K, N)
    GE.premise_tn(A, G)
    ref = GE.f64(A).T @ GE.f64(G)
    r = GE.tn_controls_row(A, G)
    _controls_bite(A.T @ G, ref, GE.tn_without_row(ref, A, G, r), GE.tn_with_row_twice(ref, A, G, r))


@pytest.mark.parametrize("M,cin,cout", [c[:3] for c in GE.PAIR_CASES])
def test_pair_exact_premise_and_controls(M, cin, cout):
    dY, WT, Z = GE.pair_inputs(M, cin, cout, exact=True)
    GE.premise_tn(Z, dY)
    dZ = GE.f64(dY) @ GE.f64(WT)
    assert np.abs(dZ).max() < GE.LIMIT and GE.same_bits(dY @ WT, dZ)
    dW = GE.f64(Z).T @ GE.f64(dY)
    r = GE.tn_controls_row(Z, dY)
    _controls_bite(Z.T @ dY, dW, GE.tn_without_row(dW, Z, dY, r), GE.tn_with_row_twice(dW, Z, dY, r))
