"""The BatchNorm bookkeeping shared by the grouped, depthwise, multi-slice and inception programs - csrc/bncols.hip
gbn_finalize_kernel, gbn_infer_kernel and the three passes gbn_bwd_part_kernel / gbn_bwd_fin_kernel / gbn_bwd_apply_kernel - called
directly through the test-only forwarders of tests/internal_shim.py, against the float64 references of tests/bn_cols_cases.py
(layouts, inputs, premises and bars are documented there; tests/test_bn_cols_cpu.py checks the premises without a GPU).

  backward   on integer inputs the partial rows, dgamma, dbeta and coef are BIT-equal to float64; dy is held to a bar derived
             from its float32 operations.  The gated gradient g is an integer here and pass 3 overwrites it (pass 1 is not a
             launcher of its own), so it is read back through dy: g = dy / scale + c1 + xhat c2 with the exact coef, where dy's
             bar is below 1e-4 and two integers are 1 apart - rint() of it IS g, and must equal the reference's g element for
             element (an element gated wrongly, or add on the wrong side of the gate, moves it by a whole number); the exact
             partial rows hold its column sums per 64-row chunk besides; kws_gbn_bwd_finish fed pass 1's rows reproduces every bit; references that are wrong on purpose
             (bn_cols_cases.MUTATIONS) are missed in a bit-exact output.
  forward    table entries and moving statistics against float64 with per-output bars of a few roundoffs; mm = NULL updates
             nothing; inference tables from random moving statistics.
  layouts    a window touches only its columns of the data, of the table [4][pitch] and its own two gradient tensors; grouped
             parameters land at q * pstride (+ boff) and the gaps keep their poison; g = 1 dense gives the window's bits; a window
             of several groups is refused without a launch.

Every output and scratch buffer is a window of a sentinel-guarded allocation; every launch is made twice and must give the same
bits."""
import ctypes

import numpy as np
import pytest
import torch

import bn_cols_cases as BC
import gemm_exact as GE
import internal_shim
from internal_shim import GbnCols, GbnRefs
from speech_recognition_amd import _lib
from test_resblock_kernels_gpu import GUARD, SENT, Guarded, P, dev, ok, twice

pytestmark = pytest.mark.gpu
U = BC.U
NAMES = list(BC.LAYOUTS)
assert SENT == BC.SENT
EPS, MOMENTUM = float(BC.BN_EPS), float(BC.BN_MOMENTUM)


@pytest.fixture(scope="module")
def lib(tmp_path_factory):
    assert torch.cuda.is_available(), "these tests need an MI355X"
    return internal_shim.load(internal_shim.build(str(tmp_path_factory.mktemp("kwst"))))


def st():
    return _lib.stream_ptr()


def f32(bits):
    return bits.view(np.float32)


def cols_of(lay):
    return GbnCols(g=lay["g"], Ng=lay["Ng"], pitch=lay["pitch"], c0=lay["c0"])


def scattered(size, idx, values, fill=None):
    """float32 [size]: `values` at `idx`; elsewhere the poison's bits (an in / out buffer) or `fill` (an input: NaN, so that a read
    outside the window shows)"""
    a = np.full(size, SENT, dtype=np.int32).view(np.float32) if fill is None else np.full(size, fill, dtype=np.float32)
    a[np.asarray(idx).reshape(-1)] = np.asarray(values, dtype=np.float32).reshape(-1)
    return a


def check_written(g, idx, what):
    """guards intact; exactly the elements `idx` of the buffer were written"""
    torch.cuda.synchronize()
    assert bool((g.buf[:GUARD] == SENT).all()) and bool((g.buf[-GUARD:] == SENT).all()), "%s wrote outside its buffer" % what
    w = g.bits() != SENT
    mask = np.zeros(g.n, dtype=bool)
    mask[np.asarray(idx).reshape(-1)] = True
    assert w[mask].all(), "%s left %d of its elements unwritten" % (what, int((~w[mask]).sum()))
    assert not w[~mask].any(), "%s wrote %d elements that are not its own" % (what, int(w[~mask].sum()))


def offset_ptr(g, floats):
    return ctypes.c_void_p(g.view.data_ptr() + 4 * floats)


# ---------------------------------------------------------------------------------------------------------------------------
# backward
# ---------------------------------------------------------------------------------------------------------------------------
def run_bwd(lib, name, inp, with_add, finish_from=None):
    """one kws_gbn_bwd (or, finish_from = (g [M, F], part bits): kws_gbn_bwd_finish) into fresh guarded buffers
    -> [dA, part, coef, grads]; checks what was written and what was not"""
    lay = BC.LAYOUTS[name]
    M, F, n = lay["M"], BC.width(lay), lay["M"] * lay["pitch"]
    didx, rl = BC.data_idx(lay), BC.refs_layout(lay)
    rows = -(-M // BC.CHUNK)
    dA = Guarded(n, init=scattered(n, didx, inp["dA"] if finish_from is None else finish_from[0]))
    y, add = dev(scattered(n, didx, inp["y"], np.nan)), dev(scattered(n, didx, inp["add"], np.nan))
    table = dev(scattered(BC.table_size(lay), BC.table_idx(lay), inp["table"], np.nan))
    coef, grads = Guarded(2 * F), Guarded(rl["size"])
    cols = cols_of(lay)
    if finish_from is None:
        part = Guarded(rows * 2 * F)
        ok(lib, lib.kwst_gbn_bwd(dA.ptr(), P(y), P(table), P(add) if with_add else None, M, ctypes.byref(cols), part.ptr(), coef.ptr(),
                                 offset_ptr(grads, rl["base"]), rl["pstride"], rl["boff"], st()), "gbn_bwd %s" % name)
        part.check("gbn_bwd %s part" % name)
    else:
        part = Guarded(rows * 2 * F, init=f32(finish_from[1]))
        ok(lib, lib.kwst_gbn_bwd_finish(dA.ptr(), P(y), P(table), M, ctypes.byref(cols), part.ptr(), rows, coef.ptr(),
                                        offset_ptr(grads, rl["base"]), rl["pstride"], rl["boff"], st()), "gbn_bwd_finish %s" % name)
        assert np.array_equal(part.bits(), finish_from[1]), "gbn_bwd_finish wrote its partial rows"
    coef.check("gbn_bwd %s coef" % name)
    # dgamma / dbeta: the layer's own two tensors (every group's), nothing of the neighbours or the gaps
    check_written(grads, np.concatenate([rl["first"], rl["second"]]), "gbn_bwd %s dgamma / dbeta" % name)
    # dA: in place on the window; the other columns of the tensor keep their poison
    check_written(dA, didx, "gbn_bwd %s dy" % name)
    return [dA, part, coef, grads]


_BWD = {}


def bwd_run(lib, name, with_add):
    """(device outputs in the window's shape, float64 reference, inputs) of one layout, run twice, made once per module"""
    key = (name, with_add)
    if key not in _BWD:
        lay = BC.LAYOUTS[name]
        M, F = lay["M"], BC.width(lay)
        rl = BC.refs_layout(lay)
        inp = BC.bwd_inputs(name)
        dA, part, coef, grads = twice(lambda: run_bwd(lib, name, inp, with_add))
        got = dict(dy=f32(dA)[BC.data_idx(lay)], part=f32(part).reshape(-1, 2, F), part_bits=part, coef=f32(coef).reshape(2, F),
                   dgamma=f32(grads)[rl["first"]], dbeta=f32(grads)[rl["second"]])
        _BWD[key] = (got, BC.bwd_ref(inp, with_add), inp)
    return _BWD[key]


@pytest.mark.parametrize("with_add", [False, True])
@pytest.mark.parametrize("name", NAMES)
def test_bwd_sums_are_exact_and_dy_meets_its_bar(lib, name, with_add):
    got, ref, inp = bwd_run(lib, name, with_add)
    BC.premise_bwd(inp, ref)
    for k in BC.EXACT_OUTPUTS:
        GE.assert_exact(got[k], ref[k], "%s of %s" % (k, name))
    # dy = scale (g - c1 - xhat c2) against float64 on the device's own (exact) coef: the bar of bn_cols_cases.bwd_ref
    err = np.abs(got["dy"].astype(np.float64) - ref["dy"])
    print("gbn_bwd %-11s add=%d  dy: worst error / bar %.3f" % (name, with_add, float((err / np.maximum(ref["dy_bar"], 1e-300)).max())))
    assert (err <= ref["dy_bar"]).all(), "dy of %s: %d elements beyond their bar" % (name, int((err > ref["dy_bar"]).sum()))
    # the gated gradient itself, which pass 3 overwrote: an integer, so dy / scale + c1 + xhat c2 names it exactly
    sc = BC.f64(inp["table"][0])
    g_rec = got["dy"].astype(np.float64) / sc + ref["coef"][0] + ref["xhat"] * ref["coef"][1]
    assert np.array_equal(np.rint(g_rec), ref["g"]) and np.abs(g_rec - ref["g"]).max() < 1e-3, "gated gradient of %s" % name


@pytest.mark.parametrize("name", NAMES)
@pytest.mark.parametrize("mutate", BC.MUTATIONS)
def test_bwd_misses_the_wrong_references(lib, mutate, name):
    got, ref, inp = bwd_run(lib, name, True)
    wrong = BC.bwd_ref(inp, True, mutate=mutate)
    assert all(GE.same_bits(got[k], ref[k]) for k in BC.EXACT_OUTPUTS)                    # (the right one is met ...)
    assert any(not GE.same_bits(got[k], wrong[k]) for k in BC.EXACT_OUTPUTS), mutate


@pytest.mark.parametrize("name", NAMES)
def test_bwd_finish_reproduces_bwd_from_its_partial_rows(lib, name):
    got, ref, inp = bwd_run(lib, name, True)
    dA, part, coef, grads = twice(lambda: run_bwd(lib, name, inp, True, finish_from=(ref["g"], got["part_bits"])))
    lay, rl = BC.LAYOUTS[name], BC.refs_layout(BC.LAYOUTS[name])
    for k, mine in (("dy", f32(dA)[BC.data_idx(lay)]), ("coef", f32(coef).reshape(2, -1)), ("dgamma", f32(grads)[rl["first"]]),
                    ("dbeta", f32(grads)[rl["second"]])):
        assert np.array_equal(mine.view(np.int32), got[k].view(np.int32)), "%s of %s" % (k, name)


@pytest.mark.parametrize("with_add", [False, True])
def test_one_dense_group_gives_the_windows_bits(lib, with_add):
    plain, window = bwd_run(lib, "plain", with_add)[0], bwd_run(lib, "window", with_add)[0]
    for k in ("dy", "part", "coef", "dgamma", "dbeta"):
        assert np.array_equal(plain[k].view(np.int32), window[k].view(np.int32)), k


def test_bwd_rows_is_one_per_64_rows(lib):
    assert [lib.kwst_gbn_bwd_rows(M) for M in (1, 63, 64, 65, 1093, 2 ** 33)] == [1, 1, 1, 2, 18, 2 ** 27]


# ---------------------------------------------------------------------------------------------------------------------------
# forward tables
# ---------------------------------------------------------------------------------------------------------------------------
def run_table(lib, name, inp, training, update=True):
    """kws_gbn_finalize (training) or kws_gbn_infer into fresh guarded buffers -> [table, state]"""
    lay = BC.LAYOUTS[name]
    rl = BC.refs_layout(lay)
    both = np.concatenate([rl["first"], rl["second"]])
    params = dev(scattered(rl["size"], both, np.concatenate([inp["gamma"], inp["beta"]]), np.nan))
    state = Guarded(rl["size"], init=scattered(rl["size"], both, np.concatenate([inp["mm"], inp["mv"]])))
    table = Guarded(BC.table_size(lay))
    cols = cols_of(lay)
    refs = GbnRefs(gamma=params.data_ptr() + 4 * rl["base"], pstride=rl["pstride"], boff=rl["boff"],
                   mm=state.view.data_ptr() + 4 * rl["base"] if (update or not training) else None, sstride=rl["pstride"], voff=rl["boff"])
    if training:
        part = dev(inp["part"])
        ok(lib, lib.kwst_gbn_finalize(P(part), inp["part"].shape[0], inp["count"], ctypes.byref(cols), ctypes.byref(refs), EPS,
                                      MOMENTUM, table.ptr(), st()), "gbn_finalize %s" % name)
    else:
        ok(lib, lib.kwst_gbn_infer(ctypes.byref(cols), ctypes.byref(refs), EPS, table.ptr(), st()), "gbn_infer %s" % name)
    # a window writes only its columns of [4][pitch]; the state keeps its neighbours and gaps
    check_written(table, BC.table_idx(lay), "gbn table %s" % name)
    check_written(state, both, "gbn state %s" % name)
    return [table, state]


def check_table(name, table_bits, state_bits, val, bar, state_keys):
    lay = BC.LAYOUTS[name]
    rl = BC.refs_layout(lay)
    t = f32(table_bits)[BC.table_idx(lay)].astype(np.float64)
    got = dict(scale=t[0], shift=t[1], mean=t[2], rstd=t[3])
    if state_keys:
        got.update(mm=f32(state_bits)[rl["first"]].astype(np.float64), mv=f32(state_bits)[rl["second"]].astype(np.float64))
    for k in ("scale", "shift", "mean", "rstd") + state_keys:
        err = np.abs(got[k] - val[k])
        assert (err <= bar[k]).all(), "%s of %s: worst error %g, its bar %g" % (k, name, err.max(), bar[k][np.argmax(err - bar[k])])


@pytest.mark.parametrize("rows", BC.FIN_ROWS)
@pytest.mark.parametrize("name", NAMES)
def test_finalize_tables_and_moving_statistics(lib, name, rows):
    inp = BC.fin_inputs(name, rows)
    val, bar = BC.fin_ref(inp)
    table, state = twice(lambda: run_table(lib, name, inp, True))
    check_table(name, table, state, val, bar, ("mm", "mv"))
    # mm = NULL: the same table, the state buffer as it was
    rl = BC.refs_layout(BC.LAYOUTS[name])
    table0, state0 = twice(lambda: run_table(lib, name, inp, True, update=False))
    assert np.array_equal(table0, table)
    assert np.array_equal(f32(state0)[rl["first"]], inp["mm"]) and np.array_equal(f32(state0)[rl["second"]], inp["mv"])


@pytest.mark.parametrize("name", NAMES)
def test_inference_tables(lib, name):
    inp = BC.params_inputs(BC.width(BC.LAYOUTS[name]), 31)
    val, bar = BC.infer_ref(inp)
    rl = BC.refs_layout(BC.LAYOUTS[name])
    table, state = twice(lambda: run_table(lib, name, inp, False))
    check_table(name, table, state, val, bar, ())
    assert np.array_equal(f32(state)[rl["first"]], inp["mm"]) and np.array_equal(f32(state)[rl["second"]], inp["mv"])


def test_plain_tables_are_the_windows_tables(lib):
    inp = BC.fin_inputs("window", 17)
    assert np.array_equal(inp["part"], BC.fin_inputs("plain", 17)["part"])
    outs = {}
    for name in ("plain", "window"):
        table, state = run_table(lib, name, inp, True)
        rl = BC.refs_layout(BC.LAYOUTS[name])
        outs[name] = (table.bits()[BC.table_idx(BC.LAYOUTS[name])], state.bits()[np.concatenate([rl["first"], rl["second"]])])
    assert np.array_equal(outs["plain"][0], outs["window"][0]) and np.array_equal(outs["plain"][1], outs["window"][1])


# ---------------------------------------------------------------------------------------------------------------------------
# the layout nobody uses
# ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("lay", [dict(g=2, Ng=10, pitch=72, c0=8, M=70), dict(g=2, Ng=10, pitch=72, c0=0, M=70),
                                 dict(g=1, Ng=20, pitch=24, c0=8, M=70)])
def test_a_window_of_several_groups_is_refused_without_a_launch(lib, lay):
    """(also: a window that does not fit its pitch)"""
    M, F, n = lay["M"], BC.width(lay), lay["M"] * lay["pitch"]
    cols = cols_of(lay)
    dA, part, coef, grads, table, state = Guarded(n), Guarded(2 * 2 * F), Guarded(2 * F), Guarded(4 * F), Guarded(4 * lay["pitch"]), Guarded(4 * F)
    y = dev(np.zeros(n, np.float32))
    refs = GbnRefs(gamma=y.data_ptr(), pstride=F, boff=F // 2, mm=state.view.data_ptr(), sstride=F, voff=F // 2)
    calls = [
        lambda: lib.kwst_gbn_bwd(dA.ptr(), P(y), P(y), None, M, ctypes.byref(cols), part.ptr(), coef.ptr(), grads.ptr(), F, F // 2, st()),
        lambda: lib.kwst_gbn_bwd_finish(dA.ptr(), P(y), P(y), M, ctypes.byref(cols), P(y), 2, coef.ptr(), grads.ptr(), F, F // 2, st()),
        lambda: lib.kwst_gbn_finalize(P(y), 2, M, ctypes.byref(cols), ctypes.byref(refs), EPS, MOMENTUM, table.ptr(), st()),
        lambda: lib.kwst_gbn_infer(ctypes.byref(cols), ctypes.byref(refs), EPS, table.ptr(), st()),
    ]
    for call in calls:
        assert call() == -1                                                   # KWS_E_INVALID
        msg = lib.kws_last_error()
        msg = msg.decode() if isinstance(msg, bytes) else msg
        assert "pitch" in msg and str(lay["pitch"]) in msg, msg
    assert all(g.untouched() for g in (dA, part, coef, grads, table, state))
