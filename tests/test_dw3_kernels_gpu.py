"""The 3-tap depthwise chain (csrc/dwconv.hip, csrc/dw_bwd_body.h) and the folds of csrc/bn.hip, called directly - the public
entry points and, through tests/internal_shim.py, the two batch launchers only the network programs call - on the exact inputs
of tests/dw3_cases.py: every tensor, partial-row fold and gradient must EQUAL the float64 reference built from oracle/layers.py
(gemm_exact.assert_exact), and wherever two kernels or two runs produce the same quantity their bits must agree.  That pins the
ReLU6 corner rule (pre > 0 && pre <= 6: 4 % of the pre-activations are 6, 9 % are 0), the fold of the partial rows as their
contract (which row holds which unit is NOT asserted) and the equivalence of the scratch and no-scratch folds.

Every output is a window of a sentinel-guarded allocation (the helpers of tests/test_resblock_kernels_gpu.py); every launch runs
twice into fresh buffers.  No bar here is a measured number: the only comparisons that are not equalities are those of
kws_bn_infer_prepare (bars derived from its roundings, dw3_cases.infer_ref) and the four that test_bn_stats_finalize_and_apply
(tests/test_kernels_gpu.py) already makes of kws_bn_stats_finalize against float64, taken over as they stand there.

Whether the wrong-on-purpose references (exclusive ReLU6 mask, a lost row, a doubled row) differ from the right one is settled
without a GPU in tests/test_dw3_cpu.py."""
import ctypes

import numpy as np
import pytest

import dw3_cases as DC
import gemm_exact as GE
import internal_shim
from oracle import layers as OL
from test_resblock_kernels_gpu import Guarded, P, dev, ok, st, twice

pytestmark = pytest.mark.gpu

AMAX_WORDS = DC.ABSMAX_SLOTS * DC.ABSMAX_STRIDE
AMAX_FILL = 0x3F800001          # what the 240 words between the slots hold: no kernel may change it


@pytest.fixture(scope="module")
def lib(tmp_path_factory):
    return internal_shim.load(internal_shim.build(str(tmp_path_factory.mktemp("kwst"))))


def f32(bits):
    return bits.view(np.float32)


def up(a):
    """upload one of the cases' cached (read-only) inputs"""
    return dev(np.array(a))


def amax_buf():
    init = np.full(AMAX_WORDS, AMAX_FILL, np.uint32)
    init[::DC.ABSMAX_STRIDE] = 0                                 # the caller zeroes the slots
    return Guarded(AMAX_WORDS, init=init.view(np.float32))


def check_amax(bits, want, what):
    """the maximum over the 16 slots is the bit pattern of `want`; the other 240 words are untouched"""
    words = bits.view(np.uint32)
    slots = words[::DC.ABSMAX_STRIDE]
    assert int(slots.max()) == int(np.float32(want).view(np.uint32)), "%s: slots hold %r, max is %r" % (
        what, float(slots.max().view(np.float32)), float(want))
    assert (np.delete(words, np.arange(0, AMAX_WORDS, DC.ABSMAX_STRIDE)) == AMAX_FILL).all(), "%s wrote between its slots" % what


def same_bits(a, b, what):
    assert np.array_equal(a, b), "%s: %d of %d words differ" % (what, int((a != b).sum()), a.size)


BN_IDS = ["bn", "nobn"]


# ---------------------------------------------------------------------------------------------------------------------------
# 1. forward
# ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("with_bn", [True, False], ids=BN_IDS)
@pytest.mark.parametrize("c", DC.CASES, ids=DC.case_id)
def test_forward(lib, c, with_bn):
    B, Lin, C, stride, pad_l, Lout = c[:6]
    inp = DC.inputs(c)
    zref = DC.fwd_ref_int(c, with_bn) if c[6] else DC.fwd_ref(c, with_bn)[0]
    y, w, bn = up(inp["y"]), up(inp["w"]), up(inp["bn"]) if with_bn else None

    def plain():
        z = Guarded(B * Lout * C)
        ok(lib, lib.kws_dwconv_fwd_f32(P(y), P(bn), P(w), z.ptr(), B, Lin, Lout, C, stride, pad_l, st()), "dwconv_fwd")
        z.check("dwconv_fwd")
        return [z]

    def with_amax():
        z, am = Guarded(B * Lout * C), amax_buf()
        ok(lib, lib.kws_dwconv_fwd_amax_f32(P(y), P(bn), P(w), z.ptr(), B, Lin, Lout, C, stride, pad_l, am.ptr(), st()),
           "dwconv_fwd_amax")
        z.check("dwconv_fwd_amax")
        am.check("dwconv_fwd_amax slots")
        return [z, am]

    zb, = twice(plain)
    GE.assert_exact(f32(zb).reshape(B, Lout, C), zref, "z")
    zb2, am = twice(with_amax)
    same_bits(zb2, zb, "z of kws_dwconv_fwd_amax_f32 against kws_dwconv_fwd_f32")
    check_amax(am, np.abs(zref).max(), "dwconv_fwd_amax")


# ---------------------------------------------------------------------------------------------------------------------------
# 2. - 5. backward: stored form, two-pass form, finalise, host-side controls
# ---------------------------------------------------------------------------------------------------------------------------
def finalize(lib, part, rows, count, C, want_dw=True, want_bn=True):
    """kws_dw_bwd_finalize into fresh guarded buffers; an output not asked for is passed as NULL and must keep its sentinel.
    With at most 256 rows the scratch buffer it is given stays unwritten."""
    dw, dgamma, dbeta, coef, scratch = Guarded(3 * C), Guarded(C), Guarded(C), Guarded(2 * C), Guarded(DC.REDUCE_SLICES * 5 * C)
    ok(lib, lib.kws_dw_bwd_finalize(part.ptr(), rows, count, C, dw.ptr() if want_dw else None, dgamma.ptr() if want_bn else None,
                                    dbeta.ptr(), coef.ptr() if want_bn else None, scratch.ptr(), st()), "dw_bwd_finalize")
    for g, wanted, name in ((dw, want_dw, "dw"), (dgamma, want_bn, "dgamma"), (dbeta, True, "dbeta"), (coef, want_bn, "coef")):
        if wanted:
            g.check("dw_bwd_finalize " + name)
        else:
            assert g.untouched(), "dw_bwd_finalize wrote %s, which it was not given" % name
    assert scratch.untouched(), "dw_bwd_finalize wrote scratch for %d rows" % rows
    return [dw, dgamma, dbeta, coef]


@pytest.mark.parametrize("with_bn", [True, False], ids=BN_IDS)
@pytest.mark.parametrize("c", DC.BWD_CASES, ids=DC.case_id)
def test_backward(lib, c, with_bn):
    B, Lin, C, stride, pad_l, Lout = c[:6]
    inp, ref = DC.inputs(c), DC.bwd_ref(c, with_bn)
    n_part = DC.part_floats(B, Lin, C)
    assert n_part == lib.kws_dwconv_bwd_part_floats(B, Lin, C)
    rows, count, N = n_part // (5 * C), B * Lin, B * Lin * C
    y, w, dz = up(inp["y"]), up(inp["w"]), up(inp["dz"])
    bn = up(inp["bn"]) if with_bn else None
    geo = (B, Lin, Lout, C, stride, pad_l)

    # ---- 2. stored form: g and the partial rows
    def stored():
        g, part = Guarded(N), Guarded(n_part)
        ok(lib, lib.kws_dwconv_bwd_f32(P(dz), P(y), P(bn), P(w), g.ptr(), part.ptr(), *geo, st()), "dwconv_bwd")
        g.check("dwconv_bwd g")
        part.check("dwconv_bwd partial rows")                    # exactly part_floats floats, none left unwritten
        return [g, part]

    gb, pb = twice(stored)
    GE.assert_exact(f32(gb).reshape(B, Lin, C), ref["g"], "g")
    fold = DC.f64(f32(pb).reshape(rows, 5, C)).sum(0)            # the contract of the rows is their fold, not their layout
    GE.assert_exact(fold.astype(np.float32), ref["sums"], "the fold of the partial rows")
    assert np.array_equal(fold, ref["sums"])
    # ---- 5. controls: a reference that lost one (b, u) row, or counted it twice, is not what the device gave
    lost, doubled = DC.control_sums(c, with_bn)
    assert not np.array_equal(fold, lost) and not np.array_equal(fold, doubled)

    # ---- 4. finalise on those rows
    part = Guarded(n_part, init=f32(pb))
    dwb, dgb, dbb, cob = twice(lambda: finalize(lib, part, rows, count, C))
    same_bits(part.bits(), pb, "dw_bwd_finalize changed the partial rows")
    GE.assert_exact(f32(dwb).reshape(3, C), ref["sums"][2:], "dw")
    GE.assert_exact(f32(dgb), ref["sums"][1], "dgamma")
    GE.assert_exact(f32(dbb), ref["sums"][0], "dbeta")
    same_bits(cob, DC.coef_of(ref["sums"], count).reshape(-1).view(np.int32), "coef")
    no_dw = twice(lambda: finalize(lib, part, rows, count, C, want_dw=False))
    same_bits(no_dw[1], dgb, "dgamma without dw")
    same_bits(no_dw[2], dbb, "dbeta without dw")
    same_bits(no_dw[3], cob, "coef without dw")
    no_bn = twice(lambda: finalize(lib, part, rows, count, C, want_bn=False))
    same_bits(no_bn[0], dwb, "dw without dgamma and coef")
    same_bits(no_bn[2], dbb, "dbeta without dgamma and coef")
    if not with_bn:
        return

    # ---- 3. two-pass form: pass 1 leaves the rows of the stored form, pass 2 writes dy from hand-made coefficients
    coef, gamma = up(inp["coef"]), up(inp["gamma"])

    def pass1():
        p1 = Guarded(n_part)
        ok(lib, lib.kws_dwconv_bwd_bn_f32(P(dz), P(y), P(bn), P(w), None, None, p1.ptr(), 1, *geo, st()), "dwconv_bwd_bn pass 1")
        p1.check("dwconv_bwd_bn pass 1")
        return [p1]

    def pass2(amax):
        def run():
            dy = Guarded(N)
            if not amax:
                ok(lib, lib.kws_dwconv_bwd_bn_f32(P(dz), P(y), P(bn), P(w), P(coef), dy.ptr(), None, 2, *geo, st()),
                   "dwconv_bwd_bn pass 2")
                dy.check("dwconv_bwd_bn pass 2")
                return [dy]
            am = amax_buf()
            ok(lib, lib.kws_dwconv_bwd_bn_amax_f32(P(dz), P(y), P(bn), P(w), P(coef), dy.ptr(), None, 2, *geo, am.ptr(), st()),
               "dwconv_bwd_bn_amax pass 2")
            dy.check("dwconv_bwd_bn_amax pass 2")
            am.check("pass 2 slots")
            return [dy, am]
        return run

    def stored_apply(amax):
        def run():
            g, p2 = Guarded(N), Guarded(n_part)
            ok(lib, lib.kws_dwconv_bwd_f32(P(dz), P(y), P(bn), P(w), g.ptr(), p2.ptr(), *geo, st()), "dwconv_bwd")
            if not amax:
                ok(lib, lib.kws_bn_bwd_apply(g.ptr(), P(y), P(bn), P(gamma), P(coef), count, C, st()), "bn_bwd_apply")
                g.check("bn_bwd_apply")
                return [g]
            am = amax_buf()
            ok(lib, lib.kws_bn_bwd_apply_amax(g.ptr(), P(y), P(bn), P(gamma), P(coef), count, C, am.ptr(), st()), "bn_bwd_apply_amax")
            g.check("bn_bwd_apply_amax")
            am.check("bn_bwd_apply slots")
            return [g, am]
        return run

    p1, = twice(pass1)
    same_bits(p1, pb, "partial rows of pass 1 against the stored form")
    dyb, = twice(pass2(False))
    GE.assert_exact(f32(dyb).reshape(B, Lin, C), ref["dy"], "dy")
    dy_max = np.abs(ref["dy"]).max()
    dyb2, am = twice(pass2(True))
    same_bits(dyb2, dyb, "dy of kws_dwconv_bwd_bn_amax_f32")
    check_amax(am, dy_max, "dwconv_bwd_bn_amax")
    dyb3, = twice(stored_apply(False))
    same_bits(dyb3, dyb, "dy of kws_dwconv_bwd_f32 + kws_bn_bwd_apply against pass 2")
    dyb4, am = twice(stored_apply(True))
    same_bits(dyb4, dyb, "dy of kws_bn_bwd_apply_amax")
    check_amax(am, dy_max, "bn_bwd_apply_amax")


# ---------------------------------------------------------------------------------------------------------------------------
# the folds on their own: synthetic integer partial rows
# ---------------------------------------------------------------------------------------------------------------------------
def slice_sums(part_h, n, W, scratch):
    """what slice_reduce_kernel leaves in the scratch buffer: the sums of its S runs of rows"""
    rows_per, S = DC.pre_reduce_plan(n, scratch)
    p = DC.f64(part_h).reshape(n, W)
    return np.stack([p[s * rows_per:(s + 1) * rows_per].sum(0) for s in range(S)])


@pytest.mark.parametrize("n,C", DC.FOLD_CASES)
def test_dw_bwd_finalize_fold(lib, n, C):
    part_h, count = DC.dw_fold_inputs(n, C)
    sums = DC.f64(part_h).sum(0)
    W = 5 * C
    got = {}
    for scratch in (False, True):
        def run():
            part = Guarded(n * W, init=part_h)
            dw, dgamma, dbeta, coef, sc = Guarded(3 * C), Guarded(C), Guarded(C), Guarded(2 * C), Guarded(DC.REDUCE_SLICES * W)
            ok(lib, lib.kws_dw_bwd_finalize(part.ptr(), n, count, C, dw.ptr(), dgamma.ptr(), dbeta.ptr(), coef.ptr(),
                                            sc.ptr() if scratch else None, st()), "dw_bwd_finalize")
            for g in (dw, dgamma, dbeta, coef):
                g.check("dw_bwd_finalize")
            sc.check("dw_bwd_finalize scratch", written=DC.scratch_floats(n, W, scratch))
            assert np.array_equal(part.get(), part_h.reshape(-1)), "dw_bwd_finalize changed its partial rows"
            return [dw, dgamma, dbeta, coef, sc]
        got[scratch] = twice(run)
    for a, b, name in zip(got[False][:4], got[True][:4], ("dw", "dgamma", "dbeta", "coef")):
        same_bits(b, a, "%s with scratch against without" % name)
    dw, dgamma, dbeta, coef, sc = got[True]
    GE.assert_exact(f32(dw).reshape(3, C), sums[2:], "dw")
    GE.assert_exact(f32(dgamma), sums[1], "dgamma")
    GE.assert_exact(f32(dbeta), sums[0], "dbeta")
    same_bits(coef, DC.coef_of(sums, count).reshape(-1).view(np.int32), "coef")
    k = DC.scratch_floats(n, W, True)
    if k:
        GE.assert_exact(f32(sc)[:k].reshape(-1, W), slice_sums(part_h, n, W, True), "the slice sums in scratch")


@pytest.mark.parametrize("n,C", DC.FOLD_CASES)
def test_bn_stats_finalize_fold(lib, n, C):
    inp = DC.stats_fold_inputs(n, C)
    part_h, count = inp["part"], inp["count"]
    W = 2 * C
    gamma, beta = up(inp["gamma"]), up(inp["beta"])
    got = {}
    for scratch in (False, True):
        def run():
            part = Guarded(n * W, init=part_h)
            bn, mm, mv, sc = Guarded(4 * C), Guarded(C, init=inp["mm"]), Guarded(C, init=inp["mv"]), Guarded(DC.REDUCE_SLICES * W)
            ok(lib, lib.kws_bn_stats_finalize(part.ptr(), n, count, C, P(gamma), P(beta), 1e-3, 0.99, mm.ptr(), mv.ptr(), bn.ptr(),
                                              sc.ptr() if scratch else None, st()), "bn_stats_finalize")
            for g in (bn, mm, mv):
                g.check("bn_stats_finalize")
            sc.check("bn_stats_finalize scratch", written=DC.scratch_floats(n, W, scratch))
            assert np.array_equal(part.get(), part_h.reshape(-1)), "bn_stats_finalize changed its partial rows"
            return [bn, mm, mv, sc]
        got[scratch] = twice(run)
    for a, b, name in zip(got[False][:3], got[True][:3], ("table", "moving mean", "moving variance")):
        same_bits(b, a, "%s with scratch against without" % name)
    bn, mm, mv, sc = got[True]
    k = DC.scratch_floats(n, W, True)
    if k:
        GE.assert_exact(f32(sc)[:k].reshape(-1, W), slice_sums(part_h, n, W, True), "the slice sums in scratch")
    # float64 from the exact sums; the kernel multiplies by the reciprocal of the count in double
    s = DC.f64(part_h).sum(0) * (1.0 / float(count))
    mean = s[0]
    var = s[1] - mean * mean
    rstd = 1.0 / np.sqrt(var + float(np.float32(1e-3)))
    table = f32(bn).reshape(4, C)
    same_bits(table[2].view(np.int32), mean.astype(np.float32).view(np.int32), "mean")
    # the four bars of test_bn_stats_finalize_and_apply (tests/test_kernels_gpu.py), as they stand there
    np.testing.assert_allclose(table[2], mean, atol=1e-5)
    np.testing.assert_allclose(table[3], rstd, rtol=1e-5)
    np.testing.assert_allclose(f32(mm), OL.bn_moving_update(DC.f64(inp["mm"]), mean), atol=1e-6)
    np.testing.assert_allclose(f32(mv), OL.bn_moving_update(DC.f64(inp["mv"]), var), rtol=1e-5)


def ptr_array(guards):
    return (ctypes.c_void_p * len(guards))(*[g.view.data_ptr() for g in guards])


def int_array(values):
    return (ctypes.c_int * len(values))(*values)


def test_dw_grad_finalize_batch(lib):
    hosts = [DC.dw_fold_inputs(rows, C)[0] for C, rows in DC.BATCH_LAYERS]
    Cs, ns = [C for C, _ in DC.BATCH_LAYERS], [rows for _, rows in DC.BATCH_LAYERS]

    def fresh():
        parts = [Guarded(h.size, init=h) for h in hosts]
        return parts, [Guarded(3 * C) for C in Cs]

    def batch():
        parts, dws = fresh()
        ok(lib, lib.kwst_dw_grad_finalize_batch(ptr_array(parts), int_array(ns), int_array(Cs), ptr_array(dws), len(Cs), st()),
           "dw_grad_finalize_batch")
        for p, d, h in zip(parts, dws, hosts):
            d.check("dw_grad_finalize_batch")
            assert np.array_equal(p.get(), h.reshape(-1)), "dw_grad_finalize_batch changed its partial rows"
        return dws

    def single():
        parts, dws = fresh()
        for p, d, C, n in zip(parts, dws, Cs, ns):
            ok(lib, lib.kws_dw_bwd_finalize(p.ptr(), n, 4 * n + 3, C, d.ptr(), None, None, None, None, st()), "dw_bwd_finalize")
            d.check("dw_bwd_finalize")
        return dws

    for b, s, h, C in zip(twice(batch), twice(single), hosts, Cs):
        same_bits(b, s, "dw of the batch against kws_dw_bwd_finalize alone (C = %d)" % C)
        GE.assert_exact(f32(b).reshape(3, C), DC.f64(h).sum(0)[2:], "dw (C = %d)" % C)

    # refused argument sets: -1, and nothing is launched
    parts, dws = fresh()
    many_p, many_d = parts * 6, dws * 6
    refused = [
        ("count = 0", (ptr_array(parts), int_array(ns), int_array(Cs), ptr_array(dws), 0)),
        ("count = 17", (ptr_array(many_p[:17]), int_array((ns * 6)[:17]), int_array((Cs * 6)[:17]), ptr_array(many_d[:17]), 17)),
        ("257 rows", (ptr_array(parts), int_array([ns[0], 257, ns[2]]), int_array(Cs), ptr_array(dws), len(Cs))),
    ]
    for why, args in refused:
        assert lib.kwst_dw_grad_finalize_batch(*args, st()) == -1, why
        assert all(d.untouched() for d in dws), "dw_grad_finalize_batch refused %s and still wrote" % why


def test_bn_infer_prepare_single_and_batch(lib):
    inps = [DC.infer_inputs(C) for C in DC.INFER_C]
    devs = [dict((k, up(v)) for k, v in inp.items()) for inp in inps]
    singles = []
    for C, inp, d in zip(DC.INFER_C, inps, devs):
        def run():
            bn = Guarded(4 * C)
            ok(lib, lib.kws_bn_infer_prepare(P(d["gamma"]), P(d["beta"]), P(d["mm"]), P(d["mv"]), DC.BN_EPS, C, bn.ptr(), st()),
               "bn_infer_prepare")
            bn.check("bn_infer_prepare")
            return [bn]
        bits, = twice(run)
        singles.append(bits)
        table = DC.f64(f32(bits).reshape(4, C))
        ref, bars = DC.infer_ref(inp)
        err = np.abs(table - ref)
        for r, name in enumerate(("scale", "shift", "moving mean", "rstd")):
            print("bn_infer_prepare C=%d %s: largest error / bar %.3f" % (C, name, float((err[r] / np.maximum(bars[r], 1e-300)).max())))
        assert (err <= bars).all(), "bn_infer_prepare C=%d: row %d is %g over its bar" % (
            C, int(np.argmax((err - bars).max(1))), float((err - bars).max()))

    def batch():
        tables = [Guarded(4 * C) for C in DC.INFER_C]
        arr = lambda k: (ctypes.c_void_p * len(devs))(*[d[k].data_ptr() for d in devs])
        ok(lib, lib.kwst_bn_infer_prepare_batch(arr("gamma"), arr("beta"), arr("mm"), arr("mv"), DC.BN_EPS, int_array(DC.INFER_C),
                                                ptr_array(tables), len(devs), st()), "bn_infer_prepare_batch")
        for t in tables:
            t.check("bn_infer_prepare_batch")                    # (the maxC workgroups overrun the narrow layers: guards intact)
        return tables

    for b, s, C in zip(twice(batch), singles, DC.INFER_C):
        same_bits(b, s, "the batch's table against kws_bn_infer_prepare alone (C = %d)" % C)
    tables = [Guarded(4 * C) for C in DC.INFER_C]
    arr = lambda k: (ctypes.c_void_p * len(devs))(*[d[k].data_ptr() for d in devs])
    for count in (0, DC.FIN_BATCH + 1):
        assert lib.kwst_bn_infer_prepare_batch(arr("gamma"), arr("beta"), arr("mm"), arr("mv"), DC.BN_EPS, int_array(DC.INFER_C),
                                               ptr_array(tables), count, st()) == -1
        assert all(t.untouched() for t in tables)
