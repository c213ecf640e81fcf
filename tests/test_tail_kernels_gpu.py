"""The classifier-tail kernels - csrc/tail.hip (ts_tail_kernel<TRAIN, TT>, small_wgrad_rows_kernel / small_wgrad_kernel with
their slab sums, colsum_kernel's three geometries, metrics_kernel, tail_post_kernel) and csrc/gconv.hip flat_tail_kernel
<TRAIN, RAW> - called directly through the test-only forwarders of tests/internal_shim.py, against the float64 references of
tests/tail_cases.py (cases, inputs, premises and bars are documented there).

  exact      small_wgrad / colsum / metrics on integer inputs: out, out_bias, every slab of the scratch and the metrics are
             BIT-equal to float64; exactly the first S K N scratch floats are written (none when S = 1); host-side controls:
             the reference with one batch row removed, or counted twice, is not what the device gave.
  identity   tail_post + the slab batch is bit-identical to the six launches it replaces, on random floats.
  float64    every output of the two fused tails: exact where the arithmetic is (per_correct, the zeroed BN slots, dropped
             positions), derived bars for element-wise outputs and direct sums, measured bars (2 x the worst error of
             profiles/tail_direct_error_vs_f64.txt, never above 5e-5 of the max norm) for the chained ones.
  controls   references that are wrong on purpose (tail_cases.MUTATIONS) must be missed by more than the bar.

Every output is a window of a sentinel-guarded allocation and every run is made twice and must give the same bits.
`python tests/test_tail_kernels_gpu.py` prints the error table of profiles/tail_direct_error_vs_f64.txt."""
import ctypes
import os
import sys

if __name__ == "__main__":
    sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import numpy as np
import pytest
import torch

import gemm_exact as GE
import internal_shim
import tail_cases as TC
from internal_shim import FlatTailArgs, TailPostArgs, TsTailArgs
from speech_recognition_amd import _lib
from test_resblock_kernels_gpu import Guarded, P, dev, ok, twice

pytestmark = pytest.mark.gpu
U = TC.U


@pytest.fixture(scope="module")
def lib(tmp_path_factory):
    assert torch.cuda.is_available(), "these tests need an MI355X"
    return internal_shim.load(internal_shim.build(str(tmp_path_factory.mktemp("kwst"))))


def st():
    return _lib.stream_ptr()


def f32(bits):
    return bits.view(np.float32)


# ---------------------------------------------------------------------------------------------------------------------------
# small_wgrad / colsum / metrics: exact
# ---------------------------------------------------------------------------------------------------------------------------
def run_wgrad(lib, dX, dD, B, K, N, scratch, bias):
    """one launch into fresh guarded buffers -> [out, out_bias, scratch]; checks what was written and what was not"""
    pl = TC.small_wgrad_plan(B, K, N, scratch)
    out, ob, ws = Guarded(K * N), Guarded(N), Guarded(TC.SLICES * K * N)
    ok(lib, lib.kwst_small_wgrad_launch(P(dX), P(dD), out.ptr(), ob.ptr() if bias else None, B, K, N,
                                        ws.ptr() if scratch else None, st()), "small_wgrad")
    out.check("small_wgrad out")
    if bias:
        ob.check("small_wgrad out_bias")
    else:
        assert ob.untouched()
    # S of the restated planner: exactly the first S K N scratch floats, none when one slice writes `out` itself
    ws.check("small_wgrad scratch", written=pl["S"] * K * N if pl["S"] > 1 else 0)
    return [out, ob, ws]


def drop_row(ref64, X, D, r):
    return ref64 - np.outer(TC.f64(X[r]), TC.f64(D[r]))


@pytest.mark.parametrize("B,K,N,scratch,bias", [c[:5] for c in TC.WGRAD_CASES])
def test_small_wgrad_is_exact_on_integer_inputs(lib, B, K, N, scratch, bias):
    X, D = TC.wgrad_inputs(B, K, N)
    TC.premise_wgrad(X, D)
    pl = TC.small_wgrad_plan(B, K, N, scratch)
    dX, dD = dev(X), dev(D)
    out_bits, ob_bits, ws_bits = twice(lambda: run_wgrad(lib, dX, dD, B, K, N, scratch, bias))
    ref = TC.f64(X).T @ TC.f64(D)
    got = f32(out_bits).reshape(K, N)
    GE.assert_exact(got, ref, "out")
    if bias:
        GE.assert_exact(f32(ob_bits), TC.f64(D).sum(axis=0), "out_bias")
    if pl["S"] > 1:
        # slab s holds rows [s rows_per, (s + 1) rows_per) of the batch, the last one what is left: S and rows_per of the planner
        slabs = f32(ws_bits)[:pl["S"] * K * N].reshape(pl["S"], K, N)
        for s in range(pl["S"]):
            r0, r1 = s * pl["rows_per"], min((s + 1) * pl["rows_per"], B)
            GE.assert_exact(slabs[s], TC.f64(X[r0:r1]).T @ TC.f64(D[r0:r1]), "slab %d" % s)
    # controls on host data: the gradient without the last batch row, without the first row of the last slice, or with either
    # counted twice, is not what the device gave
    for r in sorted(set([B - 1, (pl["S"] - 1) * pl["rows_per"]])):
        rr = r
        while not (np.abs(X[rr]).sum() * np.abs(D[rr]).sum()):
            rr -= 1
        assert not GE.same_bits(got, drop_row(ref, X, D, rr))
        assert not GE.same_bits(got, 2 * ref - drop_row(ref, X, D, rr))
        if bias and np.abs(D[rr]).sum():
            assert not GE.same_bits(f32(ob_bits), TC.f64(D).sum(axis=0) - TC.f64(D[rr]))
            assert not GE.same_bits(f32(ob_bits), TC.f64(D).sum(axis=0) + TC.f64(D[rr]))


@pytest.mark.parametrize("B,N,form", TC.COLSUM_CASES)
def test_colsum_is_exact_on_integer_inputs(lib, B, N, form):
    K = TC.COLSUM_K
    assert TC.small_wgrad_plan(B, K, N, True)["colsum"] == form
    X, D = TC.wgrad_inputs(B, K, N)
    D[B - 1, :] = np.where(D[B - 1, :] == 0, 1, D[B - 1, :])              # the last row counts in every column
    TC.premise_wgrad(X, D)
    dX, dD = dev(X), dev(D)
    out_bits, ob_bits, _ = twice(lambda: run_wgrad(lib, dX, dD, B, K, N, True, True))
    ref = TC.f64(D).sum(axis=0)
    GE.assert_exact(f32(ob_bits), ref, "out_bias")
    GE.assert_exact(f32(out_bits).reshape(K, N), TC.f64(X).T @ TC.f64(D), "out")
    for r in sorted(set([0, B - 1])):
        if np.abs(D[r]).sum():
            assert not GE.same_bits(f32(ob_bits), ref - TC.f64(D[r])) and not GE.same_bits(f32(ob_bits), ref + TC.f64(D[r]))


def test_small_wgrad_refuses_a_bias_wider_than_64(lib):
    B, K, N = 8, 16, 65
    X, D = TC.wgrad_inputs(B, K, N)
    out, ob, ws = Guarded(K * N), Guarded(N), Guarded(TC.SLICES * K * N)
    rc = lib.kwst_small_wgrad_launch(P(dev(X)), P(dev(D)), out.ptr(), ob.ptr(), B, K, N, ws.ptr(), st())
    assert rc < 0
    assert out.untouched() and ob.untouched() and ws.untouched()


@pytest.mark.parametrize("B", TC.METRICS_B)
def test_metrics_are_exact(lib, B):
    per_loss, per_correct = TC.metrics_inputs(B)
    dl, dc = dev(per_loss), dev(per_correct)

    def run():
        m = Guarded(4)
        ok(lib, lib.kwst_metrics_launch(P(dl), P(dc), B, m.ptr(), st()), "metrics")
        m.check("metrics")
        return [m]
    got = f32(twice(run)[0])
    GE.assert_exact(got[:2], np.array([TC.f64(per_loss).sum(), TC.f64(per_correct).sum()]), "metrics")
    assert got[2] == 0 and got[3] == 0
    # controls: the sums without the last element that counts, or with it twice
    r = int(np.nonzero(per_loss + per_correct)[0][-1])
    full, one = np.array([TC.f64(per_loss).sum(), TC.f64(per_correct).sum()]), np.array([TC.f64(per_loss[r]), TC.f64(per_correct[r])])
    assert not GE.same_bits(got[:2], full - one) and not GE.same_bits(got[:2], full + one)


# ---------------------------------------------------------------------------------------------------------------------------
# tail_post: one launch for six
# ---------------------------------------------------------------------------------------------------------------------------
def tail_post_inputs(B, K1, N1, K2, N2):
    rng = np.random.RandomState(B + K1 + N2)
    return dict(X2=rng.randn(B, K2).astype(np.float32), D2=(0.1 * rng.randn(B, N2)).astype(np.float32),
                X1=rng.randn(B, K1).astype(np.float32), D1=(0.1 * rng.randn(B, N1)).astype(np.float32),
                per_loss=rng.rand(B).astype(np.float32) * 3, per_correct=rng.randint(0, 2, size=B).astype(np.float32))


def tail_post_buffers(K1, N1, K2, N2):
    return dict(ws2=Guarded(TC.SLICES * K2 * N2), ws1=Guarded(TC.SLICES * K1 * N1), bias1=Guarded(N1), metrics=Guarded(4))


def tail_post_args(d, o, B, K1, N1, K2, N2, with_bias=True):
    return TailPostArgs(X2=d["X2"].data_ptr(), D2=d["D2"].data_ptr(), ws2=o["ws2"].view.data_ptr(), K2=K2, N2=N2,
                        X1=d["X1"].data_ptr(), D1=d["D1"].data_ptr(), ws1=o["ws1"].view.data_ptr(), K1=K1, N1=N1,
                        bias1=o["bias1"].view.data_ptr() if with_bias else None, per_loss=d["per_loss"].data_ptr(),
                        per_correct=d["per_correct"].data_ptr(), metrics=o["metrics"].view.data_ptr(), B=B)


@pytest.mark.parametrize("B", TC.TAIL_POST_B)
def test_tail_post_is_bit_identical_to_the_six_launches(lib, B):
    h = TC.TAIL_POST_HEADLINE
    K1, N1, K2, N2 = h["K1"], h["N1"], h["K2"], h["N2"]
    assert TC.tail_post_eligible(B, K1, N1, K2, N2)
    S_plan = TC.small_wgrad_plan(B, K2, N2, True)["S"]
    inp = tail_post_inputs(B, K1, N1, K2, N2)
    d = dict((k, dev(v)) for k, v in inp.items())

    def fused(with_bias):
        o = tail_post_buffers(K1, N1, K2, N2)
        a = tail_post_args(d, o, B, K1, N1, K2, N2, with_bias)
        S = ctypes.c_int(-7)
        ok(lib, lib.kwst_tail_post_launch(ctypes.byref(a), ctypes.byref(S), st()), "tail_post")
        assert S.value == S_plan
        o["ws2"].check("tail_post ws2", written=S.value * K2 * N2)
        o["ws1"].check("tail_post ws1", written=S.value * K1 * N1)
        o["metrics"].check("tail_post metrics")
        if with_bias:
            o["bias1"].check("tail_post bias1")
        else:
            assert o["bias1"].untouched()
        dW2, dW1 = Guarded(K2 * N2), Guarded(K1 * N1)
        wsv = (ctypes.c_void_p * 2)(o["ws2"].view.data_ptr(), o["ws1"].view.data_ptr())
        outv = (ctypes.c_void_p * 2)(dW2.view.data_ptr(), dW1.view.data_ptr())
        ok(lib, lib.kwst_reduce_slabs_batch(wsv, outv, (ctypes.c_int64 * 2)(K2 * N2, K1 * N1), (ctypes.c_int * 2)(-S.value, -S.value),
                                            2, st()), "reduce_slabs_batch")
        dW2.check("slab batch dW2")
        dW1.check("slab batch dW1")
        return [dW2, dW1, o["bias1"], o["metrics"], o["ws2"], o["ws1"]]
    dW2, dW1, bias1, metrics, ws2, ws1 = twice(lambda: fused(True))
    # the six launches: two weight gradients with their slab sums, the bias gradient, the metrics
    o2, b2, s2 = run_wgrad(lib, d["X2"], d["D2"], B, K2, N2, True, False)
    o1, b1, s1 = run_wgrad(lib, d["X1"], d["D1"], B, K1, N1, True, True)
    m = Guarded(4)
    ok(lib, lib.kwst_metrics_launch(P(d["per_loss"]), P(d["per_correct"]), B, m.ptr(), st()), "metrics")
    assert np.array_equal(dW2, o2.bits()), "dW2 differs from kws_small_wgrad_launch"
    assert np.array_equal(dW1, o1.bits()), "dW1 differs from kws_small_wgrad_launch"
    assert np.array_equal(bias1, b1.bits()), "bias1 differs from kws_small_wgrad_launch"
    assert np.array_equal(metrics, m.bits()), "metrics differ from kws_metrics_launch"
    assert np.array_equal(ws2, s2.bits()) and np.array_equal(ws1, s1.bits()), "slabs differ from kws_small_wgrad_launch"
    # and the six launches are right: float64, the bars of the weight-gradient GEMMs (test_gemm_pair_gpu.py)
    assert TC.rel_err(f32(dW2).reshape(K2, N2), TC.f64(inp["X2"]).T @ TC.f64(inp["D2"])) < 5e-6
    assert TC.rel_err(f32(dW1).reshape(K1, N1), TC.f64(inp["X1"]).T @ TC.f64(inp["D1"])) < 5e-6
    assert TC.rel_err(f32(bias1), TC.f64(inp["D1"]).sum(axis=0)) < 5e-6
    nb = fused(False)
    for a_, b_ in zip((dW2, dW1, metrics), (nb[0], nb[1], nb[3])):
        assert np.array_equal(a_, b_.bits()), "tail_post without bias1 changes another output"


@pytest.mark.parametrize("B,K1,N1,K2,N2,why", TC.TAIL_POST_REFUSED)
def test_tail_post_refuses_shapes_it_does_not_take(lib, B, K1, N1, K2, N2, why):
    assert not TC.tail_post_eligible(B, K1, N1, K2, N2)
    d = dict((k, dev(v)) for k, v in tail_post_inputs(B, K1, N1, K2, N2).items())
    o = tail_post_buffers(K1, N1, K2, N2)
    S = ctypes.c_int(-7)
    rc = lib.kwst_tail_post_launch(ctypes.byref(tail_post_args(d, o, B, K1, N1, K2, N2)), ctypes.byref(S), st())
    assert rc == 1 and S.value == -7, why
    assert all(g.untouched() for g in o.values()), why


# ---------------------------------------------------------------------------------------------------------------------------
# ts_tail
# ---------------------------------------------------------------------------------------------------------------------------
TS_OUT = ("probs", "g", "part", "xd", "fd", "dl1", "dl2", "per_loss", "per_correct", "att")


def ts_sizes(B, T, C, NC):
    return dict(probs=B * NC, g=B * T * C, part=B * 5 * C, xd=B * T * C, fd=B * 2 * C, dl1=B * T, dl2=B * NC, per_loss=B,
                per_correct=B, att=B * T)


_TS_DEV = {}


def ts_device_inputs(name):
    """the case's inputs on the device, made once; W1 of case 'w1_off' starts one float past a 16-byte aligned base"""
    if name not in _TS_DEV:
        inp = TC.ts_inputs(name)
        d = dict((k, dev(v)) for k, v in inp.items())
        if name == "w1_off":
            base = torch.zeros(inp["W1"].size + 4, dtype=torch.float32, device="cuda")
            assert base.data_ptr() % 16 == 0
            d["W1"] = base[1:1 + inp["W1"].size]
            d["W1"].copy_(torch.from_numpy(inp["W1"].reshape(-1)).cuda())
            assert d["W1"].data_ptr() % 16 == 4
        _TS_DEV[name] = (inp, d)
    return _TS_DEV[name]


def run_ts(lib, name, train=True, row_offset=0, loss_batch=None, att=True, rows=None):
    """one launch into fresh guarded buffers -> {output: Guarded}; rows = (first clip, clips) of the case to run (a shard)"""
    _, Bc, T, C, NC, _, _ = TC.TS_BY_NAME[name]
    inp, d = ts_device_inputs(name)
    r0, B = rows if rows else (0, Bc)
    o = dict((k, Guarded(n)) for k, n in ts_sizes(B, T, C, NC).items())
    a = TsTailArgs(y=d["y"].data_ptr() + 4 * r0 * T * C, bn=d["bn"].data_ptr(), W1=d["W1"].data_ptr(), b1=d["b1"].data_ptr(),
                   W2=d["W2"].data_ptr(), labels=d["labels"].data_ptr() + 4 * r0 * NC, B=B, T=T, C=C, NC=NC, seed=TC.TS_SEED,
                   step=TC.TS_STEP, keep_prob=TC.KEEP, label_smoothing=TC.SMOOTH, loss_batch=loss_batch if loss_batch else B,
                   row_offset=row_offset, train=1 if train else 0)
    for k in TS_OUT:
        setattr(a, k, None if (k == "att" and not att) else o[k].view.data_ptr())
    ok(lib, lib.kwst_ts_tail_launch(ctypes.byref(a), st()), "ts_tail %s" % name)
    for k in TS_OUT:
        if (train and (att or k != "att")) or k == "probs":
            o[k].check("ts_tail %s %s" % (name, k))
        else:
            assert o[k].untouched(), "ts_tail %s wrote %s" % (name, k)
    return o


_TS_RUNS = {}


def ts_train(lib, name, row_offset=0):
    """(device outputs as float64 arrays, float64 reference) of case `name`, run twice, made once per module"""
    key = (name, row_offset)
    if key not in _TS_RUNS:
        _, B, T, C, NC, _, _ = TC.TS_BY_NAME[name]
        inp, _ = ts_device_inputs(name)
        bits = twice(lambda: [run_ts(lib, name, row_offset=row_offset)[k] for k in TS_OUT])
        got = dict((k, f32(b).astype(np.float64)) for k, b in zip(TS_OUT, bits))
        shapes = dict(probs=(B, NC), g=(B, T, C), part=(B, 5, C), xd=(B, T * C), fd=(B, 2 * C), dl1=(B, T), dl2=(B, NC),
                      per_loss=(B,), per_correct=(B,), att=(B, T))
        got = dict((k, v.reshape(shapes[k])) for k, v in got.items())
        _TS_RUNS[key] = (got, TC.ts_tail_ref(inp, row_offset), inp)
    return _TS_RUNS[key]


def chained(got, ref, keys):
    """{output: max-norm error relative to the reference's max norm}; a reference that is all zeros must be met exactly"""
    out = {}
    for k in keys:
        if not np.abs(ref[k]).max():
            assert not np.abs(got[k]).max(), "%s must be exactly 0" % k
            out[k] = 0.0
        else:
            out[k] = TC.rel_err(got[k], ref[k])
    return out


def check_ts(name, got, ref, inp):
    B, T, C = inp["y"].shape
    keep = float(np.float32(TC.KEEP))
    errs = chained(got, ref, list(TC.TS_BARS))
    print("ts_tail %-9s " % name + "  ".join("%s %.3g" % kv for kv in sorted(errs.items())))
    for k, e in errs.items():
        assert e <= TC.TS_BARS[k], "%s of %s: error %g of the max norm, bar %g" % (k, name, e, TC.TS_BARS[k])
    assert np.array_equal(got["per_correct"], ref["per_correct"])
    if T >= 2:
        assert np.array_equal(got["att"][:, 0], got["att"][:, 1])          # the structural ties are ties on the device too
    # xd = x m1 / keep, x exact: the rounding of the constant 1 / keep, of the product, and their cross term
    assert (np.abs(got["xd"] - ref["xd"]) <= 3 * U * np.abs(ref["xd"])).all(), "xd"
    # fd, given the device's attention weights: max_t(x att) rounds once, then as xd: 4 U; the mean is a chain of T - 1
    # additions (ts_tail_kernel: sm += xs[t C + c]), a division, then as xd: (T + 3) U on non-negative terms
    a = ref["a"]
    fmax = (a * got["att"][:, :, None]).max(axis=1)
    fd_ref = np.concatenate([fmax, a.mean(axis=1)], axis=1) * ref["m2"] / keep
    bar = np.concatenate([4 * U * np.abs(fd_ref[:, :C]), (T + 3) * U * np.abs(fd_ref[:, C:])], axis=1)
    assert (np.abs(got["fd"] - fd_ref) <= bar).all(), "fd"
    assert np.array_equal(got["fd"] == 0, ref["fd"] == 0)                  # the dropped positions, exactly
    # BN partial rows, given the device's g: chains of T additions per (clip, channel) (sg += gv; sgx = fma(gv, xhat, sgx)),
    # exact terms for sum g, three roundings per term (xhat's subtraction and product, the fma) for sum g xhat
    part, g = got["part"], got["g"]
    assert not part[:, 2:].any(), "slots 2..4 of part must be exactly 0"
    for slot, terms, k in ((0, g, 0), (1, g * ref["xh"], 3)):
        err = np.abs(part[:, slot] - terms.sum(axis=1))
        assert (err <= (T + k) * U * np.abs(terms).sum(axis=1)).all(), "part slot %d" % slot
    return errs


TS_TRAIN = [c[0] for c in TC.TS_CASES]


@pytest.mark.parametrize("name", TS_TRAIN)
def test_ts_tail_train_against_float64(lib, name):
    got, ref, inp = ts_train(lib, name)
    zero_ties, pair_ties = TC.premise_ts(inp, ref)
    check_ts(name, got, ref, inp)
    if name == "saturated":
        TC.premise_saturated(ref)
        assert not got["dl2"].any() and not got["g"].any()
        # p at both clip edges on the device too
        assert (got["probs"].max(axis=1) > TC.HI32).all() and ((got["probs"] < TC.LO32).sum(axis=1) == 11).all()
    elif name == "headline":
        assert zero_ties > 0 and pair_ties > 0


def test_ts_tail_accepts_a_null_att(lib):
    got, _, _ = ts_train(lib, "nc11")
    o = run_ts(lib, "nc11", att=False)
    for k in TS_OUT[:-1]:
        assert np.array_equal(f32(o[k].bits()).astype(np.float64).reshape(got[k].shape), got[k]), k


TS_INFER = ["headline", "nc32", "nc11", "w1_off", "t1", "maxt", "big_lds"]


def ts_infer(lib, name):
    inp, _ = ts_device_inputs(name)
    bits = twice(lambda: [run_ts(lib, name, train=False)["probs"]])[0]
    ref = TC.ts_tail_ref(inp, 0, train=False)
    return TC.rel_err(f32(bits).reshape(ref["probs"].shape), ref["probs"])


@pytest.mark.parametrize("name", TS_INFER)
def test_ts_tail_infer_writes_probs_only(lib, name):
    e = ts_infer(lib, name)                                               # (run_ts asserts every other buffer untouched)
    print("ts_tail %-9s infer probs %.3g" % (name, e))
    assert e <= TC.TS_BARS["probs"]


def test_ts_tail_shards_are_bit_identical_to_the_whole_batch(lib):
    """B = 6 at row_offset 0 (held to float64 by test_ts_tail_train_against_float64[shard]) against two launches of 3 clips at
    row offsets 0 and 3 with loss_batch 6"""
    whole = run_ts(lib, "shard", loss_batch=6)
    lo = run_ts(lib, "shard", row_offset=0, loss_batch=6, rows=(0, 3))
    hi = run_ts(lib, "shard", row_offset=3, loss_batch=6, rows=(3, 3))
    got, _, _ = ts_train(lib, "shard")
    for k in TS_OUT:
        assert np.array_equal(whole[k].bits(), np.concatenate([lo[k].bits(), hi[k].bits()])), k
        assert np.array_equal(whole[k].get().astype(np.float64).reshape(got[k].shape), got[k]), k


@pytest.mark.parametrize("change,why", [(dict(T=17), "T = 17"), (dict(NC=65), "NC = 65"), (dict(T=16, C=4096), "T C beyond 160 KB")])
def test_ts_tail_refuses_without_launching(lib, change, why):
    _, B, T, C, NC, _, _ = TC.TS_BY_NAME["nc11"]
    inp, d = ts_device_inputs("nc11")
    o = dict((k, Guarded(n)) for k, n in ts_sizes(B, T, C, NC).items())
    a = TsTailArgs(y=d["y"].data_ptr(), bn=d["bn"].data_ptr(), W1=d["W1"].data_ptr(), b1=d["b1"].data_ptr(), W2=d["W2"].data_ptr(),
                   labels=d["labels"].data_ptr(), B=B, T=T, C=C, NC=NC, seed=TC.TS_SEED, step=TC.TS_STEP, keep_prob=TC.KEEP,
                   label_smoothing=TC.SMOOTH, loss_batch=B, row_offset=0, train=1)
    for k in TS_OUT:
        setattr(a, k, o[k].view.data_ptr())
    for k, v in change.items():
        setattr(a, k, v)
    assert lib.kwst_ts_tail_launch(ctypes.byref(a), st()) < 0, why
    assert all(g.untouched() for g in o.values()), why


@pytest.mark.parametrize("mutate,name,key", TC.TS_CONTROLS)
def test_ts_tail_misses_the_wrong_references(lib, mutate, name, key):
    ro = 3 if mutate == "row_offset_ignored" else 0
    got, ref, inp = ts_train(lib, name, row_offset=ro)
    wrong = TC.ts_tail_ref(inp, ro, mutate=mutate)
    bar = TC.TS_BARS.get(key, 3 * U)
    if np.abs(ref[key]).max():
        assert TC.rel_err(got[key], ref[key]) <= bar                      # (the right one is met ...)
    assert np.abs(got[key] - wrong[key]).max() > bar * max(np.abs(wrong[key]).max(), np.abs(got[key]).max())


# ---------------------------------------------------------------------------------------------------------------------------
# flat_tail
# ---------------------------------------------------------------------------------------------------------------------------
FLAT_OUT = ("probs", "fd", "dl", "dA", "per_loss", "per_correct")


def run_flat(lib, name, d, train=True, D_override=None):
    _, B, D, F, Ng, NC, has_bd, raw, layer_id, row_offset, _, _ = TC.FLAT_BY_NAME[name]
    sizes = dict(probs=B * NC, fd=B * D, dl=B * NC, dA=B * D, per_loss=B, per_correct=B)
    o = dict((k, Guarded(n)) for k, n in sizes.items())
    a = FlatTailArgs(y=d["y"].data_ptr(), bn=d["bn"].data_ptr(), Ng=Ng, Wd=d["Wd"].data_ptr(),
                     bd=d["bd"].data_ptr() if has_bd else None, labels=d["labels"].data_ptr(), B=B,
                     D=D_override if D_override else D, F=F, NC=NC, seed=TC.TS_SEED, step=TC.TS_STEP, keep_prob=TC.FLAT_KEEP,
                     loss_batch=B, row_offset=row_offset, layer_id=layer_id, raw=1 if raw else 0)
    for k in FLAT_OUT:
        setattr(a, k, o[k].view.data_ptr())
    rc = lib.kwst_flat_tail_launch(ctypes.byref(a), 1 if train else 0, st())
    if D_override:
        return rc, o
    ok(lib, rc, "flat_tail %s" % name)
    for k in FLAT_OUT:
        if train or k == "probs":
            o[k].check("flat_tail %s %s" % (name, k))
        else:
            assert o[k].untouched(), "flat_tail %s wrote %s" % (name, k)
    return rc, o


_FLAT_RUNS = {}


def flat_train(lib, name):
    if name not in _FLAT_RUNS:
        _, B, D, F, Ng, NC = TC.FLAT_BY_NAME[name][:6]
        inp = TC.flat_inputs(name)
        d = dict((k, dev(v)) for k, v in inp.items() if v is not None)
        bits = twice(lambda: [run_flat(lib, name, d)[1][k] for k in FLAT_OUT])
        shapes = dict(probs=(B, NC), fd=(B, D), dl=(B, NC), dA=(B, D), per_loss=(B,), per_correct=(B,))
        got = dict((k, f32(b).astype(np.float64).reshape(shapes[k])) for k, b in zip(FLAT_OUT, bits))
        ibits = twice(lambda: [run_flat(lib, name, d, train=False)[1]["probs"]])[0]
        got["infer_probs"] = f32(ibits).astype(np.float64).reshape(B, NC)
        _FLAT_RUNS[name] = (got, TC.flat_tail_ref(name, inp), TC.flat_tail_ref(name, inp, train=False), inp, d)
    return _FLAT_RUNS[name]


def check_flat(name, got, ref, ref_infer):
    errs = chained(got, ref, list(TC.FLAT_BARS))
    errs["infer_probs"] = TC.rel_err(got["infer_probs"], ref_infer["probs"])
    print("flat_tail %-7s " % name + "  ".join("%s %.3g" % kv for kv in sorted(errs.items())))
    for k, e in errs.items():
        bar = TC.FLAT_BARS["probs" if k == "infer_probs" else k]
        assert e <= bar, "%s of %s: error %g of the max norm, bar %g" % (k, name, e, bar)
    assert np.array_equal(got["per_correct"], ref["per_correct"])
    # fd = relu6(bn(y)) m / keep, the activation exact: as ts_tail's xd (raw: a copy, the bar is then 0 wherever it matters)
    assert (np.abs(got["fd"] - ref["fd"]) <= 3 * U * np.abs(ref["fd"])).all(), "fd"
    return errs


@pytest.mark.parametrize("name", [c[0] for c in TC.FLAT_CASES])
def test_flat_tail_against_float64(lib, name):
    got, ref, ref_infer, inp, _ = flat_train(lib, name)
    TC.premise_flat(ref)
    check_flat(name, got, ref, ref_infer)
    if TC.FLAT_BY_NAME[name][7]:
        assert np.array_equal(got["fd"], TC.f64(inp["y"]))                 # raw: the features are y itself, no dropout


def test_flat_tail_refuses_a_row_longer_than_its_lds(lib):
    _, _, _, _, d = flat_train(lib, "maxd")
    rc, o = run_flat(lib, "maxd", d, D_override=TC.FT_MAXD + 1)
    assert rc < 0
    assert all(g.untouched() for g in o.values())


@pytest.mark.parametrize("mutate,name,key", TC.FLAT_CONTROLS)
def test_flat_tail_misses_the_wrong_references(lib, mutate, name, key):
    got, ref, _, inp, _ = flat_train(lib, name)
    wrong = TC.flat_tail_ref(name, inp, mutate=mutate)
    assert np.abs(got[key] - wrong[key]).max() > 3 * U * np.abs(wrong[key]).max()


# ---------------------------------------------------------------------------------------------------------------------------
# the error table of profiles/tail_direct_error_vs_f64.txt
# ---------------------------------------------------------------------------------------------------------------------------
def error_table(lib):
    lines = ["max-norm error against float64 relative to the reference's max norm, on the inputs of tests/tail_cases.py;",
             "att_rel: the largest RELATIVE error of one attention weight (tail_cases.POOL_GAP leans on it)", ""]
    bars = TC.TS_BARS, TC.FLAT_BARS
    TC.TS_BARS = dict((k, np.inf) for k in TC.TS_BARS)
    TC.FLAT_BARS = dict((k, np.inf) for k in TC.FLAT_BARS)
    try:
        worst = {}
        for name in TS_TRAIN:
            got, ref, inp = ts_train(lib, name)
            e = check_ts(name, got, ref, inp)
            e["att_rel"] = float((np.abs(got["att"] - ref["att"]) / ref["att"]).max())
            if name in TS_INFER:
                e["probs"] = max(e["probs"], ts_infer(lib, name))
            for k, v in e.items():
                worst[k] = max(worst.get(k, 0.0), v)
            lines.append("ts_tail   %-9s " % name + "  ".join("%s %.3g" % (k, e[k]) for k in sorted(e)))
        lines.append("ts_tail   %-9s " % "worst" + "  ".join("%s %.3g" % (k, worst[k]) for k in sorted(worst)))
        worst = {}
        for c in TC.FLAT_CASES:
            got, ref, ref_infer, _, _ = flat_train(lib, c[0])
            e = check_flat(c[0], got, ref, ref_infer)
            e["probs"] = max(e["probs"], e.pop("infer_probs"))
            for k, v in e.items():
                worst[k] = max(worst.get(k, 0.0), v)
            lines.append("flat_tail %-9s " % c[0] + "  ".join("%s %.3g" % (k, e[k]) for k in sorted(e)))
        lines.append("flat_tail %-9s " % "worst" + "  ".join("%s %.3g" % (k, worst[k]) for k in sorted(worst)))
    finally:
        TC.TS_BARS, TC.FLAT_BARS = bars
    return "\n".join(lines) + "\n"


if __name__ == "__main__":
    import tempfile
    print(error_table(internal_shim.load(internal_shim.build(tempfile.mkdtemp()))))
