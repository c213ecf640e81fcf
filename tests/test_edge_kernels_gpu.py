"""The oldest entry points at their edge shapes, through the C ABI: kws_rmsprop_step, kws_sgd_momentum_step, kws_l2_loss,
kws_augment_f32/_i16, kws_tta_transform, kws_tta_combine, kws_head32to12, kws_transpose_f32 and kws_time_stretch_*.  Cases,
references, bounds and mutants are tests/edge_kernel_cases.py's (premises: tests/test_edge_kernel_cases_cpu.py).  Outputs and
in-place state are windows of sentinel-guarded allocations; device inputs stay referenced until the test has synchronised."""
import ctypes

import numpy as np
import pytest
import torch

import edge_kernel_cases as EC
from oracle import layers as OL
from oracle import stretch as OS
from speech_recognition_amd import _lib
from test_resblock_kernels_gpu import Guarded

pytestmark = pytest.mark.gpu

_KEEP = []


def dev(a):
    """upload (dtype kept); referenced until the end of the test - the library only borrows raw pointers"""
    t = torch.from_numpy(np.ascontiguousarray(a)).cuda()
    _KEEP.append(t)
    return t


def P(t, byte_offset=0):
    return None if t is None else ctypes.c_void_p(t.data_ptr() + byte_offset)


def S():
    return _lib.stream_ptr()


@pytest.fixture(autouse=True)
def _release_uploads():
    yield
    torch.cuda.synchronize()
    del _KEEP[:]


@pytest.fixture(scope="module", autouse=True)
def _need_gpu():
    assert torch.cuda.is_available(), "these tests need an MI355X"
    _lib.load()


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.int32)


# ------------------------------------------------------------------------------------------------------------------------------
# 1. RMSprop / SGD
# ------------------------------------------------------------------------------------------------------------------------------
def _opt_run(kind, n, gs):
    """OPT_STEPS steps on the device; the state is read back before each, so every step is judged on its own.
    Returns (inputs, [(before, after)])"""
    c = EC.opt_inputs(n)
    p, s = Guarded(n, init=c['p']), Guarded(n, init=c['acc'] if kind == 'rmsprop' else c['vel'])
    dl2, dgs = dev(c['l2']), [dev(g) for g in c['grads']]
    steps = []
    for t in range(EC.OPT_STEPS):
        before = (p.get(), s.get())
        if kind == 'rmsprop':
            _lib.call("kws_rmsprop_step", p.ptr(), P(dgs[t]), s.ptr(), P(dl2), n, EC.LR_RMS, EC.RHO, EC.EPS, gs, S())
        else:
            _lib.call("kws_sgd_momentum_step", p.ptr(), P(dgs[t]), s.ptr(), P(dl2), n, EC.LR_SGD, EC.MOM, gs, S())
        p.check(kind + " p")
        s.check(kind + " state")
        steps.append((before, (p.get(), s.get())))
    return c, steps


@pytest.mark.parametrize("n", EC.OPT_N)
@pytest.mark.parametrize("gs", EC.GRAD_SCALES)
@pytest.mark.parametrize("kind", ['rmsprop', 'sgd'])
def test_optimizer_steps_against_float64(kind, gs, n):
    c, steps = _opt_run(kind, n, gs)
    dead = c['regime'] == EC.DEAD
    worst_p = worst_s = 0.0
    for t, (before, after) in enumerate(steps):
        rp, rs, bad = EC.judge_step(kind, before, after, c['grads'][t], c['l2'], gs)
        worst_p, worst_s = max(worst_p, rp), max(worst_s, rs)
        assert np.isfinite(after[0]).all() and np.isfinite(after[1]).all(), t
        assert np.array_equal(bits(after[0][dead]), bits(before[0][dead])) and (after[1][dead] == 0).all(), t    # 0 / (0 + eps)
        if t == 0 and n == EC.MUTANT_N:
            for m in EC.mutants_of(kind, gs):
                out = EC.judge_step(kind, before, after, c['grads'][t], c['l2'], gs, mutant=m)[2]
                print("%s gs=%g mutant %s: %d elements outside" % (kind, gs, m, out))
                assert out >= EC.MUTANT_MIN, (m, out)
    print("%s n=%d gs=%g: largest error/bound p' %.3f, state %.3f" % (kind, n, gs, worst_p, worst_s))
    assert worst_p <= 1 and worst_s <= 1, (worst_p, worst_s)
    if n == EC.MUTANT_N:
        assert max(np.abs(a[0] - b[0]).max() for b, a in steps) > 1e-4               # it moved
    _, again = _opt_run(kind, n, gs)
    for (_, a), (_, b) in zip(steps, again):
        assert np.array_equal(bits(a[0]), bits(b[0])) and np.array_equal(bits(a[1]), bits(b[1]))


def test_misaligned_optimizer_pointers_are_refused():
    """rmsprop_kernel and adam_kernel use 16-byte accesses: a pointer off by one float is KWS_E_INVALID before any launch"""
    lib = _lib.load()
    n = 64
    bufs = [Guarded(n + 4) for _ in range(5)]
    for k in range(4):
        ptrs = [P(b.view, 4 if i == k else 0) for i, b in enumerate(bufs[:4])]
        assert lib.kws_rmsprop_step(ptrs[0], ptrs[1], ptrs[2], ptrs[3], n, 1e-3, 0.9, 1e-8, 1.0, S()) != 0
        assert b"aligned" in lib.kws_last_error()
    for k in range(5):
        ptrs = [P(b.view, 4 if i == k else 0) for i, b in enumerate(bufs)]
        assert lib.kws_adam_step(ptrs[0], ptrs[1], ptrs[2], ptrs[3], ptrs[4], n, 1e-3, 0.9, 0.999, 1e-8, 1.0, S()) != 0
        assert b"aligned" in lib.kws_last_error()
    assert all(b.untouched() for b in bufs)


# ------------------------------------------------------------------------------------------------------------------------------
# 2. l2 loss
# ------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("offset", [0, 1], ids=["aligned", "one_float_in"])
@pytest.mark.parametrize("n", EC.L2_N)
def test_l2_loss(n, offset):
    """offset 1: p and l2 are views one float into a larger allocation, the kernel's documented scalar path"""
    p, l2 = EC.l2_inputs(n)
    dp, dl = torch.zeros(n + 4, device="cuda"), torch.zeros(n + 4, device="cuda")
    dp[offset:offset + n].copy_(dev(p))
    dl[offset:offset + n].copy_(dev(l2))
    assert dp.data_ptr() % 16 == 0 and dl.data_ptr() % 16 == 0
    out = Guarded(1)
    _lib.call("kws_l2_loss", P(dp, 4 * offset), P(dl, 4 * offset), n, out.ptr(), S())
    out.check("l2_loss")
    got = float(out.get()[0])
    ref = EC.l2_ref(p, l2)
    print("l2_loss n=%d offset=%d: error/bound %.3f" % (n, offset, abs(got - ref) / EC.l2_bound(ref)))
    assert abs(got - ref) <= EC.l2_bound(ref)
    without = ref - float(l2[-1]) * float(p[-1]) ** 2
    assert abs(got - without) > EC.l2_bound(without)          # control: a sum that lost its last element


# ------------------------------------------------------------------------------------------------------------------------------
# 3. augment
# ------------------------------------------------------------------------------------------------------------------------------
def _augment(c, out_ptr):
    fn = "kws_augment_f32" if c['bank'].dtype == np.float32 else "kws_augment_i16"
    noise = None if c['noise'] is None else dev(c['noise'])
    off = None if c['off'] is None else dev(c['off'])
    return getattr(_lib.load(), fn)(P(dev(c['bank'])), c['n_clips'], c['L'], P(dev(c['idx'])), P(dev(c['fg'])), P(dev(c['shift'])),
                                    P(noise), c['noise_len'], P(off), P(dev(c['bgv'])), out_ptr, c['B'], S())


@pytest.mark.parametrize("bank_dtype", ['f32', 'i16'])
@pytest.mark.parametrize("L", EC.AUG_L)
def test_augment_every_path_bit_exact(L, bank_dtype):
    for variant in EC.AUG_VARIANTS:
        c = EC.augment_case(L, bank_dtype, variant)
        if c is None:
            continue
        out = Guarded(c['B'] * L)
        _lib.check(_augment(c, out.ptr()), "augment")
        out.check("augment %s L=%d" % (variant, L))            # (an odd L's last row is where a stray 16-byte store would show)
        got = out.get().reshape(c['B'], L)
        assert np.array_equal(got, EC.augment_case_ref(c)), variant
        if L >= 3:
            assert not np.array_equal(got, EC.augment_case_ref(c, reverse_roll=True)), variant


@pytest.mark.parametrize("bank_dtype", ['f32', 'i16'])
def test_augment_second_launch(bank_dtype):
    c = EC.augment_big_case(bank_dtype)
    out = Guarded(c['B'] * c['L'])
    _lib.check(_augment(c, out.ptr()), "augment")
    out.check("augment B=65538")
    got = out.get().reshape(c['B'], c['L'])
    ref = EC.augment_case_ref(c)
    assert np.array_equal(got[65535:], ref[65535:])            # the second launch's offset pointers
    assert np.array_equal(got, ref)
    assert not np.array_equal(got, EC.augment_case_ref(c, reverse_roll=True))


def test_augment_output_alignment():
    """L % 4 == 0 rows are written with 16-byte stores: an `out` off by one float is refused before any launch; rows of any
    other length take any float alignment"""
    c = EC.augment_case(8, 'f32', 'noise')
    out = Guarded(c['B'] * 8 + 4)
    assert _augment(c, P(out.view, 4)) != 0
    assert b"aligned" in _lib.load().kws_last_error()
    assert out.untouched()
    c = EC.augment_case(7, 'f32', 'noise')
    out = Guarded(c['B'] * 7 + 1)
    _lib.check(_augment(c, P(out.view, 4)), "augment")
    torch.cuda.synchronize()
    got = out.get()
    assert got.view(np.int32)[0] == 0x7FC0DEAD
    out.view[0] = 0.0
    out.check("augment into an odd float offset")
    assert np.array_equal(got[1:].reshape(c['B'], 7), EC.augment_case_ref(c))


# ------------------------------------------------------------------------------------------------------------------------------
# 4. TTA transform, combine, head
# ------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("L", EC.TTA_L)
def test_tta_transform_bit_exact(L):
    x = EC.tta_input(3, L)
    dx = dev(x)
    for kind in EC.TTA_KINDS:
        out = Guarded(3 * L)
        _lib.call("kws_tta_transform", P(dx), out.ptr(), 3, L, kind, S())
        out.check("tta_transform kind %d" % kind)
        assert np.array_equal(out.bits(), bits(OL.tta_transform(x, kind)).reshape(-1)), kind


def test_tta_transform_second_launch():
    B, L, kinds = EC.TTA_BIG
    x = EC.tta_input(B, L)
    dx = dev(x)
    for kind in kinds:
        out = Guarded(B * L)
        _lib.call("kws_tta_transform", P(dx), out.ptr(), B, L, kind, S())
        out.check("tta_transform B=65538")
        got, ref = out.bits().reshape(B, L), bits(OL.tta_transform(x, kind))
        assert np.array_equal(got[65535:], ref[65535:]) and np.array_equal(got, ref), kind


@pytest.mark.parametrize("n_terms,divisor", EC.COMBINE_TERMS)
def test_tta_combine_bit_exact(n_terms, divisor):
    for B in EC.COMBINE_B:
        for C in EC.COMBINE_C:
            terms, tie = EC.combine_case(n_terms, B, C)
            ref, am_ref = EC.combine_ref(terms, divisor)
            d = [dev(t) for t in terms]
            arr = (ctypes.c_void_p * n_terms)(*[t.data_ptr() for t in d])
            out, am = Guarded(B * C), Guarded(B)
            _lib.call("kws_tta_combine", arr, n_terms, divisor, out.ptr(), am.ptr(), B, C, S())
            out.check("tta_combine probabilities")
            am.check("tta_combine argmax")
            assert np.array_equal(out.bits(), bits(ref).reshape(-1)), (B, C)
            assert np.array_equal(am.bits(), am_ref), (B, C)
            if tie is not None:
                assert am.bits()[0] == tie[0]                  # the first index of a tie, as np.argmax
    # without the argmax output
    out = Guarded(B * C)
    _lib.call("kws_tta_combine", arr, n_terms, divisor, out.ptr(), None, B, C, S())
    out.check("tta_combine probabilities")
    assert np.array_equal(out.bits(), bits(ref).reshape(-1))


def test_tta_combine_and_head_refusals():
    lib = _lib.load()
    t = dev(np.zeros((4, 65), np.float32))
    arr = (ctypes.c_void_p * 9)(*[t.data_ptr()] * 9)
    out, am = Guarded(4 * 65), Guarded(4)
    mp = dev(np.zeros(65, np.int32))
    assert lib.kws_tta_combine(arr, 0, 1.0, out.ptr(), am.ptr(), 4, 12, S()) != 0
    assert lib.kws_tta_combine(arr, 9, 9.0, out.ptr(), am.ptr(), 4, 12, S()) != 0
    assert lib.kws_tta_combine(arr, 3, 0.0, out.ptr(), am.ptr(), 4, 12, S()) != 0
    assert lib.kws_head32to12(P(t), 65, P(mp), 65, out.ptr(), 4, S()) != 0
    assert out.untouched() and am.untouched()


@pytest.mark.parametrize("B", EC.HEAD_B)
@pytest.mark.parametrize("name", sorted(EC.HEAD_CASES))
def test_head(name, B):
    C_in, C_out, mp = EC.HEAD_CASES[name]
    p = EC.head_input(name, B)
    out = Guarded(B * C_out)
    _lib.call("kws_head32to12", P(dev(p)), C_in, P(dev(mp)), C_out, out.ptr(), B, S())
    out.check("head32to12")
    got = out.get().reshape(B, C_out)
    ref = EC.head_ref(p, mp, C_out)
    np.testing.assert_allclose(got, ref, rtol=EC.HEAD_RTOL, atol=0)
    if name == 'unmapped':
        assert (got[:, 3] == 0).all() and (got[:, [0, 1, 2, 4, 5]] > 0).all()
    if name != 'identity64':
        assert not np.allclose(got, EC.head_ref(p, mp, C_out, reduce='sum'), rtol=EC.HEAD_RTOL, atol=0)


# ------------------------------------------------------------------------------------------------------------------------------
# 5. transpose
# ------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("rows,cols", EC.TRANSPOSE_SHAPES)
def test_transpose_ragged_tiles(rows, cols):
    a = np.arange(rows * cols, dtype=np.float32).reshape(rows, cols)
    out = Guarded(rows * cols)
    _lib.call("kws_transpose_f32", P(dev(a)), out.ptr(), rows, cols, S())
    out.check("transpose")
    assert np.array_equal(out.get().reshape(cols, rows), a.T)


# ------------------------------------------------------------------------------------------------------------------------------
# 6. time stretch at short clips
# ------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("rate", EC.STRETCH_RATES)
@pytest.mark.parametrize("L", EC.STRETCH_L)
def test_stretch_short_clips(L, rate):
    lib = _lib.load()
    pcm = EC.stretch_pcm(L)
    x = EC.stretch_float(pcm)
    ref = EC.stretch_ref(L, rate)
    T = EC.stretch_steps(L, rate)
    Ltrim = OS.HOP * (T - 1)
    plan = ctypes.c_void_p()
    _lib.check(lib.kws_stretch_plan_create(L, rate, ctypes.byref(plan)), "kws_stretch_plan_create")
    try:
        assert lib.kws_stretch_out_samples(plan) == OS.stretched_length(L, rate) == Ltrim
        dx, dpcm = dev(x), dev(pcm)
        worst = 0.0
        for keep in EC.stretch_keeps(Ltrim):
            n = min(keep, Ltrim)
            want = np.stack([EC.stretch_want(ref[b], keep) for b in range(3)])
            out = Guarded(3 * keep)
            _lib.call("kws_time_stretch_f32", plan, P(dx), 1.0, out.ptr(), 3, keep, 0, S())
            out.check("time_stretch_f32 keep=%d" % keep)
            got = out.get().reshape(3, keep)
            err = np.abs(got - want).max()
            worst = max(worst, err)
            assert err < EC.STRETCH_ATOL, (keep, err)
            assert (got[2] == 0).all() and (got[:, n:] == 0).all()        # silence and the zero fill are exact
            if Ltrim:
                for b in range(2):                                          # control: one sample late
                    assert np.abs(got[b] - np.roll(want[b], 1)).max() > EC.STRETCH_ATOL
            else:
                assert keep == 64 and (got == 0).all()
            # int16 input: (float)pcm / 32767 on the device is the division the host made for the f32 path - the same bits
            out16 = Guarded(3 * keep)
            _lib.call("kws_time_stretch_i16", plan, P(dpcm), out16.ptr(), 3, keep, 0, S())
            out16.check("time_stretch_i16 keep=%d" % keep)
            assert np.array_equal(out16.bits(), out.bits())
            # the wav round trip: truncation to int16 / 32767 steps, read back / 32768
            q, q16 = Guarded(3 * keep), Guarded(3 * keep)
            _lib.call("kws_time_stretch_f32", plan, P(dx), 1.0, q.ptr(), 3, keep, 1, S())
            _lib.call("kws_time_stretch_i16", plan, P(dpcm), q16.ptr(), 3, keep, 1, S())
            q.check("time_stretch_f32 quantized")
            q16.check("time_stretch_i16 quantized")
            gq = q.get().reshape(3, keep)
            assert np.abs(gq - EC.stretch_want_quantized(want)).max() <= EC.LSB + 1e-9
            assert np.all(gq * 32768 == np.round(gq * 32768)) and (gq[2] == 0).all() and (gq[:, n:] == 0).all()
            assert np.array_equal(q16.bits(), q.bits())
        print("stretch L=%d rate=%g T=%d: largest error %.3g" % (L, rate, T, worst))
    finally:
        torch.cuda.synchronize()
        lib.kws_stretch_plan_destroy(plan)
