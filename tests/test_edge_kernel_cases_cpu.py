"""The premises of tests/test_edge_kernels_gpu.py, checked without a GPU: every reference of tests/edge_kernel_cases.py agrees
with the project's oracle where both apply, a float32 NumPy evaluation lies inside every derived bound, and every mutant
reference lies outside it."""
import numpy as np
import pytest

import edge_kernel_cases as EC
from oracle import features as OF
from oracle import layers as OL
from oracle import stretch as OS


# ------------------------------------------------------------------------------------------------------------------------------
# 1. optimizers
# ------------------------------------------------------------------------------------------------------------------------------
def _emulate(kind, n, gs):
    """OPT_STEPS float32 steps, each judged as the GPU test judges the device's: yields (step, before, after, grad, l2)"""
    c = EC.opt_inputs(n)
    step = EC.rmsprop_f32 if kind == 'rmsprop' else EC.sgd_f32
    state = (c['p'], c['acc'] if kind == 'rmsprop' else c['vel'])
    for t in range(EC.OPT_STEPS):
        after = step(state[0], c['grads'][t], state[1], c['l2'], gs)
        assert after[0].dtype == np.float32 and after[1].dtype == np.float32
        yield t, state, after, c['grads'][t], c['l2'], c['regime']
        state = after


def test_optimizer_inputs_hold_every_regime():
    for n in EC.OPT_N:
        c = EC.opt_inputs(n)
        r = c['regime']
        assert list(r[:4]) == [EC.DEAD, EC.TINY, EC.ORDINARY, EC.SMALL][:n]
        dead, tiny = r == EC.DEAD, r == EC.TINY
        assert all((g[dead] == 0).all() for g in c['grads']) and (c['acc'][dead | tiny] == 0).all()
        assert (c['vel'][dead | tiny] == 0).all() and (c['l2'][r != EC.ORDINARY] == 0).all()
        if tiny.any():                                   # sqrt(a') beside eps = 1e-8
            root = np.sqrt(0.1) * np.abs(c['grads'][0][tiny].astype(np.float64))
            assert np.median(root) < 1e-7 and root.max() < 1e-6
    c = EC.opt_inputs(EC.MUTANT_N)
    assert min((c['regime'] == k).sum() for k in range(4)) > 20000 and 10000 < (c['l2'] > 0).sum() < 15000
    assert set(np.unique(c['l2'])) == {np.float32(0), np.float32(1e-5)}


@pytest.mark.parametrize("gs", EC.GRAD_SCALES)
@pytest.mark.parametrize("kind", ['rmsprop', 'sgd'])
def test_float32_rule_lies_inside_the_bounds(kind, gs):
    worst = 0.0
    for n in EC.OPT_N:
        for t, before, after, grad, l2, regime in _emulate(kind, n, gs):
            rp, rs, bad = EC.judge_step(kind, before, after, grad, l2, gs)
            worst = max(worst, rp, rs)
            assert bad == 0 and rp <= 1 and rs <= 1, (n, t, rp, rs, bad)
            dead = regime == EC.DEAD
            assert np.array_equal(after[0][dead].view(np.int32), before[0][dead].view(np.int32))     # p' == p bitwise
            assert (after[1][dead] == 0).all() and np.isfinite(after[0]).all() and np.isfinite(after[1]).all()
    print("%s gs=%g: largest error/bound of the float32 rule %.3f" % (kind, gs, worst))


@pytest.mark.parametrize("gs", EC.GRAD_SCALES)
@pytest.mark.parametrize("kind", ['rmsprop', 'sgd'])
def test_every_mutant_lies_outside_the_bounds(kind, gs):
    t, before, after, grad, l2, _ = next(_emulate(kind, EC.MUTANT_N, gs))
    assert EC.judge_step(kind, before, after, grad, l2, gs)[2] == 0
    for m in EC.mutants_of(kind, gs):
        bad = EC.judge_step(kind, before, after, grad, l2, gs, mutant=m)[2]
        print("%s gs=%g mutant %s: %d elements outside" % (kind, gs, m, bad))
        assert bad >= EC.MUTANT_MIN, (m, bad)
    assert ('no_grad_scale' in EC.mutants_of(kind, gs)) == (gs != 1.0)


# ------------------------------------------------------------------------------------------------------------------------------
# 2. l2 loss
# ------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", EC.L2_N)
def test_l2_bound_and_control(n):
    p, l2 = EC.l2_inputs(n)
    ref = EC.l2_ref(p, l2)
    # the kernel's order: four float64 accumulators per thread of 1024, a tree over the threads, one cast
    terms = l2.astype(np.float64) * p.astype(np.float64) * p.astype(np.float64)
    lanes = np.zeros(4096)
    np.add.at(lanes, np.arange(n) % 4096, terms)
    got = np.float32(lanes.reshape(4, 1024).sum(0).sum())
    assert abs(float(got) - ref) <= EC.l2_bound(ref)
    without = ref - float(terms[-1])
    assert abs(float(got) - without) > EC.l2_bound(without)
    assert abs(float(np.float32(ref)) * (1 + 2e-7) - ref) > EC.l2_bound(ref)      # two units in the last place are outside


# ------------------------------------------------------------------------------------------------------------------------------
# 3. augment
# ------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("bank_dtype", ['f32', 'i16'])
@pytest.mark.parametrize("L", EC.AUG_L)
def test_augment_reference_is_the_oracle_where_both_apply(L, bank_dtype):
    for variant in EC.AUG_VARIANTS:
        c = EC.augment_case(L, bank_dtype, variant)
        if c is None:
            assert variant == 'short_noise' and L < 3
            continue
        ref = EC.augment_case_ref(c)
        assert ref.dtype == np.float32 and ref.shape == (c['B'], L) and np.isfinite(ref).all()
        bank_f = EC.bank_as_f32(c['bank'])
        if c['noise'] is None:
            rows = np.arange(c['B'])
            noise, off = np.zeros(L, np.float32), np.zeros(c['B'], np.int64)
        else:
            rows = np.nonzero((c['off'] >= 0) & (c['off'] + L <= c['noise_len']))[0]
            noise, off = c['noise'], c['off']
            assert (len(rows) >= 3) == (variant == 'noise')              # offsets 0, 3 and the exact fit are whole slices
            assert c['noise_len'] < L or variant == 'noise'
        if len(rows):
            want = OF.augment_batch(bank_f, c['idx'][rows], c['fg'][rows], c['shift'][rows], noise, off[rows], c['bgv'][rows],
                                    dtype=np.float32)
            assert np.array_equal(ref[rows].view(np.int32), want.view(np.int32))
        if L >= 3:                                                          # (at L = 1 every roll is the identity)
            assert not np.array_equal(ref, EC.augment_case_ref(c, reverse_roll=True))
        if bank_dtype == 'i16':
            assert c['bank'].min() == -32768 and c['bank'].max() == 32767
    c = EC.augment_case(L, bank_dtype, 'noise')
    nl = c['noise_len']
    assert set(c['off']) == {0, 3, nl - L, nl - L + 2, nl - 1, nl + 5, -3, -L - 1}
    assert (c['bgv'] == 0).any() and (c['bgv'] > 0).any() and (c['fg'] == 0).any() and (c['fg'] < 0).any() and (c['fg'] == 1).any()
    # a row that lies wholly outside the noise is the foreground alone
    r = int(np.nonzero(c['off'] == nl + 5)[0][0])
    alone = np.roll(EC.bank_as_f32(c['bank'])[c['idx'][r]] * c['fg'][r], int(c['shift'][r]))
    assert np.array_equal(EC.augment_case_ref(c)[r], alone)


@pytest.mark.parametrize("bank_dtype", ['f32', 'i16'])
def test_augment_big_reference(bank_dtype):
    c = EC.augment_big_case(bank_dtype)
    ref = EC.augment_case_ref(c)
    assert ref.shape == (65538, 8) and c['B'] > 65535 + 2
    for b in (0, 65534, 65535, 65536, 65537):
        o = int(c['off'][b])
        seg = np.array([c['noise'][o + t] if 0 <= o + t < c['noise_len'] else 0.0 for t in range(8)], np.float32)
        want = OF.augment(EC.bank_as_f32(c['bank'])[c['idx'][b]], c['fg'][b], c['shift'][b], seg, c['bgv'][b])
        assert np.array_equal(ref[b], want)
    assert len({ref[b].tobytes() for b in (65535, 65536, 65537, 0, 1, 2)}) == 6    # rows of the second launch are their own
    assert not np.array_equal(ref, EC.augment_case_ref(c, reverse_roll=True))


# ------------------------------------------------------------------------------------------------------------------------------
# 4. TTA transform, combine, head
# ------------------------------------------------------------------------------------------------------------------------------
def test_tta_specials_straddle_the_clip():
    sp = EC.tta_specials()
    assert len(set(sp.view(np.int32))) == 12
    y = OL.tta_transform(sp, 3)
    inside = np.abs(sp) < 1
    assert (np.abs(y[inside]) == 1).any() and (np.abs(y[inside]) < 1).any()      # the clip sets in between neighbouring floats
    seen = set()
    for L in EC.TTA_L:
        x = EC.tta_input(3, L)
        assert x.dtype == np.float32 and x.shape == (3, L)
        seen |= set(x.view(np.int32).reshape(-1)) & set(sp.view(np.int32))
        for kind in EC.TTA_KINDS:
            assert OL.tta_transform(x, kind).dtype == np.float32
        assert np.array_equal(OL.tta_transform(x, 1), x[:, (np.arange(L) + 1500) % L])
    assert len(seen) == 12


def test_combine_reference_ties_and_negative_rows():
    for n_terms, divisor in EC.COMBINE_TERMS:
        for B in EC.COMBINE_B:
            for C in EC.COMBINE_C:
                terms, tie = EC.combine_case(n_terms, B, C)
                ref, am = EC.combine_ref(terms, divisor)
                assert ref.shape == (B, C) and (ref[B - 1] < 0).all()
                assert np.allclose(ref, sum(t.astype(np.float64) for t in terms) / divisor, rtol=1e-6)
                if tie is not None:
                    assert ref[0, tie[0]] == ref[0, tie[1]] == ref[0].max() and am[0] == tie[0] < tie[1]
                    assert (ref[0] == ref[0].max()).sum() == 2
                if C >= 3:
                    assert am[0] != 0 and len(set(am)) > 1 or B == 1


def test_head_reference_is_the_oracle_on_the_real_map():
    for B in EC.HEAD_B:
        C_in, C_out, mp = EC.HEAD_CASES['real']
        p = EC.head_input('real', B)
        want = OL.head32to12(p.astype(np.float64), EC.ALL_CLASSES, EC.WANTED)
        assert np.allclose(EC.head_ref(p, mp, C_out), want, rtol=1e-14, atol=0)
        C_in, C_out, mp = EC.HEAD_CASES['unmapped']
        p = EC.head_input('unmapped', B)
        ref = EC.head_ref(p, mp, C_out)
        assert (ref[:, 3] == 0).all() and (ref[:, [0, 1, 2, 4, 5]] > 0).all() and np.allclose(ref.sum(1), 1)
        # the entries -1 and C_out are ignored: the same map without those inputs gives the same answer
        keep = [i for i, s in enumerate(mp) if 0 <= s < C_out]
        assert np.array_equal(ref, EC.head_ref(p[:, keep], mp[keep], C_out))
        for name in ('real', 'unmapped'):                # the control lies outside the bar
            C_in, C_out, mp = EC.HEAD_CASES[name]
            p = EC.head_input(name, B)
            assert not np.allclose(EC.head_ref(p, mp, C_out, reduce='sum'), EC.head_ref(p, mp, C_out), rtol=EC.HEAD_RTOL, atol=0)
    C_in, C_out, mp = EC.HEAD_CASES['identity64']
    assert C_out == 64 and np.allclose(EC.head_ref(EC.head_input('identity64', 1), mp, 64),
                                       OL.softmax(EC.head_input('identity64', 1).astype(np.float64)), rtol=1e-14)


# ------------------------------------------------------------------------------------------------------------------------------
# 6. stretch
# ------------------------------------------------------------------------------------------------------------------------------
def test_stretch_cases_cover_one_to_ten_steps():
    Ts = set()
    for L in EC.STRETCH_L:
        pcm = EC.stretch_pcm(L)
        assert pcm.dtype == np.int16 and (pcm[2] == 0).all() and (pcm[1, :600] == 0).all() and np.abs(pcm[0]).max() > 3000
        for rate in EC.STRETCH_RATES:
            T = EC.stretch_steps(L, rate)
            Ts.add(T)
            ref = EC.stretch_ref(L, rate)
            assert all(len(r) == OS.HOP * (T - 1) == OS.stretched_length(L, rate) for r in ref)
            assert (ref[2] == 0).all()
            Ltrim = OS.HOP * (T - 1)
            for keep in EC.stretch_keeps(Ltrim):
                for b in range(3):
                    want = EC.stretch_want(ref[b], keep)
                    n = min(keep, Ltrim)
                    assert len(want) == keep and (want[n:] == 0).all()
                    assert np.array_equal(want[:n], ref[b][Ltrim - n:])
                    if Ltrim and b < 2:                  # the control: one sample late is outside the bar
                        assert np.abs(np.roll(want, 1) - want).max() > 100 * EC.STRETCH_ATOL
            if rate == 1.0:                              # every step lands on a frame: the stretch is the identity
                x = EC.stretch_float(pcm).astype(np.float64)
                assert all(np.abs(ref[b] - x[b, :Ltrim]).max() < 1e-9 for b in range(3))
    assert Ts >= {1, 2, 3} and max(Ts) == 10 and min(Ts) == 1
