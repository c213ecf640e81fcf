"""kws_adam_step (csrc/optim.hip) against the float64 Keras-2.1.2 rule of tests/adam_oracle.py, and Adam through DeviceNet /
keras_api.Model: the second moment is allocated on first use, a training run reduces its loss, and a checkpoint carries both
moments and `iterations` (save -> load -> one more step equals the uninterrupted run bit for bit)."""
import numpy as np
import pytest
import torch

import adam_oracle as SO
from speech_recognition_amd import _lib
from speech_recognition_amd.keras_api import Adam, Model, RMSprop
from speech_recognition_amd.net import DeviceNet

pytestmark = pytest.mark.gpu

GUARD = 1024
SENT = 0x7FC0DEAD
# the kernel's constants are float32 (as Keras' backend variables are): 1 - float32(0.999) is 1.3e-5 away from 0.001 in relative
# terms, which the second moment shows.  The oracle is given the float32 values of the betas, so that it states the same rule.
B1, B2 = float(np.float32(0.9)), float(np.float32(0.999))


@pytest.fixture(scope="module", autouse=True)
def _need_gpu():
    assert torch.cuda.is_available(), "these tests need an MI355X"
    _lib.load()


class Guarded(object):
    """an n-float window of a sentinel-filled allocation (tests/test_guards_gpu.py's method)"""

    def __init__(self, a):
        self.buf = torch.full((a.size + 2 * GUARD,), SENT, dtype=torch.int32, device="cuda")
        self.view = self.buf[GUARD:GUARD + a.size].view(torch.float32)
        self.view.copy_(torch.from_numpy(np.ascontiguousarray(a, np.float32)).cuda())

    def intact(self):
        torch.cuda.synchronize()
        return bool((self.buf[:GUARD] == SENT).all()) and bool((self.buf[-GUARD:] == SENT).all())


def _run(n, with_l2, grad_scale, steps=10, lr=3e-4, seed=11, bias_correction=True):
    rng = np.random.RandomState(seed)
    p = (0.5 * rng.randn(n)).astype(np.float32)
    l2 = np.where(rng.rand(n) < 0.5, 1e-5 if with_l2 else 0.0, 0.0).astype(np.float32)   # (the same draws either way)
    grads = [(1e-2 * rng.randn(n) * (1.0 + t)).astype(np.float32) for t in range(steps)]
    dp, dm, dv = Guarded(p), Guarded(np.zeros(n)), Guarded(np.zeros(n))
    dl2 = torch.from_numpy(l2).cuda()
    dgs = [torch.from_numpy(g).cuda() for g in grads]
    rp, rm, rv = p.astype(np.float64), np.zeros(n), np.zeros(n)
    for t in range(1, steps + 1):
        _lib.call("kws_adam_step", _lib.ptr(dp.view), _lib.ptr(dgs[t - 1]), _lib.ptr(dm.view), _lib.ptr(dv.view), _lib.ptr(dl2),
                  n, SO.adam_lr_t(lr, t, B1, B2) if bias_correction else lr, 0.9, 0.999, 1e-8, grad_scale, _lib.stream_ptr())
        geff = grads[t - 1].astype(np.float64) * grad_scale + 2.0 * l2.astype(np.float64) * rp
        rp, rm, rv = SO.adam_step(rp, geff, rm, rv, lr, t, B1, B2)
    assert dp.intact() and dm.intact() and dv.intact(), "adam_kernel wrote outside its buffers"
    return (dp.view.cpu().numpy(), dm.view.cpu().numpy(), dv.view.cpu().numpy()), (rp, rm, rv)


@pytest.mark.parametrize("n", [100003, 1200001, 7, 2])
@pytest.mark.parametrize("with_l2,grad_scale", [(False, 1.0), (True, 1.0), (True, 0.125)])
def test_adam_kernel_ten_steps_against_float64(n, with_l2, grad_scale):
    """Ten consecutive updates on the device against ten float64 updates from the same start; n is not a multiple of 4 (the
    scalar tail runs), 1,200,001 is about the size of the flagship's parameter buffer (1,191,436 floats).  Bar for the updated weights: 2e-6 absolute, the
    bar of the RMSprop / SGD weight checks of tests/test_net_gpu.py.  Why it holds for ten steps: weights
    are drawn at 0.5 * randn (|p| < 4: a float32 rounding of p is at most 2.4e-7 per step, ten of them in the worst case 2.4e-6
    and, being independent, about 4e-7 in practice), and the update lr_t m / (sqrt(v) + eps) is at most a few lr = 3e-4 in size,
    so a relative error of a few ulp in it is below 1e-9.  Moments: relative 2e-6 (a handful of float32 roundings per step,
    damped by beta), the first moment with an absolute floor of 1e-7 (its terms cancel; |g| < 0.6).  Two runs give
    the same bits."""
    assert n % 4 != 0
    (p, m, v), (rp, rm, rv) = _run(n, with_l2, grad_scale)
    err = np.abs(p - rp).max()
    print("adam n=%d l2=%d gs=%g: max |p - p64| = %.3g" % (n, with_l2, grad_scale, err))
    assert err < 2e-6, err
    np.testing.assert_allclose(m, rm, rtol=2e-6, atol=1e-7)      # |g| < 0.6: <= 3 roundings of 0.6 x 2^-24 per step
    np.testing.assert_allclose(v, rv, rtol=2e-6, atol=1e-14)
    (p2, m2, v2), _ = _run(n, with_l2, grad_scale)
    assert np.array_equal(p, p2) and np.array_equal(m, m2) and np.array_equal(v, v2)


def test_adam_kernel_moves_and_negative_controls():
    """the same bar must break for a wrong rule: torch's placement of epsilon is indistinguishable at these gradient sizes (by
    design: both are Adam), but an update without the L2 term, without grad_scale, or with lr in place of lr_t is not"""
    n = 100003
    (p, _, _), (rp, _, _) = _run(n, True, 0.125, steps=3)
    assert np.abs(p - rp).max() < 2e-6
    rng = np.random.RandomState(11)
    p0 = (0.5 * rng.randn(n)).astype(np.float32)
    assert np.abs(p - p0).max() > 5e-4                # three steps of about lr each
    (pn, _, _), _ = _run(n, False, 0.125, steps=3)    # no L2 term on the device, oracle of the run above
    assert np.abs(pn - rp).max() > 2e-6
    (pg, _, _), _ = _run(n, True, 1.0, steps=3)
    assert np.abs(pg - rp).max() > 2e-6
    (pl, _, _), _ = _run(n, True, 0.125, steps=3, bias_correction=False)    # lr handed over in place of lr_t
    assert np.abs(pl - rp).max() > 2e-6


def test_bad_arguments_are_refused():
    t = torch.zeros(8, device="cuda")
    with pytest.raises(_lib.KwsError):
        _lib.call("kws_adam_step", _lib.ptr(t), _lib.ptr(t), _lib.ptr(t), _lib.ptr(t), _lib.ptr(t), 8, 1e-3, 0.9, 0.999, 1e-8,
                  1.0, _lib.stream_ptr())          # m and v must be two buffers
    with pytest.raises(_lib.KwsError):
        _lib.call("kws_adam_step", _lib.ptr(t), _lib.ptr(t), None, _lib.ptr(t), _lib.ptr(t), 8, 1e-3, 0.9, 0.999, 1e-8, 1.0,
                  _lib.stream_ptr())


# ------------------------------------------------------------------------------------------------------------------------------
# through DeviceNet and keras_api.Model (the time-sliced attention program: any network program takes any optimizer)
# ------------------------------------------------------------------------------------------------------------------------------
def _batch(B, num_classes, seed, L=16000):
    rng = np.random.RandomState(seed)
    t = np.arange(L) / 16000.0
    lab = rng.randint(0, num_classes, B)
    x = rng.randn(B, L) * 0.0774 + 0.05 * np.sin(2 * np.pi * 200.0 * (1 + lab)[:, None] * t[None])
    return x.astype(np.float32), np.eye(num_classes, dtype=np.float32)[lab]


def test_second_moment_is_allocated_on_first_use_only():
    net = DeviceNet(_lib.KWS_NET_TS_ATTENTION, 12)
    x, y = _batch(4, 12, 1)
    net.train_fwd_bwd(torch.from_numpy(x).cuda(), torch.from_numpy(y).cuda(), seed=1, step=0)
    net.rmsprop_step(1e-3)
    net.sgd_step(1e-3)
    assert net.slots2 is None                         # RMSprop / SGD nets keep their memory
    net.adam_step(SO.adam_lr_t(3e-4, 1))
    assert net.slots2 is not None and net.slots2.shape == net.slots.shape and float(net.slots2.abs().max()) > 0
    net.initialize()
    assert float(net.slots.abs().max()) == 0 and float(net.slots2.abs().max()) == 0


def test_device_net_adam_step_follows_the_keras_rule():
    """new weights = the Keras rule applied to the device's own gradient + 2 l2 w, 2e-6 (tests/test_net_gpu.py's check).  The
    moments element-wise: each is a sum of float32 terms rounded a few times, so |error| <= 4 x 2^-24 x the sum of the terms'
    magnitudes (the gradient and the L2 term can cancel: the bar is on the terms, not on the result)."""
    net = DeviceNet(_lib.KWS_NET_TS_ATTENTION, 12)
    m0 = v0 = np.zeros(net.n_params)
    U = 2.0 ** -24
    for t in range(1, 4):
        x, y = _batch(8, 12, 20 + t)
        net.train_fwd_bwd(torch.from_numpy(x).cuda(), torch.from_numpy(y).cuda(), seed=4, step=t)
        p0 = net.params.cpu().numpy().astype(np.float64)
        g0, reg = net.grads.cpu().numpy().astype(np.float64), 2.0 * net.l2.cpu().numpy().astype(np.float64) * p0
        net.adam_step(SO.adam_lr_t(3e-4, t, B1, B2))
        ref, m1, v1 = SO.adam_step(p0, g0 + reg, m0, v0, 3e-4, t, B1, B2)
        assert np.abs(net.params.cpu().numpy() - ref).max() < 2e-6, t
        gmag = np.abs(g0) + np.abs(reg)
        dm, dv = net.slots.cpu().numpy().astype(np.float64), net.slots2.cpu().numpy().astype(np.float64)
        assert (np.abs(dm - m1) <= 4 * U * (gmag + np.abs(m0)) + 1e-30).all(), t
        assert (np.abs(dv - v1) <= 8 * U * (gmag * gmag + v0) + 1e-38).all(), t
        m0, v0 = dm, dv


def test_model_with_adam_trains_and_checkpoints(tmp_path):
    def make():
        return Model(DeviceNet(_lib.KWS_NET_TS_ATTENTION, 12), Adam(lr=3e-4), name='adam_test')
    a = make()
    batches = [_batch(32, 12, 100)] * 12 + [_batch(32, 12, 101)]      # a fixed batch, as the test_speech_model_trains tests
    losses = [a.train_on_batch(*batches[i])[0] for i in range(12)]
    assert a.optimizer.iterations == 12
    assert np.isfinite(losses).all() and min(losses[2:]) < losses[0], losses
    path = str(tmp_path / "adam.npz")
    a.save(path)
    with np.load(path) as z:
        assert '__optimizer_slots_2__' in z.files and int(z['__optimizer_scalars__'][0]) == 12
    b = make()
    b.load_weights(path)
    assert b.optimizer.iterations == 12 and b._step == 12
    assert torch.equal(a.net.slots, b.net.slots) and torch.equal(a.net.slots2, b.net.slots2)
    la = a.train_on_batch(*batches[12])
    lb = b.train_on_batch(*batches[12])
    assert la == lb
    assert torch.equal(a.net.params, b.net.params) and torch.equal(a.net.state, b.net.state)
    assert torch.equal(a.net.slots, b.net.slots) and torch.equal(a.net.slots2, b.net.slots2)
    # `iterations` matters: the same file loaded with the counter wound back takes a different step
    c = make()
    c.load_weights(path)
    c.optimizer.iterations = 0
    c.train_on_batch(*batches[12])
    assert not torch.equal(a.net.params, c.net.params)


def _strip(src, dst, drop):
    with np.load(src) as z:
        blob = {k: z[k] for k in z.files if k not in drop}
    with open(dst, 'wb') as f:
        np.savez(f, **blob)


def test_checkpoints_of_another_optimizer(tmp_path):
    """The file records the optimizer.  State that does not fit is not reused (Adam's first moment is no RMSprop accumulator):
    the weights load, the optimizer starts fresh, a warning says so - in both directions.  A file without the record (written
    before it existed) that lacks a piece of Adam's state is refused with a ValueError that names the piece."""
    x, y = _batch(16, 12, 7)
    adam = Model(DeviceNet(_lib.KWS_NET_TS_ATTENTION, 12), Adam(lr=3e-4))
    rms = Model(DeviceNet(_lib.KWS_NET_TS_ATTENTION, 12), RMSprop())
    for m in (adam, rms):
        m.train_on_batch(x, y)
        m.train_on_batch(x, y)
    apath, rpath = str(tmp_path / "adam.npz"), str(tmp_path / "rms.npz")
    adam.save(apath)
    rms.save(rpath)
    with np.load(apath) as z:
        assert str(z['__optimizer__']) == 'Adam'
    with np.load(rpath) as z:
        assert str(z['__optimizer__']) == 'RMSprop'
        assert '__optimizer_slots_2__' not in z.files and '__optimizer_scalars__' not in z.files
    # RMSprop file -> Adam model
    m = Model(DeviceNet(_lib.KWS_NET_TS_ATTENTION, 12), Adam(lr=3e-4))
    m.train_on_batch(x, y)                            # leaves state behind that must not survive the load
    with pytest.warns(UserWarning, match="RMSprop"):
        m.load_weights(rpath)
    assert torch.equal(m.net.params, rms.net.params) and torch.equal(m.net.state, rms.net.state)
    assert m.optimizer.iterations == 0 and m._step == 2
    assert float(m.net.slots.abs().max()) == 0 and float(m.net.slots2.abs().max()) == 0
    assert abs(float(m.optimizer.lr) - 3e-4) < 1e-9   # the model's own lr, not the file's 1e-3
    # Adam file -> RMSprop model
    m = Model(DeviceNet(_lib.KWS_NET_TS_ATTENTION, 12), RMSprop())
    with pytest.warns(UserWarning, match="Adam"):
        m.load_weights(apath)
    assert torch.equal(m.net.params, adam.net.params) and float(m.net.slots.abs().max()) == 0 and m.net.slots2 is None
    # files without the record
    for drop, word in ((('__optimizer__', '__optimizer_slots_2__'), '__optimizer_slots_2__'),
                       (('__optimizer__', '__optimizer_scalars__'), '__optimizer_scalars__')):
        lpath = str(tmp_path / "legacy.npz")
        _strip(apath, lpath, drop)
        with pytest.raises(ValueError, match=word):
            Model(DeviceNet(_lib.KWS_NET_TS_ATTENTION, 12), Adam()).load_weights(lpath)
    lpath = str(tmp_path / "legacy_ok.npz")
    _strip(apath, lpath, ('__optimizer__',))
    m = Model(DeviceNet(_lib.KWS_NET_TS_ATTENTION, 12), Adam())
    m.load_weights(lpath)
    assert m.optimizer.iterations == 2 and torch.equal(m.net.slots2, adam.net.slots2)
