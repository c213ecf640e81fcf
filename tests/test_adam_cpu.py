"""CPU checks of the Adam oracle (tests/adam_oracle.py) and of the host side of keras_api.Adam.  No GPU."""
import os
import re

import numpy as np
import pytest
import torch

import adam_oracle as SO
from speech_recognition_amd import _lib, keras_api


# ------------------------------------------------------------------------------------------------------------------------------
# Adam
# ------------------------------------------------------------------------------------------------------------------------------
def test_adam_oracle_matches_hand_unrolled_three_steps():
    """one scalar parameter, three gradients, every intermediate written out (Keras 2.1.2 get_updates)"""
    lr, b1, b2, eps = 1e-3, 0.9, 0.999, 1e-8
    gs = [0.5, -0.25, 2.0]
    p0 = 1.0
    m1 = 0.1 * 0.5
    v1 = 0.001 * 0.25
    p1 = p0 - lr * np.sqrt(1 - b2) / (1 - b1) * m1 / (np.sqrt(v1) + eps)
    m2 = 0.9 * m1 + 0.1 * -0.25
    v2 = 0.999 * v1 + 0.001 * 0.0625
    p2 = p1 - lr * np.sqrt(1 - b2 ** 2) / (1 - b1 ** 2) * m2 / (np.sqrt(v2) + eps)
    m3 = 0.9 * m2 + 0.1 * 2.0
    v3 = 0.999 * v2 + 0.001 * 4.0
    p3 = p2 - lr * np.sqrt(1 - b2 ** 3) / (1 - b1 ** 3) * m3 / (np.sqrt(v3) + eps)
    p, m, v = np.array([p0]), np.zeros(1), np.zeros(1)
    for t, g in enumerate(gs, 1):
        p, m, v = SO.adam_step(p, np.array([g]), m, v, lr, t, b1, b2, eps)
    assert abs(p[0] - p3) < 1e-15 and abs(m[0] - m3) < 1e-15 and abs(v[0] - v3) < 1e-15
    # the first step of Adam moves by lr * sign(g) (up to eps), whatever the gradient's size
    assert abs((p0 - p1) - lr) < 1e-9


def test_adam_oracle_matches_torch_with_eps_zero():
    """torch.optim.Adam divides by sqrt(v) / sqrt(1 - b2^t) + eps, Keras by sqrt(v) + eps: with eps = 0 the two are the same
    rule.  Gradients are bounded away from zero so that sqrt(v) is."""
    rng = np.random.RandomState(5)
    n = 1000
    p0 = rng.randn(n)
    tp = torch.nn.Parameter(torch.from_numpy(p0.copy()))
    opt = torch.optim.Adam([tp], lr=3e-4, betas=(0.9, 0.999), eps=0.0)
    p, m, v = p0.copy(), np.zeros(n), np.zeros(n)
    for t in range(1, 21):
        g = rng.choice([-1.0, 1.0], n) * (0.1 + rng.rand(n))
        tp.grad = torch.from_numpy(g.copy())
        opt.step()
        p, m, v = SO.adam_step(p, g, m, v, 3e-4, t, eps=0.0)
        assert np.abs(tp.detach().numpy() - p).max() < 1e-12, t


def test_adam_oracle_eps_sits_beside_the_uncorrected_root():
    """what separates the Keras rule from torch's: at t = 1 and a gradient of the size of eps the two steps differ by far"""
    g = np.array([1e-8])
    p, _, _ = SO.adam_step(np.zeros(1), g, np.zeros(1), np.zeros(1), 1e-3, 1, eps=1e-8)
    keras = -1e-3 * np.sqrt(1 - 0.999) / 0.1 * (0.1 * 1e-8) / (np.sqrt(0.001) * 1e-8 + 1e-8)
    torch_rule = -1e-3 * 1e-8 / (1e-8 + 1e-8)
    assert abs(p[0] - keras) < 1e-18
    assert abs(p[0] - torch_rule) > 1e-4


def test_keras_adam_host_side():
    opt = keras_api.Adam(lr=3e-4)
    assert isinstance(opt, keras_api.Optimizer)
    assert (opt.beta_1, opt.beta_2, opt.epsilon, opt.iterations) == (0.9, 0.999, 1e-8, 0)
    assert opt.lr.value == np.float32(3e-4)
    assert abs(opt.step_size() - SO.adam_lr_t(float(np.float32(3e-4)), 1)) < 1e-18

    class Net(object):
        calls = []

        def adam_step(self, *a):
            self.calls.append(a)

    net = Net()
    for t in range(1, 4):
        opt.apply(net, 1.0)
        assert opt.iterations == t
        assert abs(net.calls[-1][0] - SO.adam_lr_t(float(np.float32(3e-4)), t)) < 1e-18
        assert net.calls[-1][1:5] == (0.9, 0.999, 1e-8, 1.0)
    # ReduceLROnPlateau writes optimizer.lr.value: the next step size follows it
    opt.lr.value = np.float32(1e-4)
    assert abs(opt.step_size() - SO.adam_lr_t(float(np.float32(1e-4)), 4)) < 1e-18
    assert opt.get_scalars() == [3]
    opt.set_scalars([7])
    assert opt.iterations == 7
    with pytest.raises(NotImplementedError):
        keras_api.Adam(decay=1e-4)
    with pytest.raises(NotImplementedError):
        keras_api.Adam(amsgrad=True)
    # the siblings carry no state beyond net.slots and lr
    assert keras_api.RMSprop().get_scalars() == [] and keras_api.SGD().extra_slots(None) == []


def test_new_entry_points_are_declared(repo_root):
    hdr = open(os.path.join(repo_root, "include", "kws_hip.h")).read()
    assert re.search(r"\bkws_adam_step\s*\(", hdr)
    assert "kws_adam_step" in _lib.SIGNATURES
    assert len(_lib.SIGNATURES["kws_adam_step"][1]) == 12
    assert _lib.ABI_VERSION == 5                      # additive: no version step
