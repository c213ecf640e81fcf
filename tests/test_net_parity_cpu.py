"""tests/net_parity.py's checkers refuse what they should: the ten family model files assert through check_train_step, so it is
the one thing between the device and the oracle.  Hand-made arrays and a stub holding `state`; no device, no oracle net."""
import copy
from types import SimpleNamespace

import numpy as np
import pytest

import net_parity as NP

BARS = NP.FAMILY_BARS
B, NC = 4, 3
MEAN, VAR = 'batch_normalization_1/moving_mean', 'batch_normalization_1/moving_variance'


def _case():
    """A three-tensor reference, the oracle stub and device data equal to the reference.  Row 3's two leading classes tie."""
    p = np.array([[0.7, 0.2, 0.1], [0.1, 0.6, 0.3], [0.2, 0.3, 0.5], [0.4, 0.4, 0.2]])
    y = np.eye(NC, dtype=np.float32)[[0, 1, 0, 0]]
    rng = np.random.RandomState(0)
    grads = {'conv1d_1/kernel': rng.randn(3, 2, 4), 'batch_normalization_1/gamma': 1e-3 * rng.randn(4), 'dense_1/bias': rng.randn(NC)}
    ora = SimpleNamespace(state={MEAN: rng.randn(4).astype(np.float32), VAR: (1 + rng.rand(4)).astype(np.float32)})
    mean, var = rng.randn(4), 1 + rng.rand(4)
    loss = 0.8125
    ref = (loss, p, grads, {'batch_stats': {1: (mean, var)}})
    weights = {k: ora.state[k].astype(np.float64) - (ora.state[k].astype(np.float64) - b) * 0.01 for k, b in ((MEAN, mean), (VAR, var))}
    dev = {'probs': p.astype(np.float32), 'metrics': np.array([B * loss, 3.0], np.float32),
           'grads': {k: v.astype(np.float32) for k, v in grads.items()}, 'weights': {k: v.astype(np.float32) for k, v in weights.items()}}
    return dev, y, ref, ora


def _grad(dev, name, delta):
    """The gradient element of largest magnitude moved by delta of the tensor's maximum"""
    g = dev['grads'][name]
    i = np.unravel_index(np.abs(g).argmax(), g.shape)
    g[i] += np.float32(delta) * g[i]


def _prob(dev, delta):
    dev['probs'][1, 2] += np.float32(delta)


def _loss(dev, delta):
    dev['metrics'][0] += np.float32(B * delta)


def _moving(dev, name, delta):
    dev['weights'][name][2] += np.float32(delta)


def _swap_tied_argmax(dev):
    dev['probs'][3, 0] -= np.float32(1e-6)       # far inside the 5e-5 bar, but class 1 now leads row 3 on the device


WRONG = {
    'probability off by 6e-5': lambda d: _prob(d, 6e-5),
    'mean loss off by 2e-4': lambda d: _loss(d, 2e-4),
    'correct count off by one': lambda d: d['metrics'].__setitem__(1, 2.0),
    'gradient element off by 3e-4 of the maximum': lambda d: _grad(d, 'batch_normalization_1/gamma', 3e-4),
    'gradient tensor missing': lambda d: d['grads'].pop('dense_1/bias'),
    'moving mean off by 1e-4': lambda d: _moving(d, MEAN, 1e-4),
    'moving variance off by 1e-4': lambda d: _moving(d, VAR, 1e-4),
    'argmax swapped at equal probabilities': _swap_tied_argmax,
}
# just under the bars: 5e-5, 1e-4, 2e-4 of the maximum, atol 5e-6 + rtol 1e-5 |reference|
ALLOWED = {
    'probability off by 4e-5': lambda d: _prob(d, 4e-5),
    'mean loss off by 8e-5': lambda d: _loss(d, 8e-5),
    'gradient element off by 1.8e-4 of the maximum': lambda d: _grad(d, 'batch_normalization_1/gamma', 1.8e-4),
    'moving mean off by 4e-6': lambda d: _moving(d, MEAN, 4e-6),
    'moving variance off by 4e-6': lambda d: _moving(d, VAR, 4e-6),
}


def test_the_family_bars_are_the_named_five():
    assert BARS == {'predict': 2e-5, 'train_probs': 5e-5, 'loss': 1e-4, 'grad': 2e-4, 'moving_mean': (5e-6, 1e-5),
                    'moving_variance': (5e-6, 1e-5)}


def test_check_train_step_passes_device_data_equal_to_the_reference(capsys):
    dev, y, ref, ora = _case()
    errs = NP.check_train_step(dev, y, ref, ora, BARS, 'stub B=4')
    assert list(errs) == list(ref[2]) and max(errs.values()) < 1e-6
    assert capsys.readouterr().out.startswith("train stub B=4: probs ")


@pytest.mark.parametrize("what", list(WRONG))
def test_check_train_step_refuses(what):
    dev, y, ref, ora = _case()
    WRONG[what](dev)
    with pytest.raises((AssertionError, KeyError)):
        NP.check_train_step(dev, y, ref, ora, BARS, what)


@pytest.mark.parametrize("what", list(ALLOWED))
def test_check_train_step_allows_just_under_the_bar(what):
    dev, y, ref, ora = _case()
    before = copy.deepcopy(dev)
    ALLOWED[what](dev)
    assert any(not np.array_equal(dev[k], before[k]) for k in ('probs', 'metrics')) or \
        any(not np.array_equal(dev[s][k], before[s][k]) for s in ('grads', 'weights') for k in dev[s])
    NP.check_train_step(dev, y, ref, ora, BARS, what)


def test_bars_without_the_moving_variance_leave_it_unchecked():
    """the residual family's entrance: check_residual_step names the moving mean only"""
    dev, y, ref, ora = _case()
    _moving(dev, VAR, 1e-4)
    bars = {k: v for k, v in BARS.items() if k != 'moving_variance'}
    NP.check_train_step(dev, y, ref, ora, bars, 'no variance')
    _moving(dev, MEAN, 1e-4)
    with pytest.raises(AssertionError):
        NP.check_train_step(dev, y, ref, ora, bars, 'no variance')


def test_check_predict():
    ref = np.array([[0.7, 0.2, 0.1], [0.25, 0.35, 0.4]])
    p = ref.astype(np.float32)
    p[0, 1] += np.float32(1.5e-5)
    NP.check_predict(p, ref, BARS, 'stub')
    p[0, 1] += np.float32(1e-5)
    with pytest.raises(AssertionError):
        NP.check_predict(p, ref, BARS, 'stub')
    tied = np.array([[0.4, 0.4, 0.2]])
    with pytest.raises(AssertionError):
        NP.check_predict(np.array([[0.4 - 1e-6, 0.4, 0.2]], np.float32), tied, BARS, 'stub')


def test_grad_errors():
    ref = {'a': np.array([[1.0, -4.0], [2.0, 0.5]]), 'zero': np.zeros(3)}
    g = {'a': np.array([1.0, -4.0, 2.0 + 4e-4, 0.5], np.float32), 'zero': np.array([0.0, 1e-8, 0.0], np.float32), 'extra': np.ones(2)}
    errs = NP.grad_errors(g, ref)
    assert list(errs) == ['a', 'zero']                                # the reference names the tensors; g['a'] gives the shape
    assert abs(errs['a'] - 1e-4) < 1e-6                               # 4e-4 of a maximum of 4
    assert abs(errs['zero'] - 0.1) < 1e-6                             # 1e-8 over the 1e-7 floor
    assert max(errs.values()) > BARS['grad'] > errs['a']
    with pytest.raises(KeyError):
        NP.grad_errors({'a': g['a']}, ref)
