#!/usr/bin/env python
"""Layer structure of the reference's xception_with_attention_model (model.py:911-983), recorded BY RUNNING the reference's own model
builder.

Build container only (needs the reference checkout):   python tests/golden/make_golden_xception.py

The recording stand-ins for keras are make_golden_dwk.py's (depthwise blocks) and make_golden_gru.py's (GRU, Bidirectional) plus what
this model adds: the framing Lambda (tensorflow.extract_image_patches with SAME length arithmetic, K.int_shape, K.reshape), a Conv1D
that also takes padding='same' and strides, MaxPool1D with padding='same' (TensorFlow's left padding recorded next to it), Add and
Multiply (input shapes, broadcast output), a softmax that records the axis it is taken over inside its Lambda, a GRU and a Dense that
record their kernel_regularizer.  Names follow Keras 2.1's per-class auto-numbering in creation order; Bidirectional's weights are
bidirectional_<n>/forward_<gru name>/... then .../backward_<gru name>/...  No reference source text is stored:
tests/golden/xception_models.json holds the recorded structure only.
"""
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import make_golden_grouped as mg  # noqa: E402
import make_golden_dwk as md  # noqa: E402
import make_golden_gru as mgru  # noqa: E402

_softmax_axis = []


def softmax(x, axis=-1):
    _softmax_axis.append(axis)
    return mg.T(x.shape)


class Lambda(md.Lambda):
    def __call__(self, x):
        del _softmax_axis[:]
        out = md.Lambda.__call__(self, x)
        if _softmax_axis:
            self.rec['softmax_axis'] = _softmax_axis[0]
        return out


def _same(L, k, s):
    Lout = -(-L // s)
    total = max((Lout - 1) * s + k - L, 0)
    return Lout, total // 2, total


class Conv1D(md.Conv1D):
    def out_shape(self, x):
        filters, k = self.args[0], self.args[1]
        s = self.kwargs.get('strides', 1)
        pad = self.kwargs.get('padding', 'valid')
        assert self.kwargs.get('dilation_rate', 1) == 1
        L = x.shape[0]
        if pad == 'same':
            Lout, pad_l, _ = _same(L, k, s)
        else:
            Lout, pad_l = (L - k) // s + 1, 0
        self.rec.update({'kernel': [k, x.shape[1], filters], 'strides': s, 'padding': pad, 'pad_left': pad_l,
                         'use_bias': self.kwargs.get('use_bias', True), 'kernel_regularizer': self.kwargs.get('kernel_regularizer'),
                         'activation': self.kwargs.get('activation'), 'input_length': L, 'output': [Lout, filters]})
        return (Lout, filters)


class MaxPool1D(mg.Layer):
    def out_shape(self, x):
        pool = self.kwargs.get('pool_size', self.args[0] if self.args else 2)
        s = self.kwargs.get('strides') or pool
        pad = self.kwargs.get('padding', 'valid')
        L = x.shape[0]
        if pad == 'same':
            Lout, pad_l, total = _same(L, pool, s)
        else:
            Lout, pad_l, total = (L - pool) // s + 1, 0, 0
        self.rec.update({'pool_size': pool, 'strides': s, 'padding': pad, 'input_length': L, 'pad_left': pad_l, 'pad_total': total,
                         'output': [Lout, x.shape[1]]})
        return (Lout, x.shape[1])


class _Merge(mg.Layer):
    def __call__(self, xs):
        assert len(xs) == 2 and xs[0].shape[0] == xs[1].shape[0]
        a, b = xs[0].shape[1], xs[1].shape[1]
        assert a == b or 1 in (a, b)
        self.rec.update({'inputs': [list(x.shape) for x in xs], 'output': [xs[0].shape[0], max(a, b)]})
        return mg.T((xs[0].shape[0], max(a, b)))


class Add(_Merge):
    pass


class Multiply(_Merge):
    pass


class GRU(mgru.GRU):
    def __init__(self, *args, **kwargs):
        mgru.GRU.__init__(self, *args, **kwargs)
        self.rec.update({'kernel_l2': (kwargs.get('kernel_regularizer') or {}).get('l2', 0.0),
                         'recurrent_l2': (kwargs.get('recurrent_regularizer') or {}).get('l2', 0.0),
                         'bias_l2': (kwargs.get('bias_regularizer') or {}).get('l2', 0.0)})


class Bidirectional(mgru.Bidirectional):
    def out_shape(self, x):
        out = mgru.Bidirectional.out_shape(self, x)
        inner = self.args[0]
        self.rec.update({k: inner.rec[k] for k in ('kernel_l2', 'recurrent_l2', 'bias_l2')})
        return out


class Dense(mg.Dense):
    def out_shape(self, x):
        out = mg.Dense.out_shape(self, x)
        self.rec['kernel_l2'] = (self.kwargs.get('kernel_regularizer') or {}).get('l2', 0.0)
        return out


def int_shape(x):
    return (None,) + tuple(x.shape)


def reshape(x, shape):
    assert shape[0] == -1
    n = 1
    for d in x.shape:
        n *= d
    m = 1
    for d in shape[1:]:
        m *= d
    assert n == m
    return mg.T(shape[1:])


def extract_image_patches(x, ksizes, strides, rates, padding):
    """[1, W, 1] -> [1, Lout, ksize]: the framing of a 1-D signal."""
    assert x.shape[0] == 1 and x.shape[2] == 1 and rates == [1, 1, 1, 1] and padding == 'SAME'
    Lout, _, _ = _same(x.shape[1], ksizes[2], strides[2])
    return mg.T((1, Lout, ksizes[2]))


def install_stubs():
    mgru.install_stubs()
    kl = sys.modules['keras.layers']
    for c in (Lambda, Conv1D, MaxPool1D, Add, Multiply, GRU, Bidirectional, Dense):
        setattr(kl, c.__name__, c)
    kl.__all__ = list(kl.__all__) + ['MaxPool1D', 'Add', 'Multiply']
    sys.modules['keras.activations'].softmax = softmax
    kb = sys.modules['keras.backend']
    kb.int_shape, kb.reshape = int_shape, reshape
    sys.modules['tensorflow'].extract_image_patches = extract_image_patches


def record(builder, input_size, num_classes):
    mg._counts.clear()
    del mg._layers[:]
    model = builder(input_size=input_size, num_classes=num_classes)
    weights = []
    for r in mg._layers:
        l2 = (r.get('kernel_regularizer') or {}).get('l2', 0.0)
        if r['class'] == 'DepthwiseConv2D':
            weights.append({'name': r['name'] + '/depthwise_kernel', 'shape': r['kernel'], 'l2': l2})
            assert not r['use_bias']
        elif r['class'] == 'Conv1D':
            weights.append({'name': r['name'] + '/kernel', 'shape': r['kernel'], 'l2': l2})
            assert not r['use_bias']
        elif r['class'] == 'BatchNormalization':
            for w in ('gamma', 'beta', 'moving_mean', 'moving_variance'):
                weights.append({'name': '%s/%s' % (r['name'], w), 'shape': [r['channels']], 'l2': 0.0, 'state': w.startswith('moving')})
        elif r['class'] == 'Bidirectional':
            for d in ('forward', 'backward'):
                for w, reg in (('kernel', 'kernel_l2'), ('recurrent_kernel', 'recurrent_l2'), ('bias', 'bias_l2')):
                    weights.append({'name': '%s/%s_%s/%s' % (r['name'], d, r['layer'], w), 'shape': r[w], 'l2': r[reg]})
        elif r['class'] == 'Dense':
            weights.append({'name': r['name'] + '/kernel', 'shape': r['kernel'], 'l2': r['kernel_l2']})
            if r['use_bias']:
                weights.append({'name': r['name'] + '/bias', 'shape': [r['kernel'][1]], 'l2': 0.0})
    return {'model_name': model.name, 'optimizer': model.optimizer.kind, 'lr': model.optimizer.lr, 'loss': model.loss,
            'input_size': input_size, 'num_classes': num_classes, 'output_shape': list(model.output_shape),
            'layers': [{k: v for k, v in r.items() if k != 'kernel_regularizer'} for r in mg._layers], 'weights': weights}


def main():
    install_stubs()
    sys.path.insert(0, mg.REF)
    import model as ref_model
    out = {'xception_with_attention': record(ref_model.xception_with_attention_model, 16000, 12),
           'xception_with_attention_4000': record(ref_model.xception_with_attention_model, 4000, 12)}
    path = os.path.join(mg.OUT, 'xception_models.json')
    with open(path, 'w') as f:
        json.dump(out, f, indent=1, sort_keys=True)
    print('wrote', path)


if __name__ == '__main__':
    main()
