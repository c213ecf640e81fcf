#!/usr/bin/env python
"""Layer structure of the reference's conv_2d_mobile_model / conv_2d_fast_model (model.py:547-639), recorded BY RUNNING the
reference's own model builders.

Build container only (needs the reference checkout):   python tests/golden/make_golden_conv2d.py

The recording stand-ins for keras are make_golden_grouped.py's (every layer class records its constructor arguments when it is
created and computes its output shape when it is called on a stand-in tensor), plus what these models add: Conv2D (strides,
dilation, bias; TensorFlow's SAME geometry recorded per axis as [front, back] pad pairs next to the output shape), MaxPool2D,
GlobalAveragePooling2D, an Activation that records which function it applies, a Lambda whose stand-in tensor takes the arithmetic
of Preprocess, and an SGD that records lr and momentum.  Names follow Keras 2.1's per-class auto-numbering in creation order.  No
reference source text is stored: tests/golden/conv2d_models.json holds the recorded structure only (layer classes, names and
arguments; weight names and shapes in order; output shapes; optimizer class, lr and momentum; loss).
"""
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import make_golden_grouped as mg  # noqa: E402
import make_golden_stacked as ms  # noqa: E402


def _pair(v):
    return [v, v] if isinstance(v, int) else list(v)


def _axis(n, k, s, d, padding):
    """-> output length, [pad in front, pad behind] of one axis (TensorFlow: the smaller half in front)"""
    span = d * (k - 1) + 1
    if padding == 'same':
        out = -(-n // s)
        total = max((out - 1) * s + span - n, 0)
        return out, [total // 2, total - total // 2]
    return (n - span) // s + 1, [0, 0]


class Arith(mg.T):
    """Stand-in tensor that lets Preprocess's (x + 0.8) / 7 through and remembers that it happened"""

    def __init__(self, shape, ops=()):
        mg.T.__init__(self, shape)
        self.ops = list(ops)

    def __add__(self, v):
        return Arith(self.shape, self.ops + [['add', v]])

    def __truediv__(self, v):
        return Arith(self.shape, self.ops + [['div', v]])

    __div__ = __truediv__


def clip(x, lo, hi):
    return Arith(x.shape, x.ops + [['clip', lo, hi]])


class Lambda(mg.Layer):
    def __call__(self, x):
        out = self.args[0](Arith(x.shape))
        rec = dict(self.rec, ops=out.ops, output=list(out.shape))
        if rec['ops']:
            mg._layers.append(rec)     # (the reference creates its Lambda layers at import: record the CALL)
        return mg.T(out.shape)


class Conv2D(mg.Layer):
    def out_shape(self, x):
        filters = self.args[0]
        kh, kw = _pair(self.kwargs['kernel_size'] if 'kernel_size' in self.kwargs else self.args[1])
        sh, sw = _pair(self.kwargs.get('strides', 1))
        dh, dw = _pair(self.kwargs.get('dilation_rate', 1))
        pad = self.kwargs.get('padding', 'valid')
        H, W, C = x.shape
        Ho, ph = _axis(H, kh, sh, dh, pad)
        Wo, pw = _axis(W, kw, sw, dw, pad)
        self.rec.update({'kernel': [kh, kw, C, filters], 'strides': [sh, sw], 'dilation_rate': [dh, dw], 'padding': pad,
                         'use_bias': self.kwargs.get('use_bias', True), 'activation': self.kwargs.get('activation'),
                         'input': [H, W, C], 'pads': [ph, pw], 'output': [Ho, Wo, filters]})
        return (Ho, Wo, filters)


class MaxPool2D(mg.Layer):
    def out_shape(self, x):
        ph, pw = _pair(self.kwargs.get('pool_size', self.args[0] if self.args else 2))
        strides = self.kwargs.get('strides')
        sh, sw = _pair(strides) if strides else (ph, pw)
        pad = self.kwargs.get('padding', 'valid')
        assert pad == 'valid'
        H, W, C = x.shape
        out = [(H - ph) // sh + 1, (W - pw) // sw + 1, C]
        self.rec.update({'pool_size': [ph, pw], 'strides': [sh, sw], 'padding': pad, 'input': [H, W, C], 'output': out})
        return tuple(out)


class GlobalAveragePooling2D(mg.Layer):
    def out_shape(self, x):
        self.rec.update({'input': list(x.shape), 'output': [x.shape[2]]})
        return (x.shape[2],)


class Activation(mg.Layer):
    def out_shape(self, x):
        f = self.args[0]
        self.rec['function'] = f if isinstance(f, str) else f.__name__
        return x.shape


class SGD(object):
    def __init__(self, lr=0.01, momentum=0.0, decay=0.0, nesterov=False):
        self.kind, self.lr, self.momentum, self.decay, self.nesterov = 'SGD', lr, momentum, decay, nesterov


def install_stubs():
    ms.install_stubs()
    kl = sys.modules['keras.layers']
    for c in (Lambda, Conv2D, MaxPool2D, GlobalAveragePooling2D, Activation):
        setattr(kl, c.__name__, c)
    kl.__all__ = list(kl.__all__) + ['Conv2D', 'MaxPool2D', 'GlobalAveragePooling2D']
    sys.modules['keras.optimizers'].SGD = SGD
    sys.modules['keras.backend'].clip = clip


def record(builder, input_size, num_classes):
    mg._counts.clear()
    del mg._layers[:]
    model = builder(input_size=input_size, num_classes=num_classes)
    weights = []
    for r in mg._layers:
        if r['class'] == 'Conv2D':
            weights.append({'name': r['name'] + '/kernel', 'shape': r['kernel']})
            if r['use_bias']:
                weights.append({'name': r['name'] + '/bias', 'shape': [r['kernel'][3]]})
        elif r['class'] == 'BatchNormalization':
            for w in ('gamma', 'beta', 'moving_mean', 'moving_variance'):
                weights.append({'name': '%s/%s' % (r['name'], w), 'shape': [r['channels']], 'state': w.startswith('moving')})
        elif r['class'] == 'Dense':
            weights.append({'name': r['name'] + '/kernel', 'shape': r['kernel']})
            if r['use_bias']:
                weights.append({'name': r['name'] + '/bias', 'shape': [r['kernel'][1]]})
    opt = model.optimizer
    return {'model_name': model.name, 'optimizer': opt.kind, 'lr': opt.lr, 'momentum': opt.momentum, 'nesterov': opt.nesterov,
            'decay': opt.decay, 'loss': model.loss, 'input_size': input_size, 'num_classes': num_classes,
            'output_shape': list(model.output_shape), 'layers': [dict(r) for r in mg._layers], 'weights': weights}


def main():
    install_stubs()
    sys.path.insert(0, mg.REF)
    import model as ref_model
    out = {'conv_2d_mobile': record(ref_model.conv_2d_mobile_model, 3920, 12),
           'conv_2d_fast': record(ref_model.conv_2d_fast_model, 3920, 12)}
    path = os.path.join(mg.OUT, 'conv2d_models.json')
    with open(path, 'w') as f:
        json.dump(out, f, indent=1, sort_keys=True)
    print('wrote', path)


if __name__ == '__main__':
    main()
