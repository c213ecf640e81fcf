#!/usr/bin/env python
"""Layer structure of the reference's conv_1d_fast_model / conv_1d_spec_model (model.py:642-713, 1249-1323), recorded BY
RUNNING the reference's own model builders.

Build container only (needs /root/reference):   python tests/golden/make_golden_grouped.py

keras / tensorflow are not installed here.  They are replaced by small recording stand-ins: every layer class records its
constructor arguments when it is created and computes its output shape when it is called on a stand-in tensor (Conv1D
VALID arithmetic, Lambda applying the reference's own slice function to a tensor that records the slice bounds, Concatenate,
Flatten, Reshape, Dense).  Names follow Keras 2.1's per-class auto-numbering in creation order (class name in snake case +
'_<n>'), and weight shapes follow Keras' conventions (Conv1D kernel [k, in_channels, filters]; BatchNormalization gamma /
beta / moving_mean / moving_variance [channels]; Dense kernel [in, out] and bias [out]).  model.compile() records the
optimizer's lr and the loss.  No reference source text is stored: tests/golden/grouped_models.json holds the recorded
structure only.
"""
import json
import os
import re
import sys
import types

REF = '/root/reference'
OUT = os.path.dirname(os.path.abspath(__file__))

_counts = {}
_layers = []


def _snake(name):
    s = re.sub('(.)([A-Z][a-z0-9]+)', r'\1_\2', name)
    return re.sub('([a-z])([A-Z])', r'\1_\2', s).lower()


class T(object):
    """Stand-in tensor: shape without the batch axis; `slice` = (start, stop) of the channel slice that made it, if any."""

    def __init__(self, shape):
        self.shape = tuple(shape)
        self.slice = None

    def __getitem__(self, idx):
        assert isinstance(idx, tuple) and len(idx) == 3 and len(self.shape) == 2
        sl = idx[2]
        start, stop = sl.start or 0, sl.stop
        width = len(range(self.shape[1])[start:stop])
        t = T((self.shape[0], width))
        t.slice = (start, stop)
        return t


class Layer(object):
    def __init__(self, *args, **kwargs):
        cls = type(self).__name__
        _counts[cls] = _counts.get(cls, 0) + 1
        self.name = kwargs.get('name') or '%s_%d' % (_snake(cls), _counts[cls])
        self.args, self.kwargs = args, kwargs
        self.rec = {'class': cls, 'name': self.name}
        _layers.append(self.rec)

    def __call__(self, x):
        out = T(self.out_shape(x))
        return out

    def out_shape(self, x):
        return x.shape


class Lambda(Layer):
    def __call__(self, x):
        out = self.args[0](x)
        if isinstance(out, T) and out.slice is not None:
            self.rec['slice'] = list(out.slice)
            self.rec['in_channels'] = x.shape[-1]
            return out
        return T(x.shape)


class Conv1D(Layer):
    def out_shape(self, x):
        filters, k = self.args[0], self.args[1]
        s = self.kwargs.get('strides', 1)
        pad = self.kwargs.get('padding', 'valid')
        assert pad == 'valid' and self.kwargs.get('dilation_rate', 1) == 1
        L = (x.shape[0] - k) // s + 1
        self.rec.update({'kernel': [k, x.shape[1], filters], 'strides': s, 'padding': pad,
                         'use_bias': self.kwargs.get('use_bias', True),
                         'kernel_regularizer': self.kwargs.get('kernel_regularizer'),
                         'input_length': x.shape[0], 'output': [L, filters]})
        return (L, filters)


class BatchNormalization(Layer):
    def out_shape(self, x):
        self.rec['channels'] = x.shape[-1]
        return x.shape


class Activation(Layer):
    pass


class Dropout(Layer):
    def out_shape(self, x):
        self.rec['rate'] = self.args[0]
        return x.shape


class Flatten(Layer):
    def out_shape(self, x):
        n = 1
        for d in x.shape:
            n *= d
        self.rec['output'] = [n]
        return (n,)


class Reshape(Layer):
    def out_shape(self, x):
        shp = list(self.args[0])
        n = 1
        for d in x.shape:
            n *= d
        if -1 in shp:
            known = 1
            for d in shp:
                known *= d if d != -1 else 1
            shp[shp.index(-1)] = n // known
        self.rec['output'] = shp
        return tuple(shp)


class Dense(Layer):
    def out_shape(self, x):
        units = self.args[0]
        self.rec.update({'kernel': [x.shape[-1], units], 'use_bias': self.kwargs.get('use_bias', True),
                         'activation': self.kwargs.get('activation')})
        return (units,)


class Concatenate(Layer):
    def __call__(self, xs):
        self.rec['inputs'] = [list(x.shape) for x in xs]
        return T((xs[0].shape[0], sum(x.shape[1] for x in xs)))


def Input(shape):
    return T(shape)


class Model(object):
    def __init__(self, inputs, outputs, name=None):
        self.name = name
        self.output_shape = outputs.shape

    def compile(self, optimizer=None, loss=None, metrics=None):
        self.optimizer, self.loss, self.metrics = optimizer, loss, metrics


class RMSprop(object):
    def __init__(self, lr=0.001, **kw):
        self.kind, self.lr = 'RMSprop', lr


def l2(c):
    return {'l2': c}


def install_stubs():
    mods = {}
    for name in ('tensorflow', 'keras', 'keras.backend', 'keras.layers', 'keras.layers.noise', 'keras.regularizers',
                 'keras.activations', 'keras.models', 'keras.applications', 'keras.applications.mobilenet',
                 'keras.optimizers', 'keras.losses', 'keras.metrics'):
        mods[name] = types.ModuleType(name)
        sys.modules[name] = mods[name]
    kl = mods['keras.layers']
    for c in (Lambda, Conv1D, BatchNormalization, Activation, Dropout, Flatten, Reshape, Dense, Concatenate, Input):
        setattr(kl, c.__name__, c)
    kl.__all__ = [c.__name__ for c in (Lambda, Conv1D, BatchNormalization, Activation, Dropout, Flatten, Reshape, Dense,
                                       Concatenate, Input)]
    mods['keras.layers.noise'].AlphaDropout = Layer
    mods['keras.regularizers'].l2 = l2
    mods['keras.activations'].softmax = 'softmax'
    mods['keras.models'].Model = Model
    mods['keras.applications.mobilenet'].DepthwiseConv2D = Layer
    mods['keras.optimizers'].RMSprop = RMSprop
    mods['keras.losses'].categorical_crossentropy = 'categorical_crossentropy'
    mods['keras.metrics'].categorical_accuracy = 'categorical_accuracy'
    k = mods['keras']
    k.backend, k.layers, k.optimizers, k.losses, k.metrics = (mods['keras.backend'], kl, mods['keras.optimizers'],
                                                              mods['keras.losses'], mods['keras.metrics'])


def record(builder, input_size, num_classes):
    _counts.clear()
    del _layers[:]
    model = builder(input_size=input_size, num_classes=num_classes)
    layers = [dict(r) for r in _layers if r['class'] not in ('Lambda',) or 'slice' in r]
    weights = []
    for r in _layers:
        if r['class'] == 'Conv1D':
            weights.append({'name': r['name'] + '/kernel', 'shape': r['kernel'],
                            'l2': (r['kernel_regularizer'] or {}).get('l2', 0.0)})
            assert not r['use_bias']
        elif r['class'] == 'BatchNormalization':
            for w in ('gamma', 'beta', 'moving_mean', 'moving_variance'):
                weights.append({'name': '%s/%s' % (r['name'], w), 'shape': [r['channels']], 'l2': 0.0,
                                'state': w.startswith('moving')})
        elif r['class'] == 'Dense':
            weights.append({'name': r['name'] + '/kernel', 'shape': r['kernel'], 'l2': 0.0})
            if r['use_bias']:
                weights.append({'name': r['name'] + '/bias', 'shape': [r['kernel'][1]], 'l2': 0.0})
    return {'model_name': model.name, 'optimizer': model.optimizer.kind, 'lr': model.optimizer.lr, 'loss': model.loss,
            'input_size': input_size, 'num_classes': num_classes, 'output_shape': list(model.output_shape),
            'layers': [{k: v for k, v in r.items() if k != 'kernel_regularizer'} for r in layers], 'weights': weights}


def main():
    install_stubs()
    sys.path.insert(0, REF)
    import model as ref_model
    out = {'conv_1d_fast': record(ref_model.conv_1d_fast_model, 16000, 12),
           'conv_1d_spec': record(ref_model.conv_1d_spec_model, 16000, 12)}
    path = os.path.join(OUT, 'grouped_models.json')
    with open(path, 'w') as f:
        json.dump(out, f, indent=1, sort_keys=True)
    print('wrote', path)


if __name__ == '__main__':
    main()
