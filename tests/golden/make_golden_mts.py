#!/usr/bin/env python
"""Layer structure of the reference's conv_1d_multi_time_sliced_model (model.py:1080-1156), recorded BY RUNNING the reference's own
model builder.

Build container only (needs the reference checkout):   python tests/golden/make_golden_mts.py

The recording stand-ins for keras are make_golden_grouped.py's and make_golden_dwk.py's (every layer class records its constructor
arguments when it is created and computes its output shape when it is called on a stand-in tensor), plus what this model adds:
MaxPool1D with padding='same' (TensorFlow's length and left padding recorded next to it), a Concatenate that records its axis,
inputs and the producers of its inputs, and a Conv1D that records bias and activation.  Every layer also records which layer made
its input (`input_from`), so that the two tensors with two consumers show in the fixture.  Names follow Keras 2.1's per-class
auto-numbering in creation order.  No reference source text is stored: tests/golden/mts_models.json holds the recorded structure
only.
"""
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import make_golden_grouped as mg  # noqa: E402
import make_golden_dwk as md  # noqa: E402


def _tag(out, name):
    out.made_by = name
    return out


class _Tracked(object):
    """Mixin: the output tensor remembers the layer that made it, the record names the layer that made the input."""

    def __call__(self, x):
        self.rec['input_from'] = getattr(x, 'made_by', 'input')
        out = super(_Tracked, self).__call__(x)
        return _tag(out, self.name)


class Lambda(_Tracked, md.Lambda):
    def __call__(self, x):
        out = self.args[0](x)
        self.rec['output'] = list(out.shape)
        self.rec['input_from'] = getattr(x, 'made_by', 'input')
        if out is x:            # PreprocessRaw is the identity
            return x
        return _tag(out, getattr(x, 'made_by', 'input'))   # shape plumbing (expand_dims / squeeze): the tensor keeps its maker


class DepthwiseConv2D(_Tracked, md.DepthwiseConv2D):
    pass


class Conv1D(_Tracked, md.Conv1D):
    pass


class BatchNormalization(_Tracked, mg.BatchNormalization):
    pass


class Activation(_Tracked, mg.Activation):
    pass


class Dropout(_Tracked, mg.Dropout):
    pass


class Reshape(_Tracked, mg.Reshape):
    pass


class MaxPool1D(_Tracked, mg.Layer):
    def out_shape(self, x):
        pool = self.kwargs.get('pool_size', self.args[0] if self.args else 2)
        s = self.kwargs.get('strides') or pool
        pad = self.kwargs.get('padding', 'valid')
        L = x.shape[0]
        if pad == 'same':
            Lout = -(-L // s)
            total = max((Lout - 1) * s + pool - L, 0)
            pad_l = total // 2
        else:
            Lout, pad_l, total = (L - pool) // s + 1, 0, 0
        self.rec.update({'pool_size': pool, 'strides': s, 'padding': pad, 'input_length': L, 'pad_left': pad_l,
                         'pad_total': total, 'output': [Lout, x.shape[1]]})
        return (Lout, x.shape[1])


class Concatenate(mg.Layer):
    def __call__(self, xs):
        axis = self.kwargs.get('axis', -1)
        assert axis == -1 and all(len(x.shape) == 2 and x.shape[0] == xs[0].shape[0] for x in xs)
        self.rec.update({'axis': axis, 'inputs': [list(x.shape) for x in xs],
                         'inputs_from': [getattr(x, 'made_by', 'input') for x in xs]})
        out = mg.T((xs[0].shape[0], sum(x.shape[1] for x in xs)))
        self.rec['output'] = list(out.shape)
        return _tag(out, self.name)


def install_stubs():
    md.install_stubs()
    kl = sys.modules['keras.layers']
    for c in (Lambda, Conv1D, BatchNormalization, Activation, Dropout, Reshape, MaxPool1D, Concatenate):
        setattr(kl, c.__name__, c)
    kl.__all__ = list(kl.__all__) + ['MaxPool1D']
    sys.modules['keras.applications.mobilenet'].DepthwiseConv2D = DepthwiseConv2D


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
            if r['use_bias']:
                weights.append({'name': r['name'] + '/bias', 'shape': [r['kernel'][2]], 'l2': 0.0})
        elif r['class'] == 'BatchNormalization':
            for w in ('gamma', 'beta', 'moving_mean', 'moving_variance'):
                weights.append({'name': '%s/%s' % (r['name'], w), 'shape': [r['channels']], 'l2': 0.0,
                                'state': w.startswith('moving')})
    return {'model_name': model.name, 'optimizer': model.optimizer.kind, 'lr': model.optimizer.lr, 'loss': model.loss,
            'input_size': input_size, 'num_classes': num_classes, 'output_shape': list(model.output_shape),
            'layers': [{k: v for k, v in r.items() if k != 'kernel_regularizer'} for r in mg._layers], 'weights': weights}


def main():
    install_stubs()
    sys.path.insert(0, mg.REF)
    import model as ref_model
    out = {'conv_1d_multi_time_sliced': record(ref_model.conv_1d_multi_time_sliced_model, 16000, 12)}
    path = os.path.join(mg.OUT, 'mts_models.json')
    with open(path, 'w') as f:
        json.dump(out, f, indent=1, sort_keys=True)
    print('wrote', path)


if __name__ == '__main__':
    main()
