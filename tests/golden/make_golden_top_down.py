#!/usr/bin/env python
"""Layer structure of the reference's conv_1d_top_down_model (model.py:1326-1397) at 16000 and 17600 samples, recorded BY RUNNING
the reference's own model builder.

Build container only (needs the reference checkout):   python tests/golden/make_golden_top_down.py

The recording stand-ins for keras are make_golden_grouped.py's and make_golden_dwk.py's (every layer class records its constructor
arguments when it is created and computes its output shape when it is called on a stand-in tensor), plus what this model adds: a
Conv1D that may carry a bias, a Lambda that records both the channel slices and the expand_dims / squeeze reshapes, and the DATA
FLOW - every stand-in tensor gets a number, every layer records which tensors it read and which it made.  The context blocks cut
a slice per group and then hand the unsliced tensor to the group's depthwise block: those slice Lambdas are recorded with
'dead': true (nothing reads what they made), and the depthwise kernels behind them with the full channel count.  Names follow
Keras 2.1's per-class auto-numbering in creation order.  No reference source text is stored: tests/golden/top_down_model.json
holds the recorded structure only.
"""
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import make_golden_dwk as md  # noqa: E402
import make_golden_grouped as mg  # noqa: E402

_seen = {}      # id(tensor) -> (number, the tensor: kept alive so that ids are not reused)


def uid(t):
    if id(t) not in _seen:
        _seen[id(t)] = (len(_seen), t)
    return _seen[id(t)][0]


class Conv1D(md.Conv1D):
    pass


class Lambda(mg.Layer):
    def __call__(self, x):
        out = self.args[0](x)
        self.rec['output'] = list(out.shape)
        if getattr(out, 'slice', None) is not None:
            start, stop = out.slice
            C = x.shape[-1]
            self.rec.update({'requested': [start, stop], 'slice': [min(start, C), min(stop, C)], 'in_channels': C,
                             'channels': out.shape[-1]})
        return out


def traced(cls):
    """cls with the numbers of the tensors a call reads and makes in its record"""
    class Traced(cls):
        def __call__(self, x):
            self.rec['reads'] = [uid(t) for t in x] if isinstance(x, (list, tuple)) else [uid(x)]
            out = cls.__call__(self, x)
            self.rec['makes'] = uid(out)
            return out
    Traced.__name__ = cls.__name__
    return Traced


def install_stubs():
    md.install_stubs()
    kl = sys.modules['keras.layers']
    kl.Conv1D = Conv1D
    kl.Lambda = Lambda
    for name in kl.__all__:
        c = getattr(kl, name)
        if isinstance(c, type):
            setattr(kl, name, traced(c))
    mob = sys.modules['keras.applications.mobilenet']
    mob.DepthwiseConv2D = traced(mob.DepthwiseConv2D)


def record(builder, input_size, num_classes):
    mg._counts.clear()
    del mg._layers[:]
    _seen.clear()
    model = builder(input_size=input_size, num_classes=num_classes)
    read = set(t for r in mg._layers for t in r.get('reads', ()))
    weights = []
    for r in mg._layers:
        l2 = (r.get('kernel_regularizer') or {}).get('l2', 0.0)
        if r['class'] == 'Lambda' and 'slice' in r:
            r['dead'] = r['makes'] not in read
        if r['class'] == 'DepthwiseConv2D':
            weights.append({'name': r['name'] + '/depthwise_kernel', 'shape': r['kernel'], 'l2': l2})
            assert not r['use_bias']
        elif r['class'] in ('Conv1D', 'Dense'):
            weights.append({'name': r['name'] + '/kernel', 'shape': r['kernel'], 'l2': l2})
            if r['use_bias']:
                weights.append({'name': r['name'] + '/bias', 'shape': [r['kernel'][-1]], 'l2': 0.0})
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
    out = {'conv_1d_top_down_%d' % L: record(ref_model.conv_1d_top_down_model, L, 12) for L in (16000, 17600)}
    path = os.path.join(mg.OUT, 'top_down_model.json')
    with open(path, 'w') as f:
        json.dump(out, f, indent=1, sort_keys=True)
    print('wrote', path)


if __name__ == '__main__':
    main()
