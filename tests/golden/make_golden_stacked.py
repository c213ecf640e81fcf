#!/usr/bin/env python
"""Layer structure of the reference's conv_1d_time_stacked_model / conv_1d_heavy_model (model.py:257-309, 409-467), recorded
BY RUNNING the reference's own model builders.

Build container only (needs the reference checkout):   python tests/golden/make_golden_stacked.py

The recording stand-ins for keras are make_golden_grouped.py's (every layer class records its constructor arguments when it
is created and computes its output shape when it is called on a stand-in tensor), plus the three things these two models add:
MaxPool1D (VALID window arithmetic), a Conv1D that also records its activation, and Adam.  Names follow Keras 2.1's per-class
auto-numbering in creation order.  No reference source text is stored: tests/golden/stacked_models.json holds the recorded
structure only (layer classes, names and arguments; weight names and shapes in order; output shapes; optimizer class and lr;
loss).
"""
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import make_golden_grouped as mg  # noqa: E402


class Conv1D(mg.Conv1D):
    def out_shape(self, x):
        out = mg.Conv1D.out_shape(self, x)
        self.rec['activation'] = self.kwargs.get('activation')
        return out


class MaxPool1D(mg.Layer):
    def out_shape(self, x):
        pool = self.kwargs.get('pool_size', self.args[0] if self.args else 2)
        s = self.kwargs.get('strides') or pool
        pad = self.kwargs.get('padding', 'valid')
        assert pad == 'valid'
        L = (x.shape[0] - pool) // s + 1
        self.rec.update({'pool_size': pool, 'strides': s, 'padding': pad, 'input_length': x.shape[0],
                         'output': [L, x.shape[1]]})
        return (L, x.shape[1])


class Adam(object):
    def __init__(self, lr=0.001, **kw):
        self.kind, self.lr = 'Adam', lr


def install_stubs():
    mg.install_stubs()
    kl = sys.modules['keras.layers']
    kl.Conv1D = Conv1D
    kl.MaxPool1D = MaxPool1D
    kl.__all__ = list(kl.__all__) + ['MaxPool1D']
    sys.modules['keras.optimizers'].Adam = Adam


def record(builder, input_size, num_classes):
    mg._counts.clear()
    del mg._layers[:]
    model = builder(input_size=input_size, num_classes=num_classes)
    weights = []
    for r in mg._layers:
        if r['class'] == 'Conv1D':
            weights.append({'name': r['name'] + '/kernel', 'shape': r['kernel'],
                            'l2': (r['kernel_regularizer'] or {}).get('l2', 0.0)})
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
    out = {'conv_1d_time_stacked': record(ref_model.conv_1d_time_stacked_model, 16000, 12),
           'conv_1d_heavy': record(ref_model.conv_1d_heavy_model, 16000, 12)}
    path = os.path.join(mg.OUT, 'stacked_models.json')
    with open(path, 'w') as f:
        json.dump(out, f, indent=1, sort_keys=True)
    print('wrote', path)


if __name__ == '__main__':
    main()
