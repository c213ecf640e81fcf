#!/usr/bin/env python
"""Layer structure of the reference's conv_1d_gru_model (model.py:470-512), recorded BY RUNNING the reference's own model builder.

Build container only (needs the reference checkout):   python tests/golden/make_golden_dwk.py

The recording stand-ins for keras are make_golden_grouped.py's (every layer class records its constructor arguments when it is
created and computes its output shape when it is called on a stand-in tensor), plus what this model adds:
keras.applications.mobilenet.DepthwiseConv2D on a [1, L, C] tensor (kernel shape [1, k, C, 1], strides, padding and the SAME /
VALID length arithmetic, with TensorFlow's left padding recorded next to it), K.expand_dims / K.squeeze inside the Lambdas, and a
Dense that records its bias.  Names follow Keras 2.1's per-class auto-numbering in creation order.  No reference source text is
stored: tests/golden/dwk_models.json holds the recorded structure only.
"""
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import make_golden_grouped as mg  # noqa: E402


def expand_dims(x, axis):
    shp = list(x.shape)
    assert axis >= 1               # axis 0 is the batch axis the stand-in tensors leave out
    shp.insert(axis - 1, 1)
    return mg.T(shp)


def squeeze(x, axis):
    shp = list(x.shape)
    assert axis >= 1 and shp[axis - 1] == 1
    del shp[axis - 1]
    return mg.T(shp)


class Lambda(mg.Layer):
    def __call__(self, x):
        out = self.args[0](x)
        self.rec['output'] = list(out.shape)
        return out


class DepthwiseConv2D(mg.Layer):
    def out_shape(self, x):
        kh, kw = self.args[0]
        s = self.kwargs.get('strides', 1)
        pad = self.kwargs.get('padding', 'valid')
        assert len(x.shape) == 3 and x.shape[0] == 1 and kh == 1 and self.kwargs.get('dilation_rate', 1) == 1
        L, C = x.shape[1], x.shape[2]
        if pad == 'same':
            Lout = -(-L // s)
            total = max((Lout - 1) * s + kw - L, 0)
            pad_l = total // 2
        else:
            Lout, pad_l = (L - kw) // s + 1, 0
        self.rec.update({'kernel': [1, kw, C, 1], 'strides': s, 'padding': pad, 'use_bias': self.kwargs.get('use_bias', True),
                         'kernel_regularizer': self.kwargs.get('kernel_regularizer'), 'input_length': L, 'pad_left': pad_l,
                         'output': [Lout, C]})
        return (1, Lout, C)


class Conv1D(mg.Conv1D):
    def out_shape(self, x):
        out = mg.Conv1D.out_shape(self, x)
        self.rec['activation'] = self.kwargs.get('activation')
        return out


def install_stubs():
    mg.install_stubs()
    kl = sys.modules['keras.layers']
    kl.Conv1D = Conv1D
    kl.Lambda = Lambda
    sys.modules['keras.applications.mobilenet'].DepthwiseConv2D = DepthwiseConv2D
    kb = sys.modules['keras.backend']
    kb.expand_dims, kb.squeeze = expand_dims, squeeze


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
                weights.append({'name': '%s/%s' % (r['name'], w), 'shape': [r['channels']], 'l2': 0.0,
                                'state': w.startswith('moving')})
        elif r['class'] == 'Dense':
            weights.append({'name': r['name'] + '/kernel', 'shape': r['kernel'], 'l2': 0.0})
            if r['use_bias']:
                weights.append({'name': r['name'] + '/bias', 'shape': [r['kernel'][1]], 'l2': 0.0})
    return {'model_name': model.name, 'optimizer': model.optimizer.kind, 'lr': model.optimizer.lr, 'loss': model.loss,
            'input_size': input_size, 'num_classes': num_classes, 'output_shape': list(model.output_shape),
            'layers': [{k: v for k, v in r.items() if k != 'kernel_regularizer'} for r in mg._layers], 'weights': weights}


def main():
    install_stubs()
    sys.path.insert(0, mg.REF)
    import model as ref_model
    out = {'conv_1d_gru': record(ref_model.conv_1d_gru_model, 16000, 12)}
    path = os.path.join(mg.OUT, 'dwk_models.json')
    with open(path, 'w') as f:
        json.dump(out, f, indent=1, sort_keys=True)
    print('wrote', path)


if __name__ == '__main__':
    main()
