#!/usr/bin/env python
"""Layer structure of the reference's conv_inception_d1_model (model.py:312-406), recorded BY RUNNING the reference's own model
builder.

Build container only (needs the reference checkout):   python tests/golden/make_golden_inception.py

The recording stand-ins for keras are make_golden_mts.py's (every layer class records its constructor arguments when it is
created, computes its output shape when it is called on a stand-in tensor and names the layer that made its input; MaxPool1D in
both paddings; a Concatenate that records its inputs and their producers) and make_golden_stacked.py's Adam, plus what this
model adds: a Conv1D with padding='same' and dilation_rate (TensorFlow's total and left padding at stride 1 recorded next to
it) and AveragePooling1D.  Names follow Keras 2.1's per-class auto-numbering in creation order.  No reference source text is
stored: tests/golden/inception_models.json holds the recorded structure only (layer classes, names and arguments; weight names
and shapes in order; output shapes; optimizer class and lr; loss).
"""
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import make_golden_grouped as mg  # noqa: E402
import make_golden_mts as mm  # noqa: E402
import make_golden_stacked as ms  # noqa: E402


class Conv1D(mm._Tracked, mg.Layer):
    def out_shape(self, x):
        filters, k = self.args[0], self.args[1]
        s = self.kwargs.get('strides', 1)
        pad = self.kwargs.get('padding', 'valid')
        dil = self.kwargs.get('dilation_rate', 1)
        assert s == 1 and pad in ('valid', 'same')
        L = x.shape[0]
        span = dil * (k - 1)
        if pad == 'same':   # TensorFlow SAME at stride 1: the effective kernel minus one, the smaller half in front
            Lout, total, pad_l = L, span, span // 2
        else:
            Lout, total, pad_l = L - span, 0, 0
        self.rec.update({'kernel': [k, x.shape[1], filters], 'strides': s, 'padding': pad, 'dilation_rate': dil,
                         'use_bias': self.kwargs.get('use_bias', True), 'activation': self.kwargs.get('activation'),
                         'kernel_regularizer': self.kwargs.get('kernel_regularizer'), 'input_length': L, 'pad_left': pad_l,
                         'pad_total': total, 'output': [Lout, filters]})
        return (Lout, filters)


class AveragePooling1D(mm._Tracked, mg.Layer):
    def out_shape(self, x):
        pool = self.kwargs.get('pool_size', self.args[0] if self.args else 2)
        s = self.kwargs.get('strides') or pool
        pad = self.kwargs.get('padding', 'valid')
        assert s == 1 and pad == 'same'
        self.rec.update({'pool_size': pool, 'strides': s, 'padding': pad, 'input_length': x.shape[0], 'pad_left': (pool - 1) // 2,
                         'pad_total': pool - 1, 'output': list(x.shape)})
        return x.shape


def install_stubs():
    mm.install_stubs()
    kl = sys.modules['keras.layers']
    kl.Conv1D = Conv1D
    kl.AveragePooling1D = AveragePooling1D
    kl.__all__ = list(kl.__all__) + ['AveragePooling1D']
    sys.modules['keras.optimizers'].Adam = ms.Adam


def main():
    install_stubs()
    sys.path.insert(0, mg.REF)
    import model as ref_model
    out = {'inception_d1': mm.record(ref_model.conv_inception_d1_model, 16000, 12)}
    path = os.path.join(mg.OUT, 'inception_models.json')
    with open(path, 'w') as f:
        json.dump(out, f, indent=1, sort_keys=True)
    print('wrote', path)


if __name__ == '__main__':
    main()
