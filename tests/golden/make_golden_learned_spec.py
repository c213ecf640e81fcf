#!/usr/bin/env python
"""Layer structure of the reference's conv_1d_learned_spec_model (model.py:1159-1246) at 16000 and 15000 samples, recorded BY
RUNNING the reference's own model builder.

Build container only (needs the reference checkout):   python tests/golden/make_golden_learned_spec.py

The recording stand-ins for keras are make_golden_grouped.py's and make_golden_dwk.py's (every layer class records its
constructor arguments when it is created and computes its output shape when it is called on a stand-in tensor), plus what this
model adds: a Conv1D that also takes padding='same' with strides (ceil(L / strides) rows, TensorFlow's left padding recorded
next to them) and a Lambda that records the slice as TensorFlow CLIPS it at the channel count (the second group of the first
context block asks for channels 180:360 of 300 and gets 120).  Names follow Keras 2.1's per-class auto-numbering in creation
order.  No reference source text is stored: tests/golden/learned_spec_model.json holds the recorded structure only.
"""
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import make_golden_dwk as md  # noqa: E402
import make_golden_grouped as mg  # noqa: E402


class Conv1D(mg.Conv1D):
    def out_shape(self, x):
        if self.kwargs.get('padding', 'valid') != 'same':
            return mg.Conv1D.out_shape(self, x)
        filters, k = self.args[0], self.args[1]
        s = self.kwargs.get('strides', 1)
        assert self.kwargs.get('dilation_rate', 1) == 1
        L = -(-x.shape[0] // s)
        total = max((L - 1) * s + k - x.shape[0], 0)
        self.rec.update({'kernel': [k, x.shape[1], filters], 'strides': s, 'padding': 'same', 'pad_left': total // 2,
                         'use_bias': self.kwargs.get('use_bias', True), 'kernel_regularizer': self.kwargs.get('kernel_regularizer'),
                         'input_length': x.shape[0], 'output': [L, filters]})
        return (L, filters)


class Lambda(mg.Lambda):
    def __call__(self, x):
        out = mg.Lambda.__call__(self, x)
        if 'slice' in self.rec:
            start, stop = self.rec['slice']
            self.rec['requested'] = [start, stop]
            self.rec['slice'] = [min(start, x.shape[-1]), min(stop, x.shape[-1])]
            self.rec['channels'] = out.shape[-1]
            assert self.rec['channels'] == self.rec['slice'][1] - self.rec['slice'][0]
        return out


def install_stubs():
    md.install_stubs()
    kl = sys.modules['keras.layers']
    kl.Conv1D = Conv1D
    kl.Lambda = Lambda


def record(builder, input_size, num_classes):
    out = mg.record(builder, input_size, num_classes)
    ragged = [r for r in out['layers'] if r['class'] == 'Lambda' and r['requested'] != r['slice']]
    assert [r['channels'] for r in ragged] == [120], ragged       # the one clipped slice: channels 180:300
    return out


def main():
    install_stubs()
    sys.path.insert(0, mg.REF)
    import model as ref_model
    out = {'conv_1d_learned_spec_%d' % L: record(ref_model.conv_1d_learned_spec_model, L, 12) for L in (16000, 15000)}
    path = os.path.join(mg.OUT, 'learned_spec_model.json')
    with open(path, 'w') as f:
        json.dump(out, f, indent=1, sort_keys=True)
    print('wrote', path)


if __name__ == '__main__':
    main()
